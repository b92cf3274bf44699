"""Writes ``tests/golden/log_strain_degenerate.npz``: logarithmic-strain J2 plasticity on ``log_strain_ref.degenerate_F()`` in mpmath
at 100 digits, by a formulation that never forms an eigenvector or a divided difference:

* ``E = logm(F^T F) / 2`` (``mpmath.logm``), the radial return with linear hardening on ``E - Ep_n`` in closed form;
* ``PK1_iJ = T : dE/dF_iJ`` by work conjugacy, the derivative of E by central differences (step 1e-30: truncation 1e-60);
* the tangent by central differences of PK1 at fixed old state (step 1e-20: truncation 1e-40, rounding 1e-60 / 1e-20).

Each point is evaluated from the natural state and from ``log_strain_ref.history_state`` (a plastic strain coaxial with nothing).
Run once (a few minutes on all cores): ``python tests/golden/make_log_strain.py``."""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import log_strain_ref as ls  # noqa: E402

DPS = 100
H_INNER = "1e-30"
H_OUTER = "1e-20"
TI, TJ = [int(i) for i in ls.TI], [int(j) for j in ls.TJ]
R3 = range(3)


def hencky(F):
    L = mp.logm(F.T * F) / 2
    return (L + L.T) / 2


def radial_return(E, Ep_n, p_n, prm):
    """(T, Ep, p, plastic) as 3x3 mpmath matrices / numbers: IsotropicLinearHardeningPlasticity.mfront:49-77 on eel_tr = E - Ep_n."""
    Ey, nu, s0, H0 = (mp.mpf(prm[k]) for k in ("E", "nu", "s0", "H0"))
    lam, mu = Ey * nu / (1 + nu) / (1 - 2 * nu), Ey / 2 / (1 + nu)
    eel = E - Ep_n
    tr = eel[0, 0] + eel[1, 1] + eel[2, 2]
    se = 2 * mu * (eel - tr / 3 * mp.eye(3))
    seq = mp.sqrt(mp.mpf(3) / 2 * sum(se[i, j] ** 2 for i in R3 for j in R3))
    f = seq - s0 - H0 * p_n
    plastic = f > 0
    Ep, p = Ep_n.copy(), p_n
    if plastic:
        dp = f / (H0 + 3 * mu)
        n = mp.mpf(3) / 2 * se / seq
        Ep = Ep_n + dp * n
        p = p_n + dp
        eel = eel - dp * n
    T = lam * tr * mp.eye(3) + 2 * mu * eel
    return T, Ep, p, plastic


def pk1(F, Ep_n, p_n, prm):
    T = radial_return(hencky(F), Ep_n, p_n, prm)[0]
    h = mp.mpf(H_INNER)
    P = mp.matrix(3, 3)
    for i in R3:
        for J in R3:
            dF = mp.matrix(3, 3)
            dF[i, J] = h
            dE = (hencky(F + dF) - hencky(F - dF)) / (2 * h)
            P[i, J] = sum(T[a, b] * dE[a, b] for a in R3 for b in R3)
    return P


def mandel(X):
    s = mp.sqrt(2)
    return [float(X[0, 0]), float(X[1, 1]), float(X[2, 2]), float(s * X[0, 1]), float(s * X[0, 2]), float(s * X[1, 2])]


def from_mandel(v):
    s = mp.sqrt(2)
    v = [mp.mpf(float(x)) for x in v]
    return mp.matrix([[v[0], v[3] / s, v[4] / s], [v[3] / s, v[1], v[5] / s], [v[4] / s, v[5] / s, v[2]]])


def one_point(args):
    F9, ep_n, p_n, prm = args
    with mp.workdps(DPS):
        F = mp.matrix(3, 3)
        for t in range(9):
            F[TI[t], TJ[t]] = mp.mpf(float(F9[t]))
        Ep_n, p_n = from_mandel(ep_n), mp.mpf(float(p_n))
        E = hencky(F)
        T, Ep, p, plastic = radial_return(E, Ep_n, p_n, prm)
        P = pk1(F, Ep_n, p_n, prm)
        h = mp.mpf(H_OUTER)
        A = np.empty((9, 9))
        for col in range(9):
            dF = mp.matrix(3, 3)
            dF[TI[col], TJ[col]] = h
            dP = (pk1(F + dF, Ep_n, p_n, prm) - pk1(F - dF, Ep_n, p_n, prm)) / (2 * h)
            A[:, col] = [float(dP[TI[r], TJ[r]]) for r in range(9)]
        return ([float(P[TI[r], TJ[r]]) for r in range(9)], A, mandel(E - Ep), float(p), mandel(Ep), bool(plastic))


def main():
    F9, labels = ls.degenerate_F()
    n = len(F9)
    out = {"F": F9, "labels": np.array(labels), "params": np.array([ls.PRM[k] for k in ("E", "nu", "s0", "H0")])}
    states = {"natural": ls.natural_state(n), "history": ls.history_state(n)}
    jobs = [(F9[k], ep[k], p[k], ls.PRM) for ep, p in states.values() for k in range(n)]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        res = pool.map(one_point, jobs, chunksize=1)
    for s, (name, (ep, p)) in enumerate(states.items()):
        r = res[s * n:(s + 1) * n]
        out[f"{name}_Ep_n"], out[f"{name}_p_n"] = ep, p
        for q, key in enumerate(("P", "A", "eel", "p", "Ep", "plastic")):
            out[f"{name}_{key}"] = np.array([x[q] for x in r])
        print(name, "plastic:", out[f"{name}_plastic"].astype(int))
    np.savez(ls.GOLDEN, **out)
    print("wrote", ls.GOLDEN)


if __name__ == "__main__":
    main()
