#!/usr/bin/env python3
"""Writes ``tests/golden/plane_stress.npz``: the two plane-stress return mappings (DXM_LAW_PS_QUADRATIC = 23, DXM_LAW_PS_POLYGON = 24)
at 50 digits (mpmath), in a formulation that shares nothing with the kernel's.

    quadratic   (C^-1 + l Q) s = C^-1 s_tr by a linear solve in the original components [xx, yy, sqrt(2) xy], l the root of
                s(l)^T Q s(l) = sig0^2 by a bracketing ``findroot``; the consistent tangent by differentiating that system:
                A - (A n)(A n)^T / (n^T A n), A = (C^-1 + l Q)^-1, n = Q s, with a 3 x 3 inverse
    polygon     principal values and axes by ``eigsy`` of the 2 x 2 stress; the active set of the projection chosen by the SIGN OF
                THE KKT MULTIPLIERS over every subset of at most two rows; the stress rebuilt from the axes

Two increments per case: the second starts from the first's plastic strain and unloads part of the batch.  The generator asserts that
every point is at least 1e-6 s* away from the yield surface, and for the polygon that every active multiplier and every inactive
row's slack is at least 1e-6 in scaled terms, so that which points count as yielded is decided without ambiguity.

    python tests/golden/make_plane_stress.py
"""
import itertools
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = mp.mpf("1e-6")
SQ2 = mp.sqrt(2)


def C_of(E, nu):
    E, nu = mp.mpf(E), mp.mpf(nu)
    return (E / (1 - nu**2)) * mp.matrix([[1, nu, 0], [nu, 1, 0], [0, 0, 1 - nu]])


def col(v):
    return mp.matrix([mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in v])


# ---- quadratic ---------------------------------------------------------------------------------------------------------------------
def quadratic_point(E, nu, sig0, q, eps, epn):
    C = C_of(E, nu)
    S = C**-1
    Q = mp.matrix([[1, mp.mpf(-1) / 2, 0], [mp.mpf(-1) / 2, 1, 0], [0, 0, mp.mpf(q)]])
    sig0 = mp.mpf(sig0)
    t = C * (eps - epn)
    f_tr = mp.sqrt((t.T * Q * t)[0]) - sig0
    assert abs(f_tr) >= MARGIN * sig0, ("too close to the surface", f_tr)
    if f_tr < 0:
        return t, epn, C, False

    def sigma(l):
        return mp.lu_solve(S + l * Q, S * t)

    def g(l):
        s = sigma(l)
        return (s.T * Q * s)[0] - sig0**2

    hi = mp.mpf(1) / mp.mpf(E)
    while g(hi) > 0:
        hi *= 2
    lam = mp.findroot(g, (mp.mpf(0), hi), solver="illinois", tol=mp.mpf("1e-90"), maxsteps=2000, verify=False)
    assert lam > 0 and abs(g(lam)) < mp.mpf("1e-40") * sig0**2
    s = sigma(lam)
    A = (S + lam * Q)**-1
    n = Q * s
    An = A * n
    T = A - (An * An.T) / (n.T * An)[0]
    return s, eps - S * s, T, True


# ---- polygon -----------------------------------------------------------------------------------------------------------------------
def polygon_point(E, nu, rows, eps, epn):
    C = C_of(E, nu)
    S = C**-1
    sstar = max(mp.mpf(r[2]) for r in rows)
    t = C * (eps - epn)
    A = mp.matrix([[t[0], t[2] / SQ2], [t[2] / SQ2, t[1]]])
    ev, V = mp.eigsy(A)
    p = mp.matrix([ev[1], ev[0]])
    v = [V[:, 1], V[:, 0]]
    Minv = C[0:2, 0:2]            # the stiffness of the principal values
    N = [mp.matrix([mp.mpf(r[0]), mp.mpf(r[1])]) for r in rows]
    d = [mp.mpf(r[2]) for r in rows]
    unit = [mp.sqrt((n.T * n)[0]) for n in N]
    slack_tr = [(d[k] - (N[k].T * p)[0]) / unit[k] for k in range(len(rows))]
    assert abs(min(slack_tr)) >= MARGIN * sstar, ("too close to the surface", slack_tr)
    accepted = []
    for size in (0, 1, 2):
        for act in itertools.combinations(range(len(rows)), size):
            if size == 0:
                c, mu = p, []
            else:
                Na = mp.matrix([[N[k][0], N[k][1]] for k in act])
                G = Na * Minv * Na.T
                if size == 2 and abs(mp.det(G)) < mp.mpf("1e-30") * abs(G[0, 0] * G[1, 1]):
                    continue
                m_ = mp.lu_solve(G, Na * p - mp.matrix([d[k] for k in act]))
                mu = [m_[i] for i in range(size)]
                c = p - Minv * Na.T * m_
            if any(m <= 0 for m in mu):
                continue
            slack = [(d[k] - (N[k].T * c)[0]) / unit[k] for k in range(len(rows)) if k not in act]
            if any(x < 0 for x in slack):
                continue
            scaled_mu = [mu[i] * mp.sqrt(((Minv * N[k]).T * (Minv * N[k]))[0]) / sstar for i, k in enumerate(act)]
            accepted.append((act, c, scaled_mu, [x / sstar for x in slack]))
    assert len(accepted) == 1, accepted
    act, c, scaled_mu, slack = accepted[0]
    assert all(m >= MARGIN for m in scaled_mu) and all(x >= MARGIN for x in slack), (act, scaled_mu, slack)
    if not act:
        return t, epn, False, act
    Sg = c[0] * v[0] * v[0].T + c[1] * v[1] * v[1].T
    s = mp.matrix([Sg[0, 0], Sg[1, 1], SQ2 * Sg[0, 1]])
    return s, eps - S * s, True, act


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def to_strain(E, nu, sig):
    S = np.array([[1.0, -nu, 0.0], [-nu, 1.0, 0.0], [0.0, 0.0, 1.0 + nu]]) / E
    return sig @ S.T


def quadratic_inputs(E, nu, sig0, q, rng):
    factors = [0.3, 0.9, 1 + 2e-5, 1.001, 1.05, 1.5, 3.0, 10.0, 1e2, 1e3, 1e4]
    sig = []
    for f in factors:
        for _ in range(3):
            v = rng.normal(size=3)
            Q = np.array([[1, -0.5, 0], [-0.5, 1, 0], [0, 0, q]])
            sig.append(v * (f * sig0 / np.sqrt(v @ Q @ v)))
    # on the axes of the diagonalising basis and in pure shear, yielded
    for v in ([1, 1, 0], [1, -1, 0], [0, 0, 1], [-1, -1, 0]):
        v = np.array(v, dtype=float)
        Q = np.array([[1, -0.5, 0], [-0.5, 1, 0], [0, 0, q]])
        sig.append(v * (2.0 * sig0 / np.sqrt(v @ Q @ v)))
    sig = np.array(sig)
    far = np.array([f >= 1e2 for f in factors for _ in range(3)] + [False] * 4)
    return sig, far


def rotate(p1, p2, theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([p1 * c * c + p2 * s * s, p1 * s * s + p2 * c * c, np.sqrt(2.0) * (p1 - p2) * c * s])


def polygon_inputs(E, nu, rows, rng):
    Minv = (E / (1 - nu**2)) * np.array([[1.0, nu], [nu, 1.0]])
    N = np.array([[r[0], r[1]] for r in rows])
    d = np.array([r[2] for r in rows])
    sstar = d.max()
    W = N @ Minv
    unitw = np.linalg.norm(W, axis=1)
    sig = []
    scales = [3e-5, 1e-2, 0.3, 2.0, 50.0, 1e3]
    # the faces: a point of the face's interior plus a multiple of M^-1 n
    for k in range(len(rows)):
        tangent = np.array([-N[k, 1], N[k, 0]]) / np.linalg.norm(N[k])
        foot = N[k] * d[k] / (N[k] @ N[k])
        # the face's extent along its tangent, from the other rows
        lo, hi = -np.inf, np.inf
        for j in range(len(rows)):
            if j == k:
                continue
            a, b = N[j] @ tangent, d[j] - N[j] @ foot
            if abs(a) > 1e-12:
                lo, hi = (max(lo, b / a), hi) if a < 0 else (lo, min(hi, b / a))
        for sc in scales:
            c = foot + tangent * (lo + (hi - lo) * rng.uniform(0.2, 0.8))
            p = c + W[k] * (sc * sstar / unitw[k])
            sig.append(rotate(p[0], p[1], rng.uniform(0, np.pi)))
    # the vertices: the interior of the normal cone
    for i, j in itertools.combinations(range(len(rows)), 2):
        det = N[i, 0] * N[j, 1] - N[i, 1] * N[j, 0]
        if abs(det) < 1e-12:
            continue
        vtx = np.linalg.solve(N[[i, j]], d[[i, j]])
        if any(N[k] @ vtx > d[k] + 1e-9 for k in range(len(rows)) if k not in (i, j)):
            continue
        for sc in scales:
            wgt = rng.uniform(0.25, 0.75)
            p = vtx + (W[i] / unitw[i] * wgt + W[j] / unitw[j] * (1 - wgt)) * (sc * sstar)
            sig.append(rotate(p[0], p[1], rng.uniform(0, np.pi)))
    # equal principal values (no shear, s0 = s1), pure shear, elastic points
    for m in (0.9, 1.7, -1.3, -4.0, 25.0):
        sig.append(np.array([m * sstar, m * sstar, 0.0]))
    for tau in (0.2, 0.8, 3.0, -40.0):
        sig.append(np.array([0.0, 0.0, np.sqrt(2.0) * tau * sstar]))
    for _ in range(8):
        v = rng.normal(size=3)
        p1, p2 = rotate_back(v)
        over = max((N[k, 0] * p1 + N[k, 1] * p2) / d[k] for k in range(len(rows)))
        sig.append(v * rng.uniform(0.1, 0.9) / over)
    return np.array(sig)


def rotate_back(v):
    m, dl, t = 0.5 * (v[0] + v[1]), 0.5 * (v[0] - v[1]), v[2] / np.sqrt(2.0)
    r = np.hypot(dl, t)
    return m + r, m - r


def second_increment(E, nu, sstar, eps1, epsp1, keep_loading, rng):
    """unload a third of the batch towards its plastic strain (elastic), reload the rest in a new direction; the far points keep going"""
    n = len(eps1)
    eps2 = np.empty_like(eps1)
    for i in range(n):
        el = eps1[i] - epsp1[i]
        kind = i % 3
        if keep_loading[i]:
            eps2[i] = eps1[i] + 0.5 * el
        elif kind == 0:
            eps2[i] = eps1[i] - rng.uniform(0.3, 0.7) * el
        else:
            v = rng.normal(size=3)
            eps2[i] = eps1[i] + to_strain(E, nu, v / np.linalg.norm(v) * sstar * rng.uniform(0.5, 3.0))
    return eps2


def run_case(tag, law, prm, sig_tr, keep_loading, rng, out, cases):
    E, nu = prm[0], prm[1]
    if law == 23:
        sstar = prm[2]
        point = lambda e, ep: quadratic_point(E, nu, prm[2], prm[3], e, ep)          # noqa: E731
    else:
        rows = [tuple(prm[3 + 3 * k: 6 + 3 * k]) for k in range(int(prm[2]))]
        sstar = max(r[2] for r in rows)

        def point(e, ep):
            s, st, pl, _ = polygon_point(E, nu, rows, e, ep)
            return s, st, C_of(E, nu), pl

    eps1 = to_strain(E, nu, sig_tr)
    n = len(eps1)
    epn = [mp.matrix([0, 0, 0]) for _ in range(n)]
    eps = eps1
    for inc in (1, 2):
        res = [point(col(eps[i]), epn[i]) for i in range(n)]
        out[f"{tag}_eps{inc}"] = eps
        out[f"{tag}_stress{inc}"] = np.array([[float(r[0][k]) for k in range(3)] for r in res])
        out[f"{tag}_state{inc}"] = np.array([[float(r[1][k]) for k in range(3)] for r in res])
        out[f"{tag}_tangent{inc}"] = np.array([[float(r[2][a, b]) for a in range(3) for b in range(3)] for r in res])
        out[f"{tag}_plastic{inc}"] = np.array([bool(r[3]) for r in res])
        epn = [r[1] for r in res]
        if inc == 1:
            eps = second_increment(E, nu, sstar, eps1, out[f"{tag}_state1"], keep_loading, rng)
    out[f"{tag}_prm"] = np.array(prm, dtype=np.float64)
    Cm = C_of(E, nu)
    out[f"{tag}_elastic"] = np.array([float(Cm[a, b]) for a in range(3) for b in range(3)])
    cases.append(dict(tag=tag, law=law, points=n, yielded=[int(out[f"{tag}_plastic{k}"].sum()) for k in (1, 2)]))


def main():
    rng = np.random.default_rng(20)
    out, cases = {}, []
    E, sig0 = 70e3, 30.0
    for q in (1.0, 1.5):
        for nu in (0.0, 0.2, 0.49):
            sig, far = quadratic_inputs(E, nu, sig0, q, rng)
            run_case(f"quad_q{int(q * 10)}_nu{int(nu * 100)}", 23, [E, nu, sig0, q, 1.0], sig, far, rng, out, cases)
    fc, ft = 30.0, 10.0
    a, b = (1 / ft - 1 / fc) / 2, (1 / ft + 1 / fc) / 2
    rankine = [(1.0, 0.0, ft), (0.0, 1.0, ft), (-1.0, 0.0, fc), (0.0, -1.0, fc)]
    l1 = [(1.0, 1.0, ft), (-1.0, -1.0, fc), (a + b, a - b, 1.0), (a - b, a + b, 1.0)]
    for nu in (0.2, 0.0):
        for name, rows in (("rankine", rankine), ("l1rankine", l1)):
            prm = [E, nu, float(len(rows))] + [v for r in rows for v in r]
            sig = polygon_inputs(E, nu, rows, rng)
            run_case(f"{name}_nu{int(nu * 100)}", 24, prm, sig, np.zeros(len(sig), dtype=bool), rng, out, cases)
    out["meta"] = np.array(json.dumps(dict(digits=mp.mp.dps, margin=float(MARGIN), cases=cases)))
    np.savez_compressed(os.path.join(HERE, "plane_stress.npz"), **out)
    for c in cases:
        print(c)


if __name__ == "__main__":
    main()
