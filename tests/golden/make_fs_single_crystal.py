"""Generator of ``fs_single_crystal_kat.npz``: the finite-strain FCC single-crystal viscoplastic law (law id 21) at 50 digits, in the
form the MFront file integrates it -- 18 unknowns, the Green-Lagrange strain ``Eel`` of the elastic part (6) and the twelve slip
increments, with 3x3 tensors, ``mu_i = m_i x n_i`` from its own slip geometry and a fourth-order stiffness.  No Mandel vector, no
reduced system, no analytic derivative of the law: the local Newton takes its Jacobian by differences at step 1e-30, and the tangent
is the CENTRAL DIFFERENCE of the converged 50-digit first Piola-Kirchhoff stress at step 1e-20 in each component of ``F``.  The
float64 restatement (``tests/fs_single_crystal_ref.py``) only supplies the starting point of each solve, which does not decide
where the iteration converges to, and is then measured against the result (``meta["restatement_deviation"]``).

Cases: two parameter sets (law 14's file constants with self-hardening only; all six interaction coefficients non-zero with
``d = 0``) x three frame classes (none, a symmetry rotation, generic) x ``dt`` in {1e-3, 0.1, 10}: 18 histories of ten increments
(virgin elastic, first yield, flow, flow, four steps of reversal through unloading into reverse flow, two steps of a
non-proportional turn with shear and rotation in ``F``), every increment ``|dF|_F <= 5e-4``.  Every step restarts from the
float64-rounded state, so that the stored outputs belong to the stored inputs exactly.

    python tests/golden/make_fs_single_crystal.py          # some minutes
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fs_single_crystal_ref as fx  # noqa: E402

mp.mp.dps = 50
TI = (0, 1, 2, 0, 1, 0, 2, 1, 2)
TJ = (0, 1, 2, 1, 0, 2, 0, 2, 1)
ZERO, ONE = mp.mpf(0), mp.mpf(1)
PARAM_SETS = (
    (dict(fx.MFRONT), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    ({**fx.MFRONT, "d": 0.0, "n": 6.0, "K": 40.0}, (1.0, 1.0, 0.6, 12.3, 1.6, 1.8)),
)
DTS = (1e-3, 0.1, 10.0)
MAXIT = 60


def eye():
    return [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]


def mm(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def tr(a):
    return [[a[j][i] for j in range(3)] for i in range(3)]


def det(a):
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
            + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))


def inv(a):
    m = mp.matrix(a) ** -1
    return [[m[i, j] for j in range(3)] for i in range(3)]


def from_vec(v):
    m = [[ZERO] * 3 for _ in range(3)]
    for t in range(9):
        m[TI[t]][TJ[t]] = mp.mpf(float(v[t]))
    return m


def to_vec(m):
    return [m[TI[t]][TJ[t]] for t in range(9)]


def slip_geometry():
    """twelve (direction, normal) pairs of integer vectors, plane-major: the library's numbering, restated"""
    out = []
    for p in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        for d in ((0, 1, -1), (1, 0, -1), (1, -1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
            if sum(x * y for x, y in zip(p, d)) == 0:
                out.append((d, p))
    assert len(out) == 12
    return out


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def interaction_matrix(h):
    """h_ij from the six coefficients [self, coplanar, Hirth, collinear, glissile, Lomer], classes decided from the geometry"""
    sys_ = slip_geometry()
    H = [[None] * 12 for _ in range(12)]
    for i, (si, ni) in enumerate(sys_):
        for j, (sj, nj) in enumerate(sys_):
            c = cross(ni, nj)
            if i == j:
                k = 0
            elif ni == nj:
                k = 1
            elif not any(cross(si, sj)):
                k = 3
            elif sum(x * y for x, y in zip(si, sj)) == 0:
                k = 2
            elif not any(cross(si, c)) or not any(cross(sj, c)):
                k = 4
            else:
                k = 5
            H[i][j] = mp.mpf(h[k])
    return H


def stiffness4(E, nu, G):
    """D_ijkl of the cubic material: the normal block is the inverse of the compliance block"""
    S = mp.matrix([[1 / E, -nu / E, -nu / E], [-nu / E, 1 / E, -nu / E], [-nu / E, -nu / E, 1 / E]]) ** -1
    D = [[[[ZERO] * 3 for _ in range(3)] for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for j in range(3):
            D[i][i][j][j] = S[i, j]
            if i != j:
                D[i][j][i][j] = D[i][j][j][i] = G
    return D


class Law:
    def __init__(self, props, h):
        g = {k: mp.mpf(v) for k, v in props.items()}
        self.g = g
        self.D = stiffness4(g["E"], g["nu"], g["G"])
        s6 = mp.sqrt(6)
        self.mu = [[[mp.mpf(d[a] * p[b]) / s6 for b in range(3)] for a in range(3)] for d, p in slip_geometry()]
        self.H = interaction_matrix(h)

    def elastic_part(self, Fetr, dg):
        A = eye()
        for i in range(12):
            for a in range(3):
                for b in range(3):
                    A[a][b] -= dg[i] * self.mu[i][a][b]
        s = mp.cbrt(det(A))
        dFpi = [[A[a][b] / s for b in range(3)] for a in range(3)]
        return mm(Fetr, dFpi), dFpi

    def second_pk(self, Eel):
        return [[sum(self.D[i][j][k][l] * Eel[k][l] for k in range(3) for l in range(3)) for j in range(3)] for i in range(3)]

    def residual(self, x, Fetr, p0, a0, dt):
        """MFront's 18 equations: feel (6, the upper triangle) and fg (12)"""
        g = self.g
        Eel = [[x[0], x[3], x[4]], [x[3], x[1], x[5]], [x[4], x[5], x[2]]]
        dg = x[6:]
        Fe, _ = self.elastic_part(Fetr, dg)
        C = mm(tr(Fe), Fe)
        out = [Eel[i][j] - (C[i][j] - (ONE if i == j else ZERO)) / 2 for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
        S = self.second_pk(Eel)
        I2E = [[(ONE if i == j else ZERO) + 2 * Eel[i][j] for j in range(3)] for i in range(3)]
        M = mm(I2E, S)
        ebp = [mp.exp(-g["b"] * (p0[j] + abs(dg[j]))) for j in range(12)]
        for i in range(12):
            tau = sum(M[a][b] * self.mu[i][a][b] for a in range(3) for b in range(3))
            r = g["tau0"] + sum(g["Q"] * self.H[i][j] * (1 - ebp[j]) for j in range(12))
            da = (dg[i] - g["d"] * a0[i] * abs(dg[i])) / (1 + g["d"] * abs(dg[i]))
            xb = g["C"] * (a0[i] + da)
            f = max(abs(tau - xb) - r, ZERO)
            sgn = 1 if tau - xb > 0 else -1
            out.append(dg[i] - dt * (f / g["K"]) ** g["n"] * sgn)
        return out

    def solve(self, Fm, Fpn, p0, a0, dt, guess, Jinv=None):
        """the root of the 18 equations from `guess`; a given inverse Jacobian is kept (chord iteration)"""
        Fpi = inv(Fpn)
        Fetr = mm(Fm, Fpi)
        x = list(guess)
        h = mp.mpf(10) ** -30
        Ji = Jinv
        for _ in range(40):
            r = self.residual(x, Fetr, p0, a0, dt)
            if Ji is not None and max(abs(v) for v in r) < mp.mpf(10) ** -45:
                break
            if Jinv is None:
                J = mp.matrix(18, 18)
                for c in range(18):
                    xp = list(x)
                    xp[c] += h
                    rp = self.residual(xp, Fetr, p0, a0, dt)
                    for k in range(18):
                        J[k, c] = (rp[k] - r[k]) / h
                Ji = J ** -1
            dx = Ji * mp.matrix(r)
            x = [x[k] - dx[k] for k in range(18)]
        else:
            raise RuntimeError("the 50-digit Newton did not converge")
        dg = x[6:]
        Fe, dFpi = self.elastic_part(Fetr, dg)
        Eel = [[x[0], x[3], x[4]], [x[3], x[1], x[5]], [x[4], x[5], x[2]]]
        S = self.second_pk(Eel)
        # Cauchy = Fe S Fe^T / det Fe, then PK1 with F
        FeS = mm(mm(Fe, S), tr(Fe))
        je = det(Fe)
        J = det(Fm)
        Finv_t = tr(inv(Fm))
        P = mm([[FeS[a][b] / je * J for b in range(3)] for a in range(3)], Finv_t)
        return x, P, dFpi, Ji


def rotate_in(R, F):
    return mm(mm(R, F), tr(R))


def rotate_out(R, P):
    return mm(mm(tr(R), P), R)


def history_increments(rng):
    """ten increments dF (3x3 float), each of Frobenius norm <= 5e-4"""
    ax = np.diag([1.0, -0.3, -0.3]) + 0.15 * rng.normal(size=(3, 3))
    ax /= np.linalg.norm(ax)
    sh = np.array([[0.0, 1.0, 0.3], [-0.6, 0.0, 0.2], [0.1, -0.4, 0.0]]) + 0.2 * np.diag(rng.normal(size=3))
    sh /= np.linalg.norm(sh)
    steps = [4.0e-4 * ax, 4.5e-4 * ax, 5e-4 * ax, 5e-4 * ax] + [-5e-4 * ax] * 4 + [5e-4 * sh] * 2
    return steps


def main():
    rng = np.random.default_rng(2121)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    frames = (None, np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), q)
    rec = {k: [] for k in ("F", "R", "has_frame", "dt", "pset", "g0", "p0", "a0", "Fp0", "stress", "tangent", "g", "p", "a", "Fp", "yielded",
                           "stage")}
    dev = {"stress": 0.0, "state": 0.0, "tangent": 0.0}
    iters_max = 0
    for ps, (props, hcoef) in enumerate(PARAM_SETS):
        law = Law(props, hcoef)
        prm = fx.param_vector(props, hcoef)
        for fr, R in enumerate(frames):
            for dt in DTS:
                incs = history_increments(rng)
                F = np.eye(3)
                st = fx.zero_state(1)
                for stage, dF in enumerate(incs):
                    assert np.linalg.norm(dF) <= 5e-4 * (1 + 1e-12)
                    F = F + dF
                    Fv = fx.to_vec(F[None])
                    ref = fx.update(Fv, st, prm, dt, R=R, maxit=MAXIT)
                    assert ref["status"][0] == 0, (ps, fr, dt, stage)
                    iters_max = max(iters_max, int(ref["iters"][0]))
                    # 50 digits, from the float64-rounded inputs
                    Rm = eye() if R is None else [[mp.mpf(float(R[i, j])) for j in range(3)] for i in range(3)]
                    Fm = rotate_in(Rm, from_vec(Fv[0]))
                    Fpn = from_vec(st["Fp"][0])
                    p0 = [mp.mpf(float(v)) for v in st["p"][0]]
                    a0 = [mp.mpf(float(v)) for v in st["a"][0]]
                    mdt = mp.mpf(dt)
                    # starting point: the float64 answer
                    kin = fx.derived(Fv, {"Fp": ref["Fp"]}, prm, R=R)["ElasticStrain"][0]
                    guess = [mp.mpf(float(v)) for v in kin] + [mp.mpf(float(v)) for v in ref["dg"][0]]
                    x, P, dFpi, Ji = law.solve(Fm, Fpn, p0, a0, mdt, guess)
                    dg = x[6:]
                    Pg = to_vec(rotate_out(Rm, P))
                    # tangent: central differences of the converged stress, chord iterations from the base solution
                    h = mp.mpf(10) ** -20
                    T = np.empty((9, 9))
                    for u in range(9):
                        col = []
                        for sgn in (1, -1):
                            Fg = from_vec(Fv[0])
                            Fg[TI[u]][TJ[u]] += sgn * h
                            _, Pp, _, _ = law.solve(rotate_in(Rm, Fg), Fpn, p0, a0, mdt, x, Jinv=Ji)
                            col.append(to_vec(rotate_out(Rm, Pp)))
                        T[:, u] = [float((a - b) / (2 * h)) for a, b in zip(*col)]
                    Fp_new = mm(inv(dFpi), Fpn)
                    g_new = [mp.mpf(float(v)) + d for v, d in zip(st["g"][0], dg)]
                    p_new = [p + abs(d) for p, d in zip(p0, dg)]
                    a_new = [a + (d - law.g["d"] * a * abs(d)) / (1 + law.g["d"] * abs(d)) for a, d in zip(a0, dg)]
                    gold = {"stress": np.array([float(v) for v in Pg]), "tangent": T, "g": np.array([float(v) for v in g_new]),
                            "p": np.array([float(v) for v in p_new]), "a": np.array([float(v) for v in a_new]),
                            "Fp": np.array([float(v) for v in to_vec(Fp_new)])}
                    yielded = max(abs(d) for d in dg) > mp.mpf(10) ** -30
                    assert yielded == bool(ref["plastic"][0]), (ps, fr, dt, stage)
                    for k in ("F", "R", "has_frame", "dt", "pset", "stage", "yielded"):
                        rec[k].append({"F": Fv[0], "R": np.eye(3) if R is None else R, "has_frame": fr, "dt": dt, "pset": ps, "stage": stage,
                                       "yielded": yielded}[k])
                    for k in ("g", "p", "a", "Fp"):
                        rec[k + "0"].append(st[k][0].copy())
                        rec[k].append(gold[k])
                    rec["stress"].append(gold["stress"])
                    rec["tangent"].append(T)
                    # the deviation of the restatement, per field, relative to the field scale of the point
                    dev["stress"] = max(dev["stress"], np.abs(ref["stress"][0] - gold["stress"]).max() / np.abs(gold["stress"]).max())
                    dev["tangent"] = max(dev["tangent"], np.abs(ref["tangent"][0] - T).max() / np.abs(T).max())
                    sscale = max(np.abs(gold[k]).max() for k in ("g", "p", "a", "Fp"))
                    dev["state"] = max(dev["state"], max(np.abs(ref[k][0] - gold[k]).max() for k in ("g", "p", "a", "Fp")) / sscale)
                    print(f"set {ps} frame {fr} dt {dt:g} stage {stage}: yielded {yielded} iters {int(ref['iters'][0])} "
                          f"|P| {np.abs(gold['stress']).max():.2f} dev {dev}", flush=True)
                    # the next step starts from the float64-rounded 50-digit state
                    st = {k: gold[k][None].copy() for k in ("g", "p", "a", "Fp")}
    out = {k: np.array(v) for k, v in rec.items()}
    frac = out["yielded"].mean()
    assert frac >= 0.5, frac
    meta = {"digits": 50, "maxit": MAXIT, "restatement_deviation": dev, "restatement_max_iters": iters_max, "yielded_fraction": float(frac),
            "param_names": list(fx.NAMES) + ["h_self", "h_coplanar", "h_Hirth", "h_collinear", "h_glissile", "h_Lomer"]}
    out["params"] = np.array([fx.param_vector(p, h) for p, h in PARAM_SETS])
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "fs_single_crystal_kat.npz"), **out)
    print(meta)


if __name__ == "__main__":
    main()
