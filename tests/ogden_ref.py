"""Restatements of the Ogden hyperelastic law (DXM_LAW_OGDEN), the spec of ``demos/mfront/hyperelasticity/Ogden.mfront`` in the
reference: stored energy ``W(F) = (mu/alpha) (J^(-alpha/3) sum c_i^a - 3) + K/2 (J - 1)^2`` with ``a = alpha/2``, ``c_i`` the
eigenvalues of ``C = F^T F``, ``J = det F``.  Three formulations, none sharing code with another:

(a) :func:`closed_form` -- vectorised numpy, the principal-axis closed form the kernel evaluates (``csrc/hyperelastic.hip``), with
    LAPACK's eigen-solver;
(b) :func:`energy_ad` -- the energy in torch, ``P = grad W``, ``A = jacfwd(grad W)`` through ``torch.linalg.eigvalsh``, evaluated
    point by point (NaN at exactly repeated eigenvalues: AD of ``eigvalsh`` divides by the gap);
(c) :func:`closed_form_mp` -- the closed form in mpmath at 60 digits with the plain divided difference (no cancellation worth the
    name at that precision) and the analytic limit at gap 0; it produced ``tests/golden/ogden_degenerate.npz``
    (:func:`write_golden`).

Vectors follow ``utils.py:168-190``: F and PK1 as ``[11, 22, 33, 12, 21, 13, 31, 23, 32]``; the tangent is ``A[row, col] =
dPK1[row] / dF[col]``; the internal state variable ``PK2Stress`` is the isochoric part of S as ``[11, 22, 33, s 12, s 13, s 23]``,
``s = sqrt(2)``."""
import os

import numpy as np

TI = np.array([0, 1, 2, 0, 1, 0, 2, 1, 2])
TJ = np.array([0, 1, 2, 1, 0, 2, 0, 2, 1])
DEFAULTS = dict(alpha=28.8, mu=27778.0, K=69444444.0)          # the .mfront file's parameters
MILD = (dict(alpha=2.0, mu=27778.0, K=277780.0), dict(alpha=4.5, mu=27778.0, K=277780.0))
GAPS = (0.0, 1e-14, 1e-10, 1e-8, 1e-6, 1e-4, 1e-2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ogden_degenerate.npz")
SQ2 = np.sqrt(2.0)


def to_matrix(F9):
    F9 = np.atleast_2d(np.asarray(F9, dtype=np.float64))
    F = np.empty((F9.shape[0], 3, 3))
    F[:, TI, TJ] = F9
    return F


def to_vector(F):
    return np.ascontiguousarray(np.asarray(F)[:, TI, TJ])


def _sinhc(y):
    y2 = y * y
    return 1.0 + y2 / 6.0 * (1.0 + y2 / 20.0 * (1.0 + y2 / 42.0 * (1.0 + y2 / 72.0 * (1.0 + y2 / 110.0))))


def _divided_difference(m, ci, cj, li, lj, pwi, pwj, ui, uj):
    """(c_i^m - c_j^m) / (c_i - c_j): m (c_i c_j)^((m-1)/2) sinhc(m h) / sinhc(h), h = (ln c_i - ln c_j) / 2, where max(|m h|, |h|) <= 0.1,
    the quotient beyond."""
    h = 0.5 * (li - lj)
    y = m * h
    series = m * np.sqrt(pwi * pwj) * _sinhc(y) / _sinhc(h)
    with np.errstate(divide="ignore", invalid="ignore"):
        quotient = (ui - uj) / (ci - cj)
    return np.where(np.maximum(np.abs(y), np.abs(h)) <= 0.1, series, quotient)


def closed_form(F9, alpha, mu, K):
    """(a): PK1 (N, 9), dP/dF (N, 9, 9), PK2Stress (N, 6) of every row of ``F9`` (N, 9); NaN rows where det F <= 0."""
    F = to_matrix(F9)
    N = F.shape[0]
    a = alpha / 2.0
    m = a - 1.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        J = np.linalg.det(F)
        # the determinant as the sum the kernel forms (LAPACK's LU rounds differently by an ulp; either is fine)
        J = (F[:, 0, 0] * (F[:, 1, 1] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 1]) - F[:, 0, 1] * (F[:, 1, 0] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 0])
             + F[:, 0, 2] * (F[:, 1, 0] * F[:, 2, 1] - F[:, 1, 1] * F[:, 2, 0]))
        J = np.where(J > 0.0, J, np.nan)
        C = np.einsum("nki,nkj->nij", F, F)
        ok = np.isfinite(C).all(axis=(1, 2))
        c = np.full((N, 3), np.nan)
        V = np.full((N, 3, 3), np.nan)
        if ok.any():
            c[ok], V[ok] = np.linalg.eigh(C[ok])
        l = np.log(c)
        ic = 1.0 / c
        pw = np.exp((a - 2.0) * l)
        u = c * pw
        f = (c * u).sum(axis=1)
        A0 = mu * np.exp(-(a / 3.0) * l.sum(axis=1)) + 0.0 * J
        p = K * (J - 1.0) * J
        q = p - A0 * f / 3.0
        S = A0[:, None] * u + q[:, None] * ic
        Si = A0[:, None] * (u - f[:, None] * ic / 3.0)
        Q2 = 0.5 * K * (2.0 * J - 1.0) * J + a * A0 * f / 9.0
        D = 2.0 * (Q2[:, None, None] * ic[:, :, None] * ic[:, None, :]
                   - (a * A0 / 3.0)[:, None, None] * (u[:, :, None] * ic[:, None, :] + u[:, None, :] * ic[:, :, None]))
        idx = np.arange(3)
        D[:, idx, idx] += 2.0 * (A0[:, None] * m * pw - q[:, None] * ic * ic)
        CC = np.einsum("nij,nMi,nJi,nPj,nLj->nMJPL", D, V, V, V, V)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            th = A0 * _divided_difference(m, c[:, i], c[:, j], l[:, i], l[:, j], pw[:, i], pw[:, j], u[:, i], u[:, j]) - q * ic[:, i] * ic[:, j]
            G = np.einsum("nM,nJ->nMJ", V[:, :, i], V[:, :, j])
            G = G + G.transpose(0, 2, 1)
            CC += th[:, None, None, None, None] * np.einsum("nMJ,nPL->nMJPL", G, G)
        S2 = np.einsum("ni,nMi,nJi->nMJ", S, V, V)
        Si2 = np.einsum("ni,nMi,nJi->nMJ", Si, V, V)
        P = np.einsum("niM,nMJ->niJ", F, S2)
        A4 = np.einsum("niM,nMJPL,nkP->niJkL", F, CC, F) + np.einsum("ik,nLJ->niJkL", np.eye(3), S2)
    A = A4[:, TI, TJ][:, :, TI, TJ]
    isv = np.stack([Si2[:, 0, 0], Si2[:, 1, 1], Si2[:, 2, 2], SQ2 * Si2[:, 0, 1], SQ2 * Si2[:, 0, 2], SQ2 * Si2[:, 1, 2]], axis=1)
    return to_vector(P), np.ascontiguousarray(A), isv


def energy_torch(F, alpha, mu, K):
    """W of one 3x3 torch matrix F."""
    import torch

    c = torch.linalg.eigvalsh(F.T @ F)
    J = torch.linalg.det(F)
    return (mu / alpha) * (J ** (-alpha / 3.0) * (c ** (alpha / 2.0)).sum() - 3.0) + 0.5 * K * (J - 1.0) ** 2


def energy_ad(F9, alpha, mu, K):
    """(b): PK1 (N, 9) and dP/dF (N, 9, 9) by differentiating the energy twice, one point at a time."""
    import torch
    from torch.func import grad, jacfwd

    W = lambda X: energy_torch(X, alpha, mu, K)   # noqa: E731
    dW = grad(W)
    d2W = jacfwd(dW)
    F = torch.from_numpy(to_matrix(F9))
    P = np.stack([dW(X).numpy() for X in F])
    A4 = np.stack([d2W(X).numpy() for X in F])
    return to_vector(P), np.ascontiguousarray(A4[:, TI, TJ][:, :, TI, TJ])


def closed_form_mp(F9, alpha, mu, K, dps=60):
    """(c): as (a) for ONE point, in mpmath at ``dps`` digits from the double-precision entries of F."""
    import mpmath as mp

    with mp.workdps(dps):
        F = mp.matrix(3, 3)
        for t in range(9):
            F[int(TI[t]), int(TJ[t])] = mp.mpf(float(F9[t]))
        a = mp.mpf(alpha) / 2
        m = a - 1
        mu, K = mp.mpf(mu), mp.mpf(K)
        J = mp.det(F)
        C = F.T * F
        cs, V = mp.eigsy(C)
        c = [cs[i] for i in range(3)]
        g = (c[0] * c[1] * c[2]) ** (-a / 3)
        f = sum(x ** a for x in c)
        A0 = mu * g
        q = K * (J - 1) * J - A0 * f / 3
        S = [A0 * x ** m + q / x for x in c]
        Si = [A0 * (x ** m - f / (3 * x)) for x in c]
        Q2 = K * (2 * J - 1) * J / 2 + a * A0 * f / 9
        D = [[2 * (Q2 / (c[i] * c[j]) - a * A0 / 3 * (c[i] ** m / c[j] + c[j] ** m / c[i])) for j in range(3)] for i in range(3)]
        for i in range(3):
            D[i][i] += 2 * (A0 * m * c[i] ** (m - 1) - q / c[i] ** 2)

        def dd(i, j):
            if c[i] == c[j]:
                return m * c[i] ** (m - 1)
            return (c[i] ** m - c[j] ** m) / (c[i] - c[j])

        th = {(i, j): A0 * dd(i, j) - q / (c[i] * c[j]) for i, j in ((0, 1), (0, 2), (1, 2))}
        n = [[V[k, i] for k in range(3)] for i in range(3)]
        R3 = range(3)
        CC = {}
        for M in R3:
            for Jx in R3:
                for P_ in R3:
                    for L in R3:
                        v = sum(D[i][j] * n[i][M] * n[i][Jx] * n[j][P_] * n[j][L] for i in R3 for j in R3)
                        for (i, j), t in th.items():
                            v += t * (n[i][M] * n[j][Jx] + n[j][M] * n[i][Jx]) * (n[i][P_] * n[j][L] + n[j][P_] * n[i][L])
                        CC[M, Jx, P_, L] = v
        S2 = [[sum(S[i] * n[i][M] * n[i][Jx] for i in R3) for Jx in R3] for M in R3]
        Si2 = [[sum(Si[i] * n[i][M] * n[i][Jx] for i in R3) for Jx in R3] for M in R3]
        P = [[sum(F[i, M] * S2[M][Jx] for M in R3) for Jx in R3] for i in R3]
        P9 = np.array([float(P[int(TI[t])][int(TJ[t])]) for t in range(9)])
        A = np.empty((9, 9))
        for r in range(9):
            i, Jx = int(TI[r]), int(TJ[r])
            for col in range(9):
                k, L = int(TI[col]), int(TJ[col])
                v = sum(F[i, M] * CC[M, Jx, P_, L] * F[k, P_] for M in R3 for P_ in R3)
                if i == k:
                    v += S2[L][Jx]
                A[r, col] = float(v)
        s2 = mp.sqrt(2)
        isv = np.array([float(Si2[0][0]), float(Si2[1][1]), float(Si2[2][2]), float(s2 * Si2[0][1]), float(s2 * Si2[0][2]), float(s2 * Si2[1][2])])
    return P9, A, isv


# ---- input families ---------------------------------------------------------------------------------------------------------
def random_F(n, seed=0, amp=0.2):
    """F = I + amp U(-1/2, 1/2), the family of the issue."""
    rng = np.random.default_rng(seed)
    F = np.eye(3)[None] + amp * (rng.random((n, 3, 3)) - 0.5)
    return to_vector(F)


def _rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def degenerate_F():
    """F = Q diag(sqrt(c)) R^T with eigenvalues of C that are two-fold (c1, c2, c2 (1 + gap)) and three-fold (c, c (1 + gap),
    c (1 + 2 gap)) degenerate up to the relative gaps GAPS; once with generic rotations Q, R and once axis-aligned (Q = R = I,
    where gap 0 is exact in floating point).  Returns (F9 (28, 9), labels)."""
    Q, R = _rotation([1.0, 2.0, -1.5], 0.7), _rotation([-0.3, 1.0, 0.8], 1.9)
    rows, labels = [], []
    for fold, base in (("two", (1.21, 0.9025, 0.9025)), ("three", (1.1025, 1.1025, 1.1025))):
        for gap in GAPS:
            c = np.array(base)
            if fold == "two":
                c[2] *= 1.0 + gap
            else:
                c[1] *= 1.0 + gap
                c[2] *= 1.0 + 2.0 * gap
            for rot in (True, False):
                F = (Q if rot else np.eye(3)) @ np.diag(np.sqrt(c)) @ (R.T if rot else np.eye(3))
                rows.append(F)
                labels.append(f"{fold}-fold gap {gap:g} {'rotated' if rot else 'axis-aligned'}")
    return to_vector(np.array(rows)), labels


PARAM_SETS = (DEFAULTS,) + MILD


def write_golden(path=GOLDEN):
    """Evaluate (c) on the degenerate family for every parameter set and store inputs and results."""
    F9, labels = degenerate_F()
    out = {"F": F9, "labels": np.array(labels)}
    for k, prm in enumerate(PARAM_SETS):
        res = [closed_form_mp(row, **prm) for row in F9]
        out[f"params{k}"] = np.array([prm["alpha"], prm["mu"], prm["K"]])
        out[f"P{k}"] = np.array([r[0] for r in res])
        out[f"A{k}"] = np.array([r[1] for r in res])
        out[f"isv{k}"] = np.array([r[2] for r in res])
    np.savez(path, **out)


def load_golden(path=GOLDEN):
    z = np.load(path)
    sets = []
    for k in range(len(PARAM_SETS)):
        al, mu, K = z[f"params{k}"]
        sets.append((dict(alpha=float(al), mu=float(mu), K=float(K)), z[f"P{k}"], z[f"A{k}"], z[f"isv{k}"]))
    return z["F"], [str(s) for s in z["labels"]], sets


def row_errors(got, want):
    """Largest error of every row relative to the row's largest reference magnitude: (N, ...) -> (N,) per trailing row axis
    flattened, i.e. for a (N, 9, 9) tangent one figure per (point, row)."""
    got, want = np.asarray(got), np.asarray(want)
    scale = np.abs(want).max(axis=-1)
    scale = np.where(scale > 0.0, scale, 1.0)
    return np.abs(got - want).max(axis=-1) / scale


def uniaxial_reference(lam, alpha, mu, K):
    """Uniaxial stretch F = diag(lam, lt, lt) with zero lateral stress: lt by bisection / Newton on the energy's own lateral
    derivative (central differences of W at high precision in mpmath), P11 = dW_reduced/dlam.  Returns (lt, P11)."""
    import mpmath as mp

    with mp.workdps(40):
        al, mu_, K_ = mp.mpf(alpha), mp.mpf(mu), mp.mpf(K)

        def W(l1, lt):
            J = l1 * lt * lt
            return mu_ / al * (J ** (-al / 3) * (l1 ** al + 2 * lt ** al) - 3) + K_ / 2 * (J - 1) ** 2

        l1 = mp.mpf(float(lam))
        lt = mp.findroot(lambda t: mp.diff(lambda s: W(l1, s), t), mp.mpf(1) / mp.sqrt(l1))
        lt = mp.mpf(float(lt))   # the lateral stretch the caller can actually impose
        P11 = mp.diff(lambda s: W(s, lt), l1)
        return float(lt), float(P11)


if __name__ == "__main__":
    write_golden()
    print("wrote", GOLDEN)
