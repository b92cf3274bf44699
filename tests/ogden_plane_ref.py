"""A numpy restatement of what ``csrc/ogden_plane.hip`` evaluates (DXM_LAW_OGDEN_PE): Ogden hyperelasticity on the 5-wide plane
deformation gradient ``[F00, F11, F22, F01, F10]`` (``utils.py:168-172``), written WITHOUT ``ogden_ref.closed_form``: the 2x2 block of
``C = F^T F`` is diagonalised in closed form by one rotation (no LAPACK), ``c2 = F22^2`` has the eigenvector ``e_z``, one divided
difference (``th01``) with the kernel's series switch, the tangent ``2 dS/dC`` in the four components ``[00, 11, 22, 01]`` only, and the
outputs are 5 / 25 / 4 wide from the start.  The law's definition -- law 7 on the embedded F, restricted -- is
``restricted_closed_form`` below, the formulation the kernel does NOT use; the GPU tests compare against that one.

Also the input families of the plane law's tests."""
import numpy as np

import ogden_ref as og

SQ2 = np.sqrt(2.0)
IDX = (0, 1, 2, 3, 4)                    # positions of [00, 11, 22, 01, 10] in the 9-vector
DROPPED = (5, 6, 7, 8)
RI = (0, 1, 2, 0, 1)                     # row / column index of entry t of the 5-vector
RJ = (0, 1, 2, 1, 0)


def embed(F5):
    F5 = np.atleast_2d(np.asarray(F5, dtype=np.float64))
    out = np.zeros((F5.shape[0], 9))
    out[:, :5] = F5
    return out


def restricted_closed_form(F5, alpha, mu, K):
    """The definition: ``ogden_ref.closed_form`` (LAPACK's 3x3 eigen-solver, three divided differences, the 9x9 block) on the embedded
    F; components 0..4 of PK1, rows and columns 0..4 of dP/dF, [xx, yy, zz, sqrt(2) xy] of PK2Stress."""
    P, A, isv = og.closed_form(embed(F5), alpha, mu, K)
    return np.ascontiguousarray(P[:, :5]), np.ascontiguousarray(A[:, :5, :5]), np.ascontiguousarray(isv[:, :4])


def _sinhc(y2):
    return 1.0 + y2 / 6.0 * (1.0 + y2 / 20.0 * (1.0 + y2 / 42.0 * (1.0 + y2 / 72.0 * (1.0 + y2 / 110.0))))


def _sym4(a, b):
    return a if a == b else 3


def plane_closed_form(F5, alpha, mu, K):
    """PK1 (N, 5), dP/dF (N, 5, 5), PK2Stress (N, 4) of every row of ``F5`` (N, 5); NaN rows where J <= 0."""
    F5 = np.atleast_2d(np.asarray(F5, dtype=np.float64))
    F00, F11, F22, F01, F10 = (F5[:, k] for k in range(5))
    a = alpha / 2.0
    m = a - 1.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        J = F22 * (F00 * F11 - F01 * F10)
        J = np.where(J > 0.0, J, np.nan)
        app = F00 * F00 + F10 * F10
        aqq = F11 * F11 + F01 * F01
        apq = F00 * F01 + F10 * F11
        # one rotation: t the smaller root of t^2 + t (aqq - app) / apq - 1 = 0
        d = aqq - app
        den = d + np.copysign(np.sqrt(d * d + 4.0 * apq * apq), d)
        t = np.where(den != 0.0, 2.0 * apq / np.where(den != 0.0, den, 1.0), 0.0)
        cs = 1.0 / np.sqrt(t * t + 1.0)
        sn = t * cs
        c = np.stack([app - t * apq, aqq + t * apq, F22 * F22], axis=1)
        n0 = np.stack([cs, -sn], axis=1)           # eigenvector of c[:, 0], in the plane
        n1 = np.stack([sn, cs], axis=1)
        l = np.log(c)
        ic = 1.0 / c
        pw = np.exp((a - 2.0) * l)
        u = c * pw
        f = (c * u).sum(axis=1)
        A0 = mu * np.exp(-(a / 3.0) * l.sum(axis=1)) + 0.0 * J
        p = K * (J - 1.0) * J
        f3 = f / 3.0
        q = p - A0 * f3
        S = A0[:, None] * u + q[:, None] * ic
        Si = A0[:, None] * (u - f3[:, None] * ic)
        Q2 = 0.5 * K * (2.0 * J - 1.0) * J + a * A0 * f / 9.0
        D = 2.0 * (Q2[:, None, None] * ic[:, :, None] * ic[:, None, :]
                   - (a * A0 / 3.0)[:, None, None] * (u[:, :, None] * ic[:, None, :] + u[:, None, :] * ic[:, :, None]))
        idx = np.arange(3)
        D[:, idx, idx] += 2.0 * (A0[:, None] * m * pw - q[:, None] * ic * ic)
        h = 0.5 * (l[:, 0] - l[:, 1])
        y = m * h
        series = m * np.sqrt(pw[:, 0] * pw[:, 1]) * _sinhc(y * y) / _sinhc(h * h)
        quotient = (u[:, 0] - u[:, 1]) / (c[:, 0] - c[:, 1])
        dd = np.where(np.maximum(np.abs(y), np.abs(h)) <= 0.1, series, quotient)
        th01 = A0 * dd - q * ic[:, 0] * ic[:, 1]
        zero, one = np.zeros_like(J), np.ones_like(J)
        # the components [00, 11, 22, 01] of E_i = n_i n_i and G01 = n0 n1 + n1 n0
        E = np.stack([np.stack([n0[:, 0] ** 2, n0[:, 1] ** 2, zero, n0[:, 0] * n0[:, 1]], axis=1),
                      np.stack([n1[:, 0] ** 2, n1[:, 1] ** 2, zero, n1[:, 0] * n1[:, 1]], axis=1),
                      np.stack([zero, zero, one, zero], axis=1)], axis=1)                          # (N, 3, 4)
        G = np.stack([2.0 * n0[:, 0] * n1[:, 0], 2.0 * n0[:, 1] * n1[:, 1], zero, n0[:, 0] * n1[:, 1] + n1[:, 0] * n0[:, 1]], axis=1)
        S4 = np.einsum("ni,niI->nI", S, E)
        Si4 = np.einsum("ni,niI->nI", Si, E)
        CC = np.einsum("nij,niI,njK->nIK", D, E, E) + th01[:, None, None] * G[:, :, None] * G[:, None, :]
        Fm = np.zeros((len(J), 3, 3))
        Fm[:, 0, 0], Fm[:, 1, 1], Fm[:, 2, 2], Fm[:, 0, 1], Fm[:, 1, 0] = F00, F11, F22, F01, F10
        P = np.empty((len(J), 5))
        A = np.empty((len(J), 5, 5))
        for r in range(5):
            i, Jx = RI[r], RJ[r]
            Ms = (2,) if i == 2 else (0, 1)
            P[:, r] = sum(Fm[:, i, M] * S4[:, _sym4(M, Jx)] for M in Ms)
            for col in range(5):
                k, L = RI[col], RJ[col]
                Ps = (2,) if k == 2 else (0, 1)
                v = sum(Fm[:, i, M] * CC[:, _sym4(M, Jx), _sym4(P_, L)] * Fm[:, k, P_] for M in Ms for P_ in Ps)
                if i == k:
                    v = v + S4[:, _sym4(L, Jx)]
                A[:, r, col] = v
    isv = np.stack([Si4[:, 0], Si4[:, 1], Si4[:, 2], SQ2 * Si4[:, 3]], axis=1)
    return P, A, isv


# ---- input families ---------------------------------------------------------------------------------------------------------
def random_F5(n, seed=0, amp=0.2):
    """F5 = [1, 1, 1, 0, 0] + amp U(-1/2, 1/2) on all five components."""
    rng = np.random.default_rng(seed)
    return np.array([1.0, 1.0, 1.0, 0.0, 0.0])[None] + amp * (rng.random((n, 5)) - 0.5)


def _from_matrix(F):
    F = np.asarray(F, dtype=np.float64)
    return np.stack([F[..., 0, 0], F[..., 1, 1], F[..., 2, 2], F[..., 0, 1], F[..., 1, 0]], axis=-1)


def _rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def special_F5():
    """The special points of the issue, (F5 (M, 5), labels): identity, volumetric, in-plane repeated eigenvalues (axis-aligned and
    rotated in the plane), an in-plane eigenvalue equal to c2, the gaps ``ogden_ref.GAPS`` between the in-plane eigenvalues and
    between one of them and c2 (each rotated by an arbitrary in-plane angle on either side), simple in-plane shear, F22 != 1."""
    rows, labels = [], []

    def add(F, label):
        rows.append(_from_matrix(F))
        labels.append(label)

    Q, R = _rot_z(0.7), _rot_z(-1.9)
    add(np.eye(3), "identity")
    add(1.05 * np.eye(3), "volumetric 1.05")
    add(0.93 * np.eye(3), "volumetric 0.93")
    add(np.diag([1.1, 1.1, 0.95]), "diag(a, a, b)")
    add(Q @ np.diag([1.1, 1.1, 0.95]) @ R.T, "diag(a, a, b) rotated in the plane")
    add(np.diag([1.1, 0.95, 1.1]), "diag(a, b, a)")
    add(Q @ np.diag([1.1, 0.95, 1.1]) @ R.T, "diag(a, b, a) rotated in the plane")
    for gap in og.GAPS:
        c = np.array([1.21, 1.21 * (1.0 + gap), 0.9025])
        add(Q @ np.diag(np.sqrt(c)) @ R.T, f"in-plane gap {gap:g} rotated")
        add(np.diag(np.sqrt(c)), f"in-plane gap {gap:g} axis-aligned")
        c = np.array([1.21, 0.9025, 1.21 * (1.0 + gap)])
        add(Q @ np.diag(np.sqrt(c)) @ R.T, f"gap {gap:g} to c2 rotated")
    # the stress of a shear g is O(mu g), a difference of parts that are O(mu): the error of a row relative to the row's own size has
    # the floor eps / g whatever evaluates it (mpmath included, from the double-precision F), so the shears start at 0.01
    for g in (0.01, 0.1, 0.3, 1.0):
        F = np.eye(3)
        F[0, 1] = g
        add(F, f"simple shear {g:g}")
    add(np.diag([1.0, 1.0, 1.3]), "F22 = 1.3 alone")
    F = np.array([[1.05, 0.08, 0.0], [-0.03, 0.97, 0.0], [0.0, 0.0, 0.8]])
    add(F, "general with F22 = 0.8")
    return np.array(rows), labels


def family(n, seed=0):
    """``n`` rows: the special points first (as many as fit), random rows behind them."""
    sp, _ = special_F5()
    sp = sp[:n]
    return np.concatenate([sp, random_F5(n - len(sp), seed=seed)], axis=0)


def errors(got, want):
    """(P, A, isv) against (P, A, isv): the largest per-row relative error of each (``ogden_ref.row_errors``; a row of the internal
    state variable is measured against the stress of its point, as in ``test_ogden_cpu.errors``)."""
    eP = og.row_errors(got[0][:, None, :], want[0][:, None, :]).max()
    eA = og.row_errors(got[1], want[1]).max()
    scale = np.maximum(np.abs(want[2]).max(axis=1), np.abs(want[0]).max(axis=1))
    scale = np.where(scale > 0.0, scale, 1.0)
    eS = (np.abs(got[2] - want[2]).max(axis=1) / scale).max()
    return float(eP), float(eA), float(eS)


def plane_uniaxial_reference(lam, alpha, mu, K):
    """Uniaxial plane-strain stretch F = diag(lam, l2, 1) with P11 = 0: l2 from the energy's own derivative in mpmath (as
    ``ogden_ref.uniaxial_reference``), P00 = dW/dlam at that l2.  Returns (l2, P00)."""
    import mpmath as mp

    with mp.workdps(40):
        al, mu_, K_ = mp.mpf(alpha), mp.mpf(mu), mp.mpf(K)

        def W(l1, l2):
            J = l1 * l2
            return mu_ / al * (J ** (-al / 3) * (l1 ** al + l2 ** al + 1) - 3) + K_ / 2 * (J - 1) ** 2

        l1 = mp.mpf(float(lam))
        l2 = mp.findroot(lambda t: mp.diff(lambda s: W(l1, s), t), mp.mpf(1) / l1)
        l2 = mp.mpf(float(l2))   # the lateral stretch the caller can actually impose
        P00 = mp.diff(lambda s: W(s, l2), l1)
        return float(l2), float(P00)
