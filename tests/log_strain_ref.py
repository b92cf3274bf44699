"""Vectorised numpy restatement of logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_J2), the behaviour of the reference's
``demos/mfront/finite_strain_elastoplasticity/LogarithmicStrainPlasticity.mfront``: the Miehe-Apel-Lambrecht construction around
the small-strain radial return with linear hardening of ``oracle/constitutive_np.py`` (Hooke, Mises, ``R(p) = s0 + H0 p``, theta = 1).

With ``C = F^T F = sum c_i n_i n_i^T``, ``e_i = ln(c_i) / 2`` and hats for components in the eigenbasis of C:

1. Hencky strain ``E = sum e_i n_i n_i^T``; ``det F <= 0`` or a non-finite F gives NaN.
2. J2 update on ``eel_tr = E - Ep_n``: ``T``, ``Ep``, ``p``, ``eel = E - Ep`` and ``Ct = c1 1x1 + c2 I_sym + c3 n x n``.
3. ``theta_ij = ln[c_i, c_j] = 1 / (sqrt(c_i c_j) sinhc(e_i - e_j))``, ``theta_ii = 1 / c_i``; ``S^_ij = theta_ij T^_ij``, ``PK1 = F S``.
4. ``gamma_akb = ln[c_a, c_k, c_b]`` (:func:`gamma`), the only cancelling quantity.
5. ``CC^_ijkl = theta_ij Ct^_ijkl theta_kl + G^_ijkl`` with ``G^`` the minor-symmetrised tensor of
   ``G(H, K) = 2 sum_akb T^_ab gamma_akb (H_ak K_kb + K_ak H_kb)``, which is
   ``G^_ijkl = d_jk M_ijl + d_ik M_jil + d_jl M_ijk + d_il M_jik``, ``M_abc = T^_ac gamma_abc``.
6. ``A[(i,J),(k,L)] = d_ik S_LJ + F_iM CC_MJPL F_kP``.

Vectors: F and PK1 in the order of ``utils.py:168-190``; the state in Mandel notation, as the Hosford law holds the same names.
TEST INFRASTRUCTURE ONLY; no GPU."""
import os

import numpy as np

from oracle import constitutive_np as onp

TI = np.array([0, 1, 2, 0, 1, 0, 2, 1, 2])
TJ = np.array([0, 1, 2, 1, 0, 2, 0, 2, 1])
PRM = dict(E=210e9, nu=0.3, s0=250e6, H0=1e6)     # the .mfront file's elasticity, the demo's material properties
KINK = 1e-9                 # tile_loop_cases.KINK
KINK_CAP = 1e-3             # tile_loop_cases.J2_KINK_CAP
SHARE = (0.2, 0.8)
AMP = 2e-3                  # random_F: the yield strain is 1.2e-3; about half of a batch yields, in either increment
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "log_strain_degenerate.npz")
GAMMA_SWITCH = 0.05         # max |d| up to which gamma takes its Taylor form
GAMMA_TERMS = 15            # n = 0 .. 14
SQ2 = np.sqrt(2.0)


def to_matrix(F9):
    F9 = np.atleast_2d(np.asarray(F9, dtype=np.float64))
    F = np.empty((F9.shape[0], 3, 3))
    F[:, TI, TJ] = F9
    return F


def to_vector(F):
    return np.ascontiguousarray(np.asarray(F)[:, TI, TJ])


def sinhc(y):
    """sinh(y) / y: the even series of ``principal_axes.hpp`` up to |y| = 0.1, the quotient beyond."""
    y = np.asarray(y, dtype=np.float64)
    y2 = y * y
    series = 1.0 + y2 / 6.0 * (1.0 + y2 / 20.0 * (1.0 + y2 / 42.0 * (1.0 + y2 / 72.0 * (1.0 + y2 / 110.0))))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        quotient = np.sinh(y) / y
    return np.where(np.abs(y) <= 0.1, series, quotient)


def theta(ci, cj):
    """First divided difference of ln: no cancellation for any pair, 1 / c at c_i = c_j."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 / (np.sqrt(ci * cj) * sinhc(0.5 * (np.log(ci) - np.log(cj))))


def gamma(ca, ck, cb):
    """Second divided difference ln[c_a, c_k, c_b] of three positive numbers (arrays of one shape), symmetric in them.  With m their
    mean and d = (c - m) / m: the Taylor form m^-2 sum_n (-1)^(n+1) / (n + 2) h_n(d) (h_n the complete homogeneous symmetric
    polynomial) where max |d| <= GAMMA_SWITCH, else (ln[hi, mid] - ln[mid, lo]) / (hi - lo) of the sorted values."""
    ca, ck, cb = (np.asarray(x, dtype=np.float64) for x in np.broadcast_arrays(ca, ck, cb))
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (ca + ck + cb) / 3.0
        d0, d1, d2 = (ca - m) / m, (ck - m) / m, (cb - m) / m
        e1, e2, e3 = d0 + d1 + d2, d0 * d1 + d0 * d2 + d1 * d2, d0 * d1 * d2
        hm3, hm2, hm1 = np.zeros_like(m), np.zeros_like(m), np.ones_like(m)     # h_-2, h_-1, h_0
        acc = -0.5 * hm1
        for n in range(1, GAMMA_TERMS):
            h = e1 * hm1 - e2 * hm2 + e3 * hm3
            acc = acc + (-1.0) ** (n + 1) / (n + 2) * h
            hm3, hm2, hm1 = hm2, hm1, h
        series = acc / (m * m)
        s = np.sort(np.stack([ca, ck, cb]), axis=0)
        lo, mid, hi = s[0], s[1], s[2]
        quotient = (theta(hi, mid) - theta(mid, lo)) / (hi - lo)
        small = np.maximum(np.abs(d0), np.maximum(np.abs(d1), np.abs(d2))) <= GAMMA_SWITCH
    return np.where(small, series, quotient)


def hencky(F9):
    """(E Mandel (N, 6), c (N, 3), V (N, 3, 3) eigenvector columns) of every row; NaN where det F <= 0 or F is not finite."""
    F = to_matrix(F9)
    N = F.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        J = (F[:, 0, 0] * (F[:, 1, 1] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 1]) - F[:, 0, 1] * (F[:, 1, 0] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 0])
             + F[:, 0, 2] * (F[:, 1, 0] * F[:, 2, 1] - F[:, 1, 1] * F[:, 2, 0]))
        C = np.einsum("nki,nkj->nij", F, F)
        ok = np.isfinite(C).all(axis=(1, 2)) & (J > 0.0)
        c = np.full((N, 3), np.nan)
        V = np.full((N, 3, 3), np.nan)
        if ok.any():
            c[ok], V[ok] = np.linalg.eigh(C[ok])
        E = np.einsum("ni,nMi,nJi->nMJ", 0.5 * np.log(c), V, V)
    return onp.tensor_to_mandel(E), c, V


def update(F9, Ep_n, p_n, E=PRM["E"], nu=PRM["nu"], s0=PRM["s0"], H0=PRM["H0"]):
    """dict(P (N, 9), A (N, 9, 9), eel (N, 6), p (N,), Ep (N, 6), plastic, f_trial, skip) of every row of ``F9`` from the old
    state (Ep_n (N, 6) Mandel, p_n (N,)); NaN rows where det F <= 0.  ``skip``: |f_trial| <= KINK s0 (either branch is right)."""
    F = to_matrix(F9)
    N = F.shape[0]
    Eh, c, V = hencky(F9)
    bad = ~np.isfinite(Eh).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = onp.j2_update(np.where(bad[:, None], 0.0, Eh), Ep_n, p_n, E, nu, onp.LinearHardening(s0, H0))
        T = onp.mandel_to_tensor(r["sig"])
        nfl = onp.mandel_to_tensor(r["n"])
        Th = np.einsum("nMi,nMJ,nJj->nij", V, T, V)
        nh = np.einsum("nMi,nMJ,nJj->nij", V, nfl, V)
        th = theta(c[:, :, None], c[:, None, :])
        S = np.einsum("nMi,nij,nJj->nMJ", V, th * Th, V)
        P = np.einsum("niM,nMJ->niJ", F, S)
        g = gamma(c[:, :, None, None], c[:, None, :, None], c[:, None, None, :])
        I3 = np.eye(3)
        c1, c2, c3 = r["coef"].T
        Ct = (c1[:, None, None, None, None] * np.einsum("ij,kl->ijkl", I3, I3)[None]
              + 0.5 * c2[:, None, None, None, None] * (np.einsum("ik,jl->ijkl", I3, I3) + np.einsum("il,jk->ijkl", I3, I3))[None]
              + c3[:, None, None, None, None] * np.einsum("nij,nkl->nijkl", nh, nh))
        M = np.einsum("nac,nabc->nabc", Th, g)
        G = (np.einsum("jk,nijl->nijkl", I3, M) + np.einsum("ik,njil->nijkl", I3, M) + np.einsum("jl,nijk->nijkl", I3, M)
             + np.einsum("il,njik->nijkl", I3, M))
        CCh = th[:, :, :, None, None] * Ct * th[:, None, None, :, :] + G
        CC = CCh
        for _ in range(4):     # one index at a time, the rotated one going to the back: four passes restore the order
            CC = np.einsum("nMi,nijkl->njklM", V, CC)
        A4 = np.einsum("nkP,niJPL->niJkL", F, np.einsum("niM,nMJPL->niJPL", F, CC)) + np.einsum("ik,nLJ->niJkL", I3, S)
    A = np.ascontiguousarray(A4[:, TI, TJ][:, :, TI, TJ])
    eel = Eh - r["epsp"]
    nanrow = np.where(bad, np.nan, 0.0)
    return dict(P=to_vector(P), A=A, eel=eel, p=r["p"] + nanrow, Ep=r["epsp"] + nanrow[:, None], plastic=r["plastic"] & ~bad,
                f_trial=r["f_trial"], skip=(np.abs(r["f_trial"]) <= KINK * s0) & ~bad, T=r["sig"] + nanrow[:, None])


# ---- input families ---------------------------------------------------------------------------------------------------------
def random_F(n, seed=0, amp=AMP):
    """F = I + amp U(-1/2, 1/2)."""
    rng = np.random.default_rng(seed)
    return to_vector(np.eye(3)[None] + amp * (rng.random((n, 3, 3)) - 0.5))


def _rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


PAIR_GAPS = (1e-7, 1e-3, 0.04, 0.06)     # relative distance of two eigenvalues of C: both sides of GAMMA_SWITCH


def degenerate_F():
    """(F9 (10, 9), labels): F = I, 1.1 I, diag(1.2, .95, .95) and a rotated copy, two eigenvalues of C apart by the relative
    PAIR_GAPS (rotated), all three within 1e-6 (rotated), one generic."""
    Q, R = _rotation([1.0, 2.0, -1.5], 0.7), _rotation([-0.3, 1.0, 0.8], 1.9)
    rows = [np.eye(3), 1.1 * np.eye(3), np.diag([1.2, 0.95, 0.95]), Q @ np.diag([1.2, 0.95, 0.95]) @ R.T]
    labels = ["identity", "1.1 identity", "uniaxial axis-aligned", "uniaxial rotated"]
    for gap in PAIR_GAPS:
        c = np.array([1.0404, 0.9801, 0.9801 * (1.0 + gap)])
        rows.append(Q @ np.diag(np.sqrt(c)) @ R.T)
        labels.append(f"pair gap {gap:g}")
    c = 1.0201 * np.array([1.0, 1.0 + 0.5e-6, 1.0 - 0.4e-6])
    rows.append(Q @ np.diag(np.sqrt(c)) @ R.T)
    labels.append("triple within 1e-6")
    rows.append(np.array([[1.07, 0.03, -0.02], [0.05, 0.96, 0.04], [0.01, -0.06, 1.02]]))
    labels.append("generic")
    return to_vector(np.array(rows)), labels


def natural_state(n):
    return np.zeros((n, 6)), np.zeros(n)


def history_state(n, seed=0):
    """A history that is coaxial with nothing: a random deviatoric plastic strain of Mandel norm 2e-3, p = 3e-3."""
    rng = np.random.default_rng(1000 + seed)
    ep = rng.standard_normal((n, 6))
    ep[:, :3] -= ep[:, :3].mean(axis=1, keepdims=True)
    ep *= 2e-3 / np.linalg.norm(ep, axis=1, keepdims=True)
    return ep, np.full(n, 3e-3)


def spliced(N, seed, amp=AMP):
    """N rows of the random family with F = I and the degenerate set spliced in at the front."""
    F = random_F(N, seed=seed, amp=amp)
    special = np.vstack([np.array([[1.0, 1, 1, 0, 0, 0, 0, 0, 0]]), degenerate_F()[0]])
    k = min(N, len(special))
    F[:k] = special[:k]
    return F


def two_increments(N, seed):
    """(F1, F2): two unrelated draws, so that the second update starts from the plastic strain the first one left, which is
    coaxial with nothing in the second."""
    return spliced(N, seed), spliced(N, seed + 7919)[::-1].copy()


def branch(F9, Ep_n, p_n, E=PRM["E"], nu=PRM["nu"], s0=PRM["s0"], H0=PRM["H0"]):
    """The update without stress and tangent: dict(plastic, skip, f_trial, Ep, p).  For whole batches of the tile-loop size."""
    Eh = hencky(F9)[0]
    bad = ~np.isfinite(Eh).all(axis=1)
    r = onp.j2_update(np.where(bad[:, None], 0.0, Eh), Ep_n, p_n, E, nu, onp.LinearHardening(s0, H0))
    return dict(plastic=r["plastic"] & ~bad, skip=(np.abs(r["f_trial"]) <= KINK * s0) & ~bad, f_trial=r["f_trial"], Ep=r["epsp"], p=r["p"])


def reference_path(increments, idx=None):
    """[update(...)] of the increments in turn from the natural state, at the points ``idx`` (all by default)."""
    n = len(increments[0]) if idx is None else len(idx)
    Ep, p = natural_state(n)
    out = []
    for F in increments:
        r = update(F if idx is None else F[idx], Ep, p)
        out.append(r)
        Ep, p = r["Ep"], r["p"]
    return out


# ---- errors -----------------------------------------------------------------------------------------------------------------
def scaled_errors(got, want, s0=PRM["s0"], E=PRM["E"], keep=None):
    """Largest scaled error of PK1, tangent, ElasticStrain, p and the hidden plastic strain: dict of five figures.  PK1 by
    max(|PK1| of the point, s0), the tangent by the row-wise maximum of the reference, the strains and p by max(own size, s0 / E)
    (at strains of 1e-6 the rounding of C near 1 alone costs 1e-16 / strain, in any reference)."""
    keep = np.ones(len(want["P"]), dtype=bool) if keep is None else np.asarray(keep)
    out = {}
    sP = np.maximum(np.abs(want["P"]).max(axis=1), s0)
    out["P"] = (np.abs(got["P"] - want["P"]).max(axis=1) / sP)[keep].max()
    sA = np.abs(want["A"]).max(axis=2)
    out["A"] = (np.abs(np.asarray(got["A"]).reshape(want["A"].shape) - want["A"]).max(axis=2) / sA)[keep].max()
    for k in ("eel", "Ep"):
        sk = np.maximum(np.abs(want[k]).max(axis=1), s0 / E)
        out[k] = (np.abs(got[k] - want[k]).max(axis=1) / sk)[keep].max()
    sp = np.maximum(np.abs(want["p"]), s0 / E)
    out["p"] = (np.abs(np.asarray(got["p"]).reshape(-1) - want["p"]) / sp)[keep].max()
    return {k: float(v) for k, v in out.items()}


def load_golden(path=GOLDEN):
    """(F (n, 9), labels, [(state name, Ep_n, p_n, dict(P, A, eel, p, Ep, plastic))])"""
    z = np.load(path)
    sets = []
    for name in ("natural", "history"):
        sets.append((name, z[f"{name}_Ep_n"], z[f"{name}_p_n"],
                     {k: z[f"{name}_{k}"] for k in ("P", "A", "eel", "p", "Ep", "plastic")}))
    return z["F"], [str(s) for s in z["labels"]], sets
