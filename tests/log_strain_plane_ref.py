"""The reference and the inputs of plane-strain logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_PE = 42, ``csrc/log_strain_plane.hip``).

The law's definition is :func:`restricted`: ``log_strain_ref.update`` (law 19's numpy restatement: LAPACK's 3x3 eigen-solver, every
divided difference, the 9x9 block) on the embedded ``F`` and the embedded old plastic strain, restricted to the components a plane
state has -- the formulation the kernel does NOT use (one rotation, ``th01``, ``g001`` and ``g110`` alone, a 4x4 change of basis).
What the restriction drops is exactly zero for such a state; :func:`restricted` reports the largest dropped entry as ``dropped`` and
the test files assert that it is 0.0.

Vectors: F and PK1 as ``[00, 11, 22, 01, 10]`` (``utils.py:168-172``), the symmetric tensors as ``[xx, yy, zz, sqrt(2) xy]``.

Inputs, all of them plane: :func:`stretch_case` (F = R_z diag(lam) Q_z^T under the ten draws of ``log_strain_cases.draw``, old states
by ``log_strain_cases.state_at`` along deviators without xz and yz), :func:`special_F5` (the rows on which the kernel's branches meet),
:func:`mixed_batch` (the special rows at the tile boundaries of a batch), :func:`history` (``log_strain_cases.HISTORY_SCHEDULE`` with
every rotation about z) and :func:`fixture_points` (what ``golden/make_log_strain_plane.py`` evaluates at 100 digits).
TEST INFRASTRUCTURE ONLY; no GPU."""
import functools
import os

import numpy as np

from dolfinx_materials_amd import conventions as cv
from oracle import constitutive_np as onp

import log_strain_cases as lc
import log_strain_ref as ls

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "log_strain_plane.npz")
KEYS = ("P", "A", "eel", "p", "Ep")
N_BATCH = lc.N_BATCH              # 4099: 64 full tiles and a ragged tail of 3
N_HISTORY = 1000
FIXTURE_PER_AMP = 3
SWAP = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])     # the quarter turn about z: exact, renames the in-plane axes


def from_matrix(F):
    F = np.asarray(F, dtype=np.float64)
    return np.stack([F[..., 0, 0], F[..., 1, 1], F[..., 2, 2], F[..., 0, 1], F[..., 1, 0]], axis=-1)


def rot_z(angle):
    """(..., 3, 3) rotations about z."""
    angle = np.asarray(angle, dtype=np.float64)
    c, s, z, o = np.cos(angle), np.sin(angle), np.zeros_like(angle), np.ones_like(angle)
    return np.stack([np.stack([c, -s, z], axis=-1), np.stack([s, c, z], axis=-1), np.stack([z, z, o], axis=-1)], axis=-2)


def restricted(F5, Ep4, p, **prm):
    """The definition: dict(P (N, 5), A (N, 5, 5), eel (N, 4), p (N,), Ep (N, 4), T (N, 4), plastic, f_trial, skip, dropped)."""
    F5 = np.atleast_2d(np.asarray(F5, dtype=np.float64))
    r = ls.update(cv.embed_plane_F(F5), cv.embed_plane_strain(np.asarray(Ep4, dtype=np.float64).reshape(len(F5), 4)), np.asarray(p, dtype=np.float64), **prm)
    ok = np.isfinite(r["P"]).all(axis=1)
    dropped = 0.0
    if ok.any():
        dropped = max(np.abs(r["P"][ok][:, 5:]).max(), np.abs(r["A"][ok][:, :5, 5:]).max(), np.abs(r["A"][ok][:, 5:, :5]).max(),
                      np.abs(r["eel"][ok][:, 4:]).max(), np.abs(r["Ep"][ok][:, 4:]).max(), np.abs(r["T"][ok][:, 4:]).max())
    return dict(P=cv.restrict_plane_F(r["P"]), A=cv.restrict_plane_F_tangent(r["A"]), eel=cv.restrict_plane_strain(r["eel"]), p=r["p"],
                Ep=cv.restrict_plane_strain(r["Ep"]), T=cv.restrict_plane_strain(r["T"]), plastic=r["plastic"], f_trial=r["f_trial"],
                skip=r["skip"], dropped=float(dropped))


def natural_state(n):
    return np.zeros((n, 4)), np.zeros(n)


# ---- the stretch family ---------------------------------------------------------------------------------------------------------
def plane_unit_deviators(rng, n):
    """Random deviatoric directions without xz and yz, (n, 6) Mandel of unit norm."""
    d = rng.standard_normal((n, 6))
    d[:, 4:] = 0.0
    d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def state_at(F5, prm, u, p_n, d6):
    """``log_strain_cases.state_at`` of the embedded F, restricted; its out-of-plane shears must be exactly zero."""
    Ep6 = lc.state_at(cv.embed_plane_F(F5), prm, u, p_n, d6)
    assert not Ep6[:, 4:].any()
    return cv.restrict_plane_strain(Ep6)


def stretch_case(k, n, amp, seed):
    """(F5 (n, 5), Ep_n (n, 4), p_n (n,)) under draw ``k``: ``log_strain_cases.stretch_case`` with R and Q rotations about z
    (principal stretches log-uniform in [1 / amp, amp], the third one along z; ln det F = U(-3, 3) s0 / E; p_n = U(0, 0.5);
    seq_trial / R_n = U(0, 2) along a random plane deviator: half of the points yield)."""
    prm = lc.draw(k)
    rng = np.random.default_rng(300_000 * k + 1000 * int(round(10 * amp)) + seed)
    h = rng.uniform(-np.log(amp), np.log(amp), (n, 3))
    lnJ = rng.uniform(-3.0, 3.0, n) * prm["s0"] / prm["E"]
    h += ((lnJ - h.sum(axis=1)) / 3.0)[:, None]
    R, Q = rot_z(rng.uniform(0.0, 2.0 * np.pi, n)), rot_z(rng.uniform(0.0, 2.0 * np.pi, n))
    F5 = from_matrix(np.einsum("nia,na,nja->nij", R, np.exp(h), Q))
    p_n = rng.uniform(0.0, 0.5, n)
    u = rng.uniform(0.0, 2.0, n)
    return F5, state_at(F5, prm, u, p_n, plane_unit_deviators(rng, n)), p_n


def batch_of(k):
    """(amp, (F5, Ep_n, p_n)): draw k's batch of N_BATCH points, the amplitudes in turn."""
    amp = lc.AMPS[k % len(lc.AMPS)]
    return amp, stretch_case(k, N_BATCH, amp, 0)


def stratum_of(amp):
    return f"amp {amp:g}"


# ---- special rows -----------------------------------------------------------------------------------------------------------------
def gamma_gap(s):
    """The relative gap g of c1 = c0 (1 + g) at which ``ls_gamma(c0, c0, c1)`` has max |d| = s: d = (2 g / 3) / (1 + g / 3)."""
    return s / (2.0 / 3.0 - s / 3.0)


def special_F5():
    """(F5 (M, 5), labels), M >= 66.  Axis-aligned rows (the rotation is the ``den == 0`` no-op or c01 == 0 exactly): a diagonal F,
    the identity, 0.5 I and 3 I, c0 == c1 exactly, c0 and c1 at relative gaps of 1e-7 and on both sides of the switch of ``ls_gamma``
    (max |d| = 0.05 (1 -+ 1e-3), for either of the two calls) and of ``ls_theta`` (|e0 - e1| = 0.1 (1 -+ 1e-3)), c2 equal to c0 or to
    c1.  Two pure in-plane rotations, simple shears on F01 and on F10, F22 alone, a uniaxial row, a general row with F22 = 0.8.  The eigenvalue-structured rows again as
    Q_z F R_z^T, and all of these multiplied on the right by the quarter turn about z, which renames the in-plane axes."""
    Q, R = rot_z(0.7), rot_z(-1.9)
    rows, labels, structured = [], [], []

    def add(F, label, rotate=False):
        rows.append(np.asarray(F, dtype=np.float64))
        labels.append(label)
        if rotate:
            structured.append(len(rows) - 1)

    add(np.diag([1.3, 0.8, 1.1]), "diagonal")
    add(np.eye(3), "identity")
    add(Q, "rotation a")
    add(R @ Q, "rotation b")
    add(0.5 * np.eye(3), "0.5 identity")
    add(3.0 * np.eye(3), "3 identity")
    for kk in (0.01, 0.5, 2.0):
        S = np.eye(3)
        S[0, 1] = kk
        add(S, f"shear {kk:g}")
    S = np.eye(3)
    S[1, 0] = -0.3
    add(S, "shear -0.3 on F10")
    add(np.diag([1.0, 1.0, 1.3]), "F22 = 1.3 alone")
    add(np.diag([1.2, 0.95, 0.95]), "uniaxial")
    add(np.diag([1.1, 1.1, 1.1 * np.sqrt(2.0)]), "exact pair 01", True)
    add(np.diag(np.sqrt([1.44, 1.44 * (1.0 + 1e-7), 0.49])), "near pair 01", True)
    for sgn in (-1.0, 1.0):
        g = gamma_gap(ls.GAMMA_SWITCH * (1.0 + sgn * 1e-3))
        add(np.diag(np.sqrt([1.2, 1.2 * (1.0 + g), 0.7])), f"gamma switch up {sgn:+g}", True)
        add(np.diag(np.sqrt([1.2, 1.2 / (1.0 + g), 0.7])), f"gamma switch down {sgn:+g}", True)
    for sgn in (-1.0, 1.0):
        y = lc.THETA_SWITCH * (1.0 + sgn * 1e-3)
        add(np.diag([1.2 * np.exp(y), 1.2, 0.7]), f"theta switch {sgn:+g}", True)
    add(np.diag([1.1, 0.9, 1.1]), "c2 equals c0", True)
    add(np.diag([0.9, 1.1, 1.1]), "c2 equals c1", True)
    add(np.array([[1.05, 0.08, 0.0], [-0.03, 0.97, 0.0], [0.0, 0.0, 0.8]]), "general with F22 = 0.8")
    for k in structured:
        rows.append(Q @ rows[k] @ R.T)
        labels.append(labels[k] + " rotated")
    n = len(rows)
    for k in range(n):
        rows.append(rows[k] @ SWAP)
        labels.append(labels[k] + " swapped")
    return from_matrix(np.array(rows)), labels


def special_state(F5, prm, seed=0):
    """A history scaled to each row: p_n = 0.1 and the trial stress at 1.5 (even rows) or 0.5 (odd rows) of the yield stress along a
    random plane deviator, around the row's own Hencky strain (``log_strain_cases.special_state``)."""
    n = len(F5)
    rng = np.random.default_rng(7100 + seed)
    u = np.where(np.arange(n) % 2 == 0, 1.5, 0.5)
    p_n = np.full(n, 0.1)
    return state_at(F5, prm, u, p_n, plane_unit_deviators(rng, n)), p_n


def special_sets(prm=None):
    """(F5, labels, {"natural": (Ep_n, p_n), "history": (Ep_n, p_n)}) of the special rows under ``prm`` (PRM by default)."""
    prm = dict(ls.PRM) if prm is None else prm
    F5, labels = special_F5()
    return F5, labels, {"natural": natural_state(len(F5)), "history": special_state(F5, prm)}


def mixed_batch(seed=0):
    """(F5, Ep_n, p_n, special (bool)) of N_BATCH rows under PRM: all four amplitudes interleaved, the special rows from the natural
    state at the front (across the boundary of tiles 0 and 1: lanes 0, 63, 64) and from their histories at the very end (the last
    full tile and the ragged tail)."""
    parts = [stretch_case(0, N_BATCH, amp, seed + 50 + q) for q, amp in enumerate(lc.AMPS)]
    pick = np.arange(N_BATCH) % len(lc.AMPS)
    F, Ep, p = (np.choose(pick.reshape((-1,) + (1,) * (parts[0][c].ndim - 1)), [x[c] for x in parts]) for c in range(3))
    Fs, labels, sets = special_sets()
    m = len(Fs)
    special = np.zeros(N_BATCH, dtype=bool)
    F[:m], Ep[:m], p[:m] = Fs, sets["natural"][0], sets["natural"][1]
    F[-m:], Ep[-m:], p[-m:] = Fs, sets["history"][0], sets["history"][1]
    special[:m] = special[-m:] = True
    return np.ascontiguousarray(F), np.ascontiguousarray(Ep), np.ascontiguousarray(p), special


def classify(F5):
    """The branches the kernel takes at every row, from its own rotation restated in numpy: dict(c (n, 3) in the kernel's order,
    theta_far (n,), g001_far (n,), g110_far (n,), rotated (n,): the rotation is not the no-op)."""
    F5 = np.atleast_2d(np.asarray(F5, dtype=np.float64))
    F00, F11, F22, F01, F10 = (F5[:, k] for k in range(5))
    app, aqq, apq = F00 * F00 + F10 * F10, F11 * F11 + F01 * F01, F00 * F01 + F10 * F11
    d = aqq - app
    den = d + np.copysign(np.sqrt(d * d + 4.0 * apq * apq), d)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den != 0.0, 2.0 * apq / den, 0.0)
    c = np.stack([app - t * apq, aqq + t * apq, F22 * F22], axis=1)
    far = []
    for i, j in ((0, 1), (1, 0)):
        m = (2.0 * c[:, i] + c[:, j]) / 3.0
        far.append(np.maximum(np.abs(c[:, i] - m), np.abs(c[:, j] - m)) / m > ls.GAMMA_SWITCH)
    e = 0.5 * np.log(c)
    return dict(c=c, theta_far=np.abs(e[:, 0] - e[:, 1]) > lc.THETA_SWITCH, g001_far=far[0], g110_far=far[1], rotated=t != 0.0)


# ---- histories ------------------------------------------------------------------------------------------------------------------
def history(k, n=N_HISTORY, seed=0):
    """``log_strain_cases.history`` restated for the plane: six increments of n points from the natural state under draw ``k``:
    dict(F (six (n, 5)), ref (six :func:`restricted` results, each from the state the one before left), out (six (n,) bool: the point
    was within the kink band in this or an earlier increment)).  A driven point (probability HISTORY_DRIVEN) gets the Hencky strain
    Q_k diag(s_k ln(amp) a + v) Q_k^T with Q_k = Q_(k-1) rot_z(0.3 or -0.3): the in-plane principal axes turn every increment, so the
    plastic strain the earlier increments left is not coaxial with C; a resting point is put back inside the surface around the
    plastic strain it carries.  F_k = R_k exp(E_k), R_k accumulating rotations about z too."""
    return _history(k, n, seed)


@functools.lru_cache(maxsize=None)
def _history(k, n, seed):
    prm = lc.draw(k)
    mu = prm["E"] / 2.0 / (1.0 + prm["nu"])
    rng = np.random.default_rng(9500 + 100 * k + seed)
    a = rng.standard_normal((n, 3))
    a -= a.mean(axis=1, keepdims=True)
    a /= np.abs(a).max(axis=1, keepdims=True)
    lnamp = rng.uniform(np.log(1.2), np.log(2.0), n)
    Q, R = rot_z(rng.uniform(0.0, 2.0 * np.pi, n)), rot_z(rng.uniform(0.0, 2.0 * np.pi, n))
    turn = rot_z(np.where(rng.random(n) < 0.5, 0.3, -0.3))
    Ep, p = natural_state(n)
    out = dict(F=[], ref=[], out=[])
    gone = np.zeros(n, dtype=bool)
    for s in lc.HISTORY_SCHEDULE:
        Q, R = Q @ turn, turn @ R
        v = rng.uniform(-3.0, 3.0, n) * prm["s0"] / prm["E"] / 3.0
        e = s * lnamp[:, None] * a + v[:, None]
        Ed = np.einsum("nia,na,nja->nij", Q, e, Q)
        u = rng.uniform(0.0, 0.9, n)
        Rn = prm["s0"] + prm["H0"] * p
        Er = (onp.mandel_to_tensor(cv.embed_plane_strain(Ep) + (u * Rn / (np.sqrt(6.0) * mu))[:, None] * plane_unit_deviators(rng, n))
              + v[:, None, None] * np.eye(3))
        driven = rng.random(n) < lc.HISTORY_DRIVEN
        Em = np.where(driven[:, None, None], Ed, Er)
        Em[:, :2, 2] = Em[:, 2, :2] = 0.0           # exactly plane (the products above leave exact zeros there already)
        w, V = np.linalg.eigh(Em)
        Fm = R @ np.einsum("nia,na,nja->nij", V, np.exp(w), V)
        assert not Fm[:, :2, 2].any() and not Fm[:, 2, :2].any()
        F5 = from_matrix(Fm)
        r = restricted(F5, Ep, p, **prm)
        gone = gone | r["skip"]
        out["F"].append(F5)
        out["ref"].append(r)
        out["out"].append(gone.copy())
        Ep, p = r["Ep"], r["p"]
    return out


# ---- the fixture's points ---------------------------------------------------------------------------------------------------------
FIXTURE_SPECIAL = tuple(
    [(lab, "history") for lab in ("diagonal", "rotation a", "0.5 identity", "3 identity", "shear 0.01", "shear 0.5", "shear 2",
                                  "exact pair 01", "near pair 01", "gamma switch up -1", "gamma switch up +1", "gamma switch down -1",
                                  "gamma switch down +1", "theta switch -1", "theta switch +1", "c2 equals c0", "c2 equals c1",
                                  "exact pair 01 rotated", "near pair 01 rotated swapped", "gamma switch up +1 rotated",
                                  "theta switch -1 rotated swapped", "c2 equals c1 rotated", "general with F22 = 0.8")]
    + [(lab, "natural") for lab in ("3 identity", "shear 0.5", "shear 2")])


def fixture_points():
    """(F5 (n, 5), Ep_n (n, 4), p_n, params (n, 4), draw (n,), amp (n,), labels): FIXTURE_PER_AMP points of every (draw, amp), the
    first of ``stretch_case(k, 64, amp, seed=1)`` that yield and the first that do not in turn (two and one, or one and two), then the
    FIXTURE_SPECIAL rows under PRM (amp 0)."""
    F, Ep, p, prms, dr, am, labels = [], [], [], [], [], [], []
    for k in range(lc.N_DRAWS):
        prm = lc.draw(k)
        for q, amp in enumerate(lc.AMPS):
            Fa, Epa, pa = stretch_case(k, 64, amp, seed=1)
            pl = restricted(Fa, Epa, pa, **prm)["plastic"]
            want = [True, False, True] if (k + q) % 2 == 0 else [False, True, False]
            idx, used = [], set()
            for w in want:
                i = next(i for i in range(64) if bool(pl[i]) == w and i not in used)
                used.add(i)
                idx.append(i)
            for i in idx:
                F.append(Fa[i]); Ep.append(Epa[i]); p.append(pa[i]); dr.append(k); am.append(amp)
                prms.append([prm[x] for x in ("E", "nu", "s0", "H0")])
                labels.append(f"draw {k} amp {amp:g} row {i}")
    Fs, slabels, sets = special_sets()
    for lab, state in FIXTURE_SPECIAL:
        i = slabels.index(lab)
        F.append(Fs[i]); Ep.append(sets[state][0][i]); p.append(sets[state][1][i]); dr.append(0); am.append(0.0)
        prms.append([ls.PRM[x] for x in ("E", "nu", "s0", "H0")])
        labels.append(f"{lab}, {state} state")
    return (np.array(F), np.array(Ep), np.array(p), np.array(prms), np.array(dr), np.array(am), labels)


def load_fixture(path=GOLDEN):
    """dict of the arrays of ``log_strain_plane.npz``: F, Ep_n, p_n, params, draw, amp, labels, P, A, eel, p, Ep, plastic."""
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    out["labels"] = [str(s) for s in out["labels"]]
    out["plastic"] = out["plastic"].astype(bool)
    return out


def strata(fx):
    """{name: row mask} of the fixture: one stratum per amp, one for the special rows."""
    out = {stratum_of(amp): fx["amp"] == amp for amp in lc.AMPS}
    out["special"] = fx["amp"] == 0.0
    return out
