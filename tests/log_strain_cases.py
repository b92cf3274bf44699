"""Seeded parameters and inputs for the finite-stretch sweep of logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_J2): shared by
``test_log_strain_finite_cpu.py`` (which pins the restatement and the input rules over them), ``test_gpu_log_strain_finite.py`` (which
holds ``log_strain_kernel`` to them) and ``golden/make_log_strain_finite.py`` (the 100-digit values).  TEST INFRASTRUCTURE ONLY.

* :func:`draw`: ten parameter sets, ``PRM`` first: E = 10^U(3, 11.5), nu in [0, 0.49] with 0.49, 0 and -0.3 forced on draws 1, 2
  and 4, s0 / E = 10^U(-4, -1.5), H0 = 0 on every third draw and U(0, 0.5) E otherwise, H0 = 10 E on draw 5.
* :func:`stretch_case`: F = R diag(lam) Q^T with principal stretches log-uniform in [1 / amp, amp] and an old state that puts the
  trial stress at U(0, 2) times the current yield stress.
* :func:`special_F`: the rows on which the kernel's branches meet (see there).
* :func:`history`: six increments from the natural state, the reference chained with ``log_strain_ref.update``.
* :func:`jacobi_np` / :func:`classify`: the kernel's own eigen-solver restated, to say which branch the kernel takes at a point."""
import functools

import numpy as np

from oracle import constitutive_np as onp

import log_strain_ref as ls

N_DRAWS = 10
AMPS = (1.1, 1.3, 2.0, 3.0)
N_BATCH = 4099                  # 64 full tiles of 64 and a ragged tail of 3
N_HISTORY = 1000
HISTORY_DRAWS = (0, 3, 5)       # PRM, an H0 = 0 draw, the H0 = 10 E draw
HISTORY_SCHEDULE = (0.4, 0.7, 0.5, -0.8, -0.9, 1.0)     # of ln(amp): grows, unloads, reverses past yield, reloads up to amp
HISTORY_DRIVEN = 0.55           # share of the points that follow the schedule in an increment; the others rest inside the surface
SWEEPS = 5                      # LS_SWEEPS
THETA_SWITCH = 0.1              # |y| up to which ls_theta takes the series
FIXTURE_PER_AMP = 3
GOLDEN = ls.GOLDEN.replace("log_strain_degenerate", "log_strain_finite")
CYCLIC = (np.eye(3), np.eye(3)[:, [1, 2, 0]], np.eye(3)[:, [2, 0, 1]])      # the identity and the two cyclic permutations


def draw(k):
    """dict(E, nu, s0, H0) of draw ``k``."""
    if k == 0:
        return dict(ls.PRM)
    rng = np.random.default_rng(1900 + k)
    E = float(10 ** rng.uniform(3, 11.5))
    nu = {1: 0.49, 2: 0.0, 4: -0.3}.get(k, float(rng.uniform(0.0, 0.49)))
    s0 = E * float(10 ** rng.uniform(-4, -1.5))
    H0 = float(rng.uniform(0.0, 0.5)) * E
    if k % 3 == 0:
        H0 = 0.0
    if k == 5:
        H0 = 10.0 * E
    return dict(E=E, nu=nu, s0=s0, H0=H0)


def rotations(rng, n):
    """n proper rotations, Haar-distributed (QR of a Gaussian matrix, signs fixed)."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    return q * np.linalg.det(q)[:, None, None]


def unit_deviators(rng, n):
    """Random deviatoric directions (n, 6), Mandel, of unit norm."""
    d = rng.standard_normal((n, 6))
    d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _dev(E6):
    out = np.array(E6)
    out[:, :3] -= out[:, :3].mean(axis=1, keepdims=True)
    return out


def state_at(F9, prm, u, p_n, d):
    """The old plastic strain that puts the trial stress of ``F9`` at ``u`` times the yield stress R_n = s0 + H0 p_n, along the
    deviator ``d``: Ep_n = dev E(F) - u R_n / (sqrt(6) mu) d, so that s_trial = 2 mu (u R_n / (sqrt(6) mu)) d has seq = u R_n."""
    mu = prm["E"] / 2.0 / (1.0 + prm["nu"])
    Rn = prm["s0"] + prm["H0"] * np.asarray(p_n)
    return _dev(ls.hencky(F9)[0]) - (np.asarray(u) * Rn / (np.sqrt(6.0) * mu))[:, None] * d


def stretch_case(k, n, amp, seed):
    """(F (n, 9), Ep_n (n, 6), p_n (n,)) under draw ``k``: principal stretches log-uniform in [1 / amp, amp], rescaled so that
    ln det F = U(-3, 3) s0 / E (a free volume change would put a pressure of K ln J on top of a deviatoric stress of s0: the error
    scale of the stress would then say nothing about the plastic part), R and Q independent rotations, p_n = U(0, 0.5), and
    seq_trial / R_n = U(0, 2) along a random deviator (:func:`state_at`): half of the points yield."""
    prm = draw(k)
    rng = np.random.default_rng(100_000 * k + 1000 * int(round(10 * amp)) + seed)
    h = rng.uniform(-np.log(amp), np.log(amp), (n, 3))
    lnJ = rng.uniform(-3.0, 3.0, n) * prm["s0"] / prm["E"]
    h += ((lnJ - h.sum(axis=1)) / 3.0)[:, None]
    R, Q = rotations(rng, n), rotations(rng, n)
    F9 = ls.to_vector(np.einsum("nia,na,nja->nij", R, np.exp(h), Q))
    p_n = rng.uniform(0.0, 0.5, n)
    u = rng.uniform(0.0, 2.0, n)
    return F9, state_at(F9, prm, u, p_n, unit_deviators(rng, n)), p_n


# ---- special rows -------------------------------------------------------------------------------------------------------------
def special_F():
    """(F9 (84, 9), labels).  Axis-aligned rows (every Jacobi rotation is the ``den == 0`` no-op, so the eigenvalues keep the order
    written here): a diagonal F, 0.5 I and 3 I, an exact pair of eigenvalues of C in each of the three positions with the third 2x
    away, a pair at relative gap 1e-7 in each position, triples with max |d| at 0.05 (1 -+ 1e-3) (the switch of ``ls_gamma``), pairs
    with |e_i - e_j| at 0.1 (1 -+ 1e-3) (the switch of ``ls_theta``).  Two pure rotations and simple shears I + k e1 x e2.  The
    eigenvalue-structured rows again as Q F R^T.  And all of these multiplied on the right by the two cyclic permutation matrices:
    rotations, which change the order in which Jacobi delivers the eigenvalues."""
    Q, R = ls._rotation([1.0, 2.0, -1.5], 0.7), ls._rotation([-0.3, 1.0, 0.8], 1.9)
    rows, labels, structured = [], [], []

    def add(F, label, rotate=False):
        rows.append(np.asarray(F, dtype=np.float64))
        labels.append(label)
        if rotate:
            structured.append(len(rows) - 1)

    add(np.diag([1.3, 0.8, 1.1]), "diagonal")
    add(Q, "rotation a")
    add(R @ Q, "rotation b")
    add(0.5 * np.eye(3), "0.5 identity")
    add(3.0 * np.eye(3), "3 identity")
    for kk in (0.01, 0.5, 2.0):
        S = np.eye(3)
        S[0, 1] = kk
        add(S, f"shear {kk:g}")
    for i, j in ((0, 1), (0, 2), (1, 2)):
        lam = np.full(3, 1.1 * np.sqrt(2.0))
        lam[[i, j]] = 1.1
        add(np.diag(lam), f"exact pair {i}{j}", True)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        c = np.full(3, 0.49)
        c[i], c[j] = 1.44, 1.44 * (1.0 + 1e-7)
        add(np.diag(np.sqrt(c)), f"near pair {i}{j}", True)
    for sgn in (-1.0, 1.0):
        s = ls.GAMMA_SWITCH * (1.0 + sgn * 1e-3)
        add(np.diag(np.sqrt(1.2 * (1.0 + s * np.array([1.0, -1.0 / 3.0, -2.0 / 3.0])))), f"triple at switch {sgn:+g}", True)
    for sgn in (-1.0, 1.0):
        y = THETA_SWITCH * (1.0 + sgn * 1e-3)
        add(np.diag([1.2 * np.exp(y), 1.2, 0.7]), f"theta pair at switch {sgn:+g}", True)
    for k in structured:
        rows.append(Q @ rows[k] @ R.T)
        labels.append(labels[k] + " rotated")
    n = len(rows)
    for q, P in enumerate(CYCLIC[1:]):
        for k in range(n):
            rows.append(rows[k] @ P)
            labels.append(labels[k] + f" perm {q + 1}")
    return ls.to_vector(np.array(rows)), labels


def special_state(F9, prm, seed=0):
    """A history scaled to each row: p_n = 0.1 and the trial stress at 1.5 (even rows) or 0.5 (odd rows) of the yield stress along
    a random deviator, around the row's own Hencky strain."""
    n = len(F9)
    rng = np.random.default_rng(7000 + seed)
    u = np.where(np.arange(n) % 2 == 0, 1.5, 0.5)
    p_n = np.full(n, 0.1)
    return state_at(F9, prm, u, p_n, unit_deviators(rng, n)), p_n


# the 24 (row, state) pairs of the special rows that go into the 100-digit fixture
FIXTURE_SPECIAL = tuple(
    [(lab, "history") for lab in ("diagonal", "rotation a", "0.5 identity", "3 identity", "shear 0.01", "shear 0.5", "shear 2",
                                  "exact pair 01", "exact pair 02", "exact pair 12", "near pair 01", "near pair 02", "near pair 12",
                                  "triple at switch -1", "triple at switch +1", "theta pair at switch -1", "theta pair at switch +1",
                                  "exact pair 02 rotated perm 1", "near pair 12 rotated perm 2", "triple at switch +1 rotated perm 1",
                                  "theta pair at switch -1 rotated perm 2")]
    + [(lab, "natural") for lab in ("3 identity", "shear 0.5", "shear 2")])


def special_sets(prm=None):
    """(F9, labels, {"natural": (Ep_n, p_n), "history": (Ep_n, p_n)}) of the special rows under ``prm`` (PRM by default)."""
    prm = dict(ls.PRM) if prm is None else prm
    F9, labels = special_F()
    return F9, labels, {"natural": ls.natural_state(len(F9)), "history": special_state(F9, prm)}


def mixed_prm_batch(seed=0):
    """(F, Ep_n, p_n, special (bool)) of N_BATCH rows under PRM: all four ``amp`` values interleaved, the special rows from the
    natural state at the front (rows 0 .. 83: across the boundary of tiles 0 and 1) and from their histories at the very end (the
    last full tile and the ragged tail)."""
    parts = [stretch_case(0, N_BATCH, amp, seed + 50 + q) for q, amp in enumerate(AMPS)]
    pick = np.arange(N_BATCH) % len(AMPS)
    F, Ep, p = (np.choose(pick.reshape((-1,) + (1,) * (parts[0][c].ndim - 1)), [x[c] for x in parts]) for c in range(3))
    Fs, labels, sets = special_sets()
    m = len(Fs)
    special = np.zeros(N_BATCH, dtype=bool)
    F[:m], Ep[:m], p[:m] = Fs, sets["natural"][0], sets["natural"][1]
    F[-m:], Ep[-m:], p[-m:] = Fs, sets["history"][0], sets["history"][1]
    special[:m] = special[-m:] = True
    return np.ascontiguousarray(F), np.ascontiguousarray(Ep), np.ascontiguousarray(p), special


# ---- histories ----------------------------------------------------------------------------------------------------------------
def history(k, n=N_HISTORY, seed=0):
    """Six increments of n points from the natural state under draw ``k``: dict(F (six (n, 9)), ref (six ``ls.update`` results, each
    from the state the one before left), out (six (n,) bool: the point was within the kink band in this or an earlier increment)).

    In every increment a point is *driven* (probability HISTORY_DRIVEN) or *rests*.  A driven point gets the Hencky strain
    E_k = Q_k diag(s_k ln(amp) a + v) Q_k^T: a is its own deviatoric direction of unit largest entry, amp its own amplitude
    (log-uniform in [1.2, 2]), s_k the schedule (grows, unloads, reverses past yield, reloads up to amp; but for the unloading step
    every |s_k| exceeds the ones before it, so that a driven point yields again even under H0 = 10 E, where the surface has grown
    to the largest stress the point has seen), v a volume change of U(-3, 3) s0 / E, and Q_k = Q_(k-1) rot(axis, 0.3): the principal axes turn every increment, so the plastic strain the
    earlier increments left is coaxial with nothing.  A resting point is put back inside the yield surface, at U(0, 0.9) of the
    yield stress from the plastic strain it carries (:func:`state_at` around Ep).  F_k = R_k exp(E_k), R_k accumulating too."""
    return _history(k, n, seed)


@functools.lru_cache(maxsize=None)
def _history(k, n, seed):
    prm = draw(k)
    mu = prm["E"] / 2.0 / (1.0 + prm["nu"])
    rng = np.random.default_rng(9000 + 100 * k + seed)
    a = rng.standard_normal((n, 3))
    a -= a.mean(axis=1, keepdims=True)
    a /= np.abs(a).max(axis=1, keepdims=True)
    lnamp = rng.uniform(np.log(1.2), np.log(2.0), n)
    Q, R = rotations(rng, n), rotations(rng, n)
    axis = rng.standard_normal((n, 3))
    turn = np.array([ls._rotation(x, 0.3) for x in axis])
    Ep, p = ls.natural_state(n)
    out = dict(F=[], ref=[], out=[])
    gone = np.zeros(n, dtype=bool)
    for s in HISTORY_SCHEDULE:
        Q, R = Q @ turn, turn @ R
        v = rng.uniform(-3.0, 3.0, n) * prm["s0"] / prm["E"] / 3.0
        e = s * lnamp[:, None] * a + v[:, None]
        Ed = np.einsum("nia,na,nja->nij", Q, e, Q)
        u = rng.uniform(0.0, 0.9, n)
        Rn = prm["s0"] + prm["H0"] * p
        Er = onp.mandel_to_tensor(Ep + (u * Rn / (np.sqrt(6.0) * mu))[:, None] * unit_deviators(rng, n)) + v[:, None, None] * np.eye(3)
        driven = rng.random(n) < HISTORY_DRIVEN
        w, V = np.linalg.eigh(np.where(driven[:, None, None], Ed, Er))
        F9 = ls.to_vector(R @ np.einsum("nia,na,nja->nij", V, np.exp(w), V))
        r = ls.update(F9, Ep, p, **prm)
        gone = gone | r["skip"]
        out["F"].append(F9)
        out["ref"].append(r)
        out["out"].append(gone.copy())
        Ep, p = r["Ep"], r["p"]
    return out


# ---- the kernel's eigen-solver, to classify inputs -------------------------------------------------------------------------------
def _rotate(A, V, p, q, r):
    app, aqq, apq, arp, arq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, p, q].copy(), A[:, r, p].copy(), A[:, r, q].copy()
    d = aqq - app
    den = d + np.copysign(np.sqrt(d * d + 4.0 * apq * apq), d)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den != 0.0, 2.0 * apq / den, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    A[:, p, p], A[:, q, q] = app - t * apq, aqq + t * apq
    A[:, p, q] = A[:, q, p] = 0.0
    A[:, r, p] = A[:, p, r] = c * arp - s * arq
    A[:, r, q] = A[:, q, r] = s * arp + c * arq
    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p], V[:, :, q] = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq


def jacobi_np(Cm, sweeps=SWEEPS):
    """(c (n, 3) in the order the kernel holds them, V (n, 3, 3) eigenvector columns, off (n,) the largest off-diagonal entry left
    relative to the largest eigenvalue): the cyclic sweeps of ``principal_axes.hpp`` in the rotation order of ``log_strain_kernel``
    ((0, 1), (0, 2), (1, 2)), with the same formulas."""
    A = np.array(Cm, dtype=np.float64)
    V = np.tile(np.eye(3), (len(A), 1, 1))
    for _ in range(sweeps):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    c = np.einsum("nii->ni", A).copy()
    off = np.abs(A[:, [0, 0, 1], [1, 2, 2]]).max(axis=1) / np.abs(c).max(axis=1)
    return c, V, off


GAMMA_CALLS = ((0, 0, 1), (1, 1, 0), (0, 0, 2), (2, 2, 0), (1, 1, 2), (2, 2, 1), (0, 1, 2))    # the order of log_strain.hip
THETA_CALLS = ((0, 1), (0, 2), (1, 2))


def classify(F9):
    """The branches ``log_strain_kernel`` takes at every row: dict(gamma_far (n, 7) bool, one column per call of GAMMA_CALLS;
    theta_far (n, 3) bool; f (n,) int: which of f0 / f1 / f2 the (0, 1, 2) call is handed, -1 where it takes its Taylor form)."""
    F = ls.to_matrix(F9)
    c = jacobi_np(np.einsum("nki,nkj->nij", F, F))[0]
    far = []
    for i, j, k in GAMMA_CALLS:
        m = (c[:, i] + c[:, j] + c[:, k]) * (1.0 / 3.0)
        d = np.abs(np.stack([c[:, i], c[:, j], c[:, k]]) - m) / m
        far.append(d.max(axis=0) > ls.GAMMA_SWITCH)
    far = np.array(far).T
    e = 0.5 * np.log(c)
    theta_far = np.array([np.abs(e[:, i] - e[:, j]) > THETA_SWITCH for i, j in THETA_CALLS]).T
    a01, a02, a12 = np.abs(c[:, 0] - c[:, 1]), np.abs(c[:, 0] - c[:, 2]), np.abs(c[:, 1] - c[:, 2])
    f = np.where((a02 >= a01) & (a02 >= a12), 1, np.where(a12 >= a01, 0, 2))
    return dict(gamma_far=far, theta_far=theta_far, f=np.where(far[:, 6], f, -1))


# ---- the fixture's points -----------------------------------------------------------------------------------------------------
def fixture_points():
    """(F (n, 9), Ep_n, p_n, params (n, 4), draw (n,), amp (n,), labels): FIXTURE_PER_AMP points of every (draw, amp), the first of
    ``stretch_case(k, 64, amp, seed=1)`` that yield and the first that do not in turn (two and one, or one and two), then the
    FIXTURE_SPECIAL rows under PRM (amp 0)."""
    F, Ep, p, prms, dr, am, labels = [], [], [], [], [], [], []
    for k in range(N_DRAWS):
        prm = draw(k)
        for q, amp in enumerate(AMPS):
            Fa, Epa, pa = stretch_case(k, 64, amp, seed=1)
            pl = ls.branch(Fa, Epa, pa, **prm)["plastic"]
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
    """dict of the arrays of ``log_strain_finite.npz``: F, Ep_n, p_n, params, draw, amp, labels, P, A, eel, p, Ep, plastic."""
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    out["labels"] = [str(s) for s in out["labels"]]
    out["plastic"] = out["plastic"].astype(bool)
    return out


def strata(fx):
    """{name: row mask} of the fixture: one stratum per amp, one for the special rows."""
    out = {f"amp {amp:g}": fx["amp"] == amp for amp in AMPS}
    out["special"] = fx["amp"] == 0.0
    return out
