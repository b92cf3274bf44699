"""Parameter draws, cyclic histories and harvested single-step cases for the FCC single-crystal viscoplastic law (law id 14), and the
driver that walks them through the C ABI: shared by ``test_single_crystal_sweep_cpu.py`` (which pins all of it with the references
alone and runs the driver on the CPU double), ``test_gpu_single_crystal_sweep.py`` (which holds the kernel to it) and
``golden/make_single_crystal_sweep.py`` (which measures the bounds at 50 digits).  TEST INFRASTRUCTURE ONLY.

Draws (``draw``): seeds 0 and 1 are the ``mfront`` and ``variant`` sets of ``single_crystal_kat.npz`` at dt = 0.1.  Seeds 2 to 9 are
stratified, so that every range is covered end to end by eight draws: n through (2, 4, 20, 2, 10, 20, 4, 6), dt through
(1e3, 1e-3, 10, 1e-3, 0.1, 1e3, 10, 1e3), K in [10, 80], tau0 in [20, 200], Q in [0, 200] (0 at seed 4), b in [1, 50], C log-uniform
in [1e3, 2e5], d in [0, 3e3] (0 at seed 7), the six interaction coefficients in [0.5, 15], E_i in [1e5, 2.5e5], nu_ij in [0.15, 0.35],
G_ij in [4e4, 1e5] (positive definite for every combination: the compliance is diagonally dominant below nu = 0.5 E_min / E_max).

Histories (``history``): per point a random frame and a random direction d; a jump to two and a half increments short of first yield (the
largest elastic scale along d, found by bisection with the restatement), 20 increments of norm h along d (first yield, developed
flow), a jump back to two and a half increments short of yielding again on the other side, 18 increments of -h d, then four increments of
norm h along a second random direction: 44 in all.  h is 1e-4 halved until the f > 1.1 K guard trips nowhere at dg = 0 and at least
99 % of the points stay at status 0 at every increment (``STEP_NORM``; seeds 0 and 1 keep the 1e-4 of the fixed-input tests).  A
point that leaves status 0 is frozen: its strain and its reference state stay what they were, it is left out of the value
comparisons from then on and counted.

Count tolerance at the yield surface (``kink``): a point whose largest trial yield function is within KINK tau0 of zero is left out
of the n_plastic comparison only (its values are compared: the law is continuous there); at most KINK_CAP of an increment's points.

Harvest (``harvest``): single steps of every branch of the local Newton, found by a fixed-seed search over the stiff-hardening
corner (Q = 200, b = 50) and over n = 2 at large dt, kept only where the branch survives perturbations of the inputs (``robust``);
stored in ``single_crystal_sweep.npz``, the search is not rerun by the tests."""
import ctypes as C
import functools

import numpy as np

import single_crystal_ref as sc

SEEDS = tuple(range(10))
N_SWEEP = 1027                         # 16 full tiles of 64 and a ragged one of 3
N_TILE = 71                            # one full tile and a ragged one of 7
MP_SAMPLE = 6                          # points per seed whose whole history is re-run at 50 digits
KINK = 1e-9                            # min_i |f_trial_i| <= KINK tau0 at a positive trial: left out of the n_plastic comparison only
KINK_CAP = 1e-4                        # the share of such points an increment may have
STATUS0_SHARE = 0.99
UP, DOWN, TURN = 20, 18, 4
N_INC = 1 + UP + 1 + DOWN + TURN       # 44
REVERSAL = 1 + UP                      # the increment of the jump back
FIELDS = ("eel", "g", "p", "a")        # state fields 0..3 of the law
EXISTING_BOUND = {"stress": 1e-12, "state": 1e-12, "tangent": 3.8e-11}
CLASSES = ("quick", "slow", "halved", "capped", "guard")

VARIANT = sc.param_vector(dict(E1=150000.0, E2=180000.0, nu12=0.25, G13=70000.0, n=6.0, K=30.0, tau0=50.0, Q=20.0, b=4.0, d=300.0,
                               C=10000.0), interaction=(1.0, 1.4, 0.7, 9.0, 1.9, 2.3))
DRAW_N = (2.0, 4.0, 20.0, 2.0, 10.0, 20.0, 4.0, 6.0)
DRAW_DT = (1e3, 1e-3, 10.0, 1e-3, 0.1, 1e3, 10.0, 1e3)
#: increment norm of every seed's history: 1e-4 halved until the history meets its conditions (``choose_step_norm``)
STEP_NORM = (1e-4, 1e-4, 3.125e-6, 1e-4, 1e-4, 1e-4, 5e-5, 1e-4, 1e-4, 2.5e-5)


# ---- draws -------------------------------------------------------------------------------------------------------------------
def _strata(master, lo, hi, log=False):
    """eight values, one in each eighth of [lo, hi], in a random order"""
    u = (master.permutation(8) + master.uniform(size=8)) / 8.0
    return np.exp(np.log(lo) + u * (np.log(hi) - np.log(lo))) if log else lo + u * (hi - lo)


@functools.lru_cache(maxsize=None)
def _table():
    master = np.random.default_rng(14_000)
    cols = {k: _strata(master, 1e5, 2.5e5) for k in ("E1", "E2", "E3")}
    cols.update({k: _strata(master, 0.15, 0.35) for k in ("nu12", "nu23", "nu13")})
    cols.update({k: _strata(master, 4e4, 1e5) for k in ("G12", "G23", "G13")})
    cols["K"], cols["tau0"] = _strata(master, 10.0, 80.0), _strata(master, 20.0, 200.0)
    cols["Q"], cols["b"] = _strata(master, 0.0, 200.0), _strata(master, 1.0, 50.0)
    cols["C"], cols["d"] = _strata(master, 1e3, 2e5, log=True), _strata(master, 0.0, 3e3)
    cols["Q"][2], cols["d"][5] = 0.0, 0.0                      # seeds 4 and 7
    h = np.array([_strata(master, 0.5, 15.0) for _ in range(6)]).T
    return cols, h


def draw(seed):
    """(22 parameters, dt) of draw ``seed``."""
    if seed == 0:
        return sc.param_vector(), 0.1
    if seed == 1:
        return VARIANT.copy(), 0.1
    cols, h = _table()
    k = seed - 2
    props = {name: float(v[k]) for name, v in cols.items()}
    props["n"] = DRAW_N[k]
    return sc.param_vector(props, interaction=tuple(float(x) for x in h[k])), DRAW_DT[k]


# ---- histories ---------------------------------------------------------------------------------------------------------------
def random_frames(rng, n):
    R = np.empty((n, 3, 3))
    for i in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[2] *= -1
        R[i] = q
    return R


def directions(rng, n):
    d = rng.normal(size=(n, 6)) * np.array([1, 1, 1, 0.7, 0.7, 0.7])
    d[np.arange(n), np.arange(n) % 3] += 1.5
    return d / np.linalg.norm(d, axis=1)[:, None]


def trial_f(eps, state, prm, R):
    """(N, 12): |tau_i - C a_i| - r_i at dg = 0, the yield functions of the trial state"""
    prm = np.asarray(prm)
    D, mu = sc.stiffness(prm), sc.schmid()
    em = np.einsum("nik,nk->ni", sc.mandel_rotation(R), eps)
    tau = (em - state["g"] @ mu) @ (mu @ D).T
    QH = prm[12] * prm[16:22][sc.interaction_classes()]
    r = prm[11] + (1.0 - np.exp(-prm[13] * state["p"])) @ QH.T
    return np.abs(tau - prm[15] * state["a"]) - r


def kink(eps, state, prm, R):
    """(N,) bool: |max_i f_trial_i| <= KINK tau0, the points where either answer to "did it yield" is right.  (The point yields when
    its largest f_i is positive: a small f_i next to a large one decides nothing, so the largest is what is looked at.)"""
    return np.abs(trial_f(eps, state, prm, R).max(axis=1)) <= KINK * np.asarray(prm)[11]


def elastic_reach(base, d, state, prm, R, hi=0.1):
    """per point the largest s in [0, hi] with base + s d still elastic from ``state`` (bisection on the trial state, 50 halvings)"""
    lo, hi = np.zeros(len(d)), np.full(len(d), float(hi))
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        pl = (trial_f(base + mid[:, None] * d, state, prm, R) > 0.0).any(axis=1)
        lo, hi = np.where(pl, lo, mid), np.where(pl, mid, hi)
    return lo


def history(seed, n, h=None):
    """The history of draw ``seed`` at n points (cached): a dict with ``prm``, ``dt``, ``R`` (n, 3, 3), ``h``, ``eps`` (N_INC total
    strains (n, 6)), ``ref`` (the N_INC results of the restatement, each from the state the one before left), ``frozen`` (N_INC (n,)
    bool: left status 0 at an earlier increment), ``kink`` (N_INC (n,) bool), ``first_fail`` (n,) int: the status that froze the
    point, 0 for none."""
    return _history(seed, n, STEP_NORM[seed] if h is None else float(h))


@functools.lru_cache(maxsize=None)
def _history(seed, n, h):
    prm, dt = draw(seed)
    rng = np.random.default_rng(14_100 + seed)
    R, d, d2 = random_frames(rng, n), directions(rng, n), directions(rng, n)
    out = dict(prm=prm, dt=dt, R=R, h=h, eps=[], ref=[], frozen=[], kink=[], first_fail=np.zeros(n, dtype=int))
    state = sc.zero_state(n)
    eps = np.zeros((n, 6))
    frozen = np.zeros(n, dtype=bool)
    for inc in range(N_INC):
        if inc == 0:
            new = np.maximum(elastic_reach(eps, d, state, prm, R) - 2.5 * h, 0.0)[:, None] * d
        elif inc == REVERSAL:
            new = eps - np.maximum(elastic_reach(eps, -d, state, prm, R) - 2.5 * h, 0.0)[:, None] * d
        elif inc < REVERSAL:
            new = eps + h * d
        elif inc < N_INC - TURN:
            new = eps - h * d
        else:
            new = eps + h * d2
        eps = np.where(frozen[:, None], eps, new)
        ref = sc.update(eps, state, prm, dt, R=R)
        out["eps"].append(eps.copy())
        out["ref"].append(ref)
        out["frozen"].append(frozen.copy())
        out["kink"].append(kink(eps, state, prm, R))
        bad = (ref["status"] != 0) & ~frozen
        out["first_fail"][bad] = ref["status"][bad]
        keep = frozen | bad
        state = {k: np.where(keep[:, None], state[k], ref[k]) for k in FIELDS}
        frozen = keep
    out["n_frozen"] = int(frozen.sum())
    return out


def history_ok(hist):
    """the conditions of a history: no guard at dg = 0, status 0 on >= 99 % of the points at every increment, the kink cap"""
    n = len(hist["R"])
    return ((hist["first_fail"] != 2).all() and all((r["status"] == 0).sum() >= STATUS0_SHARE * n for r in hist["ref"])
            and all(k.sum() <= KINK_CAP * n for k in hist["kink"]))


def choose_step_norm(seed, n=N_SWEEP):
    """1e-4 halved until ``history_ok``: what ``STEP_NORM`` records"""
    h = 1e-4
    while not history_ok(_history(seed, n, h)):
        h *= 0.5
        assert h > 1e-7
    return h


# ---- harvest -----------------------------------------------------------------------------------------------------------------
STIFF = sc.param_vector(dict(Q=200.0, b=50.0))
SOFT = sc.param_vector(dict(n=2.0))
#: (name, parameters, dt) of the corners searched: stiff hardening at every time step, n = 2 at the large ones
CORNERS = tuple((f"stiff dt={dt:g}", STIFF, dt) for dt in (1e-3, 0.1, 10.0, 1e3)) + tuple((f"n=2 dt={dt:g}", SOFT, dt) for dt in (10.0, 1e3))
PER_CLASS = 8


def classify(out):
    """class index per point of a restatement result, -1 for none of them"""
    c = np.full(len(out["status"]), -1)
    ok = out["plastic"] & (out["status"] == 0)
    c[ok & (out["halvings"] == 0) & (out["iters"] >= 3) & (out["iters"] <= 5)] = 0
    c[ok & (out["halvings"] == 0) & (out["iters"] >= 15)] = 1
    c[ok & (out["halvings"] > 0)] = 2
    c[out["status"] == 1] = 3
    c[out["status"] == 2] = 4
    return c


def harvest(n=800, verbose=False):
    """The search: per corner a cyclic proportional path of 24 increments up and 39 down at n points with random frames, for step
    norms 1e-4, 1.5e-4, 2e-4 and 3e-4; every point-step is classified and the first PER_CLASS of a class and corner that are ``robust`` are kept
    (for ``halved`` those with two or more halvings first).  Returns a dict of arrays over the kept cases: ``corner`` (index into CORNERS), ``cls``, ``R``,
    ``eps``, ``eel0``, ``g0``, ``p0``, ``a0``, ``iters``, ``halvings``, ``status``.  Conditions, asserted: over all corners at least 8
    cases of every class, at least 2 with ``halvings >= 2``, and a corner that holds a quick, a slow and a halved or capped case."""
    rec = {k: [] for k in ("corner", "cls", "R", "eps", "eel0", "g0", "p0", "a0", "iters", "halvings", "status")}
    for ci, (name, prm, dt) in enumerate(CORNERS):
        found = {c: [] for c in range(5)}
        for si, norm in enumerate((1e-4, 1.5e-4, 2e-4, 3e-4)):
            rng = np.random.default_rng(14_200 + 10 * ci + si)
            R, d = random_frames(rng, n), directions(rng, n)
            state = sc.zero_state(n)
            alive = np.ones(n, dtype=bool)
            for k in [j for j in range(1, 25)] + [24 - j for j in range(1, 40)]:
                eps = k * norm * d
                out = sc.update(eps, state, prm, dt, R=R)
                cls = classify(out)
                for i in np.nonzero(alive & (cls >= 0))[0]:
                    found[int(cls[i])].append((int(out["halvings"][i]), len(found[int(cls[i])]), dict(
                        corner=ci, cls=int(cls[i]), R=R[i], eps=eps[i], eel0=state["eel"][i], g0=state["g"][i], p0=state["p"][i],
                        a0=state["a"][i], iters=int(out["iters"][i]), halvings=int(out["halvings"][i]), status=int(out["status"][i]))))
                alive &= out["status"] == 0          # a point that failed once is not followed further
                state = {f: np.where(alive[:, None], out[f], state[f]) for f in FIELDS}
        for c, items in found.items():
            items.sort(key=lambda t: (-min(t[0], 2), t[1]) if c == 2 else t[1])
            kept = [item for _, _, item in items[:8 * PER_CLASS] if robust(item, prm, dt)][:PER_CLASS]
            if verbose:
                print(name, CLASSES[c], len(items), len(kept), flush=True)
            for item in kept:
                for k, v in item.items():
                    rec[k].append(v)
    out = {k: np.array(v) for k, v in rec.items()}
    check_harvest(out)
    return out


def robust(item, prm, dt, copies=64, size=1e-14):
    """a candidate keeps its status, halvings and iteration count when it is evaluated alone and in ``copies`` copies whose strain and
    state carry random relative perturbations of ``size``: a case on a knife edge between two branches (a halved iteration can be
    chaotic) would compare the rounding of two implementations, not their branches"""
    rng = np.random.default_rng(14_400)
    one = lambda v: np.concatenate([v[None], v[None] * (1.0 + size * rng.normal(size=(copies,) + v.shape))])  # noqa: E731
    out = sc.update(one(item["eps"]), {k: one(item[k + "0"]) for k in FIELDS}, prm, dt, R=np.repeat(item["R"][None], copies + 1, axis=0))
    alone = sc.update(item["eps"][None], {k: item[k + "0"][None] for k in FIELDS}, prm, dt, R=item["R"][None])
    return all((np.concatenate([out[k], alone[k]]) == item[k]).all() for k in ("status", "halvings", "iters"))


def check_harvest(hv):
    cls, corner = hv["cls"], hv["corner"]
    for c in range(5):
        assert (cls == c).sum() >= 8, (CLASSES[c], int((cls == c).sum()))
    assert ((cls == 2) & (hv["halvings"] >= 2)).sum() >= 2
    assert mixing_corners(hv), "no corner holds a quick, a slow and a halved or capped case"


def mixing_corners(hv):
    """the corners whose cases can fill a round with a quick, a slow and a halved or capped point"""
    out = []
    for ci in np.unique(hv["corner"]):
        have = set(hv["cls"][hv["corner"] == ci].tolist())
        if {0, 1} <= have and have & {2, 3}:
            out.append(int(ci))
    return out


def harvest_inputs(hv, m):
    """(eps, R, state) of the harvested cases of mask / index m"""
    return hv["eps"][m], hv["R"][m], {"eel": hv["eel0"][m], "g": hv["g0"][m], "p": hv["p0"][m], "a": hv["a0"][m]}


# ---- the driver: one dxm_material of the law through the C ABI ------------------------------------------------------------------
class HostArrays:
    """where "device" memory is ordinary memory: the CPU double of the library"""

    @staticmethod
    def up(a):
        return np.array(a, dtype=np.float64, order="C")

    @staticmethod
    def zeros(n, k):
        return np.zeros((n, k))

    @staticmethod
    def ptr(a):
        return a.ctypes.data

    @staticmethod
    def down(a):
        return a.copy()

    @staticmethod
    def sync():
        pass


class Handle:
    def __init__(self, lib, law, p, n, arrays=HostArrays):
        self.lib, self.n, self.mem = lib, n, arrays
        self.h = lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, self.err()

    def err(self):
        return (self.lib.dxm_last_error() or b"").decode()

    def frame(self, R):
        a = np.array(R, dtype=np.float64, order="C").reshape(self.n, 9)
        assert self.lib.dxm_set_frame_field(self.h, a.ctypes.data) == 0, self.err()
        return self

    def set_state(self, state, which=0):
        for f, k in enumerate(FIELDS):
            a = np.array(state[k], dtype=np.float64, order="C")
            assert self.lib.dxm_set_state(self.h, which, f, a.ctypes.data) == 0, self.err()
        return self

    def get_state(self, which=1):
        out = {}
        for f, k in enumerate(FIELDS):
            a = np.full((self.n, 6 if k == "eel" else 12), np.nan)
            assert self.lib.dxm_get_state(self.h, which, f, a.ctypes.data) == 0, self.err()
            out[k] = a
        return out

    def stats(self):
        from dolfinx_materials_amd import _lib

        st = _lib.Stats()
        assert self.lib.dxm_get_stats(self.h, C.byref(st)) >= 0, self.err()
        return {k: v for k, v in st.as_dict().items() if k in ("n_points", "n_plastic", "n_not_converged", "n_nan", "max_local_iters")}

    def device(self, eps, dt, stream=None):
        """dxm_integrate_device: (stress, tangent (n, 36), the new state, stats)"""
        e, f, c = self.mem.up(eps), self.mem.zeros(self.n, 6), self.mem.zeros(self.n, 36)
        assert self.lib.dxm_integrate_device(self.h, self.mem.ptr(e), dt, self.mem.ptr(f), self.mem.ptr(c), stream) == 0, self.err()
        self.mem.sync()
        return self.mem.down(f), self.mem.down(c), self.get_state(), self.stats()

    def host(self, eps, dt):
        """dxm_integrate on host buffers: (stress, tangent, the 42 state numbers per point, stats)"""
        from dolfinx_materials_amd import _lib

        eps = np.ascontiguousarray(eps, dtype=np.float64)
        f, c, isv, st = np.full((self.n, 6), np.nan), np.full((self.n, 36), np.nan), np.full((self.n, 42), np.nan), _lib.Stats()
        assert self.lib.dxm_integrate(self.h, eps.ctypes.data, dt, f.ctypes.data, isv.ctypes.data, c.ctypes.data, C.byref(st)) >= 0, self.err()
        return f, c, isv, self.stats()

    def rows(self, eps, dt, rows):
        """dxm_integrate_rows: point i writes row rows[i] of the two output arrays, which are returned whole"""
        from dolfinx_materials_amd import _lib

        eps, rows = np.ascontiguousarray(eps, dtype=np.float64), np.ascontiguousarray(rows, dtype=np.int64)
        top = int(rows.max()) + 1
        f, c, st = np.full((top, 6), -7.0), np.full((top, 36), -9.0), _lib.Stats()
        assert self.lib.dxm_integrate_rows(self.h, eps.ctypes.data, dt, f.ctypes.data, c.ctypes.data, rows.ctypes.data, C.byref(st)) >= 0, self.err()
        return f, c, self.stats()

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, self.err()
        return self

    def newton(self, maxit, rtol):
        assert self.lib.dxm_set_newton(self.h, int(maxit), float(rtol)) == 0, self.err()
        return self

    def advance(self):
        assert self.lib.dxm_advance(self.h) == 0, self.err()

    def revert(self):
        assert self.lib.dxm_revert(self.h) == 0, self.err()

    def close(self):
        self.lib.dxm_destroy(self.h)


def rel(a, b, scale=None):
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / (np.abs(b).max() if scale is None else scale))


def deviations(S, T, state, ref, m=None):
    """{"stress", "tangent", "state"}: the largest deviation relative to the field scale over the points of mask m, as
    ``test_gpu_single_crystal.check`` measures it"""
    m = np.ones(len(S), dtype=bool) if m is None else np.asarray(m)
    if not m.any():
        return {"stress": 0.0, "tangent": 0.0, "state": 0.0}
    scale = max(np.abs(ref[k][m]).max() for k in FIELDS)
    return {"stress": rel(S[m], ref["stress"][m]), "tangent": rel(np.asarray(T).reshape(-1, 6, 6)[m], ref["tangent"][m]),
            "state": max(rel(state[k][m], ref[k][m], scale) for k in FIELDS)}


def check_counts(st, ref, n, skip=None, capped=None, tag=""):
    """the launch statistics against the restatement's: n_plastic up to the kink points ``skip``, the iteration count within one.
    ``capped`` marks the frozen points that stopped at the iteration cap: what they hold on the device is no longer the restatement's
    state, so each of them may count either way, and may run up to the cap (26 with a closing halving)"""
    assert st["n_points"] == n and st["n_nan"] == 0, (tag, st)
    capped = np.zeros(n, dtype=bool) if capped is None else np.asarray(capped)
    slack = int(capped.sum())
    loose = slack + (0 if skip is None else int(np.asarray(skip).sum()))
    assert abs(st["n_plastic"] - int(ref["plastic"].sum())) <= loose, (tag, st, int(ref["plastic"].sum()))
    assert abs(st["n_not_converged"] - int((ref["status"] != 0).sum())) <= slack, (tag, st, int((ref["status"] != 0).sum()))
    # the stopping rule is an absolute 1e-14 on the slip residuals: a residual that lands on it may take one pass more or less
    its = int(ref["iters"][~capped].max(initial=0))
    assert its - 1 <= st["max_local_iters"] <= (its + 1 if slack == 0 else max(its + 1, 26)), (tag, st, its)


def walk_history(handle, hist, bounds, first=0, last=None, each=None):
    """Drive ``handle`` (virgin, frames set) through increments first .. last-1 of ``hist``: integrate on the device, compare every
    point that is not frozen with the restatement at ``bounds`` ({"stress", "tangent", "state"}), check the counts, advance.  The
    state is never set from the host.  Returns the largest deviations met."""
    worst = {"stress": 0.0, "tangent": 0.0, "state": 0.0}
    n = len(hist["R"])
    for inc in range(first, N_INC if last is None else last):
        ref = hist["ref"][inc]
        S, T, new, st = handle.device(hist["eps"][inc], hist["dt"])
        live = ~hist["frozen"][inc] & (ref["status"] == 0)
        dev = deviations(S, T, new, ref, live)
        for k, v in dev.items():
            worst[k] = max(worst[k], v)
            assert v <= bounds[k], (inc, k, v, bounds[k])
        check_counts(st, ref, n, skip=hist["kink"][inc], capped=hist["frozen"][inc] & (hist["first_fail"] == 1), tag=f"increment {inc}")
        if each is not None:
            each(inc, S, T, new, st)
        handle.advance()
    return worst


def bit_equal(a, b, same=np.array_equal):
    """two results (stress, tangent, state dict[, ...]) carry the same bits"""
    return same(a[0], b[0]) and same(a[1], b[1]) and all(same(a[2][k], b[2][k]) for k in FIELDS)


def revert_inside_history(make, hist):
    """Two handles walk to the reversal; one integrates a large step there (the strain of five increments later), reverts and then
    integrates the real step, its twin takes the real step only.  Returns both results: they must be equal bit for bit."""
    n = len(hist["R"])
    a, b = make(hist["prm"], n).frame(hist["R"]), make(hist["prm"], n).frame(hist["R"])
    for inc in range(REVERSAL):
        for h in (a, b):
            h.device(hist["eps"][inc], hist["dt"])
            h.advance()
    a.device(hist["eps"][REVERSAL + 5], hist["dt"])
    a.revert()
    ra, rb = a.device(hist["eps"][REVERSAL], hist["dt"]), b.device(hist["eps"][REVERSAL], hist["dt"])
    a.close()
    b.close()
    return ra, rb


def run_cases(make, prm, dt, eps, R, state, maxit=None):
    h = make(prm, len(eps)).frame(R).set_state(state)
    if maxit is not None:
        h.newton(maxit, 1e-14)
    out = h.device(eps, dt)
    h.close()
    return out


def harvest_against_50_digits(make, gold, corner):
    """the status-0 cases of one corner, halved ones included, against their 50-digit values at the corner's bound; returns the
    deviations"""
    hv = {k[3:]: gold[k] for k in gold.files if k.startswith("hv_")}
    m = (hv["corner"] == corner) & (hv["status"] == 0)
    _, prm, dt = CORNERS[corner]
    eps, R, state = harvest_inputs(hv, m)
    S, T, new, st = run_cases(make, prm, dt, eps, R, state)
    V = hv["state"][m]
    ref = {"stress": hv["stress"][m], "tangent": hv["tangent"][m], "eel": V[:, :6], "g": V[:, 6:18], "p": V[:, 18:30], "a": V[:, 30:42]}
    dev = deviations(S, T, new, ref)
    bound = dict(zip(("stress", "tangent", "state"), gold["hv_corner_bound"][corner]))
    for k, v in dev.items():
        assert v <= bound[k], (CORNERS[corner][0], k, v, bound[k])
    n = int(m.sum())
    assert st["n_points"] == n and st["n_plastic"] == n and st["n_not_converged"] == 0 and st["n_nan"] == 0, st
    assert abs(st["max_local_iters"] - int(hv["iters"][m].max())) <= 1, (st, int(hv["iters"][m].max()))
    return dev, bound


def failed_cases(make, hv, corner):
    """the status 1 and status 2 cases of one corner: the count, the state bits and the elastic answer of the guard-failed points,
    finite outputs of the capped ones"""
    m = (hv["corner"] == corner) & (hv["status"] != 0)
    if not m.any():
        return 0
    _, prm, dt = CORNERS[corner]
    eps, R, state = harvest_inputs(hv, m)
    ref = sc.update(eps, state, prm, dt, R=R)
    assert np.array_equal(ref["status"], hv["status"][m])
    S, T, new, st = run_cases(make, prm, dt, eps, R, state)
    n = int(m.sum())
    assert st["n_points"] == n and st["n_not_converged"] == n and st["n_plastic"] == n and st["n_nan"] == 0, st
    assert np.isfinite(S).all() and np.isfinite(T).all() and all(np.isfinite(new[k]).all() for k in FIELDS)
    g = ref["status"] == 2
    for k in FIELDS:
        assert np.array_equal(new[k][g], state[k][g]), k
    if g.any():
        D, Q = sc.stiffness(prm), sc.mandel_rotation(R[g])
        trial = np.einsum("nik,nk->ni", Q, eps[g]) - state["g"][g] @ sc.schmid()
        assert rel(S[g], np.einsum("nik,ni->nk", Q, trial @ D)) <= 1e-12
        assert rel(T.reshape(-1, 6, 6)[g], np.einsum("nri,rs,nsk->nik", Q, D, Q)) <= 1e-12
    return n


def lowered_cap(make, gold, corner, maxit=3):
    """the well-behaved cases of one corner under dxm_set_newton(maxit, 1e-14): the count of the restatement at the same cap, and the
    points that converge within it at the corner's bound"""
    hv = {k[3:]: gold[k] for k in gold.files if k.startswith("hv_")}
    m = (hv["corner"] == corner) & (hv["cls"] <= 1)
    if not m.any():
        return None
    _, prm, dt = CORNERS[corner]
    eps, R, state = harvest_inputs(hv, m)
    ref = sc.update(eps, state, prm, dt, R=R, maxit=maxit)
    S, T, new, st = run_cases(make, prm, dt, eps, R, state, maxit=maxit)
    assert st["n_not_converged"] == int((ref["status"] != 0).sum()) and st["n_plastic"] == int(m.sum()) and st["n_nan"] == 0, (st, ref["status"])
    assert np.isfinite(S).all() and np.isfinite(T).all()
    ok = ref["status"] == 0
    if not ok.all():      # no step is halved on these cases: a capped point has taken exactly maxit iterations
        assert (ref["halvings"] == 0).all() and st["max_local_iters"] == maxit == int(ref["iters"].max()), (st, maxit)
    dev = deviations(S, T, new, ref, ok)
    for k, b in zip(("stress", "tangent", "state"), gold["hv_corner_bound"][corner]):
        assert dev[k] <= b, (CORNERS[corner][0], k, dev[k], b)
    return int((~ok).sum()), int(ok.sum())


def caps_on_a_halved_case(make, hv, i):
    """Halved case i alone under every iteration cap from 2 to two short of its own count: where the restatement stops at the cap
    (in either branch: after a step, or after a halving) the kernel stops with the same count, iteration for iteration; where it
    converges the count may differ by the one pass of the absolute stopping rule.  Returns the number of caps that were hit by a
    halving."""
    _, prm, dt = CORNERS[hv["corner"][i]]
    eps, R, state = harvest_inputs(hv, [i])
    by_halving, before = 0, 0
    for maxit in range(2, int(hv["iters"][i]) - 1):
        ref = sc.update(eps, state, prm, dt, R=R, maxit=maxit)
        S, T, new, st = run_cases(make, prm, dt, eps, R, state, maxit=maxit)
        assert st["n_not_converged"] == int(ref["status"][0] != 0) and st["n_nan"] == 0, (int(i), maxit, st, ref["status"])
        assert np.isfinite(S).all() and np.isfinite(T).all()
        if ref["status"][0] == 1:
            assert st["max_local_iters"] == int(ref["iters"][0]), (int(i), maxit, st, int(ref["iters"][0]))
            by_halving += int(ref["halvings"][0] > before and ref["iters"][0] == maxit)
        else:
            assert abs(st["max_local_iters"] - int(ref["iters"][0])) <= 1, (int(i), maxit, st)
        before = int(ref["halvings"][0])
    return by_halving


# ---- round-mates: one special point in seven companies ---------------------------------------------------------------------------
YIELDED_AT = (5, 20, 41, 60)           # the four yielded points of the mixed round
PLACEMENTS = ("alone", "rank 0", "rank 1", "rank 2", "rank 3", "all yielded", "ragged tail")


def _tile(hv, where, elastic_R):
    """inputs of a tile of N_TILE points: ``where`` maps positions to harvested cases, every other point is elastic (virgin, a strain
    of norm 1e-6)"""
    n = N_TILE
    eps = np.zeros((n, 6))
    eps[:, 0], eps[:, 3] = 8e-7, 6e-7
    R = elastic_R.copy()
    state = sc.zero_state(n)
    for pos, i in where.items():
        eps[pos], R[pos] = hv["eps"][i], hv["R"][i]
        for k in FIELDS:
            state[k][pos] = hv[k + "0"][i]
    return eps, R, state


def placements(make, hv, x, same=np.array_equal):
    """Harvested case x in the seven companies of PLACEMENTS, each next to the same tile with an elastic point in its place.
    Asserts that the other points do not notice it; returns per placement (stress, tangent, state, counts) of x alone, counts being
    what it adds to (n_plastic, n_not_converged)."""
    corner = hv["corner"][x]
    _, prm, dt = CORNERS[corner]
    mine = np.nonzero(hv["corner"] == corner)[0]
    firsts = [int(mine[hv["cls"][mine] == c][0]) for c in range(5) if c != hv["cls"][x] and (hv["cls"][mine] == c).any()]
    firsts = firsts or [int(i) for i in mine if i != x]
    mates = [firsts[k % len(firsts)] for k in range(3)]                # one case of each other class the corner has, cycled to three
    filler = [i for i in mine if hv["status"][i] == 0] or list(mine)
    frames = random_frames(np.random.default_rng(14_300), N_TILE)
    out = []
    for name in PLACEMENTS:
        if name == "alone":
            pos, where = 37, {}
        elif name == "ragged tail":
            pos, where = 66, {}
        elif name == "all yielded":
            pos, where = 37, {p: filler[p % len(filler)] for p in range(N_TILE)}
        else:
            r = int(name[-1])
            pos = YIELDED_AT[r]
            where = dict(zip([p for p in YIELDED_AT if p != pos], mates))
        h = make(prm, N_TILE)
        res = []
        for special in (True, False):
            w = dict(where)
            if special:
                w[pos] = x
            else:
                w.pop(pos, None)
            eps, R, state = _tile(hv, w, frames)
            res.append(h.frame(R).set_state(state).device(eps, dt))
        h.close()
        (S, T, new, st), (S0, T0, new0, st0) = res
        rest = np.arange(N_TILE) != pos
        assert same(S[rest], S0[rest]) and same(T[rest], T0[rest]), (name, "the other points noticed the special one")
        for k in FIELDS:
            assert same(new[k][rest], new0[k][rest]), (name, k)
        assert st["n_nan"] == 0 and st0["n_nan"] == 0
        out.append((S[pos], T[pos], {k: new[k][pos] for k in FIELDS}, (st["n_plastic"] - st0["n_plastic"], st["n_not_converged"] - st0["n_not_converged"])))
    return out


def check_placements(make, hv, x, same=np.array_equal):
    """``same`` is bit identity for the kernel (16-lane rows are independent, finished rows are frozen); the CPU double, whose
    linear algebra depends on the size of the batch, passes a comparison to rounding"""
    res = placements(make, hv, x, same)
    for name, r in zip(PLACEMENTS[1:], res[1:]):
        assert bit_equal(r, res[0], same) and r[3] == res[0][3], (int(x), CLASSES[hv["cls"][x]], name)
    assert res[0][3] == (1, int(hv["status"][x] != 0)), (int(x), res[0][3])
