"""GPU: FCC single-crystal viscoplasticity (DXM_LAW_SINGLE_CRYSTAL_FCC, ``single_crystal_kernel``) through the C ABI (ctypes)
against the committed 50-digit values and the numpy restatement ``single_crystal_ref.update``; tiles built point by point, the three
frame states, grid sizes, chunks, the rows and the device-pointer forms against each other bit for bit; the guard at dg = 0.

Bound: max(1e-12, 8 x the deviation of the restatement from its 50-digit version) relative to the field scale, per field, read from
``tests/golden/single_crystal_kat.npz`` (stress 1.1e-15, state 1.3e-15: 1e-12; tangent 4.8e-12, the distance of the Jacobian of the
last-but-one iterate from the converged one: 3.8e-11).

Inputs: every accepted strain increment has norm 1e-4 (the restatement asserts that no point but the deliberate one trips the
f > 1.1 K guard: status 0 everywhere); no point is left out of any comparison."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import single_crystal_ref as sc
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_crystal_kat.npz"))
META = json.loads(str(GOLD["meta"]))
BOUND = {k: max(1e-12, 8 * v) for k, v in META["restatement_deviation"].items()}
LAW = _lib.LAW_SINGLE_CRYSTAL_FCC
PRM = sc.param_vector()
DT = 0.1
FIELDS = ("eel", "g", "p", "a")   # state fields 0..3 of the law
POOL = 512
NBIG = 100_003


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


class Handle:
    """one dxm_material of the law, driven through ctypes alone"""

    def __init__(self, p, n):
        self.lib, self.n = _lib.load(), n
        self.h = self.lib.dxm_create(LAW, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)

    def frame(self, R):
        if R is None:
            rc = self.lib.dxm_set_frame(self.h, None)
        else:
            a = np.array(R, dtype=np.float64, order="C")
            rc = self.lib.dxm_set_frame(self.h, a.ctypes.data) if a.shape == (3, 3) else self.lib.dxm_set_frame_field(self.h, a.reshape(self.n, 9).ctypes.data)
        assert rc == 0, err(self.lib)
        return self

    def set_state(self, state, which=_lib.S0):
        for f, k in enumerate(FIELDS):
            a = np.array(state[k], dtype=np.float64, order="C")
            assert self.lib.dxm_set_state(self.h, which, f, a.ctypes.data) == 0, err(self.lib)
        return self

    def get_state(self, which=_lib.S1):
        out = {}
        for f, k in enumerate(FIELDS):
            a = np.full((self.n, 6 if k == "eel" else 12), np.nan)
            assert self.lib.dxm_get_state(self.h, which, f, a.ctypes.data) == 0, err(self.lib)
            out[k] = a
        return out

    def stats(self):
        st = _lib.Stats()
        rc = self.lib.dxm_get_stats(self.h, C.byref(st))
        assert rc >= 0, err(self.lib)
        return st.as_dict()

    def device(self, eps_dev, dt=DT, stream=None):
        import torch

        f = torch.zeros((self.n, 6), dtype=torch.float64, device=eps_dev.device)
        c = torch.zeros((self.n, 36), dtype=torch.float64, device=eps_dev.device)
        assert self.lib.dxm_integrate_device(self.h, eps_dev.data_ptr(), dt, f.data_ptr(), c.data_ptr(), stream) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.stats()

    def host(self, eps, dt=DT):
        f, c, st = np.full((self.n, 6), np.nan), np.full((self.n, 36), np.nan), _lib.Stats()
        isv = np.full((self.n, 42), np.nan)
        rc = self.lib.dxm_integrate(self.h, eps.ctypes.data, dt, f.ctypes.data, isv.ctypes.data, c.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, isv, st.as_dict()

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def close(self):
        self.lib.dxm_destroy(self.h)


def rel(a, b, scale=None):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(b).max() if scale is None else scale)


def check(tag, S, T, state, ref):
    """stress, the 36 tangent entries and all 42 state numbers against `ref` (a dict like single_crystal_ref.update's)"""
    n = len(ref["stress"])
    es, et = rel(S, ref["stress"]), rel(T.reshape(n, 6, 6), ref["tangent"])
    scale = max(np.abs(ref["eel"]).max(), np.abs(ref["g"]).max(), np.abs(ref["p"]).max(), np.abs(ref["a"]).max())
    ev = max(rel(state[k], ref[k], scale) for k in FIELDS)
    print(f"single crystal parity {tag}: stress {es:.3e} (bound {BOUND['stress']:.1e}) tangent {et:.3e} ({BOUND['tangent']:.1e}) state {ev:.3e} ({BOUND['state']:.1e})")
    assert es <= BOUND["stress"] and et <= BOUND["tangent"] and ev <= BOUND["state"], (tag, es, et, ev)


def check_stats(st, ref, n):
    assert st["n_points"] == n and st["n_nan"] == 0
    assert st["n_plastic"] == int(ref["plastic"].sum())
    assert st["n_not_converged"] == int((ref["status"] != 0).sum())
    # the stopping rule is an absolute 1e-14 on the slip residuals: a residual that lands on it may take one pass more or less
    assert abs(st["max_local_iters"] - int(ref["iters"].max(initial=0))) <= 1, (st, int(ref["iters"].max(initial=0)))


@pytest.fixture(scope="module")
def pool():
    return make_pool()


def make_pool():
    """POOL points with random frames: the state after 14 increments of norm 1e-4 and the 15th strain (yielded), and the same
    directions at 2e-4 from the virgin state (elastic).  Computed once, never changed."""
    rng = np.random.default_rng(77)
    M = 2 * POOL   # candidates: kept are the first POOL that have yielded at the 15th strain and are elastic at 2e-4 from the virgin state
    d = rng.normal(size=(M, 6)) * np.array([1, 1, 1, 0.7, 0.7, 0.7])
    d[np.arange(M), np.arange(M) % 3] += 1.5
    d /= np.linalg.norm(d, axis=1)[:, None]
    R = np.array([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(M)])
    st = sc.zero_state(M)
    for k in range(1, 15):
        out = sc.update(k * 1e-4 * d, st, PRM, DT, R=R)
        assert (out["status"] == 0).all()
        st = sc.next_state(out)
    keep = sc.update(15e-4 * d, st, PRM, DT, R=R)["plastic"] & ~sc.update(2e-4 * d, sc.zero_state(M), PRM, DT, R=R)["plastic"]
    keep = np.nonzero(keep)[0][:POOL]
    assert keep.size == POOL
    d, R, st = d[keep], R[keep], {k: v[keep] for k, v in st.items()}
    return {"d": d, "R": R, "state": st}


def case(pool, n, yielded):
    """n points drawn from the pool in order; yielded[i] says whether point i carries its history and the 15th strain, or is virgin
    at 2e-4.  Returns eps, R, state, and the restatement's answer."""
    idx = np.arange(n) % POOL
    y = np.asarray(yielded, dtype=bool)
    eps = np.where(y[:, None], 15e-4, 2e-4) * pool["d"][idx]
    R = pool["R"][idx]
    state = {k: np.where(y[:, None], v[idx], 0.0) for k, v in pool["state"].items()}
    P = 3 * POOL   # the period of the inputs when the pattern of `yielded` has period 3: the restatement is evaluated once per period
    if n > P and (y == y[np.arange(n) % P]).all():
        one = sc.update(eps[:P], {k: v[:P] for k, v in state.items()}, PRM, DT, R=R[:P])
        ref = {k: v[np.arange(n) % P] for k, v in one.items()}
    else:
        ref = sc.update(eps, state, PRM, DT, R=R)
    assert (ref["status"] == 0).all() and (ref["plastic"] == y).all()
    return eps, R, state, ref


def run(h, eps, state):
    h.set_state(state)
    S, T, st = h.device(to_device(eps))
    return S, T, h.get_state(), st


def test_fixture_histories_match_their_50_digit_values():
    """every fixture point from its recorded state: per parameter set and frame class one handle (none / uniform / field)"""
    for si, prm in enumerate(GOLD["params"]):
        for fi, fcls in enumerate(META["frames"]):
            m = (GOLD["set"] == si) & (GOLD["frame"] == fi)
            n = int(m.sum())
            h = Handle(prm, n)
            if fcls == "random":
                h.frame(GOLD["R"][m])
            elif fcls != "none":
                h.frame(GOLD["R"][m][0])
            state = {"eel": GOLD["eel0"][m], "g": GOLD["g0"][m], "p": GOLD["p0"][m], "a": GOLD["a0"][m]}
            S, T, new, st = run(h, GOLD["eps"][m], state)
            ref = {k: GOLD[k][m] for k in ("stress", "tangent", "eel", "g", "p", "a")}
            check(f"golden set {si} frame {fcls}", S, T, new, ref)
            assert st["n_plastic"] == int(GOLD["plastic"][m].sum()) and st["n_not_converged"] == 0 and st["n_nan"] == 0 and st["n_points"] == n
            # iterations: the recorded count of the restatement, but for a residual that lands on the absolute 1e-14 of the stopping rule
            assert abs(st["max_local_iters"] - int(GOLD["iters"][m].max())) <= 1, (st, int(GOLD["iters"][m].max()))
            # replayed once more from the accepted state: advance, then the same strain again changes little and stays finite
            assert h.lib.dxm_advance(h.h) == 0
            S2, T2, st2 = h.device(to_device(GOLD["eps"][m]))
            assert np.isfinite(S2).all() and np.isfinite(T2).all() and st2["n_not_converged"] == 0
            h.close()


def test_the_fixture_tangent_is_not_symmetric():
    T = GOLD["tangent"]
    assert np.abs(T - T.transpose(0, 2, 1)).max() / np.abs(T).max() > 1e-8


@pytest.mark.parametrize("N", [1, 3, 4, 5, 63, 64, 65, 257])
def test_sizes_with_a_frame_field(pool, N):
    eps, R, state, ref = case(pool, N, np.arange(N) % 3 != 1)
    h = Handle(PRM, N).frame(R)
    S, T, new, st = run(h, eps, state)
    check(f"N={N}", S, T, new, ref)
    check_stats(st, ref, N)
    assert h.lib.dxm_kernel_name(h.h) == b"single_crystal_kernel<2" and h.lib.dxm_algorithmic_bytes(h.h) == 1008 + 72
    h.close()


def test_size_100003_with_a_frame_field(big):
    check(f"N={NBIG}", big["S"], big["T"], big["new"], big["ref"])
    check_stats(big["st"], big["ref"], NBIG)


TILES = {
    "wholly elastic": lambda i: np.zeros_like(i, dtype=bool),
    "one yielded point": lambda i: i == 37,
    "five yielded points: a ragged second round": lambda i: np.isin(i, (3, 17, 18, 40, 63)),
    "all 64 yielded": lambda i: i < 64,
    "a yielded point in the ragged last tile": lambda i: i == 66,
}


@pytest.mark.parametrize("name", list(TILES))
def test_tiles_by_construction(pool, name):
    N = 64 + 7
    eps, R, state, ref = case(pool, N, TILES[name](np.arange(N)))
    h = Handle(PRM, N).frame(R)
    S, T, new, st = run(h, eps, state)
    check(name, S, T, new, ref)
    check_stats(st, ref, N)
    el = ~ref["plastic"]
    # elastic points: the state slots keep the bits that were read, the tangent is Q^T D Q
    for k in ("g", "p", "a"):
        assert np.array_equal(new[k][el], state[k][el])
    h.close()


def frame_history(pool, N, y, eps, R):
    """the state the points marked y reach under ONE frame for all (the history belongs to its frame), and the restatement's answer"""
    idx = np.arange(N) % POOL
    st0 = sc.zero_state(N)
    for k in range(1, 15):
        out = sc.update(np.where(y[:, None], k * 1e-4, 0.0) * pool["d"][idx], st0, PRM, DT, R=R)
        assert (out["status"] == 0).all()
        st0 = sc.next_state(out)
    ref = sc.update(eps, st0, PRM, DT, R=R)
    assert (ref["status"] == 0).all()
    return st0, ref


def test_the_three_frame_states(pool):
    N = 257
    y = np.arange(N) % 2 == 0
    Ru = pool["R"][5]
    idx = np.arange(N) % POOL
    eps = np.where(y[:, None], 15e-4, 2e-4) * pool["d"][idx]
    st0, ref = frame_history(pool, N, y, eps, Ru)
    hu = Handle(PRM, N).frame(Ru)
    Su, Tu, newu, stu = run(hu, eps, st0)
    check("uniform frame", Su, Tu, newu, ref)
    assert hu.lib.dxm_kernel_name(hu.h) == b"single_crystal_kernel<1" and hu.lib.dxm_algorithmic_bytes(hu.h) == 1008
    hf = Handle(PRM, N).frame(np.broadcast_to(Ru, (N, 3, 3)))
    Sf, Tf, newf, stf = run(hf, eps, st0)
    assert np.array_equal(Sf, Su) and np.array_equal(Tf, Tu) and stf == stu     # a constant field: the bits of the uniform frame
    for k in FIELDS:
        assert np.array_equal(newf[k], newu[k])
    # the identity frame against no frame, to the bound
    stn0, refn = frame_history(pool, N, y, eps, None)
    hn = Handle(PRM, N)
    Sn, Tn, newn, stn = run(hn, eps, stn0)
    check("no frame", Sn, Tn, newn, refn)
    assert hn.lib.dxm_kernel_name(hn.h) == b"single_crystal_kernel<0"
    hi = Handle(PRM, N).frame(np.eye(3))
    Si, Ti, newi, sti = run(hi, eps, stn0)
    check("identity frame", Si, Ti, newi, refn)
    for h in (hu, hf, hn, hi):
        h.close()


@pytest.fixture(scope="module")
def big(pool):
    eps, R, state, ref = case(pool, NBIG, np.arange(NBIG) % 3 != 1)
    h = Handle(PRM, NBIG).frame(R)
    S, T, new, st = run(h, eps, state)
    h.close()
    return {"eps": eps, "R": R, "state": state, "S": S, "T": T, "new": new, "st": st, "ref": ref}


def test_one_workgroup_per_cu_equals_the_shipped_grid(pool):
    N = 206_147
    idx = np.arange(N) % POOL
    y = np.arange(N) % 3 != 1
    eps = np.where(y[:, None], 15e-4, 2e-4) * pool["d"][idx]
    state = {k: np.where(y[:, None], v[idx], 0.0) for k, v in pool["state"].items()}
    R = pool["R"][idx]
    out = []
    for bpc in (None, 1):
        h = Handle(PRM, N).frame(R)
        if bpc:
            h.option("blocks_per_cu", bpc)
        out.append(run(h, eps, state))
        h.close()
    (S0, T0, n0, st0), (S1, T1, n1, st1) = out
    assert np.array_equal(S0, S1) and np.array_equal(T0, T1) and st0 == st1
    for k in FIELDS:
        assert np.array_equal(n0[k], n1[k])
    assert st0["n_plastic"] == int(y.sum()) and st0["n_not_converged"] == 0 and st0["n_nan"] == 0


def test_host_buffer_form_in_chunks_and_in_one(big):
    h = Handle(PRM, NBIG).frame(big["R"])
    isv_ref = np.concatenate([big["new"][k] for k in FIELDS], axis=1)
    for chunks in (64, 3, 1):
        h.set_state(big["state"])
        h.option("max_chunks", chunks)
        S, T, isv, st = h.host(big["eps"])
        assert np.array_equal(S, big["S"]) and np.array_equal(T, big["T"]) and np.array_equal(isv, isv_ref), chunks
        assert st == big["st"], chunks
    h.close()


def test_rows_form(big):
    rows = np.ascontiguousarray(2 * np.arange(NBIG), dtype=np.int64)
    h = Handle(PRM, NBIG).frame(big["R"]).set_state(big["state"])
    flux, ct, st = np.full((2 * NBIG, 6), -7.0), np.full((2 * NBIG, 36), -9.0), _lib.Stats()
    eps = big["eps"]
    assert h.lib.dxm_integrate_rows(h.h, eps.ctypes.data, DT, flux.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)) >= 0, err(h.lib)
    assert np.array_equal(flux[rows], big["S"]) and np.array_equal(ct[rows], big["T"])
    assert np.all(flux[1::2] == -7.0) and np.all(ct[1::2] == -9.0) and st.as_dict() == big["st"]
    h.close()


def test_device_pointer_form_on_a_stream(big):
    import torch

    h = Handle(PRM, NBIG).frame(big["R"]).set_state(big["state"])
    s = torch.cuda.Stream()
    eps_dev = to_device(big["eps"])
    with torch.cuda.stream(s):
        S, T, st = h.device(eps_dev, stream=s.cuda_stream)
    assert np.array_equal(S, big["S"]) and np.array_equal(T, big["T"]) and st == big["st"]
    h.close()


def test_dt_travels_and_dt_zero_is_the_elastic_response(pool):
    N = 65
    eps, R, state, ref = case(pool, N, np.ones(N, dtype=bool))
    h = Handle(PRM, N).frame(R).set_state(state)
    S, T, st = h.device(to_device(eps), dt=0.0)
    ref0 = sc.update(eps, state, PRM, 0.0, R=R)
    check("dt = 0", S, T, h.get_state(), ref0)
    D = sc.stiffness(PRM)
    Q = sc.mandel_rotation(R)
    assert rel(T.reshape(N, 6, 6), np.einsum("nri,rs,nsk->nik", Q, D, Q)) <= BOUND["tangent"]
    S2, T2, _ = h.device(to_device(eps), dt=0.05)
    check("dt = 0.05", S2, T2, h.get_state(), sc.update(eps, state, PRM, 0.05, R=R))
    for bad in (-1.0, float("nan"), float("inf")):
        import torch

        f = torch.zeros((N, 6), dtype=torch.float64, device="cuda")
        c = torch.zeros((N, 36), dtype=torch.float64, device="cuda")
        assert h.lib.dxm_integrate_device(h.h, to_device(eps).data_ptr(), bad, f.data_ptr(), c.data_ptr(), None) == -1
        assert "dt must be finite and >= 0" in err(h.lib)
    h.close()


def test_guard_at_the_first_evaluation_leaves_the_state_bits(pool):
    """one point jumps by 5e-3 from a state with slip: f_trial > 1.1 K at dg = 0, MFront fails the integration there"""
    N = 65
    eps, R, state, ref = case(pool, N, np.ones(N, dtype=bool))
    bad = 41
    eps[bad] = 65e-4 * pool["d"][bad]
    state["eel"] = np.random.default_rng(3).normal(size=(N, 6)) * 1e-4     # written by every update, read by none
    ref = sc.update(eps, state, PRM, DT, R=R)
    assert ref["status"][bad] == 2 and (np.delete(ref["status"], bad) == 0).all()
    h = Handle(PRM, N).frame(R)
    S, T, new, st = run(h, eps, state)
    check("guard", S, T, new, ref)
    for k in FIELDS:
        assert np.array_equal(new[k][bad], state[k][bad]), k
    D, Q = sc.stiffness(PRM), sc.mandel_rotation(R[bad])[0]
    assert rel(T[bad].reshape(6, 6), Q.T @ D @ Q) <= BOUND["tangent"]
    assert st["n_not_converged"] == 1 and st["n_plastic"] == N and st["n_nan"] == 0
    h.close()


def test_law_table_row_and_refusals():
    lib = _lib.load()
    info = _lib.law_info(LAW)
    assert (info.n_grad, info.n_flux, info.n_params, info.n_isv_fields, info.n_isv_total, info.algorithmic_bytes_per_point) == (6, 6, 22, 4, 42, 1008)
    h = Handle(PRM, 5)
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h.h, layout) == -1 and "not symmetric" in err(lib)
    assert lib.dxm_tangent_size(h.h) == 36
    h.close()
    for k, v, word in ((9, 0.5, "n must be >= 1"), (10, 0.0, "K must be > 0"), (11, -1.0, "tau0"), (13, -1.0, "b must"), (14, -1.0, "d must"),
                       (15, -1.0, "C must"), (12, float("nan"), "Q must be finite"), (0, -1.0, "E1")):
        p = PRM.copy()
        p[k] = v
        assert not lib.dxm_create(LAW, (C.c_double * 22)(*p), 22, 4, 0)
        assert word in err(lib), (k, err(lib))
