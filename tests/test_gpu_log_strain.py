"""GPU: logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_J2, ``log_strain_kernel``) through ``HIPMaterial`` (ctypes -> C ABI)
against the numpy restatement ``log_strain_ref.update`` over two increments (the second from the non-coaxial history the first one
left), against the eigen-free mpmath vectors directly, a uniaxial known answer that bypasses both, the tile loop beyond its first
pass, the routes of the library against each other bit for bit, the update protocol, and two accelerated field maps on disjoint
cell subsets against one map over all cells.

Measured on an MI355X (scaled as ``log_strain_ref.scaled_errors``; BOUND = 3.2e-12): see DESIGN.md, section "Logarithmic-strain J2
plasticity"."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial

import log_strain_ref as ls
import tile_loop_cases as tc
from helpers import to_device, to_host
from test_log_strain_cpu import BOUND, PARITY_SIZES

pytestmark = pytest.mark.gpu

PRM = ls.PRM
FIELD_DIMS = (6, 1, 6)      # ElasticStrain, EquivalentPlasticStrain, the hidden PlasticStrain


def material(N, **kw):
    m = JAXMaterial(jm.LogarithmicStrainPlasticity(PRM["s0"], PRM["H0"], E=PRM["E"], nu=PRM["nu"]), lazy_isv=False, **kw)
    m.set_data_manager(N)
    return m


def state_of(m, which=_lib.S1):
    """Every state field (the hidden one included), through dxm_get_state."""
    out = []
    for f, dim in enumerate(FIELD_DIMS):
        a = np.empty((m._n, dim))
        m._chk(m._lib.dxm_get_state(m._require(), which, f, a.ctypes.data))
        out.append(a)
    return out


def check(tag, P, A, m, ref, keep=None):
    eel, p, Ep = state_of(m)
    got = dict(P=np.asarray(P), A=np.asarray(A).reshape(len(ref["P"]), 9, 9), eel=eel, p=p[:, 0], Ep=Ep)
    keep = ~ref["skip"] if keep is None else keep
    e = ls.scaled_errors(got, ref, keep=keep)
    print(f"log-strain parity {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()) + f" (bound {BOUND:.1e})")
    assert max(e.values()) <= BOUND, e
    return got


@pytest.mark.parametrize("N", PARITY_SIZES)
def test_update_matches_the_reference_over_two_increments(N):
    incs = ls.two_increments(N, seed=N)
    refs = ls.reference_path(incs)
    m = material(N)
    assert m.kernel_name.startswith("log_strain_kernel")
    assert m.internal_state_variables == {"ElasticStrain": 6, "EquivalentPlasticStrain": 1}
    for k, (F, ref) in enumerate(zip(incs, refs)):
        if k:
            m.data_manager.update()
        P, isv, A = m.integrate(F)
        st = m.last_stats
        assert st["n_nan"] == 0 and st["n_not_converged"] == 0 and st["n_points"] == N
        assert abs(st["n_plastic"] - int(ref["plastic"].sum())) <= int(ref["skip"].sum())
        got = check(f"N={N} increment {k + 1}", P, A, m, ref)
        assert np.array_equal(np.asarray(isv)[:, :6], got["eel"]) and np.array_equal(np.asarray(isv)[:, 6], got["p"])
    m.close()


def test_degenerate_set_matches_mpmath_directly():
    F, labels, sets = ls.load_golden()
    n = len(F)
    for name, Ep, p, g in sets:
        m = material(n)
        m._set_state(1, np.ascontiguousarray(p.reshape(n, 1)))
        m._set_state(2, np.ascontiguousarray(Ep))
        P, isv, A = m.integrate(F)
        assert np.isfinite(np.asarray(A)).all() and m.last_stats["n_nan"] == 0
        assert m.last_stats["n_plastic"] == int(g["plastic"].sum())
        check(f"vs mpmath, {name} state", P, A, m, g, keep=np.ones(n, dtype=bool))
        m.close()


@pytest.mark.parametrize("lam", [0.999, 1.0005, 1.05, 1.3])
def test_uniaxial_known_answer(lam):
    """F = diag(lam, lt, lt) under uniaxial stress T11: before yield T11 = E ln lam; past it the axial plastic strain is p, so
    ln lam = T11 / E + p and T11 = s0 + H0 p give T11 = (s0 + H0 ln lam) / (1 + H0 / E); ln lt = -nu T11 / E - p / 2.  The path is
    proportional in the logarithmic strain, so the one-step radial return is exact: P11 = T11 / lam, no lateral stress."""
    E, nu, s0, H0 = (PRM[k] for k in ("E", "nu", "s0", "H0"))
    le = np.log(lam)
    T11 = E * le
    p = 0.0
    if abs(T11) > s0:
        assert le > 0.0
        T11 = (s0 + H0 * le) / (1.0 + H0 / E)
        p = le - T11 / E
    lt = np.exp(-nu * T11 / E - 0.5 * p)
    F = np.tile(np.array([lam, lt, lt, 0, 0, 0, 0, 0, 0.0]), (64, 1))
    m = material(64)
    P, isv, A = m.integrate(F)
    P, isv = np.array(P), np.array(isv)
    assert np.all(P == P[0]) and np.isfinite(np.array(A)).all() and m.last_stats["n_nan"] == 0
    assert m.last_stats["n_plastic"] == (64 if p > 0.0 else 0)
    print(f"uniaxial lam={lam}: P11 {P[0, 0]:.12e} expected {T11 / lam:.12e} lateral {P[0, 1]:.3e} p {isv[0, 6]:.6e} expected {p:.6e}")
    assert abs(P[0, 0] - T11 / lam) <= BOUND * max(abs(T11 / lam), s0)
    assert abs(P[0, 1]) <= BOUND * s0 and P[0, 1] == P[0, 2] and not P[0, 3:].any()
    assert abs(isv[0, 6] - p) <= BOUND * max(p, s0 / E)
    m.close()


@pytest.fixture(scope="module")
def cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_tile_loop_past_the_first_pass(cu):
    """One workgroup per compute unit (option blocks_per_cu = 1): three full passes and a ragged fourth.  Parity on the sample of
    the late passes over two increments; then the second increment again with NaN gradients at three points: counted, and no other
    point disturbed."""
    import torch

    N = tc.size_for(cu)
    assert tc.passes(N, cu, 1) == 4
    incs = ls.two_increments(N, seed=77)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    refs = ls.reference_path(incs, sample)
    Ep, p = ls.natural_state(N)
    for k, F in enumerate(incs):        # the plastic share of every pass, over all points
        b = ls.branch(F, Ep, p)
        shares = tc.share_per_pass(b["plastic"], cu)
        print(f"log-strain tile loop increment {k + 1}: plastic share per pass {[round(s, 3) for s in shares]}")
        assert len(shares) == 4 and all(tc.SHARE[0] <= s <= tc.SHARE[1] for s in shares), shares
        assert abs(int(b["plastic"].sum())) > 0
        Ep, p = b["Ep"], b["p"]
    m = material(N)
    m.set_option("blocks_per_cu", 1)
    f = torch.zeros((N, 9), dtype=torch.float64, device="cuda:0")
    c = torch.zeros((N, 81), dtype=torch.float64, device="cuda:0")

    def launch(F):
        g = to_device(np.array(F))
        m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr())
        torch.cuda.synchronize()
        rc, st = m.stats()
        assert rc >= 0
        return to_host(f), to_host(c), state_of(m), st

    for k, (F, ref) in enumerate(zip(incs, refs)):
        if k:
            m.data_manager.update()
        P, A, state, st = launch(F)
        assert st["n_nan"] == 0 and st["n_points"] == N
        got = dict(P=P[sample], A=A[sample].reshape(-1, 9, 9), eel=state[0][sample], p=state[1][sample, 0], Ep=state[2][sample])
        e = ls.scaled_errors(got, ref, keep=~ref["skip"])
        print(f"log-strain tile loop parity increment {k + 1} ({len(sample)} points): " + " ".join(f"{q} {v:.3e}" for q, v in e.items()))
        assert max(e.values()) <= BOUND, e
    poisoned = np.array(incs[1])
    poisoned[bad, 0] = np.nan
    poisoned[bad[1], 4] = np.nan
    P2, A2, state2, st2 = launch(poisoned)
    assert st2["n_nan"] == len(bad), st2
    rest = np.setdiff1d(np.arange(N), bad)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)   # noqa: E731
    assert np.array_equal(bits(P2[rest]), bits(P[rest])) and np.array_equal(bits(A2[rest]), bits(A[rest]))
    for x, y in zip(state2, state):
        assert np.array_equal(bits(x[rest]), bits(y[rest]))
    assert np.isnan(P2[bad]).all() and np.isnan(A2[bad]).all() and all(np.isnan(x[bad]).all() for x in state2)
    m.close()


def test_inverted_and_flat_points_are_counted_not_fatal():
    N = 130
    F = ls.random_F(N, seed=9)
    F[[3, 64, 129], 2] *= -1.0          # det F < 0
    F[70] = 0.0                         # det F = 0
    m = material(N)
    P, isv, A = m.integrate(F)
    assert m.last_stats["n_nan"] == 4
    bad = np.array([3, 64, 70, 129])
    assert np.isnan(np.array(P)[bad]).all() and np.isnan(np.array(A).reshape(N, 81)[bad]).all() and np.isnan(np.array(isv)[bad]).all()
    rest = np.setdiff1d(np.arange(N), bad)
    assert np.isfinite(np.array(P)[rest]).all() and np.isfinite(np.array(A).reshape(N, 81)[rest]).all()
    m.close()


def test_routes_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    N = 100_003
    F1, F2 = ls.two_increments(N, seed=4)
    m = material(N)
    m.integrate(F1)
    m.data_manager.update()             # the routes below all start from this history
    P, isv, A = m.integrate(F2)
    P, isv, A = np.array(P), np.array(isv), np.array(A).reshape(N, 81)
    hidden = state_of(m)[2]
    dev = torch.device("cuda:0")
    g = to_device(F2)
    f = torch.empty((N, 9), dtype=torch.float64, device=dev)
    c = torch.empty((N, 81), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(f), P) and np.array_equal(to_host(c), A)
    st = state_of(m)
    assert np.array_equal(st[0], isv[:, :6]) and np.array_equal(st[1][:, 0], isv[:, 6]) and np.array_equal(st[2], hidden)
    # option packed_transfer has nothing to pack for this law: same bytes either way
    m.set_option("packed_transfer", 0)
    P0, _, A0 = m.integrate(F2)
    assert np.array_equal(np.array(P0), P) and np.array_equal(np.array(A0).reshape(N, 81), A)
    m.set_option("packed_transfer", 2)
    # rows mode over a permuted subset: the named rows get the values, the others stay as they were
    M = N + 500
    rng = np.random.default_rng(0)
    rows = np.ascontiguousarray(rng.permutation(M)[:N], dtype=np.int64)
    flux = np.full((M, 9), -7.0)
    tang = np.full((M, 81), -9.0)
    m.integrate_rows(F2, rows, flux, tang)
    assert np.array_equal(flux[rows], P) and np.array_equal(tang[rows], A)
    rest = np.setdiff1d(np.arange(M), rows)
    assert np.all(flux[rest] == -7.0) and np.all(tang[rest] == -9.0)
    assert np.array_equal(state_of(m)[2], hidden)
    m.close()


def test_refusals_on_the_handle():
    lib = _lib.load()
    prm = (C.c_double * 4)(PRM["E"], PRM["nu"], PRM["s0"], PRM["H0"])
    h = lib.dxm_create(_lib.LAW_LOG_STRAIN_J2, prm, 4, 64, 0)
    assert h
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h, layout) < 0 and b"no packed tangent record" in lib.dxm_last_error()
    assert lib.dxm_tangent_size(h) == 81
    for bad, word in (((PRM["E"], PRM["nu"], 0.0, 1e6), b"s0"), ((PRM["E"], PRM["nu"], 250e6, -1.0), b"H0"), ((0.0, 0.3, 250e6, 1e6), b"elastic constants"),
                      ((PRM["E"], 0.5, 250e6, 1e6), b"elastic constants"), ((PRM["E"], 0.3, float("nan"), 1e6), b"finite")):
        assert lib.dxm_set_params(h, (C.c_double * 4)(*bad), 4) < 0 and word in lib.dxm_last_error(), bad
    assert lib.dxm_set_param_field(h, 2, None) < 0 and b"logarithmic-strain plasticity" in lib.dxm_last_error()
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert lib.dxm_set_frame(h, eye) < 0 and b"isotropic" in lib.dxm_last_error()
    lib.dxm_destroy(h)
    assert not lib.dxm_create(_lib.LAW_LOG_STRAIN_J2, prm, 3, 64, 0)
    with pytest.raises(ValueError, match="no packed tangent record"):
        JAXMaterial(jm.LogarithmicStrainPlasticity(250e6, 1e6), tangent_layout="sym")


def test_protocol_integrate_advance_revert_and_explicit_state():
    N = 257
    Fa, Fb = ls.two_increments(N, seed=12)
    ra = ls.update(Fa, *ls.natural_state(N))
    rb = ls.update(Fb, ra["Ep"], ra["p"])
    m = material(N)
    assert not np.array(m.get_initial_state_dict()["ElasticStrain"]).any()
    for F in (Fb, Fa, Fa):                      # k updates from one initial state: the last one counts
        P, isv, A = m.integrate(F)
    ia = np.array(isv)
    check("protocol, first increment", P, A, m, ra)
    assert not np.array(m.get_initial_state_dict()["EquivalentPlasticStrain"]).any() and not state_of(m, _lib.S0)[2].any()
    assert np.array_equal(np.array(m.get_final_state_dict()["ElasticStrain"]), ia[:, :6])
    m.data_manager.revert()
    assert not np.array(m.get_final_state_dict()["ElasticStrain"]).any() and not state_of(m)[2].any()
    m.integrate(Fa)
    m.data_manager.update()
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.array(s0["ElasticStrain"]), ia[:, :6]) and np.array_equal(np.array(s0["EquivalentPlasticStrain"])[:, 0], ia[:, 6])
    assert np.array_equal(np.array(s0["DeformationGradient"]), Fa)
    Pb, isvb, Ab = m.integrate(Fb)              # the state is read: the update from the advanced state is the second increment
    check("protocol, second increment", Pb, Ab, m, rb)
    assert np.array_equal(np.array(m.get_initial_state_dict()["ElasticStrain"]), ia[:, :6])
    # explicit state in, explicit state out: the hidden field is rebuilt from (F_n, ElasticStrain_n), to rounding
    Ct, new = m.batched_constitutive_update(Fb, {k: s0[k] for k in ("DeformationGradient", "ElasticStrain", "EquivalentPlasticStrain")})
    got = dict(P=new["FirstPiolaKirchhoffStress"], A=np.asarray(Ct), eel=new["ElasticStrain"], p=new["EquivalentPlasticStrain"][:, 0], Ep=rb["Ep"])
    e = ls.scaled_errors(got, rb, keep=~rb["skip"])
    assert max(e.values()) <= BOUND, e
    # and an initial state set field by field drives the next update
    m.set_initial_state_dict({"DeformationGradient": Fa, "ElasticStrain": ia[:, :6], "EquivalentPlasticStrain": ia[:, 6:]})
    P3, _, A3 = m.integrate(Fb)
    check("protocol, state set by hand", P3, A3, m, rb)
    m.close()


@pytest.mark.parametrize("ncell,nqp", [(41, 4), (3001, 8)])
def test_two_maps_on_disjoint_cells_equal_one_map_over_all(ncell, nqp):
    """The reference's test_multimaterials property on the new law, through the accelerated field map (rows forms for the subsets)."""
    n = ncell * nqp
    rng = np.random.default_rng(2)
    perm = rng.permutation(ncell)
    parts = [np.sort(perm[: ncell // 3]).astype(np.int32), np.sort(perm[ncell // 3:]).astype(np.int32)]
    hist = list(ls.two_increments(n, seed=31))
    now = {"g": np.tile(ls.spliced(1, 0), (n, 1))}     # the state is initialised at F = I, as the demo's is
    ev = lambda c: now["g"].reshape(ncell, nqp, 9)[c].reshape(-1, 9)   # noqa: E731
    beh = lambda: jm.LogarithmicStrainPlasticity(PRM["s0"], PRM["H0"])   # noqa: E731
    whole = QuadratureFieldMap(ncell, nqp, JAXMaterial(beh()))
    subs = [QuadratureFieldMap(ncell, nqp, JAXMaterial(beh()), cells=c) for c in parts]
    for q in [whole] + subs:
        q.register_gradient("DeformationGradient", ev)
        q.initialize_state()
    fields = lambda q: {"flux": q.fluxes["FirstPiolaKirchhoffStress"].x.array, "eel": q.internal_state_variables["ElasticStrain"].x.array,   # noqa: E731
                        "p": q.internal_state_variables["EquivalentPlasticStrain"].x.array, "jac": q.jacobian_flatten.x.array}
    width = {"flux": 9, "eel": 6, "p": 1, "jac": 81}
    for k, g in enumerate(hist):
        now["g"] = g
        for q in [whole] + subs:
            q.update()
            q.advance()
        for name, w in width.items():
            want = fields(whole)[name].reshape(n, w)
            assert want.any()
            for q, cells in zip(subs, parts):
                got = fields(q)[name].reshape(n, w)
                rows = (cells[:, None] * nqp + np.arange(nqp)[None]).ravel()
                assert np.array_equal(got[rows], want[rows]), (name, k)
                rest = np.setdiff1d(np.arange(n), rows)
                assert not got[rest].any(), name          # the other cells' rows are not this map's to write
    assert np.array(fields(whole)["p"]).max() > 0.0     # the second increment started from a plastic history
    for q in [whole] + subs:
        q.close()
        q.material.close()
