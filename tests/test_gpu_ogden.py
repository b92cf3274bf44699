"""GPU: the Ogden hyperelastic law (DXM_LAW_OGDEN, ``ogden_kernel``) through ``HIPMaterial`` (ctypes -> C ABI) against the numpy
closed form ``ogden_ref.closed_form`` on the input families of ``test_ogden_cpu.py``, the routes of the library against each other
bit for bit, the update protocol, a uniaxial stretch solved independently on the CPU, and two accelerated field maps on disjoint
cell subsets against one map over all cells."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial

import ogden_ref as og
from helpers import to_device, to_host
from test_ogden_cpu import E0

pytestmark = pytest.mark.gpu

# The parity bound: 16 x the error floor E0 of the closed form itself (measured on the CPU against mpmath and AD,
# test_ogden_cpu.py) -- the factor covers the device's exp / log differing from libm by a few ulp, amplified by the exponent
# a = alpha / 2 ~ 14, which E0 already carries for libm -- and never looser than the 1e-11 of the FeFp parity tests.
FEFP_BOUND = 1e-11
BOUND = min(16 * E0, FEFP_BOUND)
EYE9 = np.array([1.0, 1, 1, 0, 0, 0, 0, 0, 0])


def inputs(N, seed):
    """N rows: the random family F = I + 0.2 U(-1/2, 1/2) with the degenerate set and F = I spliced in at the front."""
    F = og.random_F(N, seed=seed)
    deg, _ = og.degenerate_F()
    special = np.vstack([EYE9[None], deg])
    k = min(N, len(special))
    F[:k] = special[:k]
    return F


def check(P, A, isv, F, prm):
    Pr, Ar, ir = og.closed_form(F, **prm)
    n = len(F)
    eP = og.row_errors(np.asarray(P)[:, None, :], Pr[:, None, :]).max()
    eA = og.row_errors(np.asarray(A).reshape(n, 9, 9), Ar).max()
    scale = np.maximum(np.abs(ir).max(axis=1), np.abs(Pr).max(axis=1))
    scale = np.where(scale > 0.0, scale, 1.0)
    eI = (np.abs(np.asarray(isv) - ir).max(axis=1) / scale).max()
    print(f"ogden parity N={n} alpha={prm['alpha']}: P {eP:.3e} A {eA:.3e} PK2Stress {eI:.3e} (bound {BOUND:.1e})")
    assert eP <= BOUND and eA <= BOUND and eI <= BOUND, (eP, eA, eI)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 320_000])
@pytest.mark.parametrize("k", range(len(og.PARAM_SETS)))
def test_update_matches_the_closed_form(N, k):
    prm = og.PARAM_SETS[k]
    F = inputs(N, seed=N + k)
    m = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
    m.set_data_manager(N)
    assert m.kernel_name.startswith("ogden_kernel") and m.internal_state_variables == {"PK2Stress": 6}
    P, isv, A = m.integrate(F)
    st = m.last_stats
    assert st["n_nan"] == 0 and st["n_plastic"] == 0 and st["n_not_converged"] == 0
    check(P, A, isv, F, prm)
    m.close()


def test_degenerate_set_matches_mpmath_directly():
    F, labels, sets = og.load_golden()
    for prm, Pg, Ag, ig in sets:
        m = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
        m.set_data_manager(len(F))
        P, isv, A = m.integrate(F)
        eP = og.row_errors(np.asarray(P)[:, None, :], Pg[:, None, :]).max()
        eA = og.row_errors(np.asarray(A).reshape(-1, 9, 9), Ag).max()
        print(f"ogden vs mpmath alpha={prm['alpha']}: P {eP:.3e} A {eA:.3e}")
        assert eP <= BOUND and eA <= BOUND and np.isfinite(np.asarray(A)).all()
        m.close()


def test_inverted_points_are_counted_not_fatal():
    N = 130
    F = og.random_F(N, seed=9)
    F[[3, 64, 129], 2] *= -1.0          # det F < 0
    F[70] = 0.0                         # det F = 0
    m = JAXMaterial(jm.OgdenHyperelasticity())
    m.set_data_manager(N)
    m.integrate(F)
    assert m.last_stats["n_nan"] == 4
    m.close()


def test_routes_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    N = 100_003
    F = inputs(N, seed=4)
    m = JAXMaterial(jm.OgdenHyperelasticity(), lazy_isv=False)
    m.set_data_manager(N)
    P, isv, A = m.integrate(F)
    P, isv, A = np.array(P), np.array(isv), np.array(A).reshape(N, 81)
    dev = torch.device("cuda:0")
    g = to_device(F)
    f = torch.empty((N, 9), dtype=torch.float64, device=dev)
    c = torch.empty((N, 81), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(f), P) and np.array_equal(to_host(c), A)
    assert np.array_equal(np.array(m.get_final_state_dict()["PK2Stress"]), isv)
    # option packed_transfer has nothing to pack for this law: same bytes either way
    m.set_option("packed_transfer", 0)
    P0, _, A0 = m.integrate(F)
    assert np.array_equal(np.array(P0), P) and np.array_equal(np.array(A0).reshape(N, 81), A)
    m.set_option("packed_transfer", 2)
    # rows mode over a permuted subset: the named rows get the values, the others stay as they were
    M = N + 500
    rng = np.random.default_rng(0)
    rows = np.ascontiguousarray(rng.permutation(M)[:N], dtype=np.int64)
    flux = np.full((M, 9), -7.0)
    tang = np.full((M, 81), -9.0)
    m.integrate_rows(F, rows, flux, tang)
    assert np.array_equal(flux[rows], P) and np.array_equal(tang[rows], A)
    rest = np.setdiff1d(np.arange(M), rows)
    assert np.all(flux[rest] == -7.0) and np.all(tang[rest] == -9.0)
    m.close()


def test_refusals_on_the_handle():
    lib = _lib.load()
    prm = (C.c_double * 3)(28.8, 27778.0, 69444444.0)
    h = lib.dxm_create(_lib.LAW_OGDEN, prm, 3, 64, 0)
    assert h
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h, layout) < 0 and b"no packed tangent record" in lib.dxm_last_error()
    assert lib.dxm_tangent_size(h) == 81
    bad = (C.c_double * 3)(0.0, 27778.0, 69444444.0)
    assert lib.dxm_set_params(h, bad, 3) < 0 and b"alpha" in lib.dxm_last_error()
    assert lib.dxm_set_param_field(h, 1, None) < 0 and b"Ogden" in lib.dxm_last_error()
    lib.dxm_destroy(h)
    with pytest.raises(ValueError, match="no packed tangent record"):
        JAXMaterial(jm.OgdenHyperelasticity(), tangent_layout="sym")


def test_protocol_integrate_advance_revert_and_explicit_state():
    N = 257
    prm = og.DEFAULTS
    Fa, Fb = og.random_F(N, seed=1), og.random_F(N, seed=2)
    m = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
    m.set_data_manager(N)
    assert not np.array(m.get_initial_state_dict()["PK2Stress"]).any()
    for F in (Fb, Fa, Fa):                      # k updates from one initial state: the last one counts
        P, isv, A = m.integrate(F)
    ia = np.array(isv)
    assert not np.array(m.get_initial_state_dict()["PK2Stress"]).any()
    assert np.array_equal(np.array(m.get_final_state_dict()["PK2Stress"]), ia)
    m.data_manager.revert()
    assert not np.array(m.get_final_state_dict()["PK2Stress"]).any()
    m.integrate(Fa)
    m.data_manager.update()
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.array(s0["PK2Stress"]), ia) and np.array_equal(np.array(s0["DeformationGradient"]), Fa)
    Pb, isvb, _ = m.integrate(Fb)               # the state is never read: the update from the advanced state is that of a new handle
    check(Pb, m.integrate(Fb)[2], isvb, Fb, prm)
    assert np.array_equal(np.array(m.get_initial_state_dict()["PK2Stress"]), ia)
    # explicit state in, explicit state out
    Ct, new = m.batched_constitutive_update(Fb, m.natural_state(N))
    assert np.array_equal(np.array(new["FirstPiolaKirchhoffStress"]), np.array(Pb)) and np.array_equal(np.array(new["PK2Stress"]), np.array(isvb))
    assert np.asarray(Ct).reshape(N, 81).shape == (N, 81)
    m.close()


@pytest.mark.parametrize("lam", [0.7, 1.0, 1.3, 2.0])
def test_uniaxial_stretch_against_the_reduced_energy(lam):
    """F = diag(lam, lt, lt) with lt solved for zero lateral stress on the energy alone (mpmath root-find): the exactly
    degenerate case an FE run meets.  The kernel's P11 must be dW_reduced/dlam, its lateral stress zero."""
    prm = og.DEFAULTS
    lt, P11 = og.uniaxial_reference(lam, **prm)
    F = np.tile(np.array([lam, lt, lt, 0, 0, 0, 0, 0, 0.0]), (64, 1))
    m = JAXMaterial(jm.OgdenHyperelasticity(**prm))
    m.set_data_manager(64)
    P, _, A = m.integrate(F)
    P, A = np.array(P), np.array(A).reshape(64, 9, 9)
    assert np.all(P == P[0]) and np.isfinite(A).all() and m.last_stats["n_nan"] == 0
    scale = max(abs(P11), prm["K"] * abs(lam * lt * lt - 1.0))      # the stress is a difference of parts of this size
    print(f"uniaxial lam={lam}: P11 {P[0, 0]:.12e} reference {P11:.12e} lateral {P[0, 1]:.3e}")
    assert abs(P[0, 0] - P11) <= BOUND * max(scale, prm["mu"])
    # lt is the root rounded to a double: the lateral stress is what that rounding leaves, dP22/dlt * ulp(lt)
    assert abs(P[0, 1]) <= 4 * np.finfo(float).eps * lt * (abs(A[0, 1, 1]) + abs(A[0, 1, 2])) + BOUND * max(scale, prm["mu"])
    assert P[0, 1] == P[0, 2] and not P[0, 3:].any()
    m.close()


@pytest.mark.parametrize("ncell,nqp", [(41, 4), (6001, 8)])
def test_two_maps_on_disjoint_cells_equal_one_map_over_all(ncell, nqp):
    """The reference's test_multimaterials property on the new law, through the accelerated field map (rows forms for the subsets)."""
    n = ncell * nqp
    rng = np.random.default_rng(2)
    perm = rng.permutation(ncell)
    parts = [np.sort(perm[: ncell // 3]).astype(np.int32), np.sort(perm[ncell // 3:]).astype(np.int32)]
    hist = [og.random_F(n, seed=s, amp=a) for s, a in ((1, 0.05), (2, 0.2))]
    now = {"g": hist[0]}
    ev = lambda c: now["g"].reshape(ncell, nqp, 9)[c].reshape(-1, 9)   # noqa: E731
    whole = QuadratureFieldMap(ncell, nqp, JAXMaterial(jm.OgdenHyperelasticity()))
    subs = [QuadratureFieldMap(ncell, nqp, JAXMaterial(jm.OgdenHyperelasticity()), cells=c) for c in parts]
    for q in [whole] + subs:
        q.register_gradient("DeformationGradient", ev)
    fields = lambda q: {"flux": q.fluxes["FirstPiolaKirchhoffStress"].x.array, "isv": q.internal_state_variables["PK2Stress"].x.array,   # noqa: E731
                        "jac": q.jacobian_flatten.x.array}
    width = {"flux": 9, "isv": 6, "jac": 81}
    for g in hist:
        now["g"] = g
        for q in [whole] + subs:
            q.update()
            q.advance()
        for name, w in width.items():
            want = fields(whole)[name].reshape(n, w)
            for q, cells in zip(subs, parts):
                got = fields(q)[name].reshape(n, w)
                rows = (cells[:, None] * nqp + np.arange(nqp)[None]).ravel()
                assert np.array_equal(got[rows], want[rows]), name
                rest = np.setdiff1d(np.arange(n), rows)
                assert not got[rest].any(), name          # the other cells' rows are not this map's to write
    for q in [whole] + subs:
        q.close()
        q.material.close()
