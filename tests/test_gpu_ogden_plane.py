"""GPU: plane-strain Ogden hyperelasticity (DXM_LAW_OGDEN_PE = 38, ``ogden_plane_kernel``) through ``HIPMaterial`` (ctypes -> C ABI)
against the law's definition ``ogden_plane_ref.restricted_closed_form`` -- law 7's numpy closed form on the embedded F, restricted: the
formulation the kernel does NOT use (LAPACK's 3x3 eigen-solver, three divided differences, the 9 x 9 block) -- on the families of
``test_ogden_plane_cpu.py``; against law 7 of the same process; the tile loop past its first pass; the routes of the library against
each other bit for bit; inverted and flat points; every refusal on a live handle; the update protocol; a uniaxial plane-strain stretch
solved on the CPU from the energy alone.

The bound is the project's own, ``test_gpu_ogden.BOUND = min(16 E0, 1e-11)`` with the ``E0 = 2e-13`` that the plane families keep too
(``test_ogden_plane_cpu.py``, floor 3.9e-14); errors are ``ogden_ref.row_errors``.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions as cv
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial

import ogden_plane_ref as op
import ogden_ref as og
import tile_loop_cases as tlc
from helpers import to_device, to_host
from test_gpu_ogden import BOUND

pytestmark = pytest.mark.gpu

NLOOP = 206_147       # blocks_per_cu = 1: three full passes of the tile loop on 256 CUs and a ragged fourth (tile_loop_cases.size_for)
NCHUNK = 264_600      # the host path takes two chunks: full-layout laws cross in chunks of 131 072 points


def behaviour(**prm):
    return jm.OgdenHyperelasticity(**prm, hypothesis="plane_strain")


def material(n, lazy_isv=False, **prm):
    m = JAXMaterial(behaviour(**prm), lazy_isv=lazy_isv)
    m.set_data_manager(n)
    return m


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def check(tag, P, A, isv, F, prm, bound=BOUND):
    n = len(F)
    e = op.errors((np.asarray(P), np.asarray(A).reshape(n, 5, 5), np.asarray(isv)), op.restricted_closed_form(F, **prm))
    print(f"plane-strain ogden {tag} N={n} alpha={prm['alpha']}: P {e[0]:.3e} A {e[1]:.3e} PK2Stress {e[2]:.3e} (bound {bound:.1e})")
    assert max(e) <= bound, e


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", range(len(og.PARAM_SETS)))
def test_update_matches_the_restricted_closed_form(N, k):
    prm = og.PARAM_SETS[k]
    F = op.family(N, seed=N + k)
    m = material(N, **prm)
    assert m.kernel_name == "ogden_plane_kernel" and m.internal_state_variables == {"PK2Stress": 4}
    assert m.gradients == {"DeformationGradient": 5} and m.tangent_size == 25 and m.algorithmic_bytes_per_point == 312
    P, isv, A = m.integrate(F)
    st = m.last_stats
    assert st["n_nan"] == 0 and st["n_plastic"] == 0 and st["n_not_converged"] == 0 and st["max_local_iters"] == 0
    assert np.asarray(A).shape == (N, 5, 5) and np.asarray(P).shape == (N, 5) and np.asarray(isv).shape == (N, 4)
    check("parity", P, A, isv, F, prm)
    assert not np.asarray(P)[0].any() and not np.asarray(isv)[0].any()          # row 0 is F = I: stress free, exactly
    m.close()


@pytest.mark.parametrize("k", range(len(og.PARAM_SETS)))
def test_law_7_of_the_same_process_on_the_embedded_gradient(k):
    prm = og.PARAM_SETS[k]
    N = 1000
    F = op.family(N, seed=40 + k)
    m = material(N, **prm)
    P, isv, A = (np.array(x) for x in m.integrate(F))
    w = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
    w.set_data_manager(N)
    P9, isv6, A9 = (np.array(x) for x in w.integrate(cv.embed_plane_F(F)))
    assert not P9[:, 5:].any() and not isv6[:, 4:].any()                               # what the restriction drops is exactly zero
    want = (cv.restrict_plane_F(P9), cv.restrict_plane_F_tangent(A9.reshape(N, 9, 9)), cv.restrict_plane_strain(isv6))
    e = op.errors((P, A.reshape(N, 5, 5), isv), want)
    print(f"plane-strain ogden vs law 7 restricted alpha={prm['alpha']}: P {e[0]:.3e} A {e[1]:.3e} PK2Stress {e[2]:.3e} (bound {2 * BOUND:.1e})")
    assert max(e) <= 2 * BOUND, e        # each is within BOUND of the same reference
    m.close()
    w.close()


def test_tile_loop_at_one_workgroup_per_cu_equals_the_default_grid_bit_for_bit():
    torch = pytest.importorskip("torch")
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert NLOOP == tlc.size_for(256)
    print(f"tile loop: {num_cu} CUs, {tlc.passes(NLOOP, num_cu, 1)} passes at blocks_per_cu = 1, {tlc.passes(NLOOP, num_cu, 32)} at 32")
    assert tlc.passes(NLOOP, num_cu, 1) >= 4 and NLOOP % 64 != 0
    prm = og.DEFAULTS
    F = op.family(NLOOP, seed=8)
    g = to_device(F)
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for bpc in (None, 1):
        m = material(NLOOP, **prm)
        if bpc is not None:
            m.set_option("blocks_per_cu", bpc)
        f = torch.full((NLOOP + 3, 5), float("nan"), dtype=torch.float64, device="cuda:0")
        c = torch.full((NLOOP + 3, 25), float("nan"), dtype=torch.float64, device="cuda:0")
        m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), st)
        torch.cuda.synchronize()
        out.append((to_host(f), to_host(c), np.array(m.get_final_state_dict()["PK2Stress"]), m.stats()[1]["n_nan"]))
        m.close()
    a, b = out
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert a[3] == b[3] == 0
    assert np.isnan(b[0][NLOOP:]).all() and np.isnan(b[1][NLOOP:]).all()               # nothing past 5 n / 25 n doubles
    idx = tlc.reference_sample(NLOOP, num_cu)
    check("tile loop sample", b[0][idx], b[1][idx], b[2][idx], F[idx], prm)


def test_routes_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    N = NCHUNK
    assert tlc.plan_chunks(N, False, True, 64)[0] == 2
    F = op.family(N, seed=4)
    m = material(N)
    P, isv, A = m.integrate(F)
    P, isv, A = np.array(P), np.array(isv), np.array(A).reshape(N, 25)
    assert m.last_stats["n_nan"] == 0
    idx = np.r_[0:300, 131072 - 300:131072 + 300, N - 300:N]                            # both chunks and their seam
    check("host path sample", P[idx], A[idx], isv[idx], F[idx], og.DEFAULTS)
    dev = torch.device("cuda:0")
    g = to_device(F)
    f = torch.empty((N, 5), dtype=torch.float64, device=dev)
    c = torch.empty((N, 25), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(f), P) and np.array_equal(to_host(c), A)
    assert np.array_equal(np.array(m.get_final_state_dict()["PK2Stress"]), isv)
    # option packed_transfer has nothing to pack for this law: same bytes either way
    m.set_option("packed_transfer", 0)
    P0, _, A0 = m.integrate(F)
    assert np.array_equal(np.array(P0), P) and np.array_equal(np.array(A0).reshape(N, 25), A)
    m.set_option("packed_transfer", 2)
    # rows form over a permuted subset of a larger array: the named rows get the values, the others keep their fill
    M = N + 500
    rows = np.ascontiguousarray(np.random.default_rng(0).permutation(M)[:N], dtype=np.int64)
    flux = np.full((M, 5), -7.0)
    tang = np.full((M, 25), -9.0)
    m.integrate_rows(F, rows, flux, tang)
    assert np.array_equal(flux[rows], P) and np.array_equal(tang[rows], A)
    rest = np.setdiff1d(np.arange(M), rows)
    assert np.all(flux[rest] == -7.0) and np.all(tang[rest] == -9.0)
    m.close()


def test_inverted_and_flat_points_are_counted_and_leave_their_neighbours_alone():
    N = 200
    F = op.random_F5(N, seed=9)
    bad = F.copy()
    bad[[3, 64, 129], 2] *= -1.0           # F22 < 0
    bad[70, 3:] = 2.0                      # in-plane determinant < 0
    bad[191] = [0.0, 0.0, 1.0, 0.0, 0.0]   # a zero in-plane block: J = 0
    where = np.array([3, 64, 70, 129, 191])
    assert (bad[where, 2] * (bad[where, 0] * bad[where, 1] - bad[where, 3] * bad[where, 4]) <= 0.0).all()
    m = material(N)
    base = [np.array(x) for x in m.integrate(F)]
    assert m.last_stats["n_nan"] == 0
    got = [np.array(x) for x in m.integrate(bad)]
    assert m.last_stats["n_nan"] == len(where)
    ok = np.setdiff1d(np.arange(N), where)
    for a, b in zip(got, base):
        assert np.isnan(a[where].reshape(len(where), -1)).all()
        assert np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
    nonfinite = F.copy()
    nonfinite[17, 0] = np.inf
    nonfinite[130, 4] = np.nan
    m.integrate(nonfinite)
    assert m.last_stats["n_nan"] == 2
    m.close()


def test_refusals_on_the_handle_each_with_its_own_sentence():
    import plane_gradient_ref as pg
    from dolfinx_materials_amd.gradient import PlaneMesh

    lib = _lib.load()
    case = pg.quad_case("q1-x4")
    mesh = PlaneMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"], case["dphi"])
    n = mesh.npoints
    F = op.family(n, seed=3)
    m = material(n)
    before = [np.array(x) for x in m.integrate(F)]
    h = m._parts[0][0]
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h, layout) < 0 and "the plane-strain Ogden tangent dP/dF is a 5x5 block of 25 entries" in err(lib)
    assert lib.dxm_tangent_size(h) == 25
    field = np.full(n, 1.0)
    assert lib.dxm_set_param_field(h, 1, field.ctypes.data) < 0
    assert "per-point parameter fields are not served for plane-strain Ogden hyperelasticity" in err(lib)
    frame = np.eye(3)
    assert lib.dxm_set_frame(h, frame.ctypes.data) < 0 and "plane-strain Ogden hyperelasticity is isotropic" in err(lib)
    frames = np.tile(np.eye(3).reshape(9), (n, 1))
    assert lib.dxm_set_frame_field(h, frames.ctypes.data) < 0 and "plane-strain Ogden hyperelasticity is isotropic" in err(lib)
    bad = (C.c_double * 3)(0.0, 27778.0, 69444444.0)
    assert lib.dxm_set_params(h, bad, 3) < 0 and "alpha" in err(lib)
    assert lib.dxm_set_external_state_uniform(h, 0, 300.0) < 0 and "law 38 has no external state variable" in err(lib), err(lib)
    u, fl, ct = np.zeros(mesh.displacement_size), np.zeros((n, 5)), np.zeros((n, 25))
    rows, st = np.arange(n, dtype=np.int64), _lib.Stats()
    for fused in (1, 0):
        m.set_option("fused_gradient", fused)
        rcs = (lib.dxm_integrate_displacement(h, mesh._handle, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_rows(h, mesh._handle, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_device(h, mesh._handle, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
        for rc in rcs:
            assert rc < 0 and "takes the 5-wide deformation gradient [F00, F11, F22, F01, F10]" in err(lib), err(lib)
            assert "[1 + H00, 1 + H11, 1, H01, H10]" in err(lib)
    m.set_option("fused_gradient", 1)
    assert not fl.any() and not ct.any()
    with pytest.raises(ValueError, match="5x5 block of 25 entries"):
        JAXMaterial(behaviour(), tangent_layout="sym")
    assert not lib.dxm_create(37, (C.c_double * 3)(28.8, 27778.0, 69444444.0), 3, 8, 0) and "unknown law id 37" in err(lib)
    assert not lib.dxm_create(38, (C.c_double * 3)(28.8, -1.0, 69444444.0), 3, 8, 0) and "mu must be" in err(lib)
    # the handle is what it was
    after = [np.array(x) for x in m.integrate(F)]
    for a, b in zip(after, before):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert lib.dxm_kernel_name(h) == b"ogden_plane_kernel" and lib.dxm_tangent_size(h) == 25
    m.close()
    mesh.close()


def test_protocol_integrate_advance_revert_and_explicit_state():
    N = 257
    prm = og.DEFAULTS
    Fa, Fb = op.random_F5(N, seed=1), op.random_F5(N, seed=2)
    m = material(N, **prm)
    s0 = m.get_initial_state_dict()
    assert not np.array(s0["PK2Stress"]).any() and np.array_equal(np.array(s0["DeformationGradient"]), np.tile([1.0, 1, 1, 0, 0], (N, 1)))
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
    Pb, isvb, Ab = (np.array(x) for x in m.integrate(Fb))   # the state is never read: the update from the advanced state is a new handle's
    check("after advance", Pb, Ab, isvb, Fb, prm)
    assert np.array_equal(np.array(m.get_initial_state_dict()["PK2Stress"]), ia)
    # explicit state in, explicit state out; the one-point form
    Ct, new = m.batched_constitutive_update(Fb, m.natural_state(N))
    assert np.array_equal(np.array(new["FirstPiolaKirchhoffStress"]), Pb) and np.array_equal(np.array(new["PK2Stress"]), isvb)
    assert np.asarray(Ct).shape == (N, 5, 5) and np.array_equal(np.asarray(Ct), Ab.reshape(N, 5, 5))
    sig, one = m.constitutive_update(Fb[5], {})
    assert np.array_equal(np.asarray(sig), Pb[5]) and np.array_equal(np.asarray(one["PK2Stress"]).reshape(-1), isvb[5])
    # lazy internal state variables and bound outputs deliver the same bits
    lz = material(N, lazy_isv=True, **prm)
    Pl, il, Al = lz.integrate(Fb)
    assert np.array_equal(np.array(Pl), Pb) and np.array_equal(np.array(il), isvb) and np.array_equal(np.array(Al), Ab)
    lz.close()
    m.close()


@pytest.mark.parametrize("ncell,nqp", [(41, 4), (2001, 4)])
def test_two_maps_on_disjoint_cells_equal_one_map_over_all(ncell, nqp):
    """The reference's test_multimaterials property through the accelerated field map (rows forms for the subsets), as
    ``test_gpu_ogden.py`` has it for law 7."""
    n = ncell * nqp
    rng = np.random.default_rng(2)
    perm = rng.permutation(ncell)
    parts = [np.sort(perm[: ncell // 3]).astype(np.int32), np.sort(perm[ncell // 3:]).astype(np.int32)]
    hist = [op.random_F5(n, seed=s, amp=a) for s, a in ((1, 0.05), (2, 0.2))]
    now = {"g": hist[0]}
    ev = lambda c: now["g"].reshape(ncell, nqp, 5)[c].reshape(-1, 5)   # noqa: E731
    whole = QuadratureFieldMap(ncell, nqp, JAXMaterial(behaviour()))
    subs = [QuadratureFieldMap(ncell, nqp, JAXMaterial(behaviour()), cells=c) for c in parts]
    for q in [whole] + subs:
        q.register_gradient("DeformationGradient", ev)
    fields = lambda q: {"flux": q.fluxes["FirstPiolaKirchhoffStress"].x.array, "isv": q.internal_state_variables["PK2Stress"].x.array,   # noqa: E731
                        "jac": q.jacobian_flatten.x.array}
    width = {"flux": 5, "isv": 4, "jac": 25}
    for g in hist:
        now["g"] = g
        for q in [whole] + subs:
            q.update()
            q.advance()
        Pr, Ar, ir = op.restricted_closed_form(g, **og.DEFAULTS)
        got = fields(whole)
        check("field map", got["flux"].reshape(n, 5), got["jac"].reshape(n, 25), got["isv"].reshape(n, 4), g, og.DEFAULTS)
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


@pytest.mark.parametrize("lam", [0.7, 1.0, 1.3, 2.0])
def test_uniaxial_plane_strain_stretch_against_the_reduced_energy(lam):
    """F = diag(lam, l2, 1) with l2 solved for P11 = 0 on the energy alone (mpmath root-find, as ``ogden_ref.uniaxial_reference``).
    The kernel's P00 must be dW/dlam at that l2, its lateral stress zero; the out-of-plane stress P22 is what holds F22 = 1."""
    prm = og.DEFAULTS
    l2, P00 = op.plane_uniaxial_reference(lam, **prm)
    F = np.tile(np.array([lam, l2, 1.0, 0.0, 0.0]), (64, 1))
    m = material(64, **prm)
    P, _, A = m.integrate(F)
    P, A = np.array(P), np.array(A).reshape(64, 5, 5)
    assert np.all(P == P[0]) and np.isfinite(A).all() and m.last_stats["n_nan"] == 0
    scale = max(abs(P00), prm["K"] * abs(lam * l2 - 1.0))      # the stress is a difference of parts of this size
    print(f"plane uniaxial lam={lam}: l2 {l2:.15f} P00 {P[0, 0]:.12e} reference {P00:.12e} lateral {P[0, 1]:.3e} out of plane {P[0, 2]:.6e}")
    assert abs(P[0, 0] - P00) <= BOUND * max(scale, prm["mu"])
    # l2 is the root rounded to a double: the lateral stress is what that rounding leaves, dP11/dl2 * ulp(l2)
    assert abs(P[0, 1]) <= 4 * np.finfo(float).eps * l2 * abs(A[0, 1, 1]) + BOUND * max(scale, prm["mu"])
    assert not P[0, 3:].any()
    if lam == 1.0:
        assert l2 == 1.0 and not P[0].any()
    m.close()
