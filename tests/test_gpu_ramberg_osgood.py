"""GPU: the Ramberg-Osgood nonlinear elasticity law (DXM_LAW_RAMBERG_OSGOOD, ``small_strain_kernel<3, ...>``) through
``HIPMaterial`` and the C ABI, against the numpy restatement ``ramberg_osgood_ref.py`` and the reference's recorded curves
(fixtures and their origin: ``test_ramberg_osgood_cpu.py``)."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.conventions import tangent_from_coefficients, tangent_from_pack4, unpack_sym_tangent
from dolfinx_materials_amd.jaxmat import JAXMaterial

import ramberg_osgood_ref as ro
from helpers import to_device, to_host
from law_fuzz import ramberg_osgood_strains as strains
from test_ramberg_osgood_cpu import ALPHA, E, N_EXP, NU, PRM, SIG0, close, load_curves

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SQ2 = np.sqrt(2.0)


def behavior(n=N_EXP, alpha=ALPHA, sig0=SIG0):
    return jm.RambergOsgoodNonLinearElasticity(jm.LinearElasticIsotropic(E=E, nu=NU), sig0=sig0, alpha=alpha, n=n)


def check_against_ref(sig, ct, eps, prm, stats, tag="", **kw):
    """``tag``: what a failure should name next to its figure (a sweep's drawn parameters)."""
    r = ro.update(eps, *prm, **kw)
    srow = np.maximum(np.abs(r["sig"]).max(axis=1), 1e-300)
    assert np.all(np.abs(sig - r["sig"]).max(axis=1) <= 1e-12 * srow), (tag, float((np.abs(sig - r["sig"]).max(axis=1) / srow).max()))
    cscale = np.abs(r["Ct_mfront"]).max(axis=(1, 2))
    ct = np.asarray(ct).reshape(-1, 6, 6)
    err = np.abs(ct - r["Ct_mfront"]).max(axis=(1, 2)) / cscale
    assert err.max() <= 1e-11, (tag, float(err.max()))
    assert stats["n_plastic"] == int(r["newton"].sum()) and stats["n_nan"] == 0, (tag, stats)
    return r


@pytest.mark.parametrize("N", [1, 63, 64, 65, 100_003])
@pytest.mark.parametrize("n_exp,alpha", [(1.0, 0.4), (1.5, 2.0), (5.0, 0.1), (20.0, 0.4), (100.0, 0.4)])
def test_update_matches_the_restatement(N, n_exp, alpha):
    prm = (E, NU, SIG0, alpha, n_exp)
    eps = strains(N, seed=N + int(10 * n_exp))
    m = JAXMaterial(behavior(n_exp, alpha))
    m.set_data_manager(N)
    assert m.internal_state_variables == {} and m.kernel_name.startswith("small_strain_kernel<3")
    sig, isv, ct = m.integrate(eps)
    st = m.last_stats
    r = check_against_ref(sig, ct, eps, prm, st)
    assert st["n_not_converged"] == 0 and st["max_local_iters"] <= 12
    assert st["max_local_iters"] <= r["iters"].max() + 2
    if N >= 64:
        m.set_newton(maxit=1)
        m.integrate(eps)
        assert m.last_stats["n_not_converged"] > 0
    m.close()


def test_reference_curves_on_the_gpu():
    dol, mt = load_curves()
    m = JAXMaterial(jm.RambergOsgoodNonLinearElasticity.from_mfront_properties(
        {"YoungModulus": E, "PoissonRatio": NU, "YieldStrength": SIG0, "alpha": ALPHA, "n": N_EXP}),
        gradient_name="Strain", flux_name="Stress")
    m.set_data_manager(dol.shape[0])
    assert set(m.gradients) == {"Strain"} and set(m.fluxes) == {"Stress"}

    def gpu(eps):
        s, _, c = m.integrate(eps)
        return np.array(s), np.array(c)

    eps, sig = ro.plane_strain_uniaxial(dol[:, 0], gpu)
    assert np.abs(sig[:, :3] - dol[:, 1:4]).max() <= 1e-9 * np.abs(dol[:, 1:4]).max()
    assert close(sig[:, [0, 2]], dol[:, [1, 3]], 1e-9)
    assert close(sig[:, [0, 2]], mt[:, [7, 9]], 1e-4) and close(eps[:, 1:2], mt[:, 2:3], 1e-4)
    m.close()


@pytest.mark.parametrize("N", [65, 100_003])
def test_layouts_agree_bit_for_bit(N):
    torch = pytest.importorskip("torch")
    eps = strains(N, seed=2)
    out = {}
    for layout in ("full", "sym", "coef", "pack4"):
        m = JAXMaterial(behavior(), tangent_layout=layout)
        m.set_data_manager(N)
        s, _, c = m.integrate(eps)
        out[layout] = (np.array(s), np.array(c), dict(m.last_stats))
        m.close()
    sig, full = out["full"][0], out["full"][1].reshape(N, 6, 6)
    check_against_ref(sig, full, eps, PRM, out["full"][2])
    for layout in ("sym", "coef", "pack4"):
        assert np.array_equal(out[layout][0], sig) and out[layout][2] == out["full"][2], layout
    assert np.array_equal(unpack_sym_tangent(out["sym"][1]), full)
    scale = np.abs(full).max()
    assert np.abs(tangent_from_coefficients(out["coef"][1]).reshape(N, 6, 6) - full).max() <= 8 * EPS * scale
    assert np.abs(tangent_from_pack4(sig, out["pack4"][1]).reshape(N, 6, 6) - full).max() <= 8 * EPS * scale
    # the device rebuilds: bit for bit
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    ct = torch.empty((N, 36), dtype=torch.float64, device=dev)
    coef_d, sig_d, pack_d = to_device(out["coef"][1]), to_device(sig), to_device(out["pack4"][1])   # (held until the kernels ran)
    _lib.check(lib.dxm_expand_tangent_device(coef_d.data_ptr(), N, ct.data_ptr(), 0, st))
    torch.cuda.synchronize()
    assert np.array_equal(to_host(ct).reshape(N, 6, 6), full)
    ct.fill_(0.0)
    _lib.check(lib.dxm_expand_tangent_pack4_device(sig_d.data_ptr(), pack_d.data_ptr(), N, ct.data_ptr(), 0, st))
    torch.cuda.synchronize()
    assert np.array_equal(to_host(ct).reshape(N, 6, 6), full)


def test_host_paths_and_two_blocks_match_the_device_pointer_path():
    torch = pytest.importorskip("torch")
    N = 100_003
    eps = strains(N, seed=5)
    m = JAXMaterial(behavior())
    m.set_data_manager(N)
    dev = torch.device("cuda:0")
    g = to_device(eps)
    f = torch.empty((N, 6), dtype=torch.float64, device=dev)
    c = torch.empty((N, 36), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_s, want_c = to_host(f), to_host(c).reshape(N, 6, 6)
    check_against_ref(want_s, want_c, eps, PRM, m.stats()[1])
    # host-buffer form: packed transfer (pack4 + host rebuild) and the plain download
    for packed in (2, 0):
        m.set_option("packed_transfer", packed)
        s, _, ct = m.integrate(eps)
        assert np.array_equal(s, want_s) and np.array_equal(ct, want_c), packed
    m.set_option("packed_transfer", 2)
    # bound outputs
    flux_fn, jac_fn = np.zeros(N * 6), np.zeros(N * 36)
    m.bind_outputs(flux=flux_fn, tangent=jac_fn)
    m.integrate(eps)
    assert np.array_equal(flux_fn.reshape(N, 6), want_s) and np.array_equal(jac_fn.reshape(N, 6, 6), want_c)
    m.close()
    # integrate_rows
    total = N + 1000
    rows = np.ascontiguousarray(np.random.default_rng(1).permutation(total)[:N], dtype=np.int64)
    m = JAXMaterial(behavior())
    m.set_data_manager(N)
    flux_r, jac_r = np.full(total * 6, -7.0), np.full((total, 36), -7.0)
    m.integrate_rows(eps, rows, flux_r, jac_r)
    assert np.array_equal(flux_r.reshape(total, 6)[rows], want_s) and np.array_equal(jac_r[rows].reshape(N, 6, 6), want_c)
    m.close()
    # two blocks of points on one GPU
    m = JAXMaterial(behavior(), devices=[0, 0])
    m.set_data_manager(N)
    s, _, ct = m.integrate(eps)
    assert np.array_equal(s, want_s) and np.array_equal(ct, want_c)
    m.close()


def _hex_case(seed=3):
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from test_gpu_gradient import host_gradient, make_mesh

    from dolfinx_materials_amd.gradient import gauss_points_hex

    m, coords = make_mesh(4)
    rng = np.random.default_rng(seed)
    u = 2e-2 * rng.standard_normal(m.ndof) * m.h
    H = host_gradient(coords, m.conn, u, gauss_points_hex(2)).reshape(-1, 3, 3)
    return m, coords, u, H


def _mandel(H):
    e = 0.5 * (H + H.transpose(0, 2, 1))
    return np.stack([e[:, 0, 0], e[:, 1, 1], e[:, 2, 2], SQ2 * e[:, 0, 1], SQ2 * e[:, 0, 2], SQ2 * e[:, 1, 2]], axis=1)


@pytest.mark.parametrize("layout", ["full", "pack4"])
def test_fused_displacement_forms_match_gradient_then_integrate(layout):
    from dolfinx_materials_amd.gradient import Hex8Mesh, Tet4Mesh
    from test_gpu_gradient import KUHN

    m, coords, u, H = _hex_case()
    meshes = [(Hex8Mesh(coords, m.conn), _mandel(H))]
    conn = np.concatenate([m.conn[:, list(k)] for k in KUHN], axis=0).astype(np.int32)
    X, U = coords[conn], u.reshape(-1, 3)[conn]
    Ht = (U[:, 1:] - U[:, :1]).transpose(0, 2, 1) @ np.linalg.inv((X[:, 1:] - X[:, :1]).transpose(0, 2, 1))
    meshes.append((Tet4Mesh(coords, conn, nqp=4), _mandel(np.repeat(Ht, 4, axis=0))))
    for mesh, g in meshes:
        a, b = JAXMaterial(behavior(), tangent_layout=layout), JAXMaterial(behavior(), tangent_layout=layout)
        a.set_data_manager(mesh.npoints)
        b.set_data_manager(mesh.npoints)
        fa, _, ca = a.integrate_displacement(mesh, u)
        fb, _, cb = b.integrate(g)
        assert a.last_stats["n_plastic"] > 0 and a.last_stats["n_not_converged"] == 0
        assert np.abs(fa - fb).max() < 1e-9 * np.abs(fb).max() and np.abs(np.asarray(ca) - cb).max() < 1e-9 * np.abs(cb).max()
        a.close()
        b.close()


def test_protocol_is_the_elastic_laws():
    N = 300
    eps = strains(N, seed=8)
    el = JAXMaterial(jm.ElasticBehavior(jm.LinearElasticIsotropic(E=E, nu=NU)))
    m = JAXMaterial(behavior())
    for mat in (el, m):
        mat.set_data_manager(N)
    assert m.internal_state_variables == el.internal_state_variables == {}
    assert set(m.get_initial_state_dict()) == set(el.get_initial_state_dict()) == {"strain", "stress"}
    s1 = np.array(m.integrate(eps)[0])
    fin = m.get_final_state_dict()
    assert np.array_equal(fin["stress"], s1) and np.array_equal(fin["strain"], eps)
    assert np.all(np.asarray(m.get_initial_state_dict()["stress"]) == 0.0)
    m.data_manager.update()
    assert np.array_equal(np.asarray(m.get_initial_state_dict()["stress"]), s1)
    s2 = np.array(m.integrate(2 * eps)[0])
    assert np.array_equal(np.asarray(m.get_final_state_dict()["stress"]), s2)
    m.data_manager.revert()
    assert np.array_equal(np.asarray(m.get_final_state_dict()["stress"]), s1)
    # stateless: the update of a strain does not depend on what came before
    assert np.array_equal(np.array(m.integrate(eps)[0]), s1)
    for mat in (el, m):
        mat.close()


def test_quadrature_map_in_every_layout():
    from dolfinx_materials_amd.field_map import QuadratureFieldMap

    ncell, nqp = 4200, 8
    n = ncell * nqp
    hist = [strains(n, seed=s) for s in (11, 12)]
    now = {"g": hist[0]}
    ev = lambda c: now["g"].reshape(ncell, nqp, 6)[c].reshape(-1, 6)   # noqa: E731
    maps = {lay: QuadratureFieldMap(ncell, nqp, JAXMaterial(behavior(), tangent_layout=lay)) for lay in ("full", "sym", "coef", "pack4")}
    for q in maps.values():
        q.register_gradient("strain", ev)
    rows = maps["full"].dofs
    for g in hist:
        now["g"] = g
        for q in maps.values():
            q.update()
        want = maps["full"].tangent_block_values(rows=rows)
        check_against_ref(maps["full"].fluxes["stress"].x.array.reshape(n, 6), want, g, PRM, maps["full"].material.last_stats)
        for lay, q in maps.items():
            assert np.array_equal(q.fluxes["stress"].x.array, maps["full"].fluxes["stress"].x.array), lay
            got = q.tangent_block_values(rows=rows)
            if lay in ("full", "sym"):
                assert np.array_equal(got, want), lay
            else:
                assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max(), lay
        for q in maps.values():
            q.advance()
    for q in maps.values():
        q.close()
        q.material.close()


def test_material_properties_reach_the_kernel_and_bad_values_are_refused():
    N = 1000
    eps = strains(N, seed=13)
    m = JAXMaterial(behavior())
    m.set_data_manager(N)
    s100 = np.array(m.integrate(eps)[0])
    m.update_material_property("n", 5.0)
    assert m.material_properties["n"] == 5.0
    s5 = np.array(m.integrate(eps)[0])
    assert not np.array_equal(s5, s100)
    check_against_ref(s5, m.integrate(eps)[2], eps, (E, NU, SIG0, ALPHA, 5.0), m.last_stats)
    for key, bad in (("n", 0.5), ("alpha", 0.0), ("sig0", -1.0), ("elasticity.nu", 0.5)):
        with pytest.raises(_lib.DxmError):
            m.update_material_property(key, bad)
        assert m.behavior.params() == [E, NU, SIG0, ALPHA, 5.0] and m.material_properties["n"] == 5.0
        assert np.array_equal(np.array(m.integrate(eps)[0]), s5), key
    # the C ABI directly: a refused dxm_set_params changes nothing
    lib = m._lib
    h = m._handle
    bad = (C.c_double * 5)(E, NU, SIG0, ALPHA, 0.99)
    assert lib.dxm_set_params(h, bad, 5) < 0 and "n must be" in _lib.last_error(lib)
    assert np.array_equal(np.array(m.integrate(eps)[0]), s5)
    m.close()
