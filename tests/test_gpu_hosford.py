"""GPU: Hosford plasticity with linear hardening (DXM_LAW_HOSFORD_LINEAR, ``hosford_kernel``) through ``HIPMaterial`` (ctypes -> C
ABI) against the numpy restatement ``hosford_ref.update`` on every input class, two increments with ``advance`` in between; the
routes of the library against each other bit for bit; refusals; the update protocol; the local-Newton counter.

Bounds: read from ``tests/golden/hosford_degenerate.npz`` -- 8 x the largest deviation of the restatement from its 50-digit version,
never less than 1e-12 (``tests/golden/make_hosford_degenerate.py``)."""
import ctypes as C
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.conventions import unpack_sym_tangent
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial

import hosford_ref as hr
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hosford_degenerate.npz"))
B_STATE, B_TANGENT = float(GOLD["bound_state"]), float(GOLD["bound_tangent"])
P = hr.PROPS


def behaviour(a, **over):
    p = {**P, **over}
    return jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=p["E"], nu=p["nu"]), jm.LinearHardening(p["R0"], p["H"]), a=a)


def material(a, n, ep=None, p=None, props=None, **kw):
    m = JAXMaterial(behaviour(a, **(props or {})), lazy_isv=False, **kw)
    m.set_data_manager(n)
    if ep is not None:
        # a non-trivial initial state: eps_n = eps_p,n (no elastic strain), so that the hidden plastic strain is eps_p,n
        m.set_initial_state_dict({"Strain": ep, "ElasticStrain": np.zeros_like(ep), "EquivalentPlasticStrain": p})
    return m


def compare(tag, sig, isv, Ct, ref, props=None, b_state=B_STATE, b_tangent=B_TANGENT):
    """Row-scaled deviations of (sig, isv, Ct) from ``ref`` against the bounds; ``props``: the material's E and R0 if not ``PROPS``.
    Returns the four figures."""
    props = props or P
    n = ref["sig"].shape[0]
    if n == 0:
        return 0.0, 0.0, 0.0, 0.0
    sc = np.maximum(np.abs(ref["sig"]).max(axis=1), props["R0"])
    es = (np.abs(np.asarray(sig) - ref["sig"]).max(axis=1) / sc).max()
    ee = (props["E"] * np.abs(np.asarray(isv)[:, :6] - ref["eel"]).max(axis=1) / sc).max()
    ep = (props["E"] * np.abs(np.asarray(isv)[:, 6] - ref["p"]) / sc).max()
    ct = np.asarray(Ct).reshape(n, 36)
    ec = (np.abs(ct - ref["Ct"].reshape(n, 36)).max(axis=1) / np.abs(ref["Ct"]).reshape(n, 36).max(axis=1)).max()
    print(f"hosford parity {tag}: stress {es:.3e} eel {ee:.3e} p {ep:.3e} (bound {b_state:.2e})  tangent {ec:.3e} (bound {b_tangent:.2e})")
    assert es <= b_state and ee <= b_state and ep <= b_state and ec <= b_tangent, (tag, es, ee, ep, ec)
    return es, ee, ep, ec


def check_stats(st, ref):
    assert st["n_not_converged"] == 0 and st["n_nan"] == 0, st
    assert st["n_plastic"] == int(ref["plastic"].sum()), (st, int(ref["plastic"].sum()))
    assert st["max_local_iters"] <= int(ref["iters"].max(initial=0)) + 2, (st, int(ref["iters"].max(initial=0)))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 100_003])
@pytest.mark.parametrize("a", hr.EXPONENTS)
def test_two_increments_match_the_restatement(N, a):
    """Every input class, from a non-trivial state; `advance`; a second increment from the state the first one left."""
    eps1, ep0, p0 = hr.mixed_inputs(N, a, seed=N + int(a))
    m = material(a, N, ep0, p0)
    assert m.kernel_name.startswith("hosford_kernel")
    assert m.internal_state_variables == {"ElasticStrain": 6, "EquivalentPlasticStrain": 1}
    sig, isv, Ct = m.integrate(eps1)
    r1 = hr.update(eps1, ep0, p0, **P, a=a)
    assert r1["converged"].all()
    compare(f"N={N} a={a} increment 1", sig, isv, Ct, r1)
    check_stats(m.last_stats, r1)
    m.data_manager.update()
    # second increment: a further step along the first one's direction, inside the tested overshoot
    R = P["R0"] + P["H"] * r1["p"]
    seq1 = hr.flow(r1["sig"], a)[0]
    grow = np.random.default_rng(N).uniform(0.0, 0.4, N) * np.where(seq1 > 0, R / np.maximum(seq1, 1e-300), 0.0)
    eps2 = eps1 + (grow * (hr.max_overshoot(a) - 1.0) / 2.0)[:, None] * (eps1 - ep0 - (eps1 - ep0)[:, :3].mean(axis=1, keepdims=True) * np.array([1, 1, 1, 0, 0, 0.0]))
    sig2, isv2, Ct2 = m.integrate(eps2)
    r2 = hr.update(eps2, r1["ep"], r1["p"], **P, a=a)
    assert r2["converged"].all()
    compare(f"N={N} a={a} increment 2", sig2, isv2, Ct2, r2)
    safe = np.abs(r2["f_trial"]) > 1e-9 * P["R0"]     # the second trial state was not placed: keep clear of the yield kink for the count
    st = m.last_stats
    assert st["n_not_converged"] == 0 and st["n_nan"] == 0
    assert abs(st["n_plastic"] - int(r2["plastic"].sum())) <= int((~safe).sum())
    assert st["max_local_iters"] <= int(r2["iters"].max(initial=0)) + 2
    m.close()


def test_golden_set_matches_mpmath_directly():
    for a in hr.EXPONENTS:
        k = GOLD["a"] == a
        m = material(a, int(k.sum()), GOLD["ep_n"][k], GOLD["p_n"][k])
        sig, isv, Ct = m.integrate(GOLD["eps"][k])
        compare(f"golden a={a}", sig, isv, Ct, {q: GOLD[q][k] for q in ("sig", "eel", "p", "Ct")})
        assert m.last_stats["n_plastic"] == int(GOLD["plastic"][k].sum())
        m.close()


def test_a_2_equals_the_j2_linear_handle_and_the_oracle():
    from oracle import constitutive_np as onp

    N = 20_000
    eps, ep0, p0 = hr.mixed_inputs(N, 2.0, seed=7)
    m = material(2.0, N, ep0, p0)
    j2 = JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"]), jm.LinearHardening(P["R0"], P["H"])), lazy_isv=False)
    j2.set_data_manager(N)
    j2.set_initial_state_dict({"p": p0, "epsp": ep0})
    sig, isv, Ct = m.integrate(eps)
    sj, ij, Cj = j2.integrate(eps)
    ref = onp.j2_update(eps, ep0, p0, P["E"], P["nu"], onp.LinearHardening(P["R0"], P["H"]))
    safe = np.abs(ref["f_trial"]) > 1e-9 * P["R0"]
    sc = max(np.abs(ref["sig"]).max(), 1e-300)
    for name, got, want in (("oracle", np.asarray(sig), ref["sig"]), ("j2 handle", np.asarray(sig), np.asarray(sj))):
        err = np.abs(got[safe] - want[safe]).max() / sc
        print(f"a = 2 stress against the {name}: {err:.3e}")
        assert err < 1e-12
    ep_err = np.abs(np.asarray(isv)[safe, 6] - ref["p"][safe]).max() / max(np.abs(ref["p"]).max(), 1e-300)
    eel_err = np.abs(np.asarray(isv)[safe, :6] - (eps - ref["epsp"])[safe]).max() / np.abs(eps).max()
    ct_err = (np.abs(np.asarray(Ct).reshape(N, 36) - ref["Ct"].reshape(N, 36))[safe].max(axis=1) / np.abs(ref["Ct"]).reshape(N, 36)[safe].max(axis=1)).max()
    print(f"a = 2: p {ep_err:.3e} eel {eel_err:.3e} tangent {ct_err:.3e} (bound {B_TANGENT:.2e})")
    assert ep_err < 1e-12 and eel_err < 1e-12 and ct_err <= B_TANGENT
    assert m.last_stats["n_plastic"] == j2.last_stats["n_plastic"] == int(ref["plastic"].sum())
    m.close()
    j2.close()


def test_full_and_sym_layouts_and_every_route_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    N, a = 100_003, 10.0
    eps, ep0, p0 = hr.mixed_inputs(N, a, seed=11)
    m = material(a, N, ep0, p0)
    dev = torch.device("cuda:0")
    g = to_device(eps)
    f = torch.empty((N, 6), dtype=torch.float64, device=dev)
    c = torch.empty((N, 36), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    S, T = to_host(f).copy(), to_host(c).copy()
    rc, st_dev = m.stats()
    isv_dev = np.concatenate([np.array(m.get_final_state_dict()[k]).reshape(N, -1) for k in ("ElasticStrain", "EquivalentPlasticStrain")], axis=1)
    assert np.array_equal(T.reshape(N, 6, 6), T.reshape(N, 6, 6).transpose(0, 2, 1))      # exactly symmetric
    # host-buffer form, both packed_transfer settings (2: the 21 entries cross PCIe and are mirrored on the host; 0: the 36)
    for pt in (2, 0):
        m.set_option("packed_transfer", pt)
        sig, isv, Ct = m.integrate(eps)
        assert np.array_equal(np.array(sig), S) and np.array_equal(np.array(Ct).reshape(N, 36), T), pt
        assert np.array_equal(np.array(isv), isv_dev), pt
        assert {k: m.last_stats[k] for k in ("n_plastic", "n_not_converged", "max_local_iters")} == {k: st_dev[k] for k in ("n_plastic", "n_not_converged", "max_local_iters")}
    m.set_option("packed_transfer", 2)
    # bound outputs
    bf, bt = np.zeros((N, 6)), np.zeros((N, 36))
    m.bind_outputs(flux=bf, tangent=bt)
    m.integrate(eps)
    assert np.array_equal(bf, S) and np.array_equal(bt, T)
    m.close()
    # rows form with ISV row deliveries into larger arrays
    M = N + 321
    rows = np.ascontiguousarray(np.random.default_rng(0).permutation(M)[:N], dtype=np.int64)
    flux, tang = np.full((M, 6), -7.0), np.full((M, 36), -9.0)
    big = {"ElasticStrain": np.full((M, 6), -3.0), "EquivalentPlasticStrain": np.full((M, 1), -5.0)}
    m = material(a, N, ep0, p0)
    m.bind_state_outputs(big, deliver=True, rows=True)
    m.integrate_rows(eps, rows, flux, tang)
    assert np.array_equal(flux[rows], S) and np.array_equal(tang[rows], T)
    assert np.array_equal(big["ElasticStrain"][rows], isv_dev[:, :6]) and np.array_equal(big["EquivalentPlasticStrain"][rows, 0], isv_dev[:, 6])
    rest = np.setdiff1d(np.arange(M), rows)
    assert np.all(flux[rest] == -7.0) and np.all(tang[rest] == -9.0) and np.all(big["ElasticStrain"][rest] == -3.0)
    m.close()
    # the "sym" layout: identical stress and stats, the 21 entries are those of the block
    ms = material(a, N, ep0, p0, tangent_layout="sym")
    for pt in (2, 0):
        ms.set_option("packed_transfer", pt)
        sig, isv, C21 = ms.integrate(eps)
        assert np.array(C21).reshape(N, -1).shape[1] == 21
        assert np.array_equal(np.array(sig), S) and np.array_equal(unpack_sym_tangent(C21).reshape(N, 36), T)
        assert {k: ms.last_stats[k] for k in ("n_plastic", "n_not_converged", "max_local_iters")} == {k: st_dev[k] for k in ("n_plastic", "n_not_converged", "max_local_iters")}
    flux, t21 = np.full((M, 6), -7.0), np.full((M, 21), -9.0)
    ms.integrate_rows(eps, rows, flux, t21)
    assert np.array_equal(flux[rows], S) and np.array_equal(unpack_sym_tangent(t21[rows]).reshape(N, 36), T)
    ms.close()
    # two blocks on one GPU
    m2 = material(a, N, ep0, p0, devices=[0, 0])
    sig, isv, Ct = m2.integrate(eps)
    assert np.array_equal(np.array(sig), S) and np.array_equal(np.array(Ct).reshape(N, 36), T) and np.array_equal(np.array(isv), isv_dev)
    m2.close()


def test_refusals_leave_the_handle_usable():
    lib = _lib.load()
    prm = (C.c_double * 5)(P["E"], P["nu"], P["R0"], P["H"], 10.0)
    h = lib.dxm_create(_lib.LAW_HOSFORD_LINEAR, prm, 5, 64, 0)
    assert h
    for layout in (2, 3):
        assert lib.dxm_set_tangent_layout(h, layout) < 0 and b"general symmetric 6x6" in lib.dxm_last_error()
    assert lib.dxm_tangent_size(h) == 36
    assert lib.dxm_set_tangent_layout(h, 1) == 0 and lib.dxm_tangent_size(h) == 21 and lib.dxm_set_tangent_layout(h, 0) == 0
    for bad, word in (((P["E"], P["nu"], 0.0, P["H"], 10.0), b"R0"), ((P["E"], P["nu"], P["R0"], -1.0, 10.0), b"H"),
                      ((P["E"], P["nu"], P["R0"], P["H"], 1.5), b"exponent"), ((P["E"], P["nu"], P["R0"], P["H"], float("inf")), b"exponent")):
        assert lib.dxm_set_params(h, (C.c_double * 5)(*bad), 5) < 0 and word in lib.dxm_last_error()
    assert lib.dxm_set_param_field(h, 2, None) < 0 and b"Hosford" in lib.dxm_last_error()
    lib.dxm_destroy(h)
    with pytest.raises(ValueError, match="general symmetric 6x6"):
        JAXMaterial(behaviour(10.0), tangent_layout="pack4")
    with pytest.raises(ValueError, match="general symmetric 6x6"):
        JAXMaterial(behaviour(10.0), tangent_layout="coef")
    with pytest.raises(TypeError, match="linear hardening only"):
        jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"]), lambda p: 200.0 + 10.0 * p)
    # a refused property leaves the material as it was, and it still integrates
    N = 300
    eps, ep0, p0 = hr.mixed_inputs(N, 10.0, seed=3)
    m = material(10.0, N, ep0, p0)
    with pytest.raises(NotImplementedError, match="varies from point to point"):
        m.update_material_property("yield_stress.sig0", np.linspace(100.0, 300.0, N))
    with pytest.raises(_lib.DxmError, match="exponent"):
        m.update_material_property("a", 1.0)
    assert m.material_properties["a"] == 10.0
    sig, isv, Ct = m.integrate(eps)
    compare("after refusals", sig, isv, Ct, hr.update(eps, ep0, p0, **P, a=10.0))
    m.close()


def test_protocol_revert_and_update_material_property():
    N = 1000
    eps, ep0, p0 = hr.mixed_inputs(N, 10.0, seed=5)
    m = material(10.0, N, ep0, p0)
    s0 = {k: np.array(v) for k, v in m.get_initial_state_dict().items()}
    sig, isv, Ct = m.integrate(eps)
    m.data_manager.revert()
    back = m.get_final_state_dict()
    for k in ("ElasticStrain", "EquivalentPlasticStrain"):
        assert np.array_equal(np.array(back[k]), s0[k]), k
    sig2, isv2, Ct2 = m.integrate(eps)
    assert np.array_equal(np.array(sig2), np.array(sig)) and np.array_equal(np.array(Ct2), np.array(Ct))
    for key, val in (("a", 6.0), ("yield_stress.sig0", 180.0), ("yield_stress.H", 25.0), ("elasticity.E", 69e3), ("elasticity.nu", 0.31)):
        m.update_material_property(key, val)
    over = dict(E=69e3, nu=0.31, R0=180.0, H=25.0)
    sig3, isv3, Ct3 = m.integrate(eps)
    ref = hr.update(eps, ep0, p0, **over, a=6.0)
    sc = np.maximum(np.abs(ref["sig"]).max(axis=1), over["R0"])
    err = (np.abs(np.array(sig3) - ref["sig"]).max(axis=1) / sc).max()
    print(f"after update_material_property (a = 6): stress {err:.3e}")
    assert err <= B_STATE and m.last_stats["n_plastic"] == int(ref["plastic"].sum())
    m.close()


def test_one_newton_iteration_is_reported_as_not_converged():
    N = 512
    eps, ep0, p0 = hr.make_inputs("generic", N, 10.0, seed=2)
    m = material(10.0, N, ep0, p0)
    m.set_newton(maxit=1)
    m.integrate(eps)
    st = m.last_stats
    assert st["n_plastic"] == N and 0 < st["n_not_converged"] <= N and st["max_local_iters"] == 1, st
    m.set_newton()
    m.integrate(eps)
    assert m.last_stats["n_not_converged"] == 0
    m.close()


def test_field_map_over_a_cell_subset_next_to_a_voce_map():
    """The multi-material demo's configuration: Hosford on the matrix cells, von Mises + Voce on the inclusion's, one field map each."""
    ncell, nqp, a = 2001, 4, 10.0
    n = ncell * nqp
    rng = np.random.default_rng(1)
    perm = rng.permutation(ncell)
    matrix, incl = np.sort(perm[: 2 * ncell // 3]).astype(np.int32), np.sort(perm[2 * ncell // 3:]).astype(np.int32)
    eps_all = hr.mixed_inputs(n, a, seed=21, trivial_state=True)[0]
    now = {"g": np.zeros_like(eps_all)}     # the state is initialised at zero strain, as the demo's is
    ev = lambda c: now["g"].reshape(ncell, nqp, 6)[c].reshape(-1, 6)   # noqa: E731
    voce = jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"]), jm.VoceHardening(250.0, 400.0, 100.0))
    qh = QuadratureFieldMap(ncell, nqp, JAXMaterial(behaviour(a)), cells=matrix)
    qv = QuadratureFieldMap(ncell, nqp, JAXMaterial(voce, gradient_name="Strain", flux_name="Stress"), cells=incl)
    for q in (qh, qv):
        q.register_gradient("Strain", ev)
        q.initialize_state()
    now["g"] = eps_all
    for q in (qh, qv):
        q.update()
        q.advance()
    rows = (matrix[:, None] * nqp + np.arange(nqp)[None]).ravel()
    rest = np.setdiff1d(np.arange(n), rows)
    ref = hr.update(eps_all[rows], np.zeros((rows.size, 6)), np.zeros(rows.size), **P, a=a)
    sig = qh.fluxes["Stress"].x.array.reshape(n, 6)
    jac = qh.jacobian_flatten.x.array.reshape(n, 36)
    pl = qh.internal_state_variables["EquivalentPlasticStrain"].x.array.reshape(n)
    eel = qh.internal_state_variables["ElasticStrain"].x.array.reshape(n, 6)
    compare("field map, matrix cells", sig[rows], np.concatenate([eel[rows], pl[rows, None]], axis=1), jac[rows], ref)
    assert not sig[rest].any() and not jac[rest].any() and not pl[rest].any()
    assert (pl[rows] > 0).sum() == int(ref["plastic"].sum())
    assert qv.fluxes["Stress"].x.array.reshape(n, 6)[rest].any() and not qv.fluxes["Stress"].x.array.reshape(n, 6)[rows].any()
    for q in (qh, qv):
        q.close()
        q.material.close()
