"""CPU: plane-stress J2 plasticity with isotropic hardening (DXM_LAW_PS_J2_LINEAR = 30, DXM_LAW_PS_J2_VOCE = 31) without a GPU: the
numpy restatement of the kernel's in-plane form against the 50-digit fixture (built in the nested form), against the read-only
6-wide oracle with ``eps_zz`` from ``brentq``, against central differences, against the restatement of law 23 at ``H = 0`` and
against the uniaxial closed form; feasibility and monotone ``p``; the law rows and their refusals; the Python layer over the test
double ``fake_dxmat_plane_stress_j2``."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd.plane_stress import PlaneStressvonMisesHardening

import plane_stress_j2_ref as pj
import plane_stress_ref as ps
from fake_dxmat_plane_stress_j2 import FakeDxmatPlaneStressJ2

E, NU = pj.E, pj.NU


def run_history(law, prm, incs, **kw):
    """the increments from the virgin state, the state carried: the list of results"""
    p, ep, out = np.zeros(len(incs[0])), np.zeros_like(incs[0]), []
    for e in incs:
        r = pj.update(law, e, ep, p, prm, **kw)
        p, ep = r["p"], r["epsp"]
        out.append(r)
    return out


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------------
def test_the_restatement_against_the_fixture_and_the_figures_the_gpu_bounds_come_from():
    kat = pj.load_kat()
    meta = json.loads(str(kat["meta"]))
    assert meta["dps"] == 50 and meta["off_surface"] == 1e-6
    points = {pj.J2_LINEAR: 0, pj.J2_VOCE: 0}
    worst = {pj.J2_LINEAR: np.zeros(3), pj.J2_VOCE: np.zeros(3)}
    seen = []
    for tag, law, prm, eps, incs in pj.kat_cases(kat):
        points[law] += len(eps[0])
        seen.append((law, tuple(prm[2:])))
        s, Em = prm[2], prm[0]
        rs = run_history(law, prm, eps)
        for k, r in enumerate(rs):
            assert np.array_equal(r["plastic"], incs[k]["plastic"]), (tag, k)
            # the default cap is the oracle's NEWTON_MAXIT: every fixture point converges well inside it
            assert not r["not_converged"].any() and r["iters"].max() <= 9 and pj.stats(r)["n_nan"] == 0
            err = np.array([np.abs(r["stress"] - incs[k]["stress"]).max() / s, np.abs(r["tangent"] - incs[k]["tangent"]).max() / Em,
                            max(np.abs(r["p"] - incs[k]["p"]).max(), np.abs(r["epsp"] - incs[k]["epsp"]).max()) / (s / Em)])
            worst[law] = np.maximum(worst[law], err)
            # eps_zz, the unknown the nested form solves for, from the outputs alone
            ezz = conventions.plane_stress_axial_strain(Em, prm[1], r["stress"], r["epsp"])
            assert np.abs(ezz - kat[f"{tag}_ezz{k + 1}"]).max() <= 16 * pj.MEASURED[law][2] * (s / Em)
        over = rs[0]["overshoot"][rs[0]["plastic"]]
        assert over.min() <= 1.00011 and over.max() >= 0.9999e4
        # the second increment unloads part of the batch
        assert 0 < incs[1]["plastic"].sum() < len(eps[1]) and (incs[0]["plastic"] & ~incs[1]["plastic"]).any(), tag
    assert sorted(seen) == sorted([(30, (250.0, 0.0)), (30, (250.0, 5e3)), (30, (250.0, E)), (31, (350.0, 500.0, 1e3))])
    assert points[pj.J2_LINEAR] >= 250 and points[pj.J2_VOCE] >= 250
    for law in worst:
        print(law, "stress %.3e  tangent %.3e  state %.3e" % tuple(worst[law]), "recorded", pj.MEASURED[law])
        assert (worst[law] <= np.array(pj.MEASURED[law])).all() and (worst[law] >= 0.5 * np.array(pj.MEASURED[law])).all(), (law, worst[law])
        assert all(b == max(16 * m, 2e-14) for b, m in zip(pj.gpu_bounds(law), pj.MEASURED[law]))


# ---- the in-plane form against the nested one through the read-only oracle ------------------------------------------------------------------
def nested(law, prm, eps3, epsp3, p_n):
    """the 6-wide oracle on [xx, yy, zz, sqrt(2) xy, 0, 0] with eps_zz from brentq so that sig_zz = 0; the condensed tangent"""
    from scipy.optimize import brentq

    from oracle import constitutive_np as cn

    hard = cn.LinearHardening(prm[2], prm[3]) if law == pj.J2_LINEAR else cn.VoceHardening(prm[2], prm[3], prm[4])
    n = len(eps3)
    sig, ct, p, ep = np.empty((n, 3)), np.empty((n, 3, 3)), np.empty(n), np.empty((n, 3))
    idx = [0, 1, 3]
    for i in range(n):
        ep6 = np.array([[epsp3[i, 0], epsp3[i, 1], -(epsp3[i, 0] + epsp3[i, 1]), epsp3[i, 2], 0.0, 0.0]])

        def at(z):
            return cn.j2_update(np.array([[eps3[i, 0], eps3[i, 1], z, eps3[i, 2], 0.0, 0.0]]), ep6, p_n[i:i + 1], prm[0], prm[1], hard)

        span = 4.0 * (np.abs(eps3[i]).sum() + np.abs(epsp3[i]).sum() + 1e-6)
        z = brentq(lambda z: at(z)["sig"][0, 2], -span, span, xtol=1e-22, rtol=8.9e-16, maxiter=500)
        r = at(z)
        D = r["Ct"][0]
        sig[i], p[i], ep[i] = r["sig"][0, idx], r["p"][0], r["epsp"][0, idx]
        ct[i] = D[np.ix_(idx, idx)] - np.outer(D[idx, 2], D[2, idx]) / D[2, 2]
    return dict(stress=sig, tangent=ct.reshape(n, 9), p=p, epsp=ep)


def central_differences(law, prm, eps, ep, p, h):
    fd = np.empty((len(eps), 3, 3))
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        fd[:, :, c] = (pj.update(law, eps + d, ep, p, prm)["stress"] - pj.update(law, eps - d, ep, p, prm)["stress"]) / (2 * h)
    return fd.reshape(-1, 9)


@pytest.mark.parametrize("case", list(pj.CASES))
def test_in_plane_and_nested_forms_agree_and_the_condensed_tangent_is_the_derivative(case):
    law, prm = pj.CASES[case]
    s = prm[2]
    e1 = pj.random_trials(prm, 48, seed=7, lo=0.3, hi=6.0)
    r1 = pj.update(law, e1, np.zeros_like(e1), np.zeros(48), prm)
    e2 = 0.7 * e1 + pj.random_trials(prm, 48, seed=8, lo=0.3, hi=6.0)
    for eps, ep, p in ((e1, np.zeros_like(e1), np.zeros(48)), (e2, r1["epsp"], r1["p"])):
        r = pj.update(law, eps, ep, p, prm)
        o = nested(law, prm, eps, ep, p)
        err = (np.abs(r["stress"] - o["stress"]).max() / s, np.abs(r["tangent"] - o["tangent"]).max() / E,
               np.abs(r["p"] - o["p"]).max() / (s / E), np.abs(r["epsp"] - o["epsp"]).max() / (s / E))
        print(case, "in-plane against nested (stress, tangent, p, epsp):", err)
        assert max(err) <= 2e-13 and 10 <= r["plastic"].sum() < 48
        # the condensed tangent of the nested form against central differences of the in-plane stress, well inside the plastic
        # range (the step stays on one branch: trials at least 5 % beyond the surface)
        far = r["overshoot"] >= 1.05
        fd = central_differences(law, prm, eps[far], ep[far], p[far], h=2e-5 * s / E)
        err = np.abs(fd - o["tangent"][far]).max() / E
        print(case, "condensed tangent against central differences, in E:", err)
        assert err <= 1e-9 and far.sum() >= 10


@pytest.mark.parametrize("case", list(pj.CASES))
def test_the_restatements_tangent_against_central_differences_and_its_symmetry(case):
    law, prm = pj.CASES[case]
    s = prm[2]
    eps = pj.random_trials(prm, 60, seed=2, lo=1.05, hi=20.0)
    z3, z = np.zeros_like(eps), np.zeros(60)
    r = pj.update(law, eps, z3, z, prm)
    assert r["plastic"].all()
    err = np.abs(central_differences(law, prm, eps, z3, z, h=2e-5 * s / E) - r["tangent"]).max() / E
    print(case, "tangent against central differences, in E:", err)
    assert err <= 1e-9
    ct = r["tangent"].reshape(-1, 3, 3)
    assert np.abs(ct - np.swapaxes(ct, 1, 2)).max() == 0.0                                 # written from six numbers
    # an elastic point: the plane-stress C as the reference forms it, to the bit
    eps = pj.random_trials(prm, 20, seed=4, lo=0.1, hi=0.9)
    re = pj.update(law, eps, 0 * eps, np.zeros(20), prm)
    assert not re["plastic"].any() and np.array_equal(re["tangent"], np.tile(conventions.plane_stress_stiffness(E, NU).reshape(9), (20, 1)))
    assert np.array_equal(re["p"], np.zeros(20)) and np.array_equal(re["epsp"], 0 * eps)


def test_at_h_zero_the_law_is_the_quadratic_yield_set_with_q_three_halves():
    """law 23 with q = 3/2 and the consistent tangent is perfectly plastic von Mises: two statements of one projection (the multipliers
    differ by the factor 3/2 and the iterations end on their own residuals, so the two agree to rounding, not to the bit)"""
    law, prm = pj.CASES["linear_H0"]
    incs = pj.increments(prm, 200, seed=30)
    ep = np.zeros_like(incs[0])
    for r, e in zip(run_history(law, prm, incs), incs):
        q = ps.quadratic(e, ep, [E, NU, prm[2], 1.5, 1.0])
        assert np.array_equal(r["plastic"], q["plastic"])
        assert np.abs(r["stress"] - q["stress"]).max() <= 1e-13 * prm[2] and np.abs(r["tangent"] - q["tangent"]).max() <= 1e-13 * E
        assert np.abs(r["epsp"] - q["state"]).max() <= 1e-13 * prm[2] / E
        ep = q["state"]
    assert r["plastic"].sum() >= 100


@pytest.mark.parametrize("H", [5e3, E])
def test_uniaxial_tension_follows_the_closed_form(H):
    """one point, eps_xx ramps, sig_yy = 0 found by a scalar Newton on eps_yy with the returned tangent: after yield
    sig_xx = sig0 + E H / (E + H) (eps_xx - sig0 / E), p = (eps_xx - sig_xx / E), and eps_zz = eps_yy"""
    sig0 = 250.0
    prm = [E, NU, sig0, H]
    p, ep, eyy = np.zeros(1), np.zeros((1, 3)), 0.0
    for exx in np.linspace(0.0, 8.0 * sig0 / E, 17)[1:]:
        for it in range(30):
            r = pj.update(pj.J2_LINEAR, np.array([[exx, eyy, 0.0]]), ep, p, prm)
            if abs(r["stress"][0, 1]) <= 1e-13 * sig0:
                break
            eyy -= r["stress"][0, 1] / r["tangent"][0, 4]
        assert it < 12
        want = E * exx if exx <= sig0 / E else sig0 + E * H / (E + H) * (exx - sig0 / E)
        assert abs(r["stress"][0, 0] - want) <= 1e-12 * sig0 and r["stress"][0, 2] == 0.0
        assert abs(r["p"][0] - (exx - want / E)) <= 1e-12 * sig0 / E
        assert abs(conventions.plane_stress_axial_strain(E, NU, r["stress"], r["epsp"])[0] - eyy) <= 1e-12 * sig0 / E
        p, ep = r["p"], r["epsp"]
    # the uniaxial tangent modulus once sig_yy is condensed out
    D = r["tangent"][0].reshape(3, 3)
    assert abs((D[0, 0] - D[0, 1] * D[1, 0] / D[1, 1]) - E * H / (E + H)) <= 1e-10 * E


@pytest.mark.parametrize("case", list(pj.CASES))
def test_feasibility_monotone_p_and_convergence_at_the_default_cap(case):
    law, prm = pj.CASES[case]
    R, _ = pj.hardening(law, prm)
    incs = pj.increments(prm, 400, seed=30) + [pj.random_trials(prm, 400, seed=33, lo=1.0001, hi=1e4)]
    p_before, ep_before = np.zeros(400), np.zeros((400, 3))
    most = 0
    for r in run_history(law, prm, incs):
        tol = np.maximum(pj.RTOL * prm[2], pj.RTOL * r["overshoot"] * R(p_before))
        assert (pj.seq_of(r["stress"]) <= R(r["p"]) + 4 * tol + 4e-16 * pj.seq_of(r["stress"])).all()
        assert (r["p"] >= p_before).all() and np.array_equal(r["p"][~r["plastic"]], p_before[~r["plastic"]])
        assert np.array_equal(r["epsp"][~r["plastic"]], ep_before[~r["plastic"]])           # an elastic point keeps its bits
        assert not r["not_converged"].any() and pj.stats(r)["n_not_converged"] == 0
        most = max(most, int(r["iters"].max()))
        p_before, ep_before = r["p"], r["epsp"]
    print(case, "most Newton steps of a point:", most)
    assert 2 <= most <= 9 < pj.MAXIT


def test_a_non_finite_strain_takes_the_elastic_path_and_counts_once():
    law, prm = pj.CASES["voce"]
    eps = pj.random_trials(prm, 8, seed=3, lo=1.5, hi=3.0)
    r0 = pj.update(law, eps, 0 * eps, np.zeros(8), prm)
    eps2 = 1.2 * eps
    eps2[3, 1] = np.nan
    r = pj.update(law, eps2, r0["epsp"], r0["p"], prm)
    assert pj.stats(r)["n_nan"] == 1 and not r["plastic"][3] and np.isnan(r["stress"][3]).any()
    assert r["p"][3] == r0["p"][3] and np.array_equal(r["epsp"][3], r0["epsp"][3])
    keep = np.arange(8) != 3
    clean = pj.update(law, 1.2 * eps, r0["epsp"], r0["p"], prm)
    assert np.array_equal(r["stress"][keep], clean["stress"][keep]) and np.array_equal(r["tangent"][keep], clean["tangent"][keep])


# ---- the library's tables (host code: no device needed) --------------------------------------------------------------------------------
def test_law_rows_30_and_31_and_the_unassigned_id_before_them():
    assert (_lib.LAW_PS_J2_LINEAR, _lib.LAW_PS_J2_VOCE) == (30, 31)
    for law, nparams in ((30, 4), (31, 5)):
        i = _lib.law_info(law)
        assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (3, 3, nparams, 2, 4, 184)
        assert [(i.isv_name[k].decode(), i.isv_dim[k]) for k in range(2)] == [("p", 1), ("epsp", 3)]
        b = _lib.law_blocks(law)
        assert (b.n_external, b.n_blocks, b.tangent_width) == (0, 1, 9)
        k = b.block[0]
        assert (k.row_kind, k.row_index, k.col_kind, k.col_index, k.rows, k.cols) == (0, 0, 0, 0, 3, 3)
    for law in (29, 32):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_blocks(law)
    assert _lib.load().dxm_abi_version() == 6


def test_create_without_a_gpu_fails_loudly_for_the_new_laws_too():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    assert not lib.dxm_create(30, (C.c_double * 4)(E, NU, 250.0, 5e3), 4, 8, 0)
    assert b"no usable HIP device" in lib.dxm_last_error()
    with pytest.raises(_lib.DxmError, match="no usable HIP device"):
        PlaneStressvonMisesHardening(E, NU, jm.VoceHardening(350.0, 500.0, 1e3)).set_data_manager(8)


def test_the_rows_their_refusals_and_the_plan_in_the_source():
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    src = open(os.path.join(csrc, "dxmat.hip")).read()
    base = src[src.index("constexpr LawDesc plane_stress_j2_law("):]
    base = base[:base.index("\n}\n")]
    for field in ("set_refusal", "launch_refusal", "no_fused", "no_displacement", "no_frame", "no_fields", "stock_only"):
        assert f"d.{field} = " in base, field
    assert "d.set_layouts = d.launch_layouts = L_FULL;" in base and "d.alg_bytes = 184;" in base and "PSJ_BLOCKS_PER_CU" in base
    assert 'state_field(d, 0, "p", 1, 0);' in base and 'state_field(d, 1, "epsp", 3, 1);' in base and "d.n_slots = PSJ_NSLOTS;" in base
    for fn, build in (("law_ps_j2_linear", "build_linear_hardening"), ("law_ps_j2_voce", "build_voce_hardening")):
        row = src[src.index(f"constexpr LawDesc {fn}()"):]
        row = row[:row.index("\n}\n")]
        assert f"d.build = {build};" in row and "DXM_STOCK_ONLY(launch_plane_stress_j2<" in row, fn
    assert "!kLaws[29].kernel" in src and "kKernelOrder[5]" in src
    # the external-state refusal is the library's one sentence for every law without one
    assert "has no external state variable: its update reads the gradient, its parameters and its own state only" in src
    # dxmat.hip names no kernel of the new unit: its device module does not see it
    import re

    assert "plane_stress_j2_kernel<" not in re.sub(r'"[^"]*"', "", src)
    hs = open(os.path.join(csrc, "host_side.hpp")).read()
    assert "r.law == DXM_LAW_PS_J2_LINEAR || r.law == DXM_LAW_PS_J2_VOCE" in hs
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.__file__)), "include", "dxmat.h")).read()
    for words in ("DXM_LAW_PS_J2_LINEAR = 30", "DXM_LAW_PS_J2_VOCE = 31", "DXM_LAW_COUNT = 32"):
        assert words in hdr
    # the kernel calls the hardening law of the 6-wide kernels, it does not copy it
    hip = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "plane_stress_j2.hip")).read())
    assert "hardening_R<HARD>" in hip and "hardening_dR<HARD>" in hip and "exp(" not in hip and '#include "small_strain.hpp"' in hip


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_behaviour_and_material_classes():
    el = jm.LinearElasticIsotropic(E=E, nu=NU)
    b = jm.PlaneStressJ2(el, jm.LinearHardening(250.0, 5e3))
    assert (b.law, b.ngrad, b.nflux, b.params()) == (30, 3, 3, [E, NU, 250.0, 5e3]) and isinstance(b, jm.PlaneStressBehavior)
    b = jm.PlaneStressJ2(el, jm.VoceHardening(350.0, 500.0, 1e3))
    assert (b.law, b.params(), b.E, b.nu) == (31, [E, NU, 350.0, 500.0, 1e3], E, NU)
    custom = jm.CustomHardening("sig0 + K * p", "K", sig0=250.0, K=1e3)
    for y in (custom, lambda p: 250.0 + 1e3 * p, 250.0):
        with pytest.raises(TypeError, match="LinearHardening or materials.VoceHardening"):
            jm.PlaneStressJ2(el, y)
        with pytest.raises(TypeError, match="LinearHardening or materials.VoceHardening"):
            PlaneStressvonMisesHardening(E, NU, y)
    with pytest.raises(ValueError, match="hypothesis must be one of"):      # the law comes in through this module, not hypothesis=
        jm.ElasticBehavior(el, hypothesis="plane_stress")
    m = PlaneStressvonMisesHardening(E, NU, jm.VoceHardening(350.0, 500.0, 1e3))
    assert m.gradients == {"Strain": 3} and m.fluxes == {"Stress": 3} and m.internal_state_variables == {"p": 1, "epsp": 3}
    assert m.tangent_blocks == {("Stress", "Strain"): (3, 3)} and m.tangent_size == 9 and m.algorithmic_bytes_per_point == 184
    assert np.array_equal(m.C, ps.stiffness(E, NU)) and (m.E, m.nu) == (E, NU) and m.yield_stress.sigu == 500.0
    assert m.external_state_variables == {} and not m.frame_fused
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            PlaneStressvonMisesHardening(E, NU, jm.LinearHardening(250.0, 0.0), tangent_layout=layout)
    with pytest.raises(AttributeError, match="isotropic"):
        m.rotation_matrix = np.eye(3)
    s, ep = np.array([[1.0, 2.0, 3.0]]), np.array([[1e-3, 2e-3, 5e-3]])
    assert conventions.plane_stress_axial_strain(E, NU, s, ep)[0] == -NU / E * 3.0 - 3e-3


@pytest.fixture
def fake(monkeypatch):
    lib = FakeDxmatPlaneStressJ2(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    return lib


MATERIALS = {"linear": lambda: PlaneStressvonMisesHardening(E, NU, jm.LinearHardening(250.0, 5e3)),
             "voce": lambda: PlaneStressvonMisesHardening(E, NU, jm.VoceHardening(350.0, 500.0, 1e3))}


@pytest.mark.parametrize("name", list(MATERIALS))
def test_integrate_update_revert_and_the_state_dictionaries(fake, name):
    m = MATERIALS[name]()
    law, prm = m.behavior.law, m.behavior.params()
    n = 40
    m.set_data_manager(n)
    s0 = m.get_initial_state_dict()
    assert set(s0) == {"Strain", "Stress", "p", "epsp"} and np.asarray(s0["epsp"]).shape == (n, 3) and not np.asarray(s0["epsp"]).any()
    ep, p = np.zeros((n, 3)), np.zeros(n)
    for k, e in enumerate(pj.increments(prm, n, seed=8)):
        sig, isv, Ct = m.integrate(e)
        r = pj.update(law, e, ep, p, prm)
        assert np.array_equal(np.asarray(sig), r["stress"]) and np.asarray(Ct).shape == (n, 3, 3)
        assert np.array_equal(np.asarray(Ct).reshape(n, 9), r["tangent"])
        assert np.array_equal(np.asarray(isv)[:, 0], r["p"]) and np.array_equal(np.asarray(isv)[:, 1:], r["epsp"])
        assert m.last_stats["n_plastic"] == int(r["plastic"].sum()) and m.last_stats["n_nan"] == 0
        if k == 1:      # a rejected increment: s1 <- s0, then the same increment again gives the same answer
            m.data_manager.revert()
            s1 = m.get_final_state_dict()
            assert np.array_equal(np.asarray(s1["epsp"]), ep) and np.array_equal(np.asarray(s1["p"]).reshape(n), p)
            sig2, _, _ = m.integrate(e)
            assert np.array_equal(np.asarray(sig2), r["stress"])
        s1 = m.get_final_state_dict()
        assert np.array_equal(np.asarray(s1["Strain"]), e) and np.array_equal(np.asarray(s1["Stress"]), r["stress"])
        assert np.array_equal(np.asarray(s1["epsp"]), r["epsp"])
        m.data_manager.update()
        s0 = m.get_initial_state_dict()
        assert np.array_equal(np.asarray(s0["epsp"]), r["epsp"]) and np.array_equal(np.asarray(s0["p"]).reshape(n), r["p"])
        ep, p = r["epsp"], r["p"]
    assert (p > 0).sum() >= 10
    m.close()


def test_a_prestate_of_p_and_epsp(fake):
    m = MATERIALS["linear"]()
    law, prm = m.behavior.law, m.behavior.params()
    n = 24
    m.set_data_manager(n)
    p0 = np.full(n, 2e-3)
    ep0 = np.tile([2e-3, -1e-3, 5e-4], (n, 1)) * np.linspace(0.5, 1.5, n)[:, None]
    m.set_initial_state_dict({"p": p0, "epsp": ep0})
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.asarray(s0["epsp"]), ep0) and np.array_equal(np.asarray(s0["p"]).reshape(n), p0)
    eps = pj.random_trials(prm, n, seed=12, lo=0.5, hi=4.0)
    sig, isv, _ = m.integrate(eps)
    r = pj.update(law, eps, ep0, p0, prm)
    assert np.array_equal(np.asarray(sig), r["stress"]) and np.array_equal(np.asarray(isv)[:, 1:], r["epsp"]) and r["plastic"].any()
    with pytest.raises(Exception):
        m.set_initial_state_dict({"epsp": np.zeros((n, 4))})          # the 4-wide plastic strain of plane strain does not fit
    m.close()


def test_newton_controls_reach_the_handle_and_a_capped_point_is_counted(fake):
    m = MATERIALS["voce"]()
    prm = m.behavior.params()
    eps = pj.random_trials(prm, 32, seed=1, lo=50.0, hi=1e4)
    m.set_data_manager(32)
    m.set_newton(maxit=1)
    m.integrate(eps)      # (integrate reports the count, it does not raise)
    r = pj.update(pj.J2_VOCE, eps, 0 * eps, np.zeros(32), prm, maxit=1)
    assert r["not_converged"].sum() >= 16 and m.last_stats["n_not_converged"] == int(r["not_converged"].sum())
    assert m.last_stats["max_local_iters"] == 1
    m.set_newton()
    m.integrate(eps)
    assert m.last_stats["n_not_converged"] == 0 and 2 <= m.last_stats["max_local_iters"] <= 9
    m.close()
