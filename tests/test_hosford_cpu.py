"""CPU: the numpy restatement of the Hosford law (``hosford_ref.update``) against the J2 oracle at a = 2 and a = 4, against its
50-digit version on every input class (live on a few points, and on the 240 committed ones of ``tests/golden/hosford_degenerate.npz``),
tangent symmetry, the uniaxial closed form; the behaviour descriptor; the law-table row of the built library."""
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp

import hosford_ref as hr

P = hr.PROPS
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hosford_degenerate.npz"))


@pytest.mark.parametrize("a", [2.0, 4.0])
def test_a_2_and_a_4_are_von_mises(a):
    eps, ep0, p0 = hr.mixed_inputs(8000, a, seed=1)
    r = hr.update(eps, ep0, p0, **P, a=a)
    ref = onp.j2_update(eps, ep0, p0, P["E"], P["nu"], onp.LinearHardening(P["R0"], P["H"]))
    safe = np.abs(ref["f_trial"]) > 1e-9 * P["R0"]
    assert (r["plastic"] == ref["plastic"])[safe].all() and r["converged"].all()
    assert np.abs(r["sig"] - ref["sig"])[safe].max() / np.abs(ref["sig"]).max() < 1e-12
    assert np.abs(r["p"] - ref["p"])[safe].max() < 1e-12 * max(np.abs(ref["p"]).max(), 1e-300)
    assert np.abs(r["eel"] - (eps - ref["epsp"]))[safe].max() / np.abs(eps).max() < 1e-12
    n = len(eps)
    ct = (np.abs(r["Ct"] - ref["Ct"]).reshape(n, 36).max(axis=1) / np.abs(ref["Ct"]).reshape(n, 36).max(axis=1))[safe].max()
    assert ct <= float(GOLD["bound_tangent"]), ct


def test_the_committed_subset_covers_every_class_and_exponent_and_its_bounds_hold():
    assert len(GOLD["a"]) >= 200
    for a in hr.EXPONENTS:
        assert set(GOLD["cls"][GOLD["a"] == a]) == set(range(len(hr.CLASSES)))
    # the measured deviation is far from a conditioning defect (1e-9), and the bounds are 8 x it, floored at 1e-12
    assert GOLD["dev_state"].max() < 1e-9 and GOLD["dev_tangent"].max() < 1e-9
    assert float(GOLD["bound_state"]) == max(8 * GOLD["dev_state"].max(), 1e-12)
    assert float(GOLD["bound_tangent"]) == max(8 * GOLD["dev_tangent"].max(), 1e-12)
    assert np.array_equal(GOLD["props"], [P["E"], P["nu"], P["R0"], P["H"]])


@pytest.mark.parametrize("a", hr.EXPONENTS)
def test_restatement_equals_the_committed_50_digit_results(a):
    k = GOLD["a"] == a
    r = hr.update(GOLD["eps"][k], GOLD["ep_n"][k], GOLD["p_n"][k], **P, a=a)
    assert r["converged"].all() and np.array_equal(r["plastic"], GOLD["plastic"][k])
    sc = np.maximum(np.abs(GOLD["sig"][k]).max(axis=1), P["R0"])
    n = int(k.sum())
    es = (np.abs(r["sig"] - GOLD["sig"][k]).max(axis=1) / sc).max()
    ee = (P["E"] * np.abs(r["eel"] - GOLD["eel"][k]).max(axis=1) / sc).max()
    ep = (P["E"] * np.abs(r["p"] - GOLD["p"][k]) / sc).max()
    ec = (np.abs(r["Ct"] - GOLD["Ct"][k]).reshape(n, 36).max(axis=1) / np.abs(GOLD["Ct"][k]).reshape(n, 36).max(axis=1)).max()
    assert max(es, ee, ep) <= float(GOLD["bound_state"]) / 8 * 1.0000001 and ec <= float(GOLD["bound_tangent"]) / 8 * 1.0000001 or max(es, ee, ep, ec) < 1.25e-13


@pytest.mark.parametrize("cls", hr.CLASSES)
def test_restatement_equals_mpmath_live(cls):
    pytest.importorskip("mpmath")
    for a in (6.0, 20.0):
        eps, ep0, p0 = hr.make_inputs(cls, 1, a, seed=77)
        r = hr.update(eps, ep0, p0, **P, a=a)
        m = hr.update_mp(eps[0], ep0[0], p0[0], **P, a=a)
        sc = max(np.abs(m["sig"]).max(), P["R0"])
        assert bool(r["plastic"][0]) == m["plastic"]
        assert np.abs(r["sig"][0] - m["sig"]).max() / sc < 1e-13 and P["E"] * abs(r["p"][0] - m["p"]) / sc < 1e-13
        assert np.abs(r["Ct"][0] - m["Ct"]).max() / np.abs(m["Ct"]).max() < 1e-13


@pytest.mark.parametrize("a", hr.EXPONENTS)
def test_tangent_is_symmetric_and_iterations_stay_in_the_stated_domain(a):
    eps, ep0, p0 = hr.mixed_inputs(4000, a, seed=3)
    r = hr.update(eps, ep0, p0, **P, a=a)
    assert r["converged"].all() and r["iters"].max() <= 8
    asym = np.abs(r["Ct"] - r["Ct"].transpose(0, 2, 1)).max() / np.abs(r["Ct"]).max()
    assert asym < 1e-13, asym


@pytest.mark.parametrize("a", hr.EXPONENTS)
def test_uniaxial_stress_follows_the_hardening_curve(a):
    """Under monotone uniaxial stress seq = |sigma| for every a: sigma = R0 + H p along the curve.  The lateral strain that keeps the
    lateral stress zero is found by Newton on the restatement's own tangent."""
    ep, p = np.zeros((1, 6)), np.zeros(1)
    lat = 0.0
    for e11 in np.linspace(3.5e-3, 8e-3, 6):
        for _ in range(30):
            r = hr.update(np.array([[e11, lat, lat, 0, 0, 0.0]]), ep, p, **P, a=a)
            s22 = r["sig"][0, 1]
            if abs(s22) < 1e-10 * P["R0"]:
                break
            lat -= s22 / (r["Ct"][0, 1, 1] + r["Ct"][0, 1, 2])
        assert abs(s22) < 1e-10 * P["R0"] and r["plastic"][0]
        assert abs(r["sig"][0, 0] - (P["R0"] + P["H"] * r["p"][0])) < 1e-9 * P["R0"]
        assert abs(r["sig"][0, 2]) < 1e-9 * P["R0"]
        ep, p = r["ep"], r["p"]


def test_descriptor_validation_and_names():
    el = jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"])
    b = jm.HosfordIsotropicHardening(el, jm.LinearHardening(P["R0"], P["H"]))
    assert b.a == 10.0 and b.law == _lib.LAW_HOSFORD_LINEAR == 10 and b.params() == [P["E"], P["nu"], P["R0"], P["H"], 10.0]
    assert list(b.flat_properties()) == ["elasticity.E", "elasticity.nu", "yield_stress.sig0", "yield_stress.H", "a"]
    for bad in (dict(a=1.9), dict(a=float("nan")), dict(a=float("inf"))):
        with pytest.raises(ValueError, match="Hosford"):
            jm.HosfordIsotropicHardening(el, jm.LinearHardening(P["R0"], P["H"]), **bad)
    for hard in (jm.LinearHardening(0.0, 1.0), jm.LinearHardening(100.0, -1.0)):
        with pytest.raises(ValueError, match="Hosford"):
            jm.HosfordIsotropicHardening(el, hard)
    for other in (jm.VoceHardening(200.0, 300.0, 10.0), lambda p: 200.0 + p):
        with pytest.raises(TypeError, match="linear hardening only"):
            jm.HosfordIsotropicHardening(el, other)
    props = {"young_modulus": 70e3, "poisson_ratio": 0.3, "R0": 200.0, "hardening_slope": 10.0}
    assert jm.HosfordIsotropicHardening.from_mfront_properties(props).params() == [70e3, 0.3, 200.0, 10.0, 10.0]
    assert jm.HosfordIsotropicHardening.from_mfront_properties({**props, "a": 6}).a == 6.0
    with pytest.raises(ValueError, match="missing \\['R0'\\]"):
        jm.HosfordIsotropicHardening.from_mfront_properties({k: v for k, v in props.items() if k != "R0"})
    with pytest.raises(ValueError, match="unknown \\['YoungModulus'\\]"):
        jm.HosfordIsotropicHardening.from_mfront_properties({**props, "YoungModulus": 1.0})


def test_law_table_row_and_unassigned_ids():
    i = _lib.law_info(_lib.LAW_HOSFORD_LINEAR)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total) == (6, 6, 5, 2, 7)
    assert [(i.isv_name[f].decode(), i.isv_dim[f]) for f in range(2)] == [("ElasticStrain", 6), ("EquivalentPlasticStrain", 1)]
    assert i.algorithmic_bytes_per_point == 48 + 48 + 288 + 56 + 104     # the hidden plastic strain is read and written, the elastic strain written
    for law in (6, 8, 9, 11):
        with pytest.raises(_lib.DxmError, match="unknown law id"):
            _lib.law_info(law)


def test_material_surface_without_a_gpu():
    m = JAXMaterial(jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"]), jm.LinearHardening(P["R0"], P["H"])))
    assert m.gradients == {"Strain": 6} and m.fluxes == {"Stress": 6}
    assert m.internal_state_variables == {"ElasticStrain": 6, "EquivalentPlasticStrain": 1}
    assert m.tangent_blocks == {("Stress", "Strain"): (6, 6)}
    for layout in ("coef", "pack4"):
        with pytest.raises(ValueError, match="general symmetric 6x6"):
            JAXMaterial(m.behavior, tangent_layout=layout)
    assert JAXMaterial(m.behavior, tangent_layout="sym").tangent_size == 21
