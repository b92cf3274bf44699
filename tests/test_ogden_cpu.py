"""CPU: the Ogden hyperelastic law (DXM_LAW_OGDEN) -- the numpy closed form ``ogden_ref.closed_form`` (what the kernel evaluates)
against the energy differentiated twice by AD, against the mpmath vectors at exactly and nearly repeated eigenvalues
(``tests/golden/ogden_degenerate.npz``), against closed-form facts that bypass both (identity, objectivity, symmetry), and the
Python layer over a test double of the library.

Error floor.  ``E0`` below is the largest error of the closed form (a) against the mpmath and AD references over the whole input
set, per row and relative to the row's largest reference magnitude (a row of the internal state variable is measured against the
stress of its point: it is one of the two parts that stress is the sum of, and vanishes on its own for a volumetric F).  Measured
on this suite's inputs: 1.2e-13 (the AD reference at alpha = 28.8; 1.8e-14 against mpmath); ``E0`` is that figure rounded up.  The
GPU suite's bound rests on it (``test_gpu_ogden.BOUND``)."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib

import ogden_ref as og

E0 = 2e-13   # see the module docstring; asserted by test_error_floor
EYE9 = np.array([[1.0, 1, 1, 0, 0, 0, 0, 0, 0]])


def errors(got, want):
    """(P, A, isv) against (P, A[, isv]): the largest per-row relative error of each."""
    eP = og.row_errors(got[0][:, None, :], want[0][:, None, :]).max()
    eA = og.row_errors(got[1], want[1]).max()
    out = [float(eP), float(eA)]
    if len(want) > 2:
        scale = np.maximum(np.abs(want[2]).max(axis=1), np.abs(want[0]).max(axis=1))
        out.append(float((np.abs(got[2] - want[2]).max(axis=1) / scale).max()))
    return out


def floor_figures():
    figs = {}
    for k, prm in enumerate(og.PARAM_SETS):
        F = og.random_F(200, seed=1 + k)
        figs[f"AD alpha={prm['alpha']}"] = max(errors(og.closed_form(F, **prm), og.energy_ad(F, **prm)))
    F, _, sets = og.load_golden()
    for prm, Pg, Ag, ig in sets:
        figs[f"mpmath alpha={prm['alpha']}"] = max(errors(og.closed_form(F, **prm), (Pg, Ag, ig)))
    return figs


def test_error_floor():
    figs = floor_figures()
    print("ogden error floor:", figs)
    assert max(figs.values()) <= E0, figs


@pytest.mark.parametrize("k", range(len(og.PARAM_SETS)))
def test_closed_form_matches_the_energy_differentiated_twice(k):
    prm = og.PARAM_SETS[k]
    F = og.random_F(64, seed=10 + k)
    eP, eA = errors(og.closed_form(F, **prm), og.energy_ad(F, **prm))
    assert eP <= E0 and eA <= E0, (eP, eA)


def test_closed_form_matches_mpmath_at_repeated_eigenvalues():
    F, labels, sets = og.load_golden()
    assert len(labels) == 2 * 2 * len(og.GAPS) and F.shape == (len(labels), 9)
    F2, labels2 = og.degenerate_F()
    assert np.array_equal(F, F2) and labels == labels2          # the stored inputs are the generator's
    for prm, Pg, Ag, ig in sets:
        got = og.closed_form(F, **prm)
        assert np.isfinite(got[1]).all()
        e = errors(got, (Pg, Ag, ig))
        assert max(e) <= E0, (prm, e)


def test_golden_vector_reproduces_in_mpmath():
    F, labels, sets = og.load_golden()
    k = labels.index("two-fold gap 0 axis-aligned")
    prm, Pg, Ag, ig = sets[0]
    P, A, isv = og.closed_form_mp(F[k], **prm)
    assert np.array_equal(P, Pg[k]) and np.array_equal(A, Ag[k]) and np.array_equal(isv, ig[k])


@pytest.mark.parametrize("prm", og.PARAM_SETS)
def test_identity_is_stress_free_with_the_isotropic_elastic_tangent(prm):
    P, A, isv = og.closed_form(EYE9, **prm)
    assert np.array_equal(P, np.zeros((1, 9))) and np.abs(isv).max() == 0.0
    G, K = prm["mu"] * prm["alpha"] / 2.0, prm["K"]
    want = np.zeros((9, 9))
    for r in range(9):
        i, J = int(og.TI[r]), int(og.TJ[r])
        for c in range(9):
            k, L = int(og.TI[c]), int(og.TJ[c])
            want[r, c] = (K - 2.0 * G / 3.0) * float(i == J and k == L) + G * (float(i == k and J == L) + float(i == L and J == k))
    assert np.abs(A[0] - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()


def test_objectivity_and_major_symmetry():
    prm = og.DEFAULTS
    F9 = og.random_F(32, seed=3)
    Q = og._rotation([0.3, -1.0, 0.5], 1.1)
    P, A, isv = og.closed_form(F9, **prm)
    Pq, Aq, isvq = og.closed_form(og.to_vector(Q @ og.to_matrix(F9)), **prm)
    want = og.to_vector(Q @ og.to_matrix(P))
    assert np.abs(Pq - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(isvq - isv).max() <= 1e-12 * np.abs(P).max()       # S is a function of C = F^T F alone
    assert np.abs(A - A.transpose(0, 2, 1)).max() <= 1e-14 * np.abs(A).max()


def test_inverted_points_give_nan():
    F9 = np.array([[1.0, 1, -1, 0, 0, 0, 0, 0, 0], [1.0, 1, 0, 0, 0, 0, 0, 0, 0]])
    P, A, isv = og.closed_form(F9, **og.DEFAULTS)
    assert np.isnan(P).all() and np.isnan(A).all() and np.isnan(isv).all()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_behaviour_descriptor():
    b = jm.OgdenHyperelasticity(mu=2.0, alpha=4.0, K=10.0)
    assert b.law == _lib.LAW_OGDEN == 7 and b.params() == [4.0, 2.0, 10.0]
    assert b.flat_properties() == {"alpha": 4.0, "mu": 2.0, "K": 10.0}
    d = jm.OgdenHyperelasticity.from_mfront_properties({})
    assert d.params() == [28.8, 27778.0, 69444444.0] == jm.OgdenHyperelasticity().params()
    assert jm.OgdenHyperelasticity.from_mfront_properties({"mu": 3.0}).params() == [28.8, 3.0, 69444444.0]
    with pytest.raises(ValueError, match="unknown"):
        jm.OgdenHyperelasticity.from_mfront_properties({"YoungModulus": 1.0})
    for bad in (dict(alpha=0.0), dict(mu=-1.0), dict(K=0.0), dict(K=float("nan"))):
        with pytest.raises(ValueError, match="Ogden"):
            jm.OgdenHyperelasticity(**bad)


def test_law_table_row():
    with pytest.raises(_lib.DxmError, match="unknown law id"):
        _lib.law_info(6)                      # not assigned: the new law took 7
    with pytest.raises(_lib.DxmError, match="unknown law id"):
        _lib.law_info(_lib.LAW_OGDEN + 1)
    i = _lib.law_info(_lib.LAW_OGDEN)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (9, 9, 3, 1, 6, 840)
    assert i.isv_name[0] == b"PK2Stress" and i.isv_dim[0] == 6 and 72 + 72 + 648 + 48 == 840


def test_create_without_a_gpu_fails_loudly_for_the_new_law_too():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    prm = (C.c_double * 3)(28.8, 27778.0, 69444444.0)
    assert not lib.dxm_create(_lib.LAW_OGDEN, prm, 3, 8, 0)
    assert b"no usable HIP device" in lib.dxm_last_error()


@pytest.fixture
def fake(monkeypatch):
    from fake_dxmat_ogden import FakeDxmatOgden

    f = FakeDxmatOgden(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: f)
    return f


def test_material_over_the_test_double(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    n = 37
    m = JAXMaterial(jm.OgdenHyperelasticity())
    assert m.gradients == {"DeformationGradient": 9} and m.fluxes == {"FirstPiolaKirchhoffStress": 9}
    assert m.internal_state_variables == {"PK2Stress": 6}
    assert m.tangent_blocks == {("FirstPiolaKirchhoffStress", "DeformationGradient"): (9, 9)} and m.tangent_size == 81
    assert m.algorithmic_bytes_per_point == 840 and m.name == "OgdenHyperelasticity"
    m.set_data_manager(n)
    s0 = m.get_initial_state_dict()
    assert np.array_equal(s0["DeformationGradient"], np.tile(EYE9, (n, 1))) and not s0["PK2Stress"].any()
    F = og.random_F(n, seed=5)
    P, isv, A = m.integrate(F)
    Pr, Ar, ir = og.closed_form(F, **og.DEFAULTS)
    assert np.array_equal(np.array(P), Pr) and np.array_equal(np.array(A).reshape(n, 9, 9), Ar) and np.array_equal(np.array(isv), ir)
    assert A.shape == (n, 9, 9) and np.array(isv).shape == (n, 6)
    s1 = m.get_final_state_dict()
    assert set(s1) == {"DeformationGradient", "FirstPiolaKirchhoffStress", "PK2Stress"}
    assert np.array_equal(np.array(s1["PK2Stress"]), ir) and not np.array(m.get_initial_state_dict()["PK2Stress"]).any()
    m.data_manager.update()
    assert np.array_equal(np.array(m.get_initial_state_dict()["PK2Stress"]), ir)
    # explicit state in, explicit state out (a scratch material of the same behaviour), and an initial state set field by field
    Ct, new = m.batched_constitutive_update(F, m.natural_state(n))
    assert np.array_equal(np.array(new["FirstPiolaKirchhoffStress"]), Pr) and np.array_equal(np.array(new["PK2Stress"]), ir)
    assert np.array_equal(np.asarray(Ct).reshape(n, 9, 9), Ar)
    m.set_initial_state_dict({"DeformationGradient": F, "PK2Stress": 2.0 * ir})
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.array(s0["DeformationGradient"]), F) and np.array_equal(np.array(s0["PK2Stress"]), 2.0 * ir)
    # uniform property updates reach the handle; a refused value leaves descriptor and handle as they were
    m.update_material_property("mu", 1000.0)
    assert fake.last_params == [28.8, 1000.0, 69444444.0] and m.material_properties["mu"] == 1000.0
    P2 = np.array(m.integrate(F)[0])
    assert np.array_equal(P2, og.closed_form(F, 28.8, 1000.0, 69444444.0)[0])
    with pytest.raises(_lib.DxmError, match="mu must be"):
        m.update_material_property("mu", -1.0)
    assert m.behavior.mu == 1000.0 and m.material_properties["mu"] == 1000.0
    with pytest.raises(ValueError, match="Unknown material property"):
        m.update_material_property("E", 1.0)
    with pytest.raises(NotImplementedError, match="varies from point to point"):
        m.update_material_property("K", np.linspace(1.0, 2.0, n))
    m.close()


def test_refusals(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            JAXMaterial(jm.OgdenHyperelasticity(), tangent_layout=layout)
    m = JAXMaterial(jm.OgdenHyperelasticity(), property_fields=True)
    m.set_data_manager(4)
    with pytest.raises(NotImplementedError, match="Ogden"):
        m.update_material_property("K", np.array([1.0, 2.0, 3.0, 4.0]))
    # the C ABI's own words for the two things the kernel does not do
    assert fake.dxm_set_tangent_layout(m._parts[0][0], 1) < 0 and b"no packed tangent record" in fake.dxm_last_error()
    assert fake.dxm_integrate_displacement(m._parts[0][0], None, None, 0.0, None, None, None, None) < 0
    assert b"no fused displacement-gradient form" in fake.dxm_last_error()
    m.close()
