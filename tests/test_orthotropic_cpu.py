"""CPU: the numpy restatement of orthotropic elasticity in a material frame (``orthotropic_ref.update``) against the committed 50-digit
fourth-order-tensor results (``tests/golden/orthotropic_frames.npz``), ``numpy.linalg.inv``, the isotropic oracle, the exchange of
axes under a quarter turn and the cubic statement of the reference's single-crystal test; the behaviour descriptor, the law-table row
of the built library and the ``rotation_matrix`` rules of the material."""
import json
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp

import orthotropic_ref as orf

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orthotropic_frames.npz"))
META = json.loads(str(GOLD["meta"]))
SETS = orf.PARAMETER_SETS


def measured_deviation():
    worst = [0.0, 0.0]
    for name, p in SETS.items():
        sig, ct = orf.update(GOLD[f"{name}/eps"], p, GOLD[f"{name}/R"])
        for k, (got, want) in enumerate(((sig, GOLD[f"{name}/sig"]), (ct, GOLD[f"{name}/ct"]))):
            worst[k] = max(worst[k], float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


def test_the_fixture_covers_every_set_and_frame_class_and_records_the_restatements_deviation():
    assert META["sets"] == {k: list(v) for k, v in SETS.items()} and META["digits"] == 50
    for name in SETS:
        assert set(GOLD[f"{name}/labels"]) == set(orf.FRAME_CLASSES) and len(GOLD[f"{name}/eps"]) == META["points_per_set"] >= 50
        R = GOLD[f"{name}/R"]
        assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-15 and np.allclose(np.linalg.det(R), 1.0)
        near = R[GOLD[f"{name}/labels"] == "near_identity"]
        assert 0 < np.abs(near - np.eye(3)).max() < 1e-9
        assert 3e-4 < np.abs(GOLD[f"{name}/eps"]).mean() < 3e-3
    dev = measured_deviation()
    print("restatement deviation (stress, tangent):", dev)
    # measured here, stored there; the platform's einsum may round differently in the last place
    assert dev[0] <= 2 * META["restatement_deviation"]["stress"] and dev[1] <= 2 * META["restatement_deviation"]["tangent"]
    # far from a conditioning defect: the GPU bound max(1e-12, 8 x deviation) lands on 1e-12
    assert max(META["restatement_deviation"].values()) < 1e-13
    assert max(1e-12, 8 * max(META["restatement_deviation"].values())) == 1e-12


@pytest.mark.parametrize("name", list(SETS))
def test_restatement_equals_mpmath_live_on_a_few_points(name):
    pytest.importorskip("mpmath")
    for i in (0, 8, 9):   # identity, random, near identity
        sig, ct = orf.update_mp(GOLD[f"{name}/eps"][i], SETS[name], GOLD[f"{name}/R"][i])
        assert np.array_equal(sig, GOLD[f"{name}/sig"][i]) and np.array_equal(ct, GOLD[f"{name}/ct"][i])


@pytest.mark.parametrize("name", list(SETS))
def test_stiffness_is_the_inverse_of_the_compliance(name):
    p = SETS[name]
    C, H = orf.stiffness(p), orf.host_stiffness(p)
    assert np.abs(H[:3, :3] - np.linalg.inv(orf.compliance(p))).max() / np.abs(C).max() < 1e-14
    assert np.abs(H[:3, :3] @ orf.compliance(p) - np.eye(3)).max() < 1e-14
    assert np.array_equal(H, H.T) and np.array_equal(np.diag(H)[3:], [2 * p[6], 2 * p[8], 2 * p[7]])
    assert np.all(np.linalg.eigvalsh(C) > 0)


def test_isotropic_parameters_give_the_elastic_oracle_in_any_frame():
    E, nu = 70e3, 0.3
    p = SETS["isotropic"]
    eps = orf.strains(400, seed=3)
    _, R = orf.frames(400, seed=4)
    sig, ct = orf.update(eps, p, R)
    want_sig, want_ct = onp.elastic_iso(eps, E, nu)
    assert np.abs(sig - want_sig).max() / np.abs(want_sig).max() < 1e-13
    assert np.abs(ct - want_ct).max() / np.abs(want_ct).max() < 1e-13
    sig0, ct0 = orf.update(eps, p)
    assert np.abs(sig0 - want_sig).max() / np.abs(want_sig).max() < 1e-13 and np.abs(ct0 - want_ct).max() / np.abs(want_ct).max() < 1e-13


def test_quarter_turn_about_z_exchanges_axes_1_and_2():
    E1, E2, E3, nu12, nu23, nu13, G12, G23, G13 = p = SETS["strong"]
    swapped = [E2, E1, E3, nu12 * E2 / E1, nu13, nu23, G12, G13, G23]
    eps = orf.strains(200, seed=5)
    sig, ct = orf.update(eps, p, orf.axis_rotation(2, np.pi / 2))
    # the material axes are (y, -x, z): eps_m = [eps_yy, eps_xx, eps_zz, -eps_xy, eps_yz, -eps_xz] in Mandel components, the stress comes
    # back through the same permutation and signs
    perm, sign = [1, 0, 2, 3, 5, 4], np.array([1, 1, 1, -1, 1, -1.0])
    sm, cm = orf.update(eps[:, perm] * sign, p)
    back_s, back_c = np.empty_like(sm), np.empty_like(cm)
    back_s[:, perm] = sm * sign
    back_c[np.ix_(range(200), perm, perm)] = cm * np.outer(sign, sign)
    assert np.abs(sig - back_s).max() / np.abs(sig).max() < 1e-13 and np.abs(ct - back_c).max() / np.abs(ct).max() < 1e-13
    # ... which is the unrotated law with axes 1 and 2 exchanged (the signs cancel in an orthotropic stiffness)
    sig_s, ct_s = orf.update(eps, swapped)
    assert np.abs(sig - sig_s).max() / np.abs(sig).max() < 1e-13 and np.abs(ct - ct_s).max() / np.abs(ct).max() < 1e-13
    assert np.abs(ct_s[0] - orf.stiffness(p)).max() / np.abs(ct).max() > 1e-2   # and not the law itself


def test_cubic_parameters_agree_at_0_and_pi_2_and_differ_at_pi_4_and_pi_3():
    """the statement of test_mfront_single_cristal (tests/mfront/test_elastoplasticity.py:39-62) for the elastic part"""
    p = SETS["cubic"]
    eps = orf.strains(100, seed=6)
    at = {a: orf.update(eps, p, orf.axis_rotation(2, a)) for a in (0.0, np.pi / 4, np.pi / 3, np.pi / 2)}
    scale = np.abs(at[0.0][0]).max()
    assert np.abs(at[np.pi / 2][0] - at[0.0][0]).max() / scale < 1e-13
    assert np.abs(at[np.pi / 2][1] - at[0.0][1]).max() / np.abs(at[0.0][1]).max() < 1e-13
    for a in (np.pi / 4, np.pi / 3):
        assert np.abs(at[a][0] - at[0.0][0]).max() / scale > 1e-2
    # ... and the isotropic brick values do not see the frame at all
    b = [orf.update(eps, SETS["brick"], orf.axis_rotation(2, a))[0] for a in (0.0, np.pi / 4, np.pi / 3)]
    assert np.abs(b[1] - b[0]).max() / scale < 1e-13 and np.abs(b[2] - b[0]).max() / scale < 1e-13


def test_the_restatement_is_the_reference_cadence_and_q_is_orthogonal():
    eps = orf.strains(300, seed=7)
    _, R = orf.frames(300, seed=8)
    Q = orf.mandel_rotation(R)
    assert np.abs(np.einsum("nai,naj->nij", Q, Q) - np.eye(6)).max() < 1e-14
    for name, p in SETS.items():
        a, b = orf.update(eps, p, R), orf.update_reference_cadence(eps, p, R)
        assert np.abs(a[0] - b[0]).max() / np.abs(a[0]).max() < 1e-14 and np.abs(a[1] - b[1]).max() / np.abs(a[1]).max() < 1e-14


def test_law_table_row_and_unassigned_ids():
    assert _lib.LAW_ORTHOTROPIC_ELASTIC == 12
    i = _lib.law_info(12)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total) == (6, 6, 9, 0, 0)
    assert i.algorithmic_bytes_per_point == 48 + 48 + 288
    for law in (6, 8, 9, 11, 13):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
    assert _lib.load().dxm_frame_kind(None) == -1 and _lib.load().dxm_abi_version() == 6


def test_descriptor_names_and_parameter_refusals():
    p = SETS["strong"]
    b = jm.OrthotropicElasticity(*p)
    assert b.law == 12 and b.params() == p and (b.gradient_name, b.flux_name) == ("Strain", "Stress")
    assert list(b.flat_properties()) == ["YoungModulus1", "YoungModulus2", "YoungModulus3", "PoissonRatio12", "PoissonRatio23", "PoissonRatio13",
                                         "ShearModulus12", "ShearModulus23", "ShearModulus13"]
    assert list(b.flat_properties().values()) == p
    assert jm.OrthotropicElasticity.from_mfront_properties(b.flat_properties()).params() == p
    b.YoungModulus2 = 50e3
    assert b.E2 == 50e3 and b.YoungModulus2 == 50e3
    with pytest.raises(ValueError, match="missing \\['ShearModulus13'\\]"):
        jm.OrthotropicElasticity.from_mfront_properties({k: v for k, v in b.flat_properties().items() if k != "ShearModulus13"})
    for idx, value, text in ((0, 0.0, "E1 must be > 0, got 0.0"), (2, -1.0, "E3 must be > 0, got -1.0"), (7, 0.0, "G23 must be > 0"),
                             (3, float("nan"), "nu12 must be finite"), (1, float("inf"), "E2 must be finite"),
                             (3, 2.3, "not positive definite"), (4, 2.1, "not positive definite")):
        q = list(p)
        q[idx] = value
        with pytest.raises(ValueError, match=text):
            jm.OrthotropicElasticity(*q)


def test_material_surface_and_rotation_matrix_rules_without_a_gpu():
    m = JAXMaterial(jm.OrthotropicElasticity(*SETS["strong"]))
    assert m.gradients == {"Strain": 6} and m.fluxes == {"Stress": 6} and m.internal_state_variables == {}
    assert m.tangent_blocks == {("Stress", "Strain"): (6, 6)} and m.frame_fused and m.rotation_matrix is None
    assert m.material_properties["YoungModulus1"] == SETS["strong"][0]
    for layout in ("coef", "pack4"):
        with pytest.raises(ValueError, match="general symmetric 6x6"):
            JAXMaterial(m.behavior, tangent_layout=layout)
    assert JAXMaterial(m.behavior, tangent_layout="sym").tangent_size == 21
    R = orf.axis_rotation(2, np.pi / 3)
    m.rotation_matrix = R.tolist()                      # a 3x3 array-like: a uniform frame
    assert np.array_equal(m.rotation_matrix, R) and m._frame.shape == (3, 3)
    expr = object()                                     # anything else is kept for the map to evaluate (mfront.py:83)
    m.rotation_matrix = expr
    assert m.rotation_matrix is expr
    m.rotation_matrix = None
    assert m.rotation_matrix is None and m._frame is None
    with pytest.raises(ValueError, match="shape"):
        m.set_frame(np.zeros((4, 4)))
    # the hooks the reference's update() calls: the gradient is left untouched, flux and tangent too
    g = np.arange(12.0)
    _, frames = orf.frames(2, seed=1)
    frames[1] = R
    m.rotate_gradients(g, frames.ravel())
    assert np.array_equal(g, np.arange(12.0)) and m._frame.shape == (2, 9)
    m.rotate_gradients(g, np.tile(R.ravel(), 2))        # all rows equal: the uniform form
    assert m._frame.shape == (3, 3)
    f = np.arange(12.0)
    assert m.rotate_fluxes(f, frames.ravel()) is None and m.rotate_tangent_operator(f, frames.ravel()) is None and np.array_equal(f, g)
    # every other behaviour keeps rotation_matrix None, and assigning it raises
    iso = JAXMaterial(jm.ElasticBehavior(jm.LinearElasticIsotropic(E=1.0, nu=0.2)))
    assert iso.rotation_matrix is None and not iso.frame_fused
    with pytest.raises(AttributeError, match="isotropic"):
        iso.rotation_matrix = np.eye(3)
    with pytest.raises(_lib.DxmError, match="isotropic"):
        iso.set_frame(np.eye(3))
