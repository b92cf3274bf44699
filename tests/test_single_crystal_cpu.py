"""No GPU: the FCC single-crystal viscoplastic law (law id 14) as its float64 restatement ``single_crystal_ref`` against the committed
50-digit fixture, its tangent, the material-point form of the reference's ``test_mfront_single_cristal``, the interaction classes,
the row of the law table and the Python surface (behaviour class, refusals, ``dt``, frame hooks)."""
import json
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.jaxmat import JAXMaterial

import single_crystal_ref as sc

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_crystal_kat.npz"))
META = json.loads(str(GOLD["meta"]))
PRM = sc.param_vector()


def restated(m):
    """the restatement at the fixture points of mask m (one parameter set), from their recorded state"""
    prm = GOLD["params"][int(GOLD["set"][m][0])]
    state = {"eel": GOLD["eel0"][m], "g": GOLD["g0"][m], "p": GOLD["p0"][m], "a": GOLD["a0"][m]}
    has = GOLD["has_frame"][m]
    out = {}
    for flag in (False, True):
        k = has == flag
        if k.any():
            o = sc.update(GOLD["eps"][m][k], {n: v[k] for n, v in state.items()}, prm, META["dt"], R=GOLD["R"][m][k] if flag else None)
            for n, v in o.items():
                out.setdefault(n, np.zeros((int(m.sum()),) + v.shape[1:], dtype=v.dtype))[k] = v
    return out


def test_the_fixture_covers_every_cell_and_the_restatement_deviates_by_what_it_records():
    assert len(GOLD["eps"]) == 250 and META["digits"] == 50
    assert sorted(set(zip(GOLD["set"].tolist(), GOLD["frame"].tolist(), GOLD["stage"].tolist()))) == [(s, f, g) for s in range(2) for f in range(5) for g in range(5)]
    stage = GOLD["stage"]
    assert GOLD["plastic"][stage == 0].sum() == 0 and GOLD["plastic"][(stage == 2) | (stage == 4)].all()
    assert (np.abs(GOLD["g0"][stage == 3]).max(axis=1) > 0).all()      # after the reversal: slip from the way up, whatever the last increment does
    dev = {"stress": 0.0, "tangent": 0.0, "state": 0.0}
    for si in range(2):
        m = GOLD["set"] == si
        o = restated(m)
        assert (o["status"] == 0).all() and (o["halvings"] == 0).all() and o["iters"].max() <= 12
        for i in range(int(m.sum())):      # per point, as the generator measured it
            S, T = GOLD["stress"][m][i], GOLD["tangent"][m][i]
            dev["stress"] = max(dev["stress"], np.abs(o["stress"][i] - S).max() / np.abs(S).max())
            dev["tangent"] = max(dev["tangent"], np.abs(o["tangent"][i] - T).max() / np.abs(T).max())
            scale = max(np.abs(GOLD[k][m][i]).max() for k in ("eel", "g", "p", "a"))
            dev["state"] = max(dev["state"], max(np.abs(o[k][i] - GOLD[k][m][i]).max() for k in ("eel", "g", "p", "a")) / scale)
    print("restatement against 50 digits:", dev, "recorded:", META["restatement_deviation"])
    for k, v in dev.items():
        assert v <= 2 * META["restatement_deviation"][k] + 1e-16, (k, v)
    assert max(META["restatement_deviation"]["stress"], META["restatement_deviation"]["state"]) < 1e-14
    assert META["restatement_deviation"]["tangent"] < 1e-11


def test_tangent_against_central_differences_and_its_antisymmetric_part():
    m = (GOLD["set"] == 0) & (GOLD["stage"] >= 1)
    o = restated(m)
    n = int(m.sum())
    prm = GOLD["params"][0]
    state = {"eel": GOLD["eel0"][m], "g": GOLD["g0"][m], "p": GOLD["p0"][m], "a": GOLD["a0"][m]}
    R = np.where(GOLD["has_frame"][m][:, None, None], GOLD["R"][m], np.eye(3))      # the identity frame is no frame, to round-off
    h = 1e-8
    fd = np.zeros((n, 6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        fd[:, :, k] = (sc.update(GOLD["eps"][m] + e, state, prm, META["dt"], R=R)["stress"] - sc.update(GOLD["eps"][m] - e, state, prm, META["dt"], R=R)["stress"]) / (2 * h)
    scale = np.abs(o["tangent"]).max()
    err = np.abs(fd - o["tangent"]).max() / scale
    print("tangent against central differences:", err)
    assert err <= 1e-7
    T = GOLD["tangent"][m]
    anti50, anti = 0.5 * (T - T.transpose(0, 2, 1)), 0.5 * (o["tangent"] - o["tangent"].transpose(0, 2, 1))
    assert np.abs(anti - anti50).max() / scale <= max(1e-12, 8 * META["restatement_deviation"]["tangent"])
    assert np.abs(anti50).max() / np.abs(T).max() > 1e-8      # the fixture cannot degenerate to symmetric blocks
    assert META["max_antisymmetric_part"] > 1e-8


def test_material_point_form_of_the_reference_single_crystal_test():
    """strain [exx, eyy, 0, exy, 0, 0] with sigma_yy = sigma_xy = 0 by Newton with the law's own tangent; 50 increments to 5e-3,
    dt = 0.1, the crystal turned about z by 0, pi/4, pi/3, pi/2 (four points of one batch)"""
    R = np.array([sc.rot_z(a) for a in (0.0, np.pi / 4, np.pi / 3, np.pi / 2)])
    st = sc.zero_state(4)
    eps = np.zeros((4, 6))
    free = [1, 3]
    first, outer_max, it_max, halv = None, 0, 0, 0
    for k in range(1, 51):
        eps[:, 0] = k * 1e-4
        for outer in range(1, 30):
            out = sc.update(eps, st, PRM, 0.1, R=R)
            assert (out["status"] == 0).all()
            r = out["stress"][:, free]
            if np.abs(r).max() <= 1e-9:
                break
            K = out["tangent"][:, free][:, :, free]
            eps[:, free] -= np.linalg.solve(K, r[:, :, None])[:, :, 0]
        else:
            raise AssertionError("the outer Newton did not converge")
        outer_max, it_max, halv = max(outer_max, outer), max(it_max, out["iters"].max()), halv + out["halvings"].sum()
        st = sc.next_state(out)
        if k == 1:
            first = out["stress"][:, 0].copy()
    sxx = out["stress"][:, 0]
    print("sigma_xx at 0 / 45 / 60 / 90 degrees:", sxx, "local iterations <=", it_max, "halvings", halv, "outer iterations <=", outer_max)
    assert np.abs(first - first[0]).max() <= 1e-9 * abs(first[0])          # cubic elasticity with these constants: the same first increment
    assert abs(sxx[0] - sxx[3]) <= 1e-9 * abs(sxx[0])
    assert abs(sxx[1] - sxx[0]) > 0.1 * abs(sxx[0]) and abs(sxx[2] - sxx[0]) > 0.1 * abs(sxx[0])
    assert halv == 0 and it_max <= 12
    # the values of the 50-digit law on the same path (tests/golden/make_single_crystal.py::material_point_path: its own state, its own
    # outer Newton to 1e-25).  The outer Newton here stops at a residual stress of 1e-9, which moves sigma_xx by as much times a
    # stiffness ratio of order one: 1e-9 of the 23 ... 470 it is compared with, taken as 1e-9 relative
    assert np.allclose(GOLD["mp_angles"], [0.0, np.pi / 4, np.pi / 3, np.pi / 2])
    print("50 digits:", GOLD["mp_last_sxx"], "deviation", np.abs(sxx - GOLD["mp_last_sxx"]) / GOLD["mp_last_sxx"])
    assert (np.abs(sxx - GOLD["mp_last_sxx"]) <= 1e-9 * GOLD["mp_last_sxx"]).all()
    assert (np.abs(first - GOLD["mp_first_sxx"]) <= 1e-9 * GOLD["mp_first_sxx"]).all()


def test_interaction_classes_and_slip_systems():
    cls = sc.interaction_classes()
    assert np.array_equal(cls, cls.T)
    for row in cls:      # self, coplanar, Hirth, collinear, glissile, Lomer
        assert np.bincount(row, minlength=6).tolist() == [1, 2, 2, 1, 4, 2]
    n, s, plane = sc.systems()
    assert len(n) == 12 and (np.einsum("ij,ij->i", n, s) == 0).all() and plane.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    mu = sc.schmid()
    assert np.allclose(mu[:, :3].sum(axis=1), 0.0) and np.allclose((mu ** 2).sum(axis=1), 0.5)
    D = sc.stiffness(PRM)
    assert np.linalg.matrix_rank(mu @ D @ mu.T, tol=1e-6) == 5      # why the local Newton pivots


def test_law_table_row_and_unassigned_ids():
    assert _lib.LAW_SINGLE_CRYSTAL_FCC == 14
    i = _lib.law_info(14)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total) == (6, 6, 22, 4, 42)
    assert i.algorithmic_bytes_per_point == 48 + 288 + 48 + 288 + 336 == 1008
    assert [i.isv_name[f].decode() for f in range(4)] == ["ElasticStrain", "ViscoplasticSlip", "EquivalentViscoplasticSlip", "BackStrain"]
    assert [i.isv_dim[f] for f in range(4)] == [6, 12, 12, 12]
    for law in (13, 15):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
    assert _lib.load().dxm_abi_version() == 6


def test_behaviour_class_parameters_and_refusals():
    b = jm.MericCailletaudSingleCrystalViscoPlasticity.from_mfront_properties({"YoungModulus1": 208000.0})
    assert b.law == 14 and np.array_equal(b.params(), PRM) and len(b.params()) == 22
    assert b.interaction == (1.0, 1.0, 0.6, 12.3, 1.6, 1.8) and b.YoungModulus1 == 208000.0
    b.YoungModulus1 = 150e3
    b.K = 30.0
    assert b.params()[0] == 150e3 and b.params()[10] == 30.0
    with pytest.raises(ValueError, match="YoungModulus1 is required"):
        jm.MericCailletaudSingleCrystalViscoPlasticity.from_mfront_properties({})
    for kw, text in ((dict(n=0.5), "n must be >= 1, got 0.5"), (dict(K=0.0), "K must be > 0, got 0.0"), (dict(tau0=-1.0), "tau0 must be >= 0, got -1.0"),
                     (dict(b=-1.0), "b must be >= 0"), (dict(d=-2.0), "d must be >= 0, got -2.0"), (dict(C=-1.0), "C must be >= 0"),
                     (dict(Q=float("nan")), "Q must be finite"), (dict(interaction=(1, 2, 3)), "six coefficients")):
        with pytest.raises(ValueError, match=text):
            jm.MericCailletaudSingleCrystalViscoPlasticity(*PRM[:9], **kw)
    with pytest.raises(ValueError, match="E1 must be > 0"):
        jm.MericCailletaudSingleCrystalViscoPlasticity(-1.0, *PRM[1:9])


def test_material_surface_dt_and_frame_rules_without_a_gpu():
    b = jm.MericCailletaudSingleCrystalViscoPlasticity.from_mfront_properties({"YoungModulus1": 208000.0})
    m = JAXMaterial(b)
    assert m.gradients == {"Strain": 6} and m.fluxes == {"Stress": 6}
    assert m.internal_state_variables == {"ElasticStrain": 6, "ViscoplasticSlip": 12, "EquivalentViscoplasticSlip": 12, "BackStrain": 12}
    assert m.tangent_blocks == {("Stress", "Strain"): (6, 6)} and m.frame_fused and m.rotation_matrix is None
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="not symmetric"):
            JAXMaterial(b, tangent_layout=layout)
    # dt: the attribute when the call names none (mfront.py:267), the argument otherwise
    assert m.dt == 0.0 and m._dt(None) == 0.0
    m.dt = 1e-1
    assert m._dt(None) == 0.1 and m._dt(0.25) == 0.25 and m._dt(0) == 0.0
    R = sc.rot_z(np.pi / 3)
    m.rotation_matrix = R.tolist()
    assert np.array_equal(m.rotation_matrix, R) and m._frame.shape == (3, 3)
    g = np.arange(12.0)
    m.rotate_gradients(g, np.concatenate([R.ravel(), np.eye(3).ravel()]))
    assert np.array_equal(g, np.arange(12.0)) and m._frame.shape == (2, 9)
    assert m.rotate_fluxes(g, np.tile(R.ravel(), 2)) is None and m.rotate_tangent_operator(g, np.tile(R.ravel(), 2)) is None
    m.rotation_matrix = None
    assert m._frame is None
