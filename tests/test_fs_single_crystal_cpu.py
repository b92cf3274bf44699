"""CPU: the finite-strain FCC single-crystal law (law id 21) -- the conditions on the 50-digit fixture, the float64 restatement
against it (the origin of the GPU bounds), known answers that bypass the fixture, the Python descriptor, the law-table row.

Measured deviations of the restatement from the fixture (per point, relative to the field's scale at the point): stress 2.6e-12
(an unloaded point: the Green-Lagrange strain is a difference of numbers near 1), tangent 7.7e-12 (the distance of the last-but-one
iterate from the root), state 6.7e-16.  GPU bounds max(1e-12, 8 x): 2.1e-11, 6.2e-11, 1e-12.

Small-strain limit, measured: the stress differs from law 14's restatement by 4.8e-4 of its scale at |F - I| = 4e-4 and by 1.2e-4
at 1e-4 (the elastic range; it falls linearly with the strain)."""
import ctypes as C

import numpy as np
import pytest

from dolfinx_materials_amd import _lib
import dolfinx_materials_amd.materials as jm

import fs_single_crystal_cases as cs
import fs_single_crystal_ref as fx
import single_crystal_ref as sc

GOLD, META = cs.GOLD, cs.META
EYE9 = np.array([1.0, 1, 1, 0, 0, 0, 0, 0, 0])


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_fixture_conditions():
    n = len(GOLD["F"])
    assert n == 180 and sorted(set(GOLD["pset"])) == [0, 1] and sorted(set(GOLD["has_frame"])) == [0, 1, 2]
    assert sorted(set(GOLD["dt"])) == [1e-3, 0.1, 10.0] and sorted(set(GOLD["stage"])) == list(range(10))
    # every increment |dF|_F <= 5e-4: the histories are runs of ten consecutive points that start from the identity
    F = GOLD["F"].reshape(18, 10, 9)
    prev = np.concatenate([np.broadcast_to(EYE9, (18, 1, 9)), F[:, :-1]], axis=1)
    assert np.linalg.norm(F - prev, axis=2).max() <= 5e-4 * (1 + 1e-9)
    assert np.array_equal(GOLD["Fp0"].reshape(18, 10, 9)[:, 0], np.broadcast_to(EYE9, (18, 9)))
    # the stages: virgin elastic first, yielded at the second and third, unloading elastic, flow again in the reversal or the turn,
    # which has shear and rotation in F
    y = GOLD["yielded"].reshape(18, 10)
    assert not y[:, 0].any() and y[:, 1:4].all() and not y[:, 4].any() and y[:, 7:].any(axis=1).all()
    skew = fx.to_mat(F[:, 9] - F[:, 7])
    assert (np.abs(skew - skew.transpose(0, 2, 1)).max(axis=(1, 2)) > 1e-4).all()
    assert GOLD["yielded"].mean() >= 0.5 and META["yielded_fraction"] == GOLD["yielded"].mean()
    # the parameter sets: the file's constants with self-hardening only; all six coefficients and d = 0
    p0, p1 = GOLD["params"]
    assert np.array_equal(p0, fx.param_vector()) and np.array_equal(p0[10:], [1, 0, 0, 0, 0, 0])
    assert (p1[10:] != 0).all() and p1[8] == 0.0
    # frames: none, a symmetry rotation of the cube, generic
    R = GOLD["R"]
    assert np.array_equal(R[GOLD["has_frame"] == 0], np.broadcast_to(np.eye(3), (60, 3, 3)))
    Rs = R[GOLD["has_frame"] == 1][0]
    assert sorted(np.abs(Rs).ravel()) == [0] * 6 + [1] * 3 and np.linalg.det(Rs) == 1
    Rg = R[GOLD["has_frame"] == 2][0]
    assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-15 and np.abs(Rg).min() > 1e-2
    # the tangent has no symmetry to exploit
    T = GOLD["tangent"]
    assert np.abs(T - T.transpose(0, 2, 1)).max() / np.abs(T).max() > 1e-6


def test_restatement_converges_everywhere_and_its_deviation_is_the_recorded_one():
    worst = {"stress": 0.0, "tangent": 0.0, "state": 0.0}
    iters = 0
    for pset in (0, 1):
        for dt in (1e-3, 0.1, 10.0):
            inp, gold = cs.fixture_group(pset, dt)
            out = fx.update(inp["F"], inp["state"], GOLD["params"][pset], dt, R=inp["R"], maxit=cs.MAXIT)
            assert (out["status"] == 0).all() and np.array_equal(out["plastic"], gold["plastic"])
            iters = max(iters, int(out["iters"].max()))
            for k, v in zip(("stress", "tangent", "state"), cs.errors(out, gold)):
                worst[k] = max(worst[k], v)
    print("restatement against the 50-digit fixture:", worst, "iterations", iters)
    assert iters == META["restatement_max_iters"] <= 26
    for k, v in worst.items():
        assert v == pytest.approx(META["restatement_deviation"][k], rel=1e-6), k
    assert cs.BOUND == {k: max(1e-12, 8 * v) for k, v in META["restatement_deviation"].items()}
    assert 1e-12 <= cs.BOUND["stress"] <= 3e-11 and cs.BOUND["tangent"] <= 1e-10 and cs.BOUND["state"] == 1e-12


def svk(F, prm):
    """St-Venant-Kirchhoff closed form for Fp = I: P = F S, A[(iJ),(kL)] = delta_ik S_LJ + F_iM D_MJPL F_kP"""
    c11, c12, g2 = fx.cubic(prm)
    D = np.zeros((3, 3, 3, 3))
    for i in range(3):
        for j in range(3):
            D[i, i, j, j] = c11 if i == j else c12
            if i != j:
                D[i, j, i, j] = D[i, j, j, i] = g2 / 2
    Fm = fx.to_mat(F)
    E = 0.5 * (np.swapaxes(Fm, 1, 2) @ Fm - np.eye(3))
    S = np.einsum("ijkl,nkl->nij", D, E)
    A4 = np.einsum("ik,nlj->nijkl", np.eye(3), S) + np.einsum("nim,mjpl,nkp->nijkl", Fm, D, Fm)
    A = np.empty((len(F), 9, 9))
    for t in range(9):
        for u in range(9):
            A[:, t, u] = A4[:, fx.TI[t], fx.TJ[t], fx.TI[u], fx.TJ[u]]
    return fx.to_vec(Fm @ S), A


# The Green-Lagrange strain is a difference of numbers near 1: each of its entries carries a few units of 1.1e-16 whichever way it is
# summed, and the stress c11 times that.  Eight units: 2.5e-10 (MPa), absolute
SVK_STRESS = 8 * 1.1e-16 * fx.cubic(cs.PRM)[0]


def test_dt_zero_and_sub_yield_steps_are_st_venant_kirchhoff():
    rng = np.random.default_rng(4)
    n = 12
    F = EYE9 + 3e-3 * rng.normal(size=(n, 9))          # far beyond yield
    P, A = svk(F, cs.PRM)
    out = fx.update(F, fx.zero_state(n), cs.PRM, 0.0)
    assert out["plastic"].all() and (out["status"] == 0).all()
    assert np.abs(out["stress"] - P).max() <= SVK_STRESS and np.abs(out["tangent"] - A).max() <= 1e-13 * np.abs(A).max()
    assert not out["g"].any() and np.array_equal(out["Fp"], fx.zero_state(n)["Fp"])
    Fs = EYE9 + 2e-4 * rng.normal(size=(n, 9))         # below yield
    P, A = svk(Fs, cs.PRM)
    out = fx.update(Fs, fx.zero_state(n), cs.PRM, 0.1)
    assert not out["plastic"].any()
    assert np.abs(out["stress"] - P).max() <= SVK_STRESS and np.abs(out["tangent"] - A).max() <= 1e-13 * np.abs(A).max()


def test_objectivity_and_frames():
    F, R, state, ref = cs.case(30, np.arange(30) % 3 != 1)
    Q = rotation(8)
    QF = fx.to_vec(Q @ fx.to_mat(F))
    out = fx.update(QF, state, cs.PRM, cs.DT, R=R, maxit=cs.MAXIT)
    # P(QF) = Q P(F) with the state unchanged, under the frame of each point: R (Q F) R^T = (R Q R^T) F_m is a rotation of F_m from the left
    assert np.abs(out["stress"] - fx.to_vec(Q @ fx.to_mat(ref["stress"]))).max() <= 1e-10 * np.abs(ref["stress"]).max()
    for k in cs.STATE:
        assert np.abs(out[k] - ref[k]).max() <= 1e-12
    # without a material frame the law is objective as it stands: a rotation after the deformation leaves Fe^T Fe alone
    no = {k: v for k, v in state.items()}
    a = fx.update(F, no, cs.PRM, cs.DT, maxit=cs.MAXIT)
    b = fx.update(QF, no, cs.PRM, cs.DT, maxit=cs.MAXIT)
    assert np.abs(b["stress"] - fx.to_vec(Q @ fx.to_mat(a["stress"]))).max() <= 1e-10 * np.abs(a["stress"]).max()
    assert np.abs(b["Fp"] - a["Fp"]).max() <= 1e-13 and np.abs(b["g"] - a["g"]).max() <= 1e-13
    # a frame R equals the rotated frameless result: F_m = R F R^T, P = R^T P_m R, the tangent rotated accordingly
    Rm = rotation(9)
    Fm = fx.to_vec(Rm @ fx.to_mat(F) @ Rm.T)
    m = fx.update(Fm, state, cs.PRM, cs.DT, maxit=cs.MAXIT)
    f = fx.update(F, state, cs.PRM, cs.DT, R=Rm, maxit=cs.MAXIT)
    assert np.abs(f["stress"] - fx.to_vec(Rm.T @ fx.to_mat(m["stress"]) @ Rm)).max() <= 1e-10 * np.abs(m["stress"]).max()
    assert np.abs(f["tangent"] - fx.rotate_tangent(m["tangent"], np.broadcast_to(Rm, (30, 3, 3)))).max() <= 1e-9 * np.abs(m["tangent"]).max()
    for k in cs.STATE:
        assert np.abs(f[k] - m[k]).max() <= 1e-12


def test_tangent_is_the_derivative_of_the_stress():
    F, R, state, ref = cs.case(18, np.ones(18, dtype=bool))
    h = 1e-7
    T = np.empty((18, 9, 9))
    for u in range(9):
        e = np.zeros(9)
        e[u] = h
        T[:, :, u] = (fx.update(F + e, state, cs.PRM, cs.DT, R=R, maxit=cs.MAXIT)["stress"]
                      - fx.update(F - e, state, cs.PRM, cs.DT, R=R, maxit=cs.MAXIT)["stress"]) / (2 * h)
    assert np.abs(T - ref["tangent"]).max() <= 2e-6 * np.abs(T).max()


def test_small_strain_limit_is_law_14():
    """for |F - I| -> 0 the stress approaches the small-strain law's with the same constants; the difference falls linearly"""
    rng = np.random.default_rng(12)
    n = 16
    H = rng.normal(size=(n, 3, 3))
    H /= np.linalg.norm(H, axis=(1, 2))[:, None, None]
    p14 = sc.param_vector({"E1": 208000.0}, interaction=(1.0, 0, 0, 0, 0, 0))
    diff = []
    for amp in (4e-4, 1e-4):
        out = fx.update(fx.to_vec(np.eye(3) + amp * H), fx.zero_state(n), cs.PRM, cs.DT)
        eps = 0.5 * amp * (H + H.transpose(0, 2, 1))
        ss = sc.update(np.array([sc.mandel(e) for e in eps]), sc.zero_state(n), p14, cs.DT)
        sig = np.zeros((n, 3, 3))
        for I, (i, j) in enumerate(sc.IJ):
            sig[:, i, j] = sig[:, j, i] = ss["stress"][:, I] / (1.0 if I < 3 else sc.SQ2)
        diff.append(np.abs(fx.to_mat(out["stress"]) - sig).max() / np.abs(sig).max())
    print("small-strain limit: relative stress difference at 4e-4 and 1e-4:", diff)
    assert diff[0] < 5e-3 and diff[1] < diff[0] / 3 and diff[1] > diff[0] / 5


def test_iteration_cap_keeps_the_state_and_answers_elastically():
    F, R, state, ref = cs.case(18, np.ones(18, dtype=bool))
    assert ref["iters"].max() >= 6
    out = fx.update(F, state, cs.PRM, cs.DT, R=R, maxit=3)
    capped = out["status"] == 1
    assert capped.any() and (ref["iters"][capped] > 3).all() and (ref["iters"][~capped] <= 3).all()
    el = fx.update(F, state, cs.PRM, 0.0, R=R)
    for k in cs.STATE:
        assert np.array_equal(out[k][capped], state[k][capped])
    assert np.array_equal(out["stress"][capped], el["stress"][capped]) and np.array_equal(out["tangent"][capped], el["tangent"][capped])


# ---- the Python layer and the law table ----------------------------------------------------------------------------------------------
PROPS = dict(E=208000.0, nu=0.3, G=80000.0, n=10.0, K=25.0, Q=11.43, b=2.1, tau0=66.62, d=494.0, C=14363.0)


def test_behaviour_descriptor_and_refusals():
    b = jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity(**PROPS)
    assert b.law == _lib.LAW_FS_SINGLE_CRYSTAL_FCC == 21 and np.array_equal(b.params(), fx.param_vector())
    assert isinstance(b, jm.FiniteStrainBehavior) and (b.gradient_name, b.flux_name) == ("DeformationGradient", "FirstPiolaKirchhoffStress")
    assert b.interaction == (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    d = jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity.from_mfront_properties(PROPS)
    assert d.params() == b.params()
    for k in PROPS:   # the file gives no defaults: all ten
        with pytest.raises(ValueError, match="missing"):
            jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity.from_mfront_properties({q: v for q, v in PROPS.items() if q != k})
    with pytest.raises(ValueError, match="unknown"):
        jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity.from_mfront_properties({**PROPS, "YoungModulus1": 1.0})
    for k, v in (("E", 0.0), ("G", -1.0), ("K", 0.0), ("nu", 0.5), ("nu", -1.0), ("n", 0.5), ("tau0", -1.0), ("b", -1.0), ("d", -1.0), ("C", -1.0),
                 ("Q", float("nan")), ("E", float("inf"))):
        with pytest.raises(ValueError, match=f"finite-strain single-crystal viscoplasticity: .*{k}"):
            jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity(**{**PROPS, k: v})
    with pytest.raises(ValueError, match="six coefficients"):
        jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity(**PROPS, interaction=(1.0, 0.0))
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            JAXMaterial(b, tangent_layout=layout)


def test_derived_state_restates_mfronts_other_variables():
    F, R, state, ref = cs.case(30, np.arange(30) % 2 == 0)
    b = jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity(**PROPS)
    got = b.derived_state(F, {"PlasticPartOfTheDeformationGradient": ref["Fp"]}, rotation=R)
    want = fx.derived(F, {"Fp": ref["Fp"]}, cs.PRM, R=R)
    assert set(got) == {"ElasticStrain", "ElasticPartOfTheDeformationGradient", "ResolvedShearStress"}
    for k in got:
        assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k


def test_zero_rows_of_the_plastic_part_become_the_identity():
    from dolfinx_materials_amd.hip_material import _fp_rows

    a = np.zeros((4, 9))
    a[1] = EYE9 + 1e-3
    a[3] = [1, 1, 1, 0.5, 0, 0, 0, 0, 0]
    out = _fp_rows(a)
    assert np.array_equal(out[0], EYE9) and np.array_equal(out[2], EYE9) and np.array_equal(out[1], a[1]) and np.array_equal(out[3], a[3])
    assert not a[0].any()   # the caller's array is left alone
    bad = a.copy()
    bad[1] = [1, 1, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="row 1 is singular and not all zero"):
        _fp_rows(bad)


def test_law_table_row():
    i = _lib.law_info(_lib.LAW_FS_SINGLE_CRYSTAL_FCC)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (9, 9, 16, 4, 45, 1512)
    assert 72 + 360 + 72 + 648 + 360 == 1512
    assert [i.isv_name[f] for f in range(4)] == [b"PlasticSlip", b"EquivalentViscoplasticSlip", b"BackStrain", b"PlasticPartOfTheDeformationGradient"]
    assert [i.isv_dim[f] for f in range(4)] == [12, 12, 12, 9] == [d for _, d in fx.FIELDS]
    b = _lib.law_blocks(_lib.LAW_FS_SINGLE_CRYSTAL_FCC)
    assert (b.n_external, b.n_blocks, b.tangent_width) == (0, 1, 81)
    for law in (20, 22):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
    assert _lib.load().dxm_abi_version() == 6


def test_create_without_a_gpu_fails_loudly_for_the_new_law_too():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    assert not lib.dxm_create(_lib.LAW_FS_SINGLE_CRYSTAL_FCC, (C.c_double * 16)(*cs.PRM), 16, 8, 0)
    assert b"no usable HIP device" in lib.dxm_last_error()


def test_refusal_texts_of_the_library_row():
    import os

    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "dxmat.hip")).read()
    row = src[src.index("constexpr LawDesc law_fs_single_crystal()"):]
    row = row[:row.index("\n}\n")]
    for field in ("set_refusal", "launch_refusal", "no_fused", "no_displacement", "no_fields", "stock_only"):
        assert f"d.{field} = " in row, field
    assert "d.rate_dependent = true" in row and "d.unit_fields = 1u << 3" in row and "d.no_frame" not in row
    # dxmat.hip names no kernel of the new unit: its device assembly stays the parent's
    import re

    assert "fs_single_crystal_kernel<" not in re.sub(r'"[^"]*"', "", src)
