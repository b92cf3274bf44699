"""CPU: the two heat-transfer laws (DXM_LAW_HEAT_STATIONARY = 16, DXM_LAW_HEAT_PHASE_CHANGE = 17) without a GPU: the numpy restatement
against the 50-digit fixture and against central differences, the law rows and ``dxm_law_blocks_get`` of every assigned law, the
behaviour classes and their refusals, the ``HIPMaterial`` surface (three tangent blocks, ``external_state_variables``), and the
``QuadratureFieldMap`` with a registered Temperature over the test double ``fake_dxmat_heat``."""
import ctypes as C
import json

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.field_map import QuadratureFieldMap, evaluate_block
from dolfinx_materials_amd.jaxmat import JAXMaterial

import heat_transfer_ref as ht
from fake_dxmat_heat import FakeDxmatHeat

ASSIGNED = (0, 1, 2, 3, 4, 5, 7, 10, 12, 14, 16, 17)
KAT = ht.load_kat()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_every_boundary_point_and_the_restatement_deviates_by_what_it_records():
    meta = json.loads(str(KAT["meta"]))
    assert meta["digits"] == 50 and meta["points"] <= 300 and len(meta["cases"]) == 4
    for law, tag, prm, g, T, exp, recorded in ht.kat_cases(KAT):
        got = ht.group_values(law, ht.update(law, g, T, prm))
        assert set(got) == set(exp) == set(recorded)
        for name in exp:
            dev = ht.relative_deviation(got[name], exp[name])
            print(tag, name, dev, recorded[name])
            assert dev == recorded[name] and dev <= 1e-12, (tag, name)
        if law == ht.PHASE_CHANGE:
            Ts, Tl = ht.solidus_liquidus(prm)
            for edge in (Ts, prm[0], Tl, np.nextafter(Ts, -np.inf), np.nextafter(Ts, np.inf), np.nextafter(Tl, -np.inf), np.nextafter(Tl, np.inf)):
                assert (T == edge).any(), (tag, edge)
            branch = ht.phase_change(g, T, prm)["branch"]
            assert all((branch == b).sum() >= 20 for b in (0, 1, 2)), np.bincount(branch)
            # the branch at the ends of the transition is the file's: T < Ts is solid, T > Tl liquid, both ends belong to the transition
            assert branch[T == Ts] == 1 and branch[T == Tl] == 1
            assert branch[T == np.nextafter(Ts, -np.inf)] == 0 and branch[T == np.nextafter(Tl, np.inf)] == 2
    assert prm[6] == 1.0   # the last case is the demo's Tsmooth


def test_the_transition_follows_the_file_not_the_demos_prose():
    prm = ht.PHASE_CHANGE_DEFAULTS
    Tm, ks, cs, kl, cl, dh, Tsm = prm
    out = ht.phase_change(np.ones((1, 3)), Tm, prm)
    assert out["tangent"][0, 12] == (cs + cl) / 2 + dh / Tsm != dh / Tsm
    assert out["tangent"][0, 9] == -(kl - ks) / Tsm and out["k"][0] == pytest.approx((ks + kl) / 2, rel=1e-12)


@pytest.mark.parametrize("law,prm", [(ht.STATIONARY, ht.STATIONARY_DEFAULTS), (ht.PHASE_CHANGE, ht.PHASE_CHANGE_DEFAULTS),
                                     (ht.PHASE_CHANGE, ht.PHASE_CHANGE_DEFAULTS[:6] + (1.0,))])
def test_each_block_against_central_differences_inside_each_branch(law, prm):
    rng = np.random.default_rng(4)
    if law == ht.STATIONARY:
        T = rng.uniform(280.0, 1500.0, 30)
    else:
        Ts, Tl = ht.solidus_liquidus(prm)
        w = Tl - Ts
        T = np.concatenate([rng.uniform(400.0, Ts - 5.0, 10), rng.uniform(Ts + 0.25 * w, Tl - 0.25 * w, 10), rng.uniform(Tl + 5.0, 1400.0, 10)])
    n = len(T)
    g = rng.normal(size=(n, 3)) * 100.0
    out = ht.update(law, g, T, prm)
    ct = out["tangent"]
    # dj/dg: j is linear in g, a difference of any size is exact up to rounding
    for c in range(3):
        dg = np.zeros(3)
        dg[c] = 1.0
        col = (ht.update(law, g + dg, T, prm)["flux"] - ht.update(law, g - dg, T, prm)["flux"]) / 2.0
        assert np.abs(col - ct[:, [c, 3 + c, 6 + c]]).max() <= 1e-9 * np.abs(ct[:, :9]).max()
    assert not ct[:, [1, 2, 3, 5, 6, 7]].any()
    # d/dT: steps that stay inside the branch (the transition is 0.1 K wide by default)
    h = 1e-3 if law == ht.STATIONARY else 1e-3 * min(1.0, prm[6])
    up, dn = ht.update(law, g, T + h, prm), ht.update(law, g, T - h, prm)
    if law == ht.PHASE_CHANGE:
        assert np.array_equal(up["branch"], dn["branch"])
    dj = (up["flux"] - dn["flux"]) / (2 * h)
    assert np.abs(dj - ct[:, 9:12]).max() <= 1e-6 * max(np.abs(ct[:, 9:12]).max(), 1e-300)
    if law == ht.PHASE_CHANGE:
        dh = (up["enthalpy"] - dn["enthalpy"]) / (2 * h)
        assert np.abs(dh - ct[:, 12]).max() <= 1e-6 * np.abs(ct[:, 12]).max()


# ---- the library's tables (host code: no device needed) ----------------------------------------------------------------------
def test_law_rows_16_and_17_and_the_unassigned_ids_around_them():
    assert (_lib.LAW_HEAT_STATIONARY, _lib.LAW_HEAT_PHASE_CHANGE) == (16, 17)
    i = _lib.law_info(16)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (3, 3, 2, 0, 0, 120)
    i = _lib.law_info(17)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (3, 3, 7, 1, 1, 136)
    assert i.isv_name[0].decode() == "Enthalpy" and i.isv_dim[0] == 1
    for law in (15, 18):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_blocks(law)
    assert _lib.load().dxm_abi_version() == 6 and C.sizeof(_lib.LawInfo) == 72


def _blocks(law):
    b = _lib.law_blocks(law)
    return b, [(k.row_kind, k.row_index, k.col_kind, k.col_index, k.rows, k.cols) for k in list(b.block)[: b.n_blocks]]


def test_law_blocks_of_every_assigned_law():
    for law in ASSIGNED:
        info = _lib.law_info(law)
        b, blocks = _blocks(law)
        if law in (16, 17):
            continue
        assert b.n_external == 0 and b.n_blocks == 1 and blocks == [(0, 0, 0, 0, info.n_flux, info.n_grad)], law
        assert b.tangent_width == info.n_flux * info.n_grad and b.external_name[0] is None
    b, blocks = _blocks(16)
    assert (b.n_external, b.n_blocks, b.tangent_width) == (1, 2, 12) and b.external_name[0] == b"Temperature" and b.external_default[0] == 293.15
    assert blocks == [(0, 0, 0, 0, 3, 3), (0, 0, 1, 0, 3, 1)]
    b, blocks = _blocks(17)
    assert (b.n_external, b.n_blocks, b.tangent_width) == (1, 3, 13) and b.external_name[0] == b"Temperature"
    assert blocks == [(0, 0, 0, 0, 3, 3), (0, 0, 1, 0, 3, 1), (1, 0, 1, 0, 1, 1)]
    assert all(law in ASSIGNED or law in (6, 8, 9, 11, 13, 15) for law in range(18))


# ---- behaviour classes ----------------------------------------------------------------------------------------------------------
def test_behaviour_classes_parameters_and_refusals():
    s = jm.StationaryHeatTransfer()
    assert s.law == 16 and s.params() == [0.0375, 2.165e-4] and s.get_parameter("A") == 0.0375 and s.get_parameter("B") == 2.165e-4
    assert (s.gradient_name, s.flux_name, s.ngrad, s.nflux) == ("TemperatureGradient", "HeatFlux", 3, 3)
    assert s.external_state_variables == {"Temperature": 1} and isinstance(s, jm.HeatTransferBehavior)
    s.A = 1
    assert s.params()[0] == 1.0 and s.flat_properties() == {"A": 1.0, "B": 2.165e-4}
    p = jm.HeatTransferPhaseChange()
    assert p.law == 17 and tuple(p.params()) == ht.PHASE_CHANGE_DEFAULTS and p.get_parameter("MeltingTemperature") == 933.15
    q = jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0})
    assert q.params()[6] == 1.0 and q.params()[:6] == p.params()[:6]
    assert jm.HeatTransferPhaseChange(Tsmooth=0.5).Tsmooth == 0.5
    assert list(p.flat_properties()) == ["MeltingTemperature", "SolidConductivity", "SolidHeatCapacity", "LiquidConductivity", "LiquidHeatCapacity",
                                         "FusionEnthalpy", "Tsmooth"]
    with pytest.raises(ValueError, match="Tsmooth must be > 0, got 0.0"):
        jm.HeatTransferPhaseChange(Tsmooth=0.0)
    with pytest.raises(ValueError, match="SolidConductivity must be finite, got nan"):
        jm.HeatTransferPhaseChange(SolidConductivity=float("nan"))
    with pytest.raises(ValueError, match="B must be finite, got inf"):
        jm.StationaryHeatTransfer(B=float("inf"))
    with pytest.raises(ValueError, match="unknown \\['Tsmoth'\\]"):
        jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmoth": 1.0})
    with pytest.raises(ValueError, match="has no parameter 'C'"):
        s.get_parameter("C")


def test_material_surface_without_a_device():
    m = JAXMaterial(jm.HeatTransferPhaseChange())
    assert m.gradients == {"TemperatureGradient": 3} and m.fluxes == {"HeatFlux": 3} and m.internal_state_variables == {"Enthalpy": 1}
    assert m.external_state_variables == {"Temperature": 1}
    assert m.tangent_blocks == {("HeatFlux", "TemperatureGradient"): (3, 3), ("HeatFlux", "Temperature"): (3, 1), ("Enthalpy", "Temperature"): (1, 1)}
    assert list(m.tangent_blocks) == [("HeatFlux", "TemperatureGradient"), ("HeatFlux", "Temperature"), ("Enthalpy", "Temperature")]
    assert m.tangent_size == 13 and m.algorithmic_bytes_per_point == 136 and not m.frame_fused
    s = JAXMaterial(jm.StationaryHeatTransfer())
    assert s.tangent_blocks == {("HeatFlux", "TemperatureGradient"): (3, 3), ("HeatFlux", "Temperature"): (3, 1)} and s.tangent_size == 12
    assert s.internal_state_variables == {} and s.algorithmic_bytes_per_point == 120
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            JAXMaterial(jm.StationaryHeatTransfer(), tangent_layout=layout)
    with pytest.raises(AttributeError, match="isotropic"):
        s.rotation_matrix = np.eye(3)
    with pytest.raises(NotImplementedError, match="external state variable 'Pressure'"):
        s.update_external_state_variable("Pressure", 1.0)


def test_the_other_laws_report_what_they_did_and_still_raise():
    el = jm.LinearElasticIsotropic(E=200e3, nu=0.3)
    cases = [(jm.ElasticBehavior(el), {("stress", "strain"): (6, 6)}, 36),
             (jm.vonMisesIsotropicHardening(el, jm.LinearHardening(sig0=250.0, H=1e3)), {("stress", "strain"): (6, 6)}, 36),
             (jm.FeFpJ2Plasticity(el, jm.LinearHardening(sig0=250.0, H=1e3)), {("PK1", "F"): (9, 9)}, 81),
             (jm.OgdenHyperelasticity(), {("FirstPiolaKirchhoffStress", "DeformationGradient"): (9, 9)}, 81)]
    for b, blocks, size in cases:
        m = JAXMaterial(b)
        assert m.tangent_blocks == blocks and m.tangent_size == size and m.external_state_variables == {}
        for call in (m.initialize_external_state_variable, m.update_external_state_variable):
            with pytest.raises(NotImplementedError, match="external state variable 'Temperature': the HIP laws"):
                call("Temperature", 300.0)
    assert JAXMaterial(cases[1][0], tangent_layout="sym").tangent_size == 21 and JAXMaterial(cases[1][0], tangent_layout="pack4").tangent_size == 4


# ---- the map over the CPU double --------------------------------------------------------------------------------------------------
NCELL, NQP = 29, 4
N = NCELL * NQP


@pytest.fixture
def fake(monkeypatch):
    lib = FakeDxmatHeat(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    return lib


def _temperatures(prm, n, seed):
    rng = np.random.default_rng(seed)
    Ts, Tl = ht.solidus_liquidus(prm)
    T = np.concatenate([rng.uniform(300.0, Ts - 1, n // 3), rng.uniform(Ts, Tl, n // 3), rng.uniform(Tl + 1, 1400.0, n - 2 * (n // 3))])
    return rng.permutation(T)


@pytest.mark.parametrize("subset", [False, True])
def test_map_update_with_a_registered_temperature_blocks_and_enthalpy(fake, subset):
    prm = ht.PHASE_CHANGE_DEFAULTS[:6] + (1.0,)
    cells = np.sort(np.random.default_rng(5).permutation(NCELL)[: 2 * NCELL // 3]).astype(np.int32) if subset else None
    rows = np.arange(N) if cells is None else (cells[:, None] * NQP + np.arange(NQP)[None]).ravel()
    rest = np.setdiff1d(np.arange(N), rows)
    m = JAXMaterial(jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0}))
    q = QuadratureFieldMap(NCELL, NQP, m, cells=cells)
    assert set(q.jacobians) == set(m.tangent_blocks) and q.jacobian_width == 13
    g = np.random.default_rng(2).normal(size=(N, 3)) * 50.0
    T = [_temperatures(prm, N, 7)]
    q.register_gradient("TemperatureGradient", lambda c: g.reshape(NCELL, NQP, 3)[c].reshape(-1, 3))
    q.register_external_state_variable("Temperature", lambda c: T[0].reshape(NCELL, NQP)[c].reshape(-1, 1))
    assert fake.ext_calls == [("field", len(rows))]                       # the rows of the map's own points, not all cells
    assert np.array_equal(q.external_state_variables["Temperature"].function.x.array[rows], T[0][rows])
    for step in range(2):
        q.update()
        ref = ht.phase_change(g[rows], T[0][rows], prm)
        flux = q.fluxes["HeatFlux"].x.array.reshape(N, 3)
        assert np.array_equal(flux[rows], ref["flux"]) and not flux[rest].any()
        jac = q.jacobian_flatten.x.array.reshape(N, 13)
        assert np.array_equal(jac[rows], ref["tangent"]) and not jac[rest].any()
        K = evaluate_block(q.jacobians[("HeatFlux", "TemperatureGradient")], rows)
        assert K.shape == (len(rows), 3, 3) and np.array_equal(K, -ref["k"][:, None, None] * np.eye(3))
        dj = evaluate_block(q.jacobians[("HeatFlux", "Temperature")], rows)
        assert dj.shape == (len(rows), 3, 1) and np.array_equal(dj[:, :, 0], ref["tangent"][:, 9:12])
        c = evaluate_block(q.jacobians[("Enthalpy", "Temperature")], rows)
        assert c.shape == (len(rows), 1, 1) and np.array_equal(c[:, 0, 0], ref["tangent"][:, 12])
        h = np.asarray(q.internal_state_variables["Enthalpy"].x.array)
        assert np.array_equal(h[rows], ref["enthalpy"]) and not h[rest].any()
        assert m.last_stats["n_nan"] == 0
        q.advance()
        assert np.array_equal(np.asarray(m.get_initial_state_dict()["Enthalpy"]).reshape(-1), ref["enthalpy"])
        T[0] = _temperatures(prm, N, 11)      # the evaluator is read again by the next update()
    assert fake.ext_calls == [("field", len(rows))] * 3 and m.algorithmic_bytes_per_point == 144


def test_map_with_a_number_and_an_array_for_the_temperature(fake):
    m = JAXMaterial(jm.StationaryHeatTransfer())
    q = QuadratureFieldMap(NCELL, NQP, m)
    g = np.random.default_rng(3).normal(size=(N, 3))
    q.register_gradient("TemperatureGradient", lambda c: g.reshape(NCELL, NQP, 3)[c].reshape(-1, 3))
    q.update()                                                            # nothing registered: 293.15 (mfront.py:109-110)
    assert np.array_equal(q.fluxes["HeatFlux"].x.array.reshape(N, 3), ht.stationary(g, 293.15)["flux"])
    q.register_external_state_variable("Temperature", 500.0)
    assert fake.ext_calls == [("uniform", 500.0)] and m.algorithmic_bytes_per_point == 120
    q.update()
    assert np.array_equal(q.jacobian_flatten.x.array.reshape(N, 12), ht.stationary(g, 500.0)["tangent"])
    T = np.linspace(300.0, 900.0, N)
    q.register_external_state_variable("Temperature", T)
    q.update()
    assert np.array_equal(q.fluxes["HeatFlux"].x.array.reshape(N, 3), ht.stationary(g, T)["flux"]) and m.algorithmic_bytes_per_point == 128
    with pytest.raises(_lib.DxmError, match="Temperature is not finite at point 3"):
        m.update_external_state_variable("Temperature", np.where(np.arange(N) == 3, np.nan, T))
    q.update()                                                            # the refusal left the field as it was
    assert np.array_equal(q.fluxes["HeatFlux"].x.array.reshape(N, 3), ht.stationary(g, T)["flux"])
    with pytest.raises(ValueError, match=f"5 values for {N} Gauss points"):
        m.update_external_state_variable("Temperature", np.arange(5.0))


def test_explicit_state_update_reads_the_materials_temperature(fake):
    n = 12
    m = JAXMaterial(jm.HeatTransferPhaseChange())
    m.set_data_manager(n)
    g = np.random.default_rng(1).normal(size=(n, 3))
    T = _temperatures(ht.PHASE_CHANGE_DEFAULTS, n, 3)
    m.update_external_state_variable("Temperature", T)
    ct, new = m.batched_constitutive_update(g, {})
    ref = ht.phase_change(g, T, ht.PHASE_CHANGE_DEFAULTS)
    assert ct.shape == (n, 13) and np.array_equal(ct, ref["tangent"])
    assert np.array_equal(new["HeatFlux"], ref["flux"]) and np.array_equal(new["Enthalpy"][:, 0], ref["enthalpy"])
    assert np.array_equal(new["TemperatureGradient"], g)
    assert not np.asarray(m.get_final_state_dict()["Enthalpy"]).any()          # the material's own state is untouched
    m.update_external_state_variable("Temperature", 950.0)
    j, one = m.constitutive_update(g[0], {})
    assert np.array_equal(j, ht.phase_change(g[:1], 950.0, ht.PHASE_CHANGE_DEFAULTS)["flux"][0])
    m.update_external_state_variable("Temperature", T)
    with pytest.raises(_lib.DxmError, match="one gradient row per Gauss point"):
        m.batched_constitutive_update(g[:5], {})
