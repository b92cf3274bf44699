"""CPU: the two plane-stress return mappings (DXM_LAW_PS_QUADRATIC = 23, DXM_LAW_PS_POLYGON = 24) without a GPU: the numpy restatement
against the 50-digit fixture, against SLSQP, against the projection's own variational inequality and against central differences;
the law rows; the refusals of the build functions and of the Python classes; the hidden-state rebuild (a prestress included) and the
protocol over the test double ``fake_dxmat_plane_stress``; and the reference's ``generic.Material`` driven with the restatement where
its cvxpy classes solve a conic program."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd.plane_stress import L1Rankine, PlaneStressPolygon, PlaneStressvonMises, Rankine

import plane_stress_ref as ps
from fake_dxmat_plane_stress import FakeDxmatPlaneStress

E, NU, SIG0, FC, FT = 70e3, 0.2, 30.0, 30.0, 10.0      # demos/cvxpy/cvxpy_return_mapping.py
CLASSES = {"vonmises": (ps.QUADRATIC, [E, NU, SIG0, 1.0, 1.0]), "mises32": (ps.QUADRATIC, [E, NU, SIG0, 1.5, 1.0]),
           "rankine": (ps.POLYGON, ps.polygon_params(E, NU, ps.rankine_planes(FT, FC))),
           "l1rankine": (ps.POLYGON, ps.polygon_params(E, NU, ps.l1rankine_planes(FT, FC)))}


random_trials = ps.random_trials


# ---- the restatement against the fixture -------------------------------------------------------------------------------------------
def test_the_restatement_against_the_fixture_and_the_figures_the_gpu_bounds_come_from():
    kat = ps.load_kat()
    meta = json.loads(str(kat["meta"]))
    assert meta["digits"] == 50 and meta["margin"] == 1e-6
    points = {ps.QUADRATIC: 0, ps.POLYGON: 0}
    worst = {ps.QUADRATIC: np.zeros(3), ps.POLYGON: np.zeros(3)}
    for tag, law, prm, eps, incs in ps.kat_cases(kat):
        points[law] += len(eps[0])
        s, Em = ps.scale(law, prm), prm[0]
        for tangent in ((0, 1) if law == ps.QUADRATIC else (0,)):
            p = prm.copy()
            if law == ps.QUADRATIC:
                p[4] = tangent
            state = np.zeros_like(eps[0])
            for k in range(2):
                r = ps.update(law, eps[k], state, p)
                assert np.array_equal(r["plastic"], incs[k]["plastic"]), (tag, k)
                assert not r["not_converged"].any() and r["iters"].max() <= 8
                want = incs[k]["tangent"] if tangent else np.tile(kat[tag + "_elastic"], (len(eps[k]), 1))
                err = np.array([np.abs(r["stress"] - incs[k]["stress"]).max() / s, np.abs(r["tangent"] - want).max() / Em,
                                np.abs(r["state"] - incs[k]["state"]).max() / (s / Em)])
                worst[law] = np.maximum(worst[law], err)
                state = r["state"]
        # the second increment unloads part of the batch
        assert 0 < incs[1]["plastic"].sum() < len(eps[1]) and (incs[0]["plastic"] & ~incs[1]["plastic"]).any(), tag
    assert points[ps.QUADRATIC] >= 200 and points[ps.POLYGON] >= 200
    for law in worst:
        print(law, "stress %.3e  tangent %.3e  state %.3e" % tuple(worst[law]), "recorded", ps.MEASURED[law])
        assert (worst[law] <= np.array(ps.MEASURED[law])).all() and (worst[law] >= 0.5 * np.array(ps.MEASURED[law])).all(), (law, worst[law])
        assert all(b == max(16 * m, 2e-14) for b, m in zip(ps.gpu_bounds(law), ps.MEASURED[law]))


# ---- against an optimiser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vonmises", "mises32", "rankine", "l1rankine"])
def test_the_restatement_against_slsqp(name):
    from scipy.optimize import minimize

    law, prm = CLASSES[name]
    s = ps.scale(law, prm)
    eps = random_trials(law, prm, 300, seed=11)
    r = ps.update(law, eps, np.zeros_like(eps), prm)
    trial = eps @ ps.stiffness(prm[0], prm[1]).T / s            # in units of s*
    Sn = ps.compliance(prm[0], prm[1]) * prm[0]
    prm_unit = np.array(prm, dtype=float)
    if law == ps.QUADRATIC:
        prm_unit[2] = 1.0
    else:
        for k in range(int(prm[2])):
            prm_unit[5 + 3 * k] /= s
    rows = ps.planes_of(prm_unit) if law == ps.POLYGON else None

    def slack(x):
        """>= 0 inside.  The polygon: one entry per row on the ordered principal values, each smooth away from equal principal
        values (the largest violation alone has a kink at every vertex, where SLSQP stalls 1e-5 s* off)"""
        if rows is None:
            return 1.0 - x @ ps.q_matrix(prm[3]) @ x
        p1, p2 = ps.principal(x[None])
        return np.array([d - (n1 * p1[0] + n2 * p2[0]) for n1, n2, d in rows])

    worst = 0.0
    for i in np.flatnonzero(r["plastic"]):
        t = trial[i]
        x0 = t * 0.5 / (1.0 + ps.violation(law, t[None], prm_unit)[0])
        res = minimize(lambda x: 0.5 * (x - t) @ Sn @ (x - t), x0, jac=lambda x: Sn @ (x - t), method="SLSQP",
                       constraints=[dict(type="ineq", fun=slack)], options=dict(maxiter=500, ftol=1e-16))
        worst = max(worst, np.abs(res.x - r["stress"][i] / s).max())
    print(name, "largest deviation from SLSQP, in s*:", worst, "over", int(r["plastic"].sum()), "yielded points")
    assert r["plastic"].sum() >= 150 and worst <= 1e-5


# ---- against the projection's own characterisation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vonmises", "mises32", "rankine", "l1rankine"])
def test_feasibility_and_the_variational_inequality_on_every_yielded_point(name):
    law, prm = CLASSES[name]
    s = ps.scale(law, prm)
    eps = random_trials(law, prm, 400, seed=5)
    r = ps.update(law, eps, np.zeros_like(eps), prm)
    ps.check_projection(law, prm, eps @ ps.stiffness(prm[0], prm[1]).T, r["stress"], r["plastic"], np.random.default_rng(3))
    assert r["plastic"].sum() >= 200 and (~r["plastic"]).sum() >= 50 and s > 0


def test_consistent_tangent_against_central_differences():
    for name in ("vonmises", "mises32"):
        law, prm = CLASSES[name]
        eps = random_trials(law, prm, 60, seed=2, lo=1.2, hi=5.0)
        r = ps.update(law, eps, np.zeros_like(eps), prm)
        assert r["plastic"].all()
        h = 1e-5 * SIG0 / E
        fd = np.empty((len(eps), 3, 3))
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            up, dn = ps.update(law, eps + d, np.zeros_like(eps), prm), ps.update(law, eps - d, np.zeros_like(eps), prm)
            fd[:, :, c] = (up["stress"] - dn["stress"]) / (2 * h)
        err = np.abs(fd.reshape(-1, 9) - r["tangent"]).max() / E
        print(name, "tangent against central differences, in E:", err)
        assert err <= 1e-6
        ct = r["tangent"].reshape(-1, 3, 3)
        assert np.abs(ct - np.swapaxes(ct, 1, 2)).max() == 0.0                                 # written from six numbers
        # the tangent annihilates the normal of the surface: n^T D = 0
        n = r["stress"] @ ps.q_matrix(prm[3])
        assert np.abs(np.einsum("ni,nij->nj", n, ct)).max() <= 1e-9 * E * SIG0
    # an elastic point of a tangent = 1 handle, and every point of a tangent = 0 handle: C as the reference forms it
    law, prm = CLASSES["vonmises"]
    eps = random_trials(law, prm, 20, seed=4, lo=0.1, hi=0.9)
    Cflat = conventions.plane_stress_stiffness(E, NU).reshape(9)
    assert np.array_equal(ps.update(law, eps, 0 * eps, prm)["tangent"], np.tile(Cflat, (20, 1)))
    eps = random_trials(law, prm, 20, seed=4, lo=1.5, hi=3.0)
    assert np.array_equal(ps.update(law, eps, 0 * eps, prm[:4] + [0.0])["tangent"], np.tile(Cflat, (20, 1)))
    assert np.allclose(conventions.plane_stress_compliance(E, NU) @ conventions.plane_stress_stiffness(E, NU), np.eye(3), atol=1e-15)


# ---- the library's tables (host code: no device needed) ----------------------------------------------------------------------------
def test_law_rows_23_and_24_and_the_unassigned_ids_around_them():
    assert (_lib.LAW_PS_QUADRATIC, _lib.LAW_PS_POLYGON) == (23, 24)
    i = _lib.law_info(23)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (3, 3, 5, 0, 0, 168)
    i = _lib.law_info(24)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (3, 3, 15, 0, 0, 168)
    for law in (23, 24):
        b = _lib.law_blocks(law)
        assert (b.n_external, b.n_blocks, b.tangent_width) == (0, 1, 9)
        k = b.block[0]
        assert (k.row_kind, k.row_index, k.col_kind, k.col_index, k.rows, k.cols) == (0, 0, 0, 0, 3, 3)
    for law in (22, 25):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_blocks(law)
    assert _lib.load().dxm_abi_version() == 6


def test_create_without_a_gpu_fails_loudly_for_the_new_laws_too():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    assert not lib.dxm_create(23, (C.c_double * 5)(E, NU, SIG0, 1.0, 0.0), 5, 8, 0)
    assert b"no usable HIP device" in lib.dxm_last_error()
    prm = ps.polygon_params(E, NU, ps.rankine_planes(FT, FC))
    assert not lib.dxm_create(24, (C.c_double * 15)(*prm), 15, 8, 0)
    assert b"no usable HIP device" in lib.dxm_last_error()
    with pytest.raises(_lib.DxmError, match="no usable HIP device"):
        Rankine(E, NU, FT, FC).set_data_manager(8)


def test_refusal_texts_of_the_library_rows_and_build_functions():
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "dxmat.hip")).read()
    for fn in ("law_ps_quadratic", "law_ps_polygon"):
        row = src[src.index(f"constexpr LawDesc {fn}()"):]
        row = row[:row.index("\n}\n")]
        for field in ("set_refusal", "launch_refusal", "no_fused", "no_displacement", "no_frame", "no_fields", "stock_only"):
            assert f"d.{field} = " in row, (fn, field)
    base = src[src.index("constexpr LawDesc plane_stress_law("):]
    base = base[:base.index("\n}\n")]
    assert "d.set_layouts = d.launch_layouts = L_FULL;" in base and "d.alg_bytes = 168;" in base and "PS_BLOCKS_PER_CU" in base
    assert "d.n_isv_fields = 0;" in base and "d.n_fields = 1;" in base and 'state_field(d, 0, "PlasticStrain", 3, 0);' in base
    build = src[src.index("static int build_ps_quadratic("):src.index("// ---- launchers")]
    for words in ("E must be > 0", "nu must lie in (-1, 1)", "sig0 must be > 0", "the shear weight q must be > 0", "tangent must be 0",
                  "d must be > 0", "has a zero normal", "not symmetric under the exchange of the principal stresses",
                  "the number of half-planes M must be an integer"):
        assert words in build, words
    # the kernels' unit is named by no kernel in dxmat.hip, and the plan moves the nine entries as they are
    hs = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "host_side.hpp")).read()
    assert "r.law == DXM_LAW_PS_QUADRATIC || r.law == DXM_LAW_PS_POLYGON" in hs


def test_what_the_build_functions_refuse_restated():
    from fake_dxmat_plane_stress import refusal

    good = [E, NU, SIG0, 1.0, 0.0]
    assert refusal(23, good) is None
    for k, bad, words in ((0, 0.0, "E must be > 0"), (1, 1.0, "nu must lie"), (1, -1.0, "nu must lie"), (2, 0.0, "sig0 must be > 0"),
                          (3, -1.0, "q must be > 0"), (4, 2.0, "tangent must be 0"), (2, float("nan"), "sig0 must be finite")):
        p = list(good)
        p[k] = bad
        assert words in refusal(23, p), (k, bad)
    assert refusal(23, [E, 0.7, SIG0, 1.5, 1.0]) is None       # plane stress: nu up to 1
    rk = ps.rankine_planes(FT, FC)
    assert refusal(24, ps.polygon_params(E, NU, rk)) is None and refusal(24, ps.polygon_params(E, NU, ps.l1rankine_planes(FT, FC))) is None
    assert "symmetric" in refusal(24, ps.polygon_params(E, NU, [rk[0], rk[3]]))          # Rankine's two "ordered" rows only
    assert "symmetric" in refusal(24, ps.polygon_params(E, NU, [(1.0, 0.0, FT), (0.0, 1.0, FT + 1.0)]))
    assert "d must be > 0" in refusal(24, ps.polygon_params(E, NU, [(1.0, 1.0, 0.0)]))
    assert "zero normal" in refusal(24, ps.polygon_params(E, NU, [(0.0, 0.0, 1.0)]))
    p = ps.polygon_params(E, NU, rk)
    p[2] = 5.0
    assert "integer" in refusal(24, p)
    p[2] = 2.5
    assert "integer" in refusal(24, p)


def test_the_ordered_rows_alone_let_the_projection_leave_the_set():
    """why the list must be closed under the exchange: with Rankine's rows s_I <= ft and s_II >= -fc alone, the nearest point of that
    wedge to an ordered trial can have s_I < s_II beyond ft, which the full set excludes"""
    full = ps.polygon_params(E, NU, ps.rankine_planes(FT, FC))
    sig_tr = np.array([[3.0 * FT, 2.5 * FT, 0.0]])
    eps = sig_tr @ ps.compliance(E, NU).T
    ok = ps.polygon(eps, 0 * eps, full)["stress"][0]
    assert np.allclose(ok, [FT, FT, 0.0], atol=1e-12)
    wedge = [(1.0, 0.0, FT), (0.0, -1.0, FC)]
    c, rec, verts = ps.polygon_constants([E, NU, 2.0] + [v for r in wedge for v in r] + [0.0] * 6)
    n1, n2, d, w1, w2, nw, _ = rec[0]
    step = (n1 * sig_tr[0, 0] + n2 * sig_tr[0, 1] - d) / nw
    left = np.array([sig_tr[0, 0] - w1 * step, sig_tr[0, 1] - w2 * step])
    assert left[1] > FT + 1.0        # s_II = 2.5 ft - nu 2 ft: outside the Rankine square


# ---- the Python classes ---------------------------------------------------------------------------------------------------------------
def test_the_classes_carry_the_demos_names_signatures_and_sizes():
    m = PlaneStressvonMises(E=E, nu=NU, sig0=SIG0)
    assert m.gradients == {"Strain": 3} and m.fluxes == {"Stress": 3} and m.internal_state_variables == {}
    assert m.tangent_blocks == {("Stress", "Strain"): (3, 3)} and m.tangent_size == 9 and m.algorithmic_bytes_per_point == 168
    assert m.behavior.law == 23 and m.behavior.params() == [E, NU, SIG0, 1.0, 0.0] and m.name == "PlaneStressQuadraticYield"
    assert np.array_equal(m.C, ps.stiffness(E, NU)) and (m.E, m.nu, m.sig0) == (E, NU, SIG0)
    assert PlaneStressvonMises(E, NU, SIG0, shear_weight=1.5, tangent="consistent").behavior.params() == [E, NU, SIG0, 1.5, 1.0]
    r = Rankine(E=E, nu=NU, fc=FC, ft=FT)
    assert r.behavior.law == 24 and r.behavior.params() == ps.polygon_params(E, NU, ps.rankine_planes(FT, FC)) and (r.ft, r.fc) == (FT, FC)
    assert L1Rankine(E, NU, FT, FC).behavior.params() == ps.polygon_params(E, NU, ps.l1rankine_planes(FT, FC))
    g = PlaneStressPolygon(E, NU, [(1.0, 1.0, 5.0)])
    assert g.behavior.params() == [E, NU, 1.0, 1.0, 1.0, 5.0] + [0.0] * 9 and g.gradients == {"Strain": 3}
    assert isinstance(m.behavior, jm.PlaneStressBehavior) and not m.frame_fused and m.external_state_variables == {}


def test_the_classes_refuse_bad_parameters_early():
    for kw, words in ((dict(E=0.0, nu=NU, sig0=SIG0), "E must be > 0"), (dict(E=E, nu=1.0, sig0=SIG0), "-1 < nu < 1"),
                      (dict(E=E, nu=NU, sig0=0.0), "sig0 must be finite and > 0"), (dict(E=E, nu=NU, sig0=float("nan")), "sig0"),
                      (dict(E=E, nu=NU, sig0=SIG0, shear_weight=0.0), "shear weight q"),
                      (dict(E=E, nu=NU, sig0=SIG0, tangent="secant"), "'elastic' or 'consistent'")):
        with pytest.raises(ValueError, match=words):
            PlaneStressvonMises(**kw)
    for cls in (Rankine, L1Rankine):
        with pytest.raises(ValueError, match="ft and fc must be finite and > 0"):
            cls(E, NU, 0.0, FC)
        with pytest.raises(ValueError, match="ft and fc must be finite and > 0"):
            cls(E, NU, FT, float("inf"))
        with pytest.raises(ValueError, match="a consistent tangent of the polygonal law"):
            cls(E, NU, FT, FC, tangent="consistent")
    rk = ps.rankine_planes(FT, FC)
    with pytest.raises(ValueError, match="not symmetric under the exchange"):
        PlaneStressPolygon(E, NU, [rk[0], rk[3]])
    with pytest.raises(ValueError, match="d must be > 0"):
        PlaneStressPolygon(E, NU, [(1.0, 1.0, -1.0)])
    with pytest.raises(ValueError, match="zero normal"):
        PlaneStressPolygon(E, NU, [(0.0, 0.0, 1.0)])
    with pytest.raises(ValueError, match="between 1 and 4 half-planes"):
        PlaneStressPolygon(E, NU, rk + [(1.0, 1.0, 50.0)])
    with pytest.raises(ValueError, match="between 1 and 4 half-planes"):
        PlaneStressPolygon(E, NU, [])
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            Rankine(E, NU, FT, FC, tangent_layout=layout)
    with pytest.raises(AttributeError, match="isotropic"):
        Rankine(E, NU, FT, FC).rotation_matrix = np.eye(3)


# ---- the protocol over the CPU double ---------------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    lib = FakeDxmatPlaneStress(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    return lib


def demo_paths():
    """``plot_stress_paths`` of the demo: 21 radial strain paths, 19 increments"""
    theta = np.linspace(0, 2 * np.pi, 21)
    Eps = np.vstack([np.array([1e-3 * np.cos(t), 1e-3 * np.sin(t), 0]) for t in theta])
    return Eps, np.linspace(0, 1, 20)[1:]


MATERIALS = {"vonmises": lambda: PlaneStressvonMises(E=E, nu=NU, sig0=SIG0), "rankine": lambda: Rankine(E=E, nu=NU, fc=FC, ft=FT),
             "l1rankine": lambda: L1Rankine(E=E, nu=NU, fc=FC, ft=FT)}


@pytest.mark.parametrize("name", list(MATERIALS))
def test_integrate_update_revert_and_the_state_dictionaries(fake, name):
    m = MATERIALS[name]()
    law, prm = m.behavior.law, m.behavior.params()
    Eps, ts = demo_paths()
    m.set_data_manager(len(Eps))
    s0 = m.get_initial_state_dict()
    assert set(s0) == {"Strain", "Stress"} and not np.asarray(s0["Strain"]).any() and not np.asarray(s0["Stress"]).any()
    state = np.zeros((len(Eps), 3))
    for k, t in enumerate(ts):
        sig, isv, Ct = m.integrate(t * Eps)
        r = ps.update(law, t * Eps, state, prm)
        assert np.array_equal(np.asarray(sig), r["stress"]) and np.asarray(Ct).reshape(-1, 9).shape == (21, 9)
        assert np.array_equal(np.asarray(Ct).reshape(-1, 9), r["tangent"]) and np.asarray(isv).size == 0
        assert m.last_stats["n_plastic"] == int(r["plastic"].sum()) and m.last_stats["n_not_converged"] == 0
        if k == 9:      # a rejected increment: s1 <- s0, then the same increment again gives the same answer
            m.data_manager.revert()
            s1 = m.get_final_state_dict()
            assert np.array_equal(np.asarray(s1["Strain"]), ts[k - 1] * Eps)
            sig2, _, _ = m.integrate(t * Eps)
            assert np.array_equal(np.asarray(sig2), r["stress"])
        s1 = m.get_final_state_dict()
        assert np.array_equal(np.asarray(s1["Strain"]), t * Eps) and np.array_equal(np.asarray(s1["Stress"]), r["stress"])
        m.data_manager.update()
        s0 = m.get_initial_state_dict()
        assert np.array_equal(np.asarray(s0["Strain"]), t * Eps) and np.array_equal(np.asarray(s0["Stress"]), r["stress"])
        state = r["state"]
    # every yielded path ends on its surface
    v = ps.violation(law, r["stress"], prm)
    assert r["plastic"].sum() >= 15 and np.abs(v[r["plastic"]]).max() <= 1e-12 * ps.scale(law, prm)
    m.close()


@pytest.mark.parametrize("name", list(MATERIALS))
def test_the_hidden_state_is_rebuilt_from_strain_and_stress_a_prestress_included(fake, name):
    m = MATERIALS[name]()
    law, prm = m.behavior.law, m.behavior.params()
    n = 16
    m.set_data_manager(n)
    rng = np.random.default_rng(8)
    # a prestress inside the set with a zero strain: the next trial is sigma_n + C eps
    pre = ps.sample_admissible(law, prm, n, rng) * 0.8
    m.set_initial_state_dict({"Stress": pre})
    h = m._parts[0][0]
    got = np.empty((n, 3))
    assert fake.dxm_get_state(h, 0, 0, got.ctypes.data) == 0
    S = ps.compliance(E, NU)
    assert np.array_equal(got, -(pre @ S.T))
    eps = random_trials(law, prm, n, seed=9, lo=0.2, hi=3.0)
    sig, _, _ = m.integrate(eps)
    r = ps.update(law, eps, -(pre @ S.T), prm)
    assert np.array_equal(np.asarray(sig), r["stress"])
    el = ~r["plastic"]
    assert el.any() and np.abs(np.asarray(sig)[el] - (pre[el] + eps[el] @ ps.stiffness(E, NU).T)).max() <= 1e-12 * ps.scale(law, prm)
    # strain and stress together, and the strain alone (the stress of s0 stays what it was)
    eps_n = eps * 0.5
    m.set_initial_state_dict({"Strain": eps_n, "Stress": pre})
    fake.dxm_get_state(h, 0, 0, got.ctypes.data)
    assert np.array_equal(got, eps_n - pre @ S.T)
    m.set_initial_state_dict({"Strain": 0 * eps_n})
    fake.dxm_get_state(h, 0, 0, got.ctypes.data)
    assert np.array_equal(got, -(pre @ S.T))
    with pytest.raises(AssertionError, match="unknown field"):
        m.set_initial_state_dict({"PlasticStrain": got})
    m.close()


def test_newton_controls_reach_the_handle_and_a_capped_point_is_counted(fake):
    m = PlaneStressvonMises(E, NU, SIG0, shear_weight=1.5)
    prm = m.behavior.params()
    eps = random_trials(ps.QUADRATIC, prm, 32, seed=1, lo=50.0, hi=1e4)
    m.set_data_manager(32)
    m.set_newton(maxit=1)
    m.integrate(eps)      # (integrate reports the count, it does not raise)
    r = ps.update(ps.QUADRATIC, eps, 0 * eps, prm, maxit=1)
    assert r["not_converged"].sum() >= 16 and m.last_stats["n_not_converged"] == int(r["not_converged"].sum())
    assert m.last_stats["max_local_iters"] == 1
    m.set_newton()
    m.integrate(eps)
    assert m.last_stats["n_not_converged"] == 0 and 2 <= m.last_stats["max_local_iters"] <= 8
    m.close()


# ---- the reference's generic.Material with the restatement where its classes solve a conic program -----------------------------------------
@pytest.mark.parametrize("name", list(MATERIALS))
def test_the_same_state_semantics_through_the_references_material(fake, name):
    from oracle.ref_import import import_reference, reference_available

    if not reference_available():
        pytest.skip("the reference tree is absent")
    generic, _ = import_reference()
    mine = MATERIALS[name]()
    law, prm = mine.behavior.law, mine.behavior.params()
    Cm, Sm = ps.stiffness(E, NU), ps.compliance(E, NU)

    class Projected(generic.Material):
        """the reference's protocol (state = the strain and the stress of the last accepted increment), the closest point taken
        from the restatement"""

        @property
        def gradients(self):
            return {"Strain": 3}

        @property
        def fluxes(self):
            return {"Stress": 3}

        def constitutive_update(self, eps, state, dt):
            plastic_strain = state["Strain"] - Sm @ state["Stress"]
            out = ps.update(law, eps[None], plastic_strain[None], prm)
            state["Strain"], state["Stress"] = eps, out["stress"][0]
            return Cm, state

    ref = Projected()
    Eps, ts = demo_paths()
    ref.set_data_manager(len(Eps))
    mine.set_data_manager(len(Eps))
    s = ps.scale(law, prm)
    for k, t in enumerate(ts):
        sig_r, _, Ct_r = ref.integrate(t * Eps)
        sig_m, _, Ct_m = mine.integrate(t * Eps)
        # the reference carries (strain, stress), the kernel the plastic strain: the same trial up to the rounding of C^-1 sigma
        assert np.abs(np.asarray(sig_m) - sig_r).max() <= 1e-12 * s, k
        assert np.array_equal(np.asarray(Ct_m).reshape(-1, 3, 3), np.asarray(Ct_r))
        if k % 5 == 4:
            ref.data_manager.revert()
            mine.data_manager.revert()
            a, b = ref.get_final_state_dict(), mine.get_final_state_dict()
        else:
            ref.data_manager.update()
            mine.data_manager.update()
            a, b = ref.get_initial_state_dict(), mine.get_initial_state_dict()
        assert set(a) == set(b) == {"Strain", "Stress"}
        assert np.array_equal(np.asarray(b["Strain"]), a["Strain"]) and np.abs(np.asarray(b["Stress"]) - a["Stress"]).max() <= 1e-12 * s
    mine.close()
