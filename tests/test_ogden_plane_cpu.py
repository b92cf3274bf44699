"""CPU: plane-strain Ogden hyperelasticity (DXM_LAW_OGDEN_PE = 38), the law 7 of ``test_ogden_cpu.py`` on the 5-wide deformation
gradient ``[F00, F11, F22, F01, F10]``.

1. The restriction that defines the law is exact: for an embedded F the dropped components of PK1 and the dropped rows x kept columns
   (and kept rows x dropped columns) of the 9 x 9 tangent of ``ogden_ref.closed_form`` are zero (below ``E0`` of the row scale;
   measured: exactly 0.0 on every family).
2. Error floor of the restricted closed form on the plane families against ``ogden_ref.closed_form_mp`` (mpmath, 60 digits;
   ``energy_ad`` where mpmath does not import): measured 3.9e-14 (P), 2.9e-14 (A), 1.2e-14 (PK2Stress), so ``E0 = 2e-13`` of
   ``test_ogden_cpu.py`` holds for them and no ``E0P`` is needed.
3. The restatement of what the kernel evaluates (``ogden_plane_ref.plane_closed_form``: one closed-form rotation, one divided
   difference) against the restricted one: at most ``4 E0`` -- two formulations, each with floor ``E0`` against the truth, a factor 2
   for the two eigen-solvers.  Measured: 1.4e-13 (P at alpha = 28.8), 2.8e-14 (A), 1.1e-14 (PK2Stress).
4. The Python layer over a test double of the library, the law table row and the conventions helpers.
5. The transfer plans of law 38 in a stand-alone harness built with AddressSanitizer and UBSan and run directly.

The simple shears of the families start at 0.01: the stress of a shear g is O(mu g), a difference of parts that are O(mu), so the error
of a row relative to the row's own size has the floor eps / g whatever evaluates it (measured 7e-9 at g = 1e-8 for the mpmath
evaluation of the double-precision F itself)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions as cv

import ogden_plane_ref as op
import ogden_ref as og
from test_ogden_cpu import E0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE5 = np.array([[1.0, 1, 1, 0, 0]])


def families(k):
    sp, _ = op.special_F5()
    return np.concatenate([sp, op.random_F5(200, seed=1 + k)], axis=0)


@pytest.fixture(scope="module")
def restricted():
    """The restricted closed form of every parameter set on its family, evaluated once."""
    return [(prm, families(k), op.restricted_closed_form(families(k), **prm)) for k, prm in enumerate(og.PARAM_SETS)]


def test_special_points_cover_the_families_of_the_issue():
    sp, labels = op.special_F5()
    assert sp.shape == (len(labels), 5) and len(set(labels)) == len(labels)
    for word in ("identity", "volumetric", "diag(a, a, b)", "diag(a, a, b) rotated", "diag(a, b, a)", "simple shear", "F22 ="):
        assert any(word in s for s in labels), word
    for gap in og.GAPS:
        assert f"in-plane gap {gap:g} rotated" in labels and f"gap {gap:g} to c2 rotated" in labels
    assert np.array_equal(sp[0], EYE5[0]) and np.array_equal(op.family(10, seed=0)[:10], sp[:10])
    assert np.array_equal(op.random_F5(7, seed=3), op.family(len(sp) + 7, seed=3)[len(sp):])


def test_restriction_is_exact():
    for k, prm in enumerate(og.PARAM_SETS):
        F9 = op.embed(families(k))
        assert np.array_equal(F9, cv.embed_plane_F(families(k))) and not F9[:, 5:].any()
        P, A, isv = og.closed_form(F9, **prm)
        scale = np.abs(P).max(axis=1)
        scale = np.where(scale > 0.0, scale, 1.0)
        eP = (np.abs(P[:, 5:]).max(axis=1) / scale).max()
        eI = (np.abs(isv[:, 4:]).max(axis=1) / scale).max()
        rows = np.abs(A).max(axis=2)                                      # (N, 9): the scale of every row
        e_kd = (np.abs(A[:, :5, 5:]).max(axis=2) / rows[:, :5]).max()     # kept rows x dropped columns
        e_dk = (np.abs(A[:, 5:, :5]).max(axis=2) / rows[:, 5:]).max()     # dropped rows x kept columns
        print(f"restriction alpha={prm['alpha']}: dropped P {eP:.1e} PK2Stress {eI:.1e} A kept x dropped {e_kd:.1e} dropped x kept {e_dk:.1e}")
        assert max(eP, eI, e_kd, e_dk) <= E0


def _truth(F5, prm):
    try:
        import mpmath  # noqa: F401
    except ImportError:
        P, A = og.energy_ad(op.embed(F5), **prm)
        return "AD", (P[:, :5], A[:, :5, :5])
    res = [og.closed_form_mp(row, **prm) for row in op.embed(F5)]
    return "mpmath", (np.array([r[0][:5] for r in res]), np.array([r[1][:5, :5] for r in res]), np.array([r[2][:4] for r in res]))


def test_error_floor_of_the_restricted_closed_form(restricted):
    sp, _ = op.special_F5()
    n = len(sp) + 16
    figs = {}
    for prm, F, got in restricted:
        name, want = _truth(F[:n], prm)
        if name == "AD":          # AD of eigvalsh divides by the gap: the exactly repeated points have no AD reference
            ok = np.isfinite(want[1]).all(axis=(1, 2))
            e = (og.row_errors(got[0][:n][ok][:, None, :], want[0][ok][:, None, :]).max(), og.row_errors(got[1][:n][ok], want[1][ok]).max())
        else:
            e = op.errors(tuple(x[:n] for x in got), want)
        figs[f"{name} alpha={prm['alpha']}"] = tuple(float(x) for x in e)
    print("plane-strain ogden error floor (P, A, PK2Stress):", figs)
    assert max(max(v) for v in figs.values()) <= E0, figs


def test_the_restatement_of_the_kernel_matches_the_restricted_closed_form(restricted):
    for prm, F, want in restricted:
        got = op.plane_closed_form(F, **prm)
        assert got[0].shape == (len(F), 5) and got[1].shape == (len(F), 5, 5) and got[2].shape == (len(F), 4)
        assert np.isfinite(got[1]).all()
        e = op.errors(got, want)
        print(f"plane restatement vs restricted closed form alpha={prm['alpha']}: P {e[0]:.3e} A {e[1]:.3e} PK2Stress {e[2]:.3e} (bound {4 * E0:.1e})")
        assert max(e) <= 4 * E0, (prm, e)


@pytest.mark.parametrize("prm", og.PARAM_SETS)
def test_identity_is_stress_free_and_inverted_points_give_nan(prm):
    P, A, isv = op.plane_closed_form(EYE5, **prm)
    assert np.array_equal(P, np.zeros((1, 5))) and np.abs(isv).max() == 0.0
    G, K = prm["mu"] * prm["alpha"] / 2.0, prm["K"]
    want = np.zeros((5, 5))
    for r in range(5):
        i, J = op.RI[r], op.RJ[r]
        for c in range(5):
            k, L = op.RI[c], op.RJ[c]
            want[r, c] = (K - 2.0 * G / 3.0) * float(i == J and k == L) + G * (float(i == k and J == L) + float(i == L and J == k))
    assert np.abs(A[0] - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()
    bad = np.array([[1.0, 1, -1, 0, 0], [1.0, 1, 1, 2, 2], [0.0, 0, 1, 0, 0], [1.0, 1, 0, 0, 0]])    # F22 < 0, in-plane det < 0, a zero row, flat
    for fn in (op.plane_closed_form, op.restricted_closed_form):
        P, A, isv = fn(bad, **prm)
        assert np.isnan(P).all() and np.isnan(A).all() and np.isnan(isv).all()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_behaviour_descriptor():
    b = jm.OgdenHyperelasticity(mu=2.0, alpha=4.0, K=10.0, hypothesis="plane_strain")
    assert b.law == _lib.LAW_OGDEN_PE == 38 and (b.ngrad, b.nflux) == (5, 5) and b.params() == [4.0, 2.0, 10.0]
    assert b.hypothesis == "plane_strain" and (b.gradient_name, b.flux_name) == ("DeformationGradient", "FirstPiolaKirchhoffStress")
    d = jm.OgdenHyperelasticity.from_mfront_properties({"mu": 3.0}, hypothesis="plane_strain")
    assert d.law == 38 and d.params() == [28.8, 3.0, 69444444.0]
    # "3d" and the default are what they were
    for c in (jm.OgdenHyperelasticity(), jm.OgdenHyperelasticity(hypothesis="3d"), jm.OgdenHyperelasticity.from_mfront_properties({}),
              jm.OgdenHyperelasticity.from_mfront_properties({}, hypothesis="3d")):
        assert c.law == _lib.LAW_OGDEN == 7 and (c.ngrad, c.nflux) == (9, 9) and "law" not in vars(c) and "hypothesis" not in vars(c)
    with pytest.raises(NotImplementedError, match="axisymmetric"):
        jm.OgdenHyperelasticity(hypothesis="axisymmetric")
    with pytest.raises(ValueError, match="hypothesis must be one of"):
        jm.OgdenHyperelasticity(hypothesis="plane_stress")
    with pytest.raises(ValueError, match="Ogden"):
        jm.OgdenHyperelasticity(mu=-1.0, hypothesis="plane_strain")


def test_law_table_row_and_header():
    with pytest.raises(_lib.DxmError, match="unknown law id"):
        _lib.law_info(37)                      # not assigned
    with pytest.raises(_lib.DxmError, match="unknown law id"):
        _lib.law_info(39)
    i = _lib.law_info(_lib.LAW_OGDEN_PE)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (5, 5, 3, 1, 4, 312)
    assert i.isv_name[0] == b"PK2Stress" and i.isv_dim[0] == 4 and 40 + 40 + 200 + 32 == 312
    b = _lib.law_blocks(_lib.LAW_OGDEN_PE)
    assert b.n_blocks == 1 and b.tangent_width == 25 and b.n_external == 0 and (b.block[0].rows, b.block[0].cols) == (5, 5)
    header = open(os.path.join(ROOT, "include", "dxmat.h")).read()
    assert "DXM_LAW_OGDEN_PE = 38," in header and "DXM_LAW_COUNT = 39\n" in header and "#define DXM_ABI_VERSION 6" in header


def test_conventions_round_trip():
    assert cv.PLANE_F_IDX == (0, 1, 2, 3, 4)
    F5 = op.random_F5(9, seed=2)
    F9 = cv.embed_plane_F(F5)
    assert F9.shape == (9, 9) and np.array_equal(cv.restrict_plane_F(F9), F5) and not F9[:, 5:].any()
    T = cv.nsym_to_tensor(F9)
    assert np.array_equal(T[:, 0, 1], F5[:, 3]) and np.array_equal(T[:, 1, 0], F5[:, 4]) and np.array_equal(T[:, 2, 2], F5[:, 2])
    assert not T[:, 2, :2].any() and not T[:, :2, 2].any()
    A = np.arange(2 * 81, dtype=float).reshape(2, 9, 9)
    assert np.array_equal(cv.restrict_plane_F_tangent(A), A[:, :5, :5]) and cv.restrict_plane_F_tangent(A).flags.c_contiguous
    assert cv.embed_plane_F(F5.reshape(3, 3, 5)).shape == (3, 3, 9)
    for fn, bad in ((cv.embed_plane_F, np.zeros((2, 4))), (cv.restrict_plane_F, np.zeros((2, 5))), (cv.restrict_plane_F_tangent, np.zeros((2, 5, 5)))):
        with pytest.raises(ValueError):
            fn(bad)


@pytest.fixture
def fake(monkeypatch):
    from fake_dxmat_ogden_plane import FakeDxmatOgdenPlane

    f = FakeDxmatOgdenPlane(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: f)
    return f


def test_material_over_the_test_double(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    n = 37
    m = JAXMaterial(jm.OgdenHyperelasticity(hypothesis="plane_strain"))
    assert m.gradients == {"DeformationGradient": 5} and m.fluxes == {"FirstPiolaKirchhoffStress": 5}
    assert m.internal_state_variables == {"PK2Stress": 4}
    assert m.tangent_blocks == {("FirstPiolaKirchhoffStress", "DeformationGradient"): (5, 5)} and m.tangent_size == 25
    assert m.algorithmic_bytes_per_point == 312 and m.name == "OgdenHyperelasticity" and m.rotation_matrix is None
    m.set_data_manager(n)
    s0 = m.get_initial_state_dict()
    assert np.array_equal(s0["DeformationGradient"], np.tile(EYE5, (n, 1))) and not s0["PK2Stress"].any()
    assert np.array_equal(m.natural_state(3)["DeformationGradient"], np.tile(EYE5, (3, 1)))
    F = op.family(n, seed=5)
    P, isv, A = m.integrate(F)
    Pr, Ar, ir = op.restricted_closed_form(F, **og.DEFAULTS)
    assert np.array_equal(np.array(P), Pr) and np.array_equal(np.array(A).reshape(n, 5, 5), Ar) and np.array_equal(np.array(isv), ir)
    assert A.shape == (n, 5, 5) and np.array(isv).shape == (n, 4)
    s1 = m.get_final_state_dict()
    assert set(s1) == {"DeformationGradient", "FirstPiolaKirchhoffStress", "PK2Stress"}
    assert np.array_equal(np.array(s1["PK2Stress"]), ir) and not np.array(m.get_initial_state_dict()["PK2Stress"]).any()
    m.data_manager.update()
    assert np.array_equal(np.array(m.get_initial_state_dict()["PK2Stress"]), ir)
    assert np.array_equal(np.array(m.get_initial_state_dict()["DeformationGradient"]), F)
    # explicit state in, explicit state out, the one-point form, and an initial state set field by field
    Ct, new = m.batched_constitutive_update(F, m.natural_state(n))
    assert np.array_equal(np.array(new["FirstPiolaKirchhoffStress"]), Pr) and np.array_equal(np.array(new["PK2Stress"]), ir)
    assert np.asarray(Ct).shape == (n, 5, 5) and np.array_equal(np.asarray(Ct), Ar)
    sig, one = m.constitutive_update(F[12], {})
    assert np.array_equal(np.asarray(sig), Pr[12]) and np.array_equal(np.asarray(one["PK2Stress"]).reshape(-1), ir[12])
    m.set_initial_state_dict({"DeformationGradient": F, "PK2Stress": 2.0 * ir})
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.array(s0["DeformationGradient"]), F) and np.array_equal(np.array(s0["PK2Stress"]), 2.0 * ir)
    m.update_material_property("mu", 1000.0)
    assert fake.last_params == [28.8, 1000.0, 69444444.0]
    assert np.array_equal(np.array(m.integrate(F)[0]), op.restricted_closed_form(F, 28.8, 1000.0, 69444444.0)[0])
    with pytest.raises(_lib.DxmError, match="mu must be"):
        m.update_material_property("mu", -1.0)
    m.close()
    # the default hypothesis over the same double: law 7, 9 wide, as before
    m9 = JAXMaterial(jm.OgdenHyperelasticity())
    assert m9.gradients == {"DeformationGradient": 9} and m9.tangent_size == 81 and m9.internal_state_variables == {"PK2Stress": 6}
    m9.close()


def test_refusals(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    b = jm.OgdenHyperelasticity(hypothesis="plane_strain")
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="5x5 block of 25 entries"):
            JAXMaterial(b, tangent_layout=layout)
    m = JAXMaterial(b)
    m.set_data_manager(4)
    with pytest.raises(AttributeError, match="isotropic"):
        m.rotation_matrix = np.eye(3)
    with pytest.raises(NotImplementedError, match="varies from point to point"):
        m.update_material_property("K", np.array([1.0, 2.0, 3.0, 4.0]))
    assert fake.dxm_set_tangent_layout(m._parts[0][0], 1) < 0 and b"5x5 block of 25 entries" in fake.dxm_last_error()
    assert fake.dxm_integrate_displacement(m._parts[0][0], None, None, 0.0, None, None, None, None) < 0
    assert b"[1 + H00, 1 + H11, 1, H01, H10]" in fake.dxm_last_error()
    m.close()


def test_the_refusal_sentences_of_the_test_double_are_the_librarys():
    import fake_dxmat_ogden_plane as fk

    src = open(os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "dxmat.hip")).read()
    row = src[src.index("constexpr LawDesc law_ogden_pe()"):src.index("// positional: row i is law id i")]
    joined = "".join(__import__("re").findall(r'"((?:[^"\\]|\\.)*)"', row))
    assert fk.SET_REFUSAL in joined and fk.NO_DISPLACEMENT in joined
    assert "d.no_fused = d.no_displacement =" in row and "d.set_layouts = d.launch_layouts = L_FULL;" in row and "d.alg_bytes = 312;" in row
    assert "d.build = build_ogden;" in row and "d.no_fields" in row and "d.no_frame" in row and "d.stock_only" in row


# ---- the transfer plans -----------------------------------------------------------------------------------------------------------
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "ogden_plane_plan_harness.cpp")
HDR = os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "host_side.hpp")
OUT = os.path.join(ROOT, "tests", "_san")


@pytest.fixture(scope="module")
def harness():
    cc = next((c for c in (CLANG, shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ogden_plane_plans_asan_ubsan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cmd = [cc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plans_of_plane_strain_ogden(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 broken statements" in r.stdout, r.stdout + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) == 3840
