"""CPU: plane-strain Hosford plasticity (DXM_LAW_PE_HOSFORD_LINEAR = 40), law 10 of ``test_hosford_cpu.py`` on the 4-wide strain
``[xx, yy, zz, sqrt(2) xy]``.

1. The restriction that defines the law is exact: for an embedded strain the out-of-plane stress, elastic strain and tangent coupling
   of ``hosford_ref.update`` are exactly 0.0, the restatement converges on every class, and its tangent is symmetric.
2. The golden set ``tests/golden/hosford_plane.npz`` (``make_hosford_plane.py``): the restatement against the stored 50-digit rows
   within the stored bounds, which sit on their floor of 1e-12.
3. The Python layer over a test double of the library, the law table row, the header lines.
4. The transfer plans of law 40 in a stand-alone harness built with AddressSanitizer and UBSan and run directly."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions as cv

import hosford_plane_ref as hp
import hosford_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hosford_plane.npz"))
P = hp.PROPS


def behaviour(a=10.0, hypothesis="plane_strain", **over):
    p = {**P, **over}
    return jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=p["E"], nu=p["nu"]), jm.LinearHardening(p["R0"], p["H"]), a=a,
                                        hypothesis=hypothesis)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_input_classes_have_their_property():
    assert hp.CLASSES == ("generic", "elastic", "below", "above", "inplane_equal", "zz_equal", "near", "axis_aligned", "volumetric", "zero")
    assert hp.EXPONENTS == hr.EXPONENTS
    lam, mu = hr.lame(P["E"], P["nu"])
    for a in hp.EXPONENTS:
        for cls in hp.CLASSES:
            eps, ep, p = hp.make_inputs(cls, 24, a, seed=3)
            assert eps.shape == ep.shape == (24, 4) and p.shape == (24,)
            e = eps - ep
            seq = hr.flow(hr._deviatoric_stress(cv.embed_plane_strain(e), mu), a)[0]
            ratio = seq / (P["R0"] + P["H"] * p)
            if cls in ("generic", "inplane_equal", "zz_equal", "near", "axis_aligned"):
                assert (ratio > 1.04).all() and (ratio <= hr.max_overshoot(a) * (1 + 1e-9)).all(), (cls, a)
            if cls == "elastic":
                assert (ratio < 0.91).all()
            if cls in ("below", "above"):
                assert np.allclose(ratio, 1.0, atol=2e-6) and ((ratio < 1).all() if cls == "below" else (ratio > 1).all())
            if cls == "inplane_equal":
                assert np.array_equal(e[:, 0], e[:, 1]) and not e[:, 3].any()          # isotropic in-plane block, exactly
            if cls == "axis_aligned":
                assert not e[:, 3].any() and (e[:, 0] != e[:, 1]).all()
            if cls == "zz_equal":
                assert np.array_equal(e[1::2, 1], e[1::2, 2]) and not e[1::2, 3].any() and e[::2, 3].any()
            if cls == "near":
                T = hr.to_tensor(cv.embed_plane_strain(e))[:, :2, :2]
                w = np.linalg.eigvalsh(T)
                gap = np.abs(w[:, 1] - w[:, 0])      # strains stay below 2e-2 at an overshoot of 3: gaps of 1e-12 ... 1e-3 of that
                assert (gap <= 1.1e-3 * 2e-2).all() and (gap[::4] <= 1.1e-12 * 2e-2).all() and (gap[3::4] > 1e-8).all()
            if cls == "volumetric":
                assert np.array_equal(e[:, 0], e[:, 1]) and np.array_equal(e[:, 0], e[:, 2]) and not e[:, 3].any()
            if cls == "zero":
                assert not eps.any() and not ep.any() and not p.any()


@pytest.mark.parametrize("a", hp.EXPONENTS)
def test_restricted_reference_is_law_10_on_the_embedding_and_drops_exact_zeros(a):
    for k, cls in enumerate(hp.CLASSES):
        eps, ep, p = hp.make_inputs(cls, 40, a, seed=50 + k)
        r = hp.update(eps, ep, p, **P, a=a)
        w = hr.update(cv.embed_plane_strain(eps), cv.embed_plane_strain(ep), p, **P, a=a)
        assert r["converged"].all() and r["dropped"] == 0.0, (cls, a, r["dropped"])
        assert not w["sig"][:, 4:].any() and not w["eel"][:, 4:].any() and not w["Ct"][:, :4, 4:].any() and not w["Ct"][:, 4:, :4].any()
        assert np.array_equal(r["sig"], w["sig"][:, :4]) and np.array_equal(r["Ct"], w["Ct"][:, :4, :4]) and np.array_equal(r["p"], w["p"])
        assert np.array_equal(r["eel"], w["eel"][:, :4]) and np.array_equal(r["ep"], w["ep"][:, :4])
        assert r["sig"].shape == (40, 4) and r["Ct"].shape == (40, 4, 4)
        asym = np.abs(r["Ct"] - r["Ct"].transpose(0, 2, 1)).max() / np.abs(r["Ct"]).max()
        assert asym <= 1e-13, (cls, a, asym)
        if cls in ("elastic", "below", "volumetric", "zero"):
            assert not r["plastic"].any()
        elif cls != "zero":
            assert r["plastic"].all(), (cls, a)


def test_golden_set_and_its_bounds():
    assert GOLD["eps"].shape == (250, 4) and GOLD["Ct"].shape == (250, 4, 4) and GOLD["sig"].shape == (250, 4)
    assert sorted(set(GOLD["a"])) == list(hp.EXPONENTS) and sorted(set(GOLD["cls"])) == list(range(len(hp.CLASSES)))
    bs, bc = float(GOLD["bound_state"]), float(GOLD["bound_tangent"])
    assert bs == max(8 * GOLD["dev_state"].max(), 1e-12) and bc == max(8 * GOLD["dev_tangent"].max(), 1e-12)
    assert bs == 1e-12 and bc == 1e-12                     # both on the floor: the restatement is within 1.6e-14 of its 50-digit version
    for a in hp.EXPONENTS:
        k = GOLD["a"] == a
        got = hp.update(GOLD["eps"][k], GOLD["ep_n"][k], GOLD["p_n"][k], **P, a=a)
        es, ec = hp.errors(got, {q: GOLD[q][k] for q in ("sig", "eel", "p", "Ct")}, P["E"], P["R0"])
        print(f"hosford plane golden a={a}: restatement vs 50 digits stress/state {es.max():.2e} tangent {ec.max():.2e}")
        assert es.max() <= bs / 8 and ec.max() <= bc / 8 and (got["plastic"] == GOLD["plastic"][k]).all()
    # a sample recomputed in 50 digits: the file is what its generator writes
    pytest.importorskip("mpmath")
    for i in (3, 121, 247):
        m = hp.update_mp(GOLD["eps"][i], GOLD["ep_n"][i], GOLD["p_n"][i], **P, a=float(GOLD["a"][i]))
        assert np.array_equal(m["sig"], GOLD["sig"][i]) and np.array_equal(m["Ct"], GOLD["Ct"][i]) and m["p"] == GOLD["p"][i]


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_behaviour_descriptor():
    b = behaviour(a=6.0)
    assert b.law == _lib.LAW_PE_HOSFORD_LINEAR == 40 and (b.ngrad, b.nflux) == (4, 4) and b.params() == [P["E"], P["nu"], P["R0"], P["H"], 6.0]
    assert b.hypothesis == "plane_strain" and (b.gradient_name, b.flux_name) == ("Strain", "Stress")
    props = {"young_modulus": 70e3, "poisson_ratio": 0.3, "R0": 200.0, "hardening_slope": 10.0}
    d = jm.HosfordIsotropicHardening.from_mfront_properties(props, hypothesis="plane_strain")
    assert d.law == 40 and d.params() == [70e3, 0.3, 200.0, 10.0, 10.0] and (d.ngrad, d.nflux) == (4, 4)
    assert jm.HosfordIsotropicHardening.from_mfront_properties({**props, "a": 4.0}, hypothesis="plane_strain").params()[4] == 4.0
    # "3d" and the default are what they were
    for c in (behaviour(hypothesis="3d"), jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=70e3, nu=0.3), jm.LinearHardening(200.0, 10.0)),
              jm.HosfordIsotropicHardening.from_mfront_properties(props), jm.HosfordIsotropicHardening.from_mfront_properties(props, hypothesis="3d")):
        assert c.law == _lib.LAW_HOSFORD_LINEAR == 10 and (c.ngrad, c.nflux) == (6, 6) and "law" not in vars(c) and "hypothesis" not in vars(c)
        assert c.params() == [70e3, 0.3, 200.0, 10.0, 10.0]
    with pytest.raises(NotImplementedError, match="axisymmetric"):
        behaviour(hypothesis="axisymmetric")
    with pytest.raises(ValueError, match="hypothesis must be one of"):
        behaviour(hypothesis="plane_stress")
    with pytest.raises(ValueError, match="hypothesis must be one of"):
        jm.HosfordIsotropicHardening.from_mfront_properties(props, hypothesis="2d")
    with pytest.raises(ValueError, match="Hosford: R0 must be > 0"):
        behaviour(R0=-1.0)
    with pytest.raises(TypeError, match="linear hardening only"):
        jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=70e3, nu=0.3), lambda p: 200.0, hypothesis="plane_strain")


def test_law_table_row_and_header():
    for unknown in (39, 41):
        with pytest.raises(_lib.DxmError, match="unknown law id"):
            _lib.law_info(unknown)
    i = _lib.law_info(_lib.LAW_PE_HOSFORD_LINEAR)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (4, 4, 5, 2, 5, 304)
    assert [i.isv_name[k] for k in range(2)] == [b"ElasticStrain", b"EquivalentPlasticStrain"] and [i.isv_dim[k] for k in range(2)] == [4, 1]
    assert 32 + 40 + 32 + 128 + 72 == 304
    b = _lib.law_blocks(_lib.LAW_PE_HOSFORD_LINEAR)
    assert b.n_blocks == 1 and b.tangent_width == 16 and b.n_external == 0 and (b.block[0].rows, b.block[0].cols) == (4, 4)
    header = open(os.path.join(ROOT, "include", "dxmat.h")).read()
    assert "DXM_LAW_PE_HOSFORD_LINEAR = 40," in header and "DXM_LAW_COUNT = 41\n" in header and "DXM_LAW_COUNT = 39\n" in header
    assert "#define DXM_ABI_VERSION 6" in header and "id 39 is not assigned" in header
    assert len(re.findall(r"^\s*DXM_LAW_COUNT = \d+\s*$", header, flags=re.M)) == 1          # one enumerator; the earlier counts are comment lines
    # no new entry point
    assert "hosford" not in "".join(re.findall(r"\bdxm_\w+\(", header)).lower()


@pytest.fixture
def fake(monkeypatch):
    from fake_dxmat_hosford_plane import FakeDxmatHosfordPlane

    f = FakeDxmatHosfordPlane(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: f)
    return f


def test_material_over_the_test_double(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    n, a = 37, 10.0
    m = JAXMaterial(behaviour(a), lazy_isv=False)
    assert m.gradients == {"Strain": 4} and m.fluxes == {"Stress": 4}
    assert m.internal_state_variables == {"ElasticStrain": 4, "EquivalentPlasticStrain": 1}
    assert m.tangent_blocks == {("Stress", "Strain"): (4, 4)} and m.tangent_size == 16
    assert m.algorithmic_bytes_per_point == 304 and m.name == "HosfordIsotropicHardening" and m.rotation_matrix is None
    m.set_data_manager(n)
    s0 = m.get_initial_state_dict()
    assert set(s0) == {"Strain", "Stress", "ElasticStrain", "EquivalentPlasticStrain"}
    assert all(not np.array(v).any() for v in s0.values()) and np.array(s0["Strain"]).shape == (n, 4)
    nat = m.natural_state(3)
    assert nat["Strain"].shape == (3, 4) and nat["ElasticStrain"].shape == (3, 4) and not any(np.array(v).any() for v in nat.values())
    # two increments with an advance between
    eps1 = hp.mixed_inputs(n, a, seed=5, trivial_state=True)[0]
    sig, isv, Ct = m.integrate(eps1)
    r1 = hp.update(eps1, np.zeros((n, 4)), np.zeros(n), **P, a=a)
    assert np.array_equal(np.array(sig), r1["sig"]) and np.array_equal(np.array(Ct).reshape(n, 4, 4), r1["Ct"])
    assert np.array_equal(np.array(isv), np.concatenate([r1["eel"], r1["p"][:, None]], axis=1)) and np.array(Ct).shape == (n, 4, 4)
    assert m.last_stats["n_plastic"] == int(r1["plastic"].sum()) > 0 and m.last_stats["n_not_converged"] == 0
    m.data_manager.update()
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.array(s0["ElasticStrain"]), r1["eel"]) and np.array_equal(np.array(s0["EquivalentPlasticStrain"]).reshape(n), r1["p"])
    assert np.array_equal(np.array(s0["Strain"]), eps1) and np.array_equal(np.array(s0["Stress"]), r1["sig"])
    eps2 = 1.2 * eps1
    sig2, isv2, Ct2 = m.integrate(eps2)
    r2 = hp.update(eps2, r1["ep"], r1["p"], **P, a=a)
    assert np.array_equal(np.array(sig2), r2["sig"]) and np.array_equal(np.array(Ct2).reshape(n, 4, 4), r2["Ct"])
    # the hidden field is rebuilt as Strain_n - ElasticStrain_n, in four components
    eps_n, eel_n, p_n = hp.make_inputs("generic", n, a, seed=9)[0] * 0.5, 1e-4 * np.random.default_rng(0).standard_normal((n, 4)), np.full(n, 0.01)
    m.set_initial_state_dict({"Strain": eps_n, "ElasticStrain": eel_n, "EquivalentPlasticStrain": p_n})
    h = m._parts[0][0]
    hidden = np.zeros((n, 4))
    assert fake.dxm_get_state(h, _lib.S0, 2, hidden.ctypes.data) == 0 and np.array_equal(hidden, eps_n - eel_n)
    sig3, _, _ = m.integrate(eps2)
    r3 = hp.update(eps2, eps_n - eel_n, p_n, **P, a=a)
    assert np.array_equal(np.array(sig3), r3["sig"])
    with pytest.raises(ValueError):
        m.set_initial_state_dict({"ElasticStrain": np.zeros((n, 6))})
    # explicit state in, explicit state out; the one-point form
    C4, new = m.batched_constitutive_update(eps1, m.natural_state(n))
    assert np.array_equal(np.array(new["Stress"]), r1["sig"]) and np.array_equal(np.array(new["ElasticStrain"]), r1["eel"])
    assert np.asarray(C4).shape == (n, 4, 4) and np.array_equal(np.asarray(C4), r1["Ct"])
    one_sig, one = m.constitutive_update(eps1[12], {})
    assert np.array_equal(np.asarray(one_sig), r1["sig"][12]) and np.array_equal(np.asarray(one["ElasticStrain"]).reshape(-1), r1["eel"][12])
    # a property
    m.update_material_property("a", 6.0)
    assert fake.last_params == [P["E"], P["nu"], P["R0"], P["H"], 6.0] and m.material_properties["a"] == 6.0
    m.set_initial_state_dict(m.natural_state(n))
    assert np.array_equal(np.array(m.integrate(eps1)[0]), hp.update(eps1, np.zeros((n, 4)), np.zeros(n), **P, a=6.0)["sig"])
    with pytest.raises(_lib.DxmError, match="exponent"):
        m.update_material_property("a", 1.0)
    assert m.material_properties["a"] == 6.0
    m.close()
    # the default hypothesis is law 10, 6 wide, as before (the double does not serve it)
    assert behaviour(hypothesis="3d").law == 10


def test_refusals(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    b = behaviour()
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="general symmetric 4x4 block of 16 entries"):
            JAXMaterial(b, tangent_layout=layout)
    m = JAXMaterial(b)
    m.set_data_manager(4)
    with pytest.raises(AttributeError, match="isotropic"):
        m.rotation_matrix = np.eye(3)
    with pytest.raises(NotImplementedError, match="varies from point to point"):
        m.update_material_property("yield_stress.sig0", np.array([1.0, 2.0, 3.0, 4.0]))
    assert m.external_state_variables == {}
    with pytest.raises(Exception, match="Temperature|external state"):
        m.update_external_state_variable("Temperature", 300.0)
    h = m._parts[0][0]
    for layout in (1, 2, 3):
        assert fake.dxm_set_tangent_layout(h, layout) < 0 and b"general symmetric 4x4 block of 16 entries" in fake.dxm_last_error()
    assert fake.dxm_set_param_field(h, 2, None) < 0 and b"per-point parameter fields are not served for plane-strain Hosford" in fake.dxm_last_error()
    assert fake.dxm_integrate_displacement(h, None, None, 0.0, None, None, None, None) < 0
    assert b"not served on a mesh that is not two-dimensional" in fake.dxm_last_error()
    assert fake.dxm_set_newton(h, 0, 1e-14) < 0 and fake.dxm_set_newton(h, 25, 1e-14) == 0
    # the handle still integrates
    eps = hp.make_inputs("generic", 4, 10.0, seed=1, trivial_state=True)[0]
    assert np.array_equal(np.array(m.integrate(eps)[0]), hp.update(eps, np.zeros((4, 4)), np.zeros(4), **P, a=10.0)["sig"])
    m.close()


def test_the_refusal_sentences_of_the_test_double_are_the_librarys():
    import fake_dxmat_hosford_plane as fk

    src = open(os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "dxmat.hip")).read()
    row = src[src.index("constexpr LawDesc law_pe_hosford()"):src.index("// positional: row i is law id i")]
    joined = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', row))
    for sentence in (fk.SET_REFUSAL, fk.NO_DISPLACEMENT, fk.NO_FIELDS, fk.STOCK_ONLY):
        assert sentence in joined, sentence
    # the widths, L_FULL only, the plane gradient kind and kNoFrame come from what the plane-strain rows share
    assert 'LawDesc d = plane_strain_law(DXM_LAW_PE_HOSFORD_LINEAR, 5, 304, "hosford_plane_kernel");' in row
    shared = src[src.index("constexpr LawDesc plane_strain_law("):src.index("constexpr void pe_j2_state(")]
    assert "d.set_layouts = d.launch_layouts = L_FULL;" in shared and "d.plane_kind = GRAD_PLANE_STRAIN4;" in shared and "d.no_frame = kNoFrame;" in shared
    assert "d.alg_bytes = alg_bytes;" in shared and "d.n_grad = d.n_flux = PE_DIM;" in shared
    assert "d.no_fused = d.no_displacement =" in row and "d.set_refusal = d.launch_refusal =" in row
    assert "d.build = build_hosford;" in row and "d.residency_kernel = DXM_STOCK_ONLY(hosford_plane_kernel_fn);" in row
    assert "!kLaws[39].kernel" in src and "{}, law_pe_hosford(),\n};" in src
    # build_hosford's sentences, which the double repeats
    for words in ("Hosford: R0 must be finite and > 0, got %g", "Hosford: the hardening slope H must be finite and >= 0, got %g",
                  "Hosford: the exponent a must be a finite number >= 2, got %g", "invalid elastic constants E=%g nu=%g"):
        assert words in src
    host = open(os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "host_side.hpp")).read()
    assert "r.law == DXM_LAW_PE_HOSFORD_LINEAR" in host[host.index("const bool plain_block"):host.index("const bool gsym")]


# ---- the transfer plans -----------------------------------------------------------------------------------------------------------
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "hosford_plane_plan_harness.cpp")
HDR = os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "host_side.hpp")
OUT = os.path.join(ROOT, "tests", "_san")


@pytest.fixture(scope="module")
def harness():
    cc = next((c for c in (CLANG, shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "hosford_plane_plans_asan_ubsan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cmd = [cc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plans_of_plane_strain_hosford(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 broken statements" in r.stdout, r.stdout + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) == 2880
