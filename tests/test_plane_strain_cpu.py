"""CPU: the plane-strain hypothesis (DXM_LAW_PE_ELASTIC_ISO = 26, DXM_LAW_PE_J2_LINEAR = 27, DXM_LAW_PE_J2_VOCE = 28) without a GPU: the
4-component restatement ``plane_strain_ref`` against the 6-wide oracle on the embedded input, against a known answer that owes the
oracle nothing and against central differences; the library's tables and refusal sentences; the Python layer over the test double
``fake_dxmat_plane_strain``; and two of the reference's own plane-strain tests replayed over the quadrature map."""
import ctypes as C
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp
from oracle.ref_import import REFERENCE_ROOT, reference_available

import plane_strain_ref as pe
from fake_dxmat_plane_strain import REFUSAL, FakeDxmatPlaneStrain

N_ORACLE = 4161        # the largest size of the GPU parity test, which runs on the first N of these points
BOUND = 1e-13          # of the field scale: sig0 for stresses, E for tangents, sig0 / E for strains (the issue's figure)


def hard_of(law, prm):
    return onp.LinearHardening(prm[2], prm[3]) if law == pe.J2_LINEAR else onp.VoceHardening(prm[2], prm[3], prm[4])


def oracle_history(law, prm, incs):
    """the 6-wide oracle on the embedded increments: [(result, kink mask)]"""
    ep, p, out = np.zeros((len(incs[0]), 6)), np.zeros(len(incs[0])), []
    for e in incs:
        r = onp.j2_update(conventions.embed_plane_strain(e), ep, p, prm[0], prm[1], hard_of(law, prm))
        out.append((r, np.abs(r["f_trial"]) <= pe.KINK * prm[2]))
        ep, p = r["epsp"], r["p"]
    return out


# ---- the restatement against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zz", [True, False], ids=["eps_zz", "eps_zz=0"])
@pytest.mark.parametrize("case", list(pe.CASES))
def test_the_restatement_equals_the_embedded_and_restricted_oracle(case, zz):
    law, prm = pe.CASES[case]
    sig0, Em = prm[2], prm[0]
    incs = pe.increments(N_ORACLE, sig0, Em, zz=zz)
    ep, p = np.zeros((N_ORACLE, 4)), np.zeros(N_ORACLE)
    shares = []
    for k, (e, (o, skip)) in enumerate(zip(incs, oracle_history(law, prm, incs))):
        r = pe.update(law, e, ep, p, prm)
        # the restriction loses nothing: what the oracle holds out of the plane is exactly zero
        assert not o["sig"][:, 4:].any() and not o["epsp"][:, 4:].any() and not o["Ct"][:, :4, 4:].any() and not o["Ct"][:, 4:, :4].any()
        assert skip.sum() == 0 and skip.mean() < 0.01, (case, k, int(skip.sum()))      # none at all for this seed
        keep = ~skip
        assert np.array_equal(r["plastic"][keep], o["plastic"][keep])
        err = {"stress": np.abs(r["stress"] - conventions.restrict_plane_strain(o["sig"]))[keep].max() / sig0,
               "tangent": np.abs(r["tangent"].reshape(-1, 4, 4) - conventions.restrict_plane_strain_tangent(o["Ct"]))[keep].max() / Em,
               "epsp": np.abs(r["epsp"] - conventions.restrict_plane_strain(o["epsp"]))[keep].max() / (sig0 / Em),
               "p": np.abs(r["p"] - o["p"])[keep].max() / (sig0 / Em)}
        print(case, zz, k, int(r["plastic"].sum()), err)
        assert max(err.values()) <= BOUND, (case, k, err)
        assert not r["not_converged"].any() and np.array_equal(r["iters"], o["iters"])
        shares.append(r["plastic"].mean())
        ep, p = r["epsp"], r["p"]
    assert 0.3 < shares[0] < 0.8 and shares[1] == 0.0 and shares[2] > shares[0]      # load, unload, reload beyond


def test_the_elastic_restatement_equals_the_oracle_and_the_4x4_block():
    law, prm = pe.ELASTIC_CASE
    eps = pe.strains(N_ORACLE, pe.SIG0, pe.E, seed=5)
    r = pe.update(law, eps, prm=prm)
    sig, Ct = onp.elastic_iso(conventions.embed_plane_strain(eps), prm[0], prm[1])
    assert not sig[:, 4:].any() and not Ct[:, :4, 4:].any()
    assert np.abs(r["stress"] - sig[:, :4]).max() <= BOUND * pe.SIG0
    assert np.abs(r["tangent"].reshape(-1, 4, 4) - conventions.restrict_plane_strain_tangent(Ct)).max() <= BOUND * pe.E
    assert np.array_equal(r["tangent"][0].reshape(4, 4), pe.stiffness(*prm)) and pe.stats(law, r)["n_plastic"] == 0


def test_embed_and_restrict():
    v = np.arange(8.0).reshape(2, 4)
    e = conventions.embed_plane_strain(v)
    assert e.shape == (2, 6) and np.array_equal(e[:, :4], v) and not e[:, 4:].any()
    assert np.array_equal(conventions.restrict_plane_strain(e), v)
    Cm = np.arange(36.0).reshape(6, 6)
    assert np.array_equal(conventions.restrict_plane_strain_tangent(Cm), Cm[:4, :4])
    for bad, fn in ((np.zeros(6), conventions.embed_plane_strain), (np.zeros(4), conventions.restrict_plane_strain),
                    (np.zeros((4, 4)), conventions.restrict_plane_strain_tangent)):
        with pytest.raises(ValueError):
            fn(bad)


# ---- the tangent against central differences -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["linear_H5e3", "voce"])
def test_restated_tangent_against_central_differences(case):
    """bound and exclusion of ``tests/test_oracle.py::test_tangent_matches_central_differences``, the same check of the 6-wide law:
    h = 1e-8, points within 1e-4 sig0 of the kink left out, 2e-8 of the largest tangent entry"""
    law, prm = pe.CASES[case]
    n = 300
    a, _, c = pe.increments(n, prm[2], prm[0], seed=31)
    first = pe.update(law, a, np.zeros((n, 4)), np.zeros(n), prm)
    r = pe.update(law, c, first["epsp"], first["p"], prm)
    h = 1e-8
    fd = np.zeros((n, 4, 4))
    for j in range(4):
        d = np.zeros(4)
        d[j] = h
        fd[:, :, j] = (pe.update(law, c + d, first["epsp"], first["p"], prm)["stress"] - pe.update(law, c - d, first["epsp"], first["p"], prm)["stress"]) / (2 * h)
    ct = r["tangent"].reshape(n, 4, 4)
    safe = r["plastic"] & (np.abs(r["f_trial"]) > 1e-4 * prm[2])
    assert safe.sum() >= 100
    assert np.abs(fd[safe] - ct[safe]).max() < 2e-8 * np.abs(ct).max()
    assert np.array_equal(ct, ct.transpose(0, 2, 1))                    # entries are k3 * (ni * nj): exactly symmetric


# ---- the library's tables (host code: no device needed) -------------------------------------------------------------------------------
def test_law_rows_26_to_28_and_the_unassigned_ids_around_them():
    assert (_lib.LAW_PE_ELASTIC_ISO, _lib.LAW_PE_J2_LINEAR, _lib.LAW_PE_J2_VOCE) == (26, 27, 28)
    want = {26: (4, 4, 2, 0, 0, 192), 27: (4, 4, 4, 2, 5, 272), 28: (4, 4, 5, 2, 5, 272)}
    for law, row in want.items():
        i = _lib.law_info(law)
        assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == row
        if law != 26:
            assert [(i.isv_name[f].decode(), i.isv_dim[f]) for f in range(2)] == [("p", 1), ("epsp", 4)]
        b = _lib.law_blocks(law)
        assert (b.n_external, b.n_blocks, b.tangent_width) == (0, 1, 16)
        k = b.block[0]
        assert (k.row_kind, k.row_index, k.col_kind, k.col_index, k.rows, k.cols) == (0, 0, 0, 0, 4, 4)
    for law in (25, 29):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_blocks(law)
    assert _lib.load().dxm_abi_version() == 6


def test_create_without_a_gpu_fails_loudly_for_the_new_laws_too():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    for law, prm in ((26, [pe.E, pe.NU]), (27, pe.CASES["linear_H5e3"][1]), (28, pe.CASES["voce"][1])):
        assert not lib.dxm_create(law, (C.c_double * len(prm))(*prm), len(prm), 8, 0)
        assert b"no usable HIP device" in lib.dxm_last_error()
    with pytest.raises(_lib.DxmError, match="no usable HIP device"):
        JAXMaterial(jm.ElasticBehavior(jm.LinearElasticIsotropic(E=pe.E, nu=pe.NU), hypothesis="plane_strain")).set_data_manager(8)


def test_refusal_sentences_and_what_the_rows_declare():
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    src = open(os.path.join(csrc, "dxmat.hip")).read()
    base = src[src.index("constexpr LawDesc plane_strain_law("):]
    base = base[:base.index("\n}\n")]
    for field in ("set_refusal", "launch_refusal", "no_fields", "no_fused", "no_displacement", "no_frame", "stock_only"):
        assert f"d.{field} = " in base or f"d.{field} = d." in base or f" = d.{field} = " in base, field
    assert "d.set_layouts = d.launch_layouts = L_FULL;" in base and "d.no_frame = kNoFrame;" in base and "PE_BLOCKS_PER_CU" in base
    for words in ("the plane-strain tangent is a 4x4 block of 16 entries", "per-point parameter fields are not served under the plane-strain hypothesis",
                  "the plane-strain laws take a 4-wide strain", "dxm_integrate_displacement*", "fused displacement gradient",
                  "the plane-strain laws take the stock hardening laws only"):
        assert words in base, words
    assert REFUSAL.split(":")[0] in base
    # the three rows: the parameters of laws 0 / 1 / 2 through their build functions, the state of the two J2 laws, the grids
    for fn, build, extra in (("law_pe_elastic", "build_elastic", "192"), ("law_pe_j2_linear", "build_linear_hardening", "pe_j2_state(d);"),
                             ("law_pe_j2_voce", "build_voce_hardening", "PE_BLOCKS_PER_CU_VOCE")):
        row = src[src.index(f"constexpr LawDesc {fn}()"):]
        row = row[:row.index("\n}\n")]
        assert f"d.build = {build};" in row and extra in row and "DXM_STOCK_ONLY(launch_plane_strain<" in row, fn
    state = src[src.index("constexpr void pe_j2_state("):]
    assert 'state_field(d, 0, "p", 1, 0);' in state[:400] and 'state_field(d, 1, "epsp", PE_DIM, 1);' in state[:400]
    assert "UNMEASURED" in src[src.index("// The plane-strain forms of laws 0 / 1 / 2"):src.index("constexpr LawDesc plane_strain_law(")]
    # the external-state refusal is the library's one sentence for every law without one
    assert "has no external state variable: its update reads the gradient, its parameters and its own state only" in src
    assert "!kLaws[25].kernel" in src and "kKernelOrder[5]" in src
    # the host path moves the 16 entries as they are
    hs = open(os.path.join(csrc, "host_side.hpp")).read()
    assert "r.law == DXM_LAW_PE_ELASTIC_ISO || r.law == DXM_LAW_PE_J2_LINEAR || r.law == DXM_LAW_PE_J2_VOCE" in hs
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.__file__)), "include", "dxmat.h")).read()
    for words in ("DXM_LAW_PE_ELASTIC_ISO = 26", "DXM_LAW_PE_J2_LINEAR = 27", "DXM_LAW_PE_J2_VOCE = 28", "DXM_LAW_COUNT = 29"):
        assert words in hdr


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
EL = jm.LinearElasticIsotropic(E=pe.E, nu=pe.NU)


def behaviours(hypothesis):
    kw = {} if hypothesis is None else {"hypothesis": hypothesis}
    return (jm.ElasticBehavior(EL, **kw), jm.vonMisesIsotropicHardening(EL, jm.LinearHardening(250.0, 5e3), **kw),
            jm.vonMisesIsotropicHardening(EL, jm.VoceHardening(350.0, 500.0, 1e3), **kw))


def test_behaviours_at_both_hypotheses():
    for hyp in (None, "3d"):
        for b, law in zip(behaviours(hyp), (0, 1, 2)):
            assert (b.law, b.ngrad, b.nflux, b.hypothesis) == (law, 6, 6, "3d")
    for b, law in zip(behaviours("plane_strain"), (26, 27, 28)):
        assert (b.law, b.ngrad, b.nflux, b.hypothesis) == (law, 4, 4, "plane_strain")
    assert behaviours("plane_strain")[1].params() == behaviours("3d")[1].params() == [pe.E, pe.NU, 250.0, 5e3]
    assert behaviours("plane_strain")[2].params() == [pe.E, pe.NU, 350.0, 500.0, 1e3]
    with pytest.raises(NotImplementedError, match="axisymmetric.*follow-up"):
        jm.ElasticBehavior(EL, hypothesis="axisymmetric")
    with pytest.raises(NotImplementedError, match="axisymmetric"):
        jm.vonMisesIsotropicHardening(EL, jm.LinearHardening(250.0, 5e3), hypothesis="axisymmetric")
    with pytest.raises(ValueError, match="hypothesis must be one of"):
        jm.ElasticBehavior(EL, hypothesis="plane_stress")
    custom = jm.CustomHardening("sig0 + K * p", "K", sig0=250.0, K=1e3)
    for y in (custom, lambda p: 250.0 + 1e3 * p):
        with pytest.raises(TypeError, match="LinearHardening or materials.VoceHardening"):
            jm.vonMisesIsotropicHardening(EL, y, hypothesis="plane_strain")
    assert jm.vonMisesIsotropicHardening(EL, custom).law == 2      # "3d" takes it as before


@pytest.fixture
def fake(monkeypatch):
    lib = FakeDxmatPlaneStrain(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    return lib


def test_names_and_sizes_of_the_materials(fake):
    for b, isv, nbytes in zip(behaviours("plane_strain"), ({}, {"p": 1, "epsp": 4}, {"p": 1, "epsp": 4}), (192, 272, 272)):
        m = JAXMaterial(b)
        assert m.gradients == {"strain": 4} and m.fluxes == {"stress": 4} and m.internal_state_variables == isv
        assert m.tangent_blocks == {("stress", "strain"): (4, 4)} and m.tangent_size == 16 and m.algorithmic_bytes_per_point == nbytes
        for layout in ("sym", "coef", "pack4"):
            with pytest.raises(ValueError, match="no packed tangent record"):
                JAXMaterial(b, tangent_layout=layout)
    for b in behaviours("3d"):
        m = JAXMaterial(b)
        assert m.gradients == {"strain": 6} and m.fluxes == {"stress": 6} and m.tangent_blocks == {("stress", "strain"): (6, 6)}
    m = JAXMaterial(behaviours("plane_strain")[1], gradient_name="Strain", flux_name="Stress")     # MFront's names
    assert m.gradients == {"Strain": 4} and m.fluxes == {"Stress": 4} and m.tangent_blocks == {("Stress", "Strain"): (4, 4)}


@pytest.mark.parametrize("which", [1, 2], ids=["linear", "voce"])
def test_integrate_update_revert_and_the_state_dictionaries(fake, which):
    b = behaviours("plane_strain")[which]
    law, prm = b.law, b.params()
    n = 40
    m = JAXMaterial(b)
    m.set_data_manager(n)
    s0 = m.get_initial_state_dict()
    assert set(s0) == {"strain", "stress", "p", "epsp"} and np.asarray(s0["epsp"]).shape == (n, 4) and not np.asarray(s0["epsp"]).any()
    ep, p = np.zeros((n, 4)), np.zeros(n)
    incs = pe.increments(n, prm[2], prm[0], seed=8)
    for k, e in enumerate(incs):
        sig, isv, Ct = m.integrate(e)
        r = pe.update(law, e, ep, p, prm)
        assert np.array_equal(np.asarray(sig), r["stress"]) and np.asarray(Ct).shape == (n, 4, 4)
        assert np.array_equal(np.asarray(Ct).reshape(n, 16), r["tangent"])
        assert np.array_equal(np.asarray(isv)[:, 0], r["p"]) and np.array_equal(np.asarray(isv)[:, 1:], r["epsp"])
        assert m.last_stats["n_plastic"] == int(r["plastic"].sum()) and m.last_stats["n_nan"] == 0
        if k == 1:      # a rejected increment: s1 <- s0, then the same increment again gives the same answer
            m.data_manager.revert()
            s1 = m.get_final_state_dict()
            assert np.array_equal(np.asarray(s1["epsp"]), ep) and np.array_equal(np.asarray(s1["p"]).reshape(n), p)
            sig2, _, _ = m.integrate(e)
            assert np.array_equal(np.asarray(sig2), r["stress"])
        s1 = m.get_final_state_dict()
        assert np.array_equal(np.asarray(s1["strain"]), e) and np.array_equal(np.asarray(s1["stress"]), r["stress"])
        assert np.array_equal(np.asarray(s1["epsp"]), r["epsp"])
        m.data_manager.update()
        s0 = m.get_initial_state_dict()
        assert np.array_equal(np.asarray(s0["epsp"]), r["epsp"]) and np.array_equal(np.asarray(s0["p"]).reshape(n), r["p"])
        ep, p = r["epsp"], r["p"]
    assert (p > 0).sum() >= 10
    m.close()


def test_a_prestate_of_p_and_epsp(fake):
    b = behaviours("plane_strain")[1]
    law, prm = b.law, b.params()
    n = 24
    m = JAXMaterial(b)
    m.set_data_manager(n)
    p0 = np.full(n, 2e-3)
    ep0 = np.tile([2e-3, -1e-3, -1e-3, 0.0], (n, 1)) * np.linspace(0.5, 1.5, n)[:, None]
    m.set_initial_state_dict({"p": p0, "epsp": ep0})
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.asarray(s0["epsp"]), ep0) and np.array_equal(np.asarray(s0["p"]).reshape(n), p0)
    eps = pe.strains(n, prm[2], prm[0], seed=12)
    sig, isv, _ = m.integrate(eps)
    r = pe.update(law, eps, ep0, p0, prm)
    assert np.array_equal(np.asarray(sig), r["stress"]) and np.array_equal(np.asarray(isv)[:, 1:], r["epsp"]) and r["plastic"].any()
    with pytest.raises(Exception):
        m.set_initial_state_dict({"epsp": np.zeros((n, 6))})          # the 6-wide plastic strain of the "3d" law does not fit
    m.close()


def test_newton_controls_reach_the_handle_and_a_capped_point_is_counted(fake):
    b = behaviours("plane_strain")[2]
    prm = b.params()
    eps = 4.0 * pe.strains(32, prm[2], prm[0], seed=1)
    m = JAXMaterial(b)
    m.set_data_manager(32)
    m.set_newton(maxit=1)
    m.integrate(eps)
    r = pe.update(28, eps, np.zeros((32, 4)), np.zeros(32), prm, maxit=1)
    assert r["not_converged"].sum() >= 8 and m.last_stats["n_not_converged"] == int(r["not_converged"].sum())
    assert m.last_stats["max_local_iters"] == 1
    m.set_newton()
    m.integrate(eps)
    assert m.last_stats["n_not_converged"] == 0 and 2 <= m.last_stats["max_local_iters"] <= 8
    m.close()


# ---- a known answer that owes the oracle nothing ---------------------------------------------------------------------------------------
def uniaxial_plane_strain_tension(material, steps=50, exx_max=2e-2, sig0=250.0):
    """``tests/mfront/test_elastoplasticity.py:31-36`` on one point: eps_xx ramps, eps_zz = 0, sig_yy = 0 found by a scalar Newton on
    eps_yy with the returned tangent.  Returns (final stress, most Newton iterations of a step)."""
    eyy, worst = 0.0, 0
    for exx in np.linspace(0.0, exx_max, steps + 1)[1:]:
        for it in range(1, 30):
            sig, _, Ct = material.integrate(np.array([[exx, eyy, 0.0, 0.0]]))
            sig, Ct = np.asarray(sig)[0], np.asarray(Ct).reshape(4, 4)
            if abs(sig[1]) <= 1e-10 * sig0:
                break
            eyy -= sig[1] / Ct[1, 1]
        worst = max(worst, it)
        material.data_manager.update()
    return sig.copy(), worst


def test_uniaxial_plane_strain_tension_ends_on_the_known_answer(fake):
    sig0 = 250.0
    m = JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=70e3, nu=0.3), jm.LinearHardening(sig0, 1e-6), hypothesis="plane_strain"))
    m.set_data_manager(1)
    sig, worst = uniaxial_plane_strain_tension(m, sig0=sig0)
    print("final stress", sig, "most iterations of a step", worst)
    assert np.allclose(sig[:3], 2 / np.sqrt(3) * np.array([sig0, 0.0, sig0 / 2]), rtol=1e-2, atol=1e-8)
    assert worst < 12 and sig[3] == 0.0
    m.close()


# ---- the reference's tests replayed over the quadrature map -----------------------------------------------------------------------------
def mfront_like_material():
    """the material of tests/mfront/test_multimaterials.py:75-90 and test_initialization.py:44-58"""
    return JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=70e3, nu=0.3), jm.LinearHardening(250.0, 5e3), hypothesis="plane_strain"),
                       gradient_name="Strain", flux_name="Stress")


def test_two_maps_on_disjoint_cells_equal_one_map_on_all(fake):
    """``test_multimaterials.py:171-172``: 2 x 2 quadrilaterals with 4 points each; the left and the right column hold their own
    material (the same law), and the fields of the two maps add up to those of the one map over all cells and never overlap"""
    ncell, nqp = 4, 4
    n = ncell * nqp
    left, right = np.array([0, 2]), np.array([1, 3])
    maps = [QuadratureFieldMap(ncell, nqp, mfront_like_material(), cells=c) for c in (None, left, right)]
    now = {}
    for q in maps:
        assert q.jacobian_flatten.dim == 16 and q.fluxes["Stress"].dim == 4 and q.internal_state_variables["epsp"].dim == 4
        assert np.asarray(q.jacobians[("Stress", "Strain")], dtype=object).shape == (4, 4)
        q.register_gradient("Strain", lambda c: now["eps"].reshape(ncell, nqp * 4)[c])
    incs = pe.increments(n, 250.0, 70e3, seed=44, zz=False)
    ep, p = np.zeros((n, 4)), np.zeros(n)
    for e in incs:
        now["eps"] = e
        for q in maps:
            q.update()
        full, l, r = (q.fluxes["Stress"].x.array for q in maps)
        assert full.shape == (n * 4,) and not (l * r).any() and np.array_equal(full, l + r)
        jf, jl, jr = (q.jacobian_flatten.x.array for q in maps)
        assert jf.shape == (n * 16,) and not (jl * jr).any() and np.array_equal(jf, jl + jr)
        ref = pe.update(27, e, ep, p, mfront_like_material().behavior.params())
        assert np.array_equal(full.reshape(n, 4), ref["stress"]) and np.array_equal(jf.reshape(n, 16), ref["tangent"])
        for q in maps:
            q.advance()
        e4 = [q.internal_state_variables["epsp"].x.array.reshape(n, 4) for q in maps]
        assert np.array_equal(e4[0], ref["epsp"]) and np.array_equal(e4[0], e4[1] + e4[2])
        ep, p = ref["epsp"], ref["p"]
    assert (p > 0).any()
    for q in maps:
        q.close()


def test_update_initial_state_lays_a_4_wide_stress_out_point_after_point(fake):
    """``test_initialization.py:100-110``: one cell, four points, ``np.tile(s0, 4)``"""
    q = QuadratureFieldMap(1, 4, mfront_like_material())
    s0 = np.array([1.0, 2.0, 3.0, 4.0])
    q.update_initial_state("Stress", s0)
    assert np.array_equal(q.fluxes["Stress"].x.array, np.tile(s0, 4))
    q.update_initial_state("Stress", 2 * s0)
    assert np.array_equal(q.fluxes["Stress"].x.array, np.tile(2 * s0, 4))
    assert np.array_equal(np.asarray(q.material.get_initial_state_dict()["Stress"]), np.tile(2 * s0, (4, 1)))
    q.update_initial_state("p", 3e-3)
    assert np.array_equal(q.internal_state_variables["p"].x.array, np.full(4, 3e-3))
    q.close()


@pytest.mark.skipif(not reference_available(), reason="needs the reference tree (build container only)")
def test_the_references_own_quadrature_map_class_with_a_4_wide_material(fake):
    """the class a dolfinx user gets, ``accelerate(QuadratureMap)`` over the reference's code and the dolfinx doubles: the same
    two checks, with the 16-wide ``jacobian_flatten`` the reference's constructor builds"""
    from dolfinx_materials_amd.quadrature_map import accelerate
    from oracle import dolfinx_doubles as dd

    ncell, nqp = 4, 4
    n = ncell * nqp
    with dd.installed(REFERENCE_ROOT) as qm:
        Q = accelerate(qm.QuadratureMap)
        now = {}
        maps = []
        for cells in (None, np.array([0, 2], dtype=np.int32), np.array([1, 3], dtype=np.int32)):
            q = Q(dd.Mesh(ncell, "quadrilateral", 2), 2, mfront_like_material(), cells=cells)
            q.register_gradient("Strain", dd.PointwiseExpression(lambda c: now["eps"].reshape(ncell, nqp * 4)[c], 4))
            maps.append(q)
        assert maps[0].jacobian_flatten.x.array.shape == (n * 16,)
        for e in pe.increments(n, 250.0, 70e3, seed=44, zz=False):
            now["eps"] = e
            for q in maps:
                q.update()
            full, l, r = (q.fluxes["Stress"].x.array for q in maps)
            assert full.shape == (n * 4,) and full.any() and not (l * r).any() and np.array_equal(full, l + r)
            for q in maps:
                q.advance()
        s0 = np.array([1.0, 2.0, 3.0, 4.0])
        maps[0].update_initial_state("Stress", s0)
        assert np.array_equal(maps[0].fluxes["Stress"].x.array, np.tile(s0, n))
        for q in maps:
            q.close()
