"""CPU: logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_J2) -- the numpy restatement ``log_strain_ref.update`` (what the
kernel evaluates) against the eigen-free mpmath vectors of ``tests/golden/log_strain_degenerate.npz``, its second divided
difference of the logarithm against mpmath on its own, its tangent against central differences of its own stress, facts that
bypass all of these (major symmetry, objectivity), the seeded inputs of the GPU suite against the project's kink and share rules,
and the Python layer over a test double of the library.

Error floor.  ``E0`` is the largest scaled error (``log_strain_ref.scaled_errors``) of the restatement against the golden over the
degenerate set from both states: measured 1.08e-13 (PK1 of the stretch-1.2 points; tangent 4.6e-14, state 5.4e-14); ``E0`` is that
figure rounded up.  The GPU suite's bound rests on it: ``BOUND = min(16 E0, 1e-11)``, as ``test_gpu_ogden.py`` sets its own."""
import ctypes as C
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib

import log_strain_ref as ls
import tile_loop_cases as tc

E0 = 2e-13   # see the module docstring; asserted by test_error_floor
BOUND = min(16 * E0, 1e-11)
GAMMA_E0 = 2e-14   # ls.gamma against mpmath: 1.1e-14 measured over spreads 1e-9 .. 1 (6.7e-16 on the Taylor branch), rounded up
PARITY_SIZES = (1, 63, 64, 65, 1000)
CU = 256           # the tile-loop case of the GPU suite, at the size of a 256-CU device
EYE9 = np.array([[1.0, 1, 1, 0, 0, 0, 0, 0, 0]])


def floor_figures():
    F, labels, sets = ls.load_golden()
    return {name: ls.scaled_errors(ls.update(F, Ep, p), g) for name, Ep, p, g in sets}


def test_error_floor():
    figs = floor_figures()
    worst = max(max(v.values()) for v in figs.values())
    print(f"log-strain error floor E0 = {worst:.3e}: {figs}")
    assert worst <= E0, figs


def test_golden_is_the_generators_set_with_both_branches():
    F, labels, sets = ls.load_golden()
    F2, labels2 = ls.degenerate_F()
    assert np.array_equal(F, F2) and labels == labels2 and len(labels) == 10
    n = len(F)
    for (name, Ep, p, g), st in zip(sets, (ls.natural_state(n), ls.history_state(n))):
        assert np.array_equal(Ep, st[0]) and np.array_equal(p, st[1])
        r = ls.update(F, Ep, p)
        assert np.array_equal(r["plastic"], g["plastic"].astype(bool)) and not r["skip"].any(), name
        assert np.isfinite(r["A"]).all()
    nat = sets[0][3]["plastic"].astype(bool)
    assert nat.any() and (~nat).any() and sets[1][3]["plastic"].all()
    # both forms of the second divided difference occur: pair gaps on either side of the switch
    c = ls.hencky(F)[1]
    d = np.abs(c - c.mean(axis=1, keepdims=True)).max(axis=1) / c.mean(axis=1)
    assert (d <= ls.GAMMA_SWITCH).sum() >= 4 and (d > ls.GAMMA_SWITCH).sum() >= 2


def test_second_divided_difference_against_mpmath():
    import mpmath as mp

    rng = np.random.default_rng(5)
    n = 4000
    base = np.exp(rng.uniform(-0.7, 0.7, n))
    spread = 10.0 ** rng.uniform(-9, 0, n)
    c = base[:, None] * (1.0 + spread[:, None] * rng.uniform(-0.5, 0.5, (n, 3)))
    c[::7, 1] = c[::7, 0]                    # exact pairs
    c[::11, 2] = c[::11, 1]                  # with the line above: exact triples at multiples of 77
    c[::13] = c[::13][:, [2, 0, 1]]          # and in any position
    got = ls.gamma(c[:, 0], c[:, 1], c[:, 2])
    want = np.empty(n)
    with mp.workdps(60):
        for k in range(n):
            x = sorted(mp.mpf(float(v)) for v in c[k])

            def dd1(a, b):
                return 1 / a if a == b else (mp.log(a) - mp.log(b)) / (a - b)

            if x[0] == x[2]:
                want[k] = float(-1 / (2 * x[0] ** 2))
            elif x[0] == x[1]:
                want[k] = float((dd1(x[1], x[2]) - 1 / x[0]) / (x[2] - x[0]))
            elif x[1] == x[2]:
                want[k] = float((1 / x[2] - dd1(x[0], x[1])) / (x[2] - x[0]))
            else:
                want[k] = float((dd1(x[2], x[1]) - dd1(x[1], x[0])) / (x[2] - x[0]))
    err = np.abs(got - want) / np.abs(want)
    small = np.abs(c / c.mean(axis=1, keepdims=True) - 1.0).max(axis=1) <= ls.GAMMA_SWITCH
    print(f"gamma vs mpmath: worst {err.max():.3e} (Taylor form on {small.sum()} triples: {err[small].max():.3e}, quotient on {(~small).sum()}: "
          f"{err[~small].max():.3e})")
    assert small.sum() > 1000 and (~small).sum() > 300
    assert err.max() <= GAMMA_E0
    # symmetric in its three arguments
    for perm in ([1, 0, 2], [2, 1, 0], [1, 2, 0]):
        other = ls.gamma(*c[:, perm].T)
        assert np.abs(other - got).max() <= GAMMA_E0 * np.abs(got).max()


def _central_differences(F, Ep, p, h):
    A = np.empty((len(F), 9, 9))
    for col in range(9):
        d = np.zeros(9)
        d[col] = h
        A[:, :, col] = (ls.update(F + d, Ep, p)["P"] - ls.update(F - d, Ep, p)["P"]) / (2 * h)
    return A


@pytest.mark.parametrize("state", ["natural", "history"])
@pytest.mark.parametrize("amp,branch", [(0.2, "plastic"), (5e-4, "elastic")])
def test_tangent_matches_central_differences_of_the_stress(state, amp, branch):
    """h = 1e-6: the difference floor is 1e-10 to 2.5e-9 of the point's largest tangent entry (rounding 1e-16 |PK1| / h against
    |A| ~ E, truncation h^2 |A'''| / 6).  At stretches of order ``amp`` = 0.2 every point yields; the elastic branch is taken at
    amp = 5e-4 from the natural state and, with the history (a plastic strain of 2e-3), at F = exp(Ep_n) (I + amp U) around it."""
    N = 300
    Ep, p = ls.natural_state(N) if state == "natural" else ls.history_state(N, seed=3)
    F = ls.random_F(N, seed=21, amp=amp)
    if branch == "elastic" and state == "history":
        from oracle import constitutive_np as onp

        T = onp.mandel_to_tensor(Ep)
        expEp = np.eye(3)[None] + T + 0.5 * T @ T + T @ T @ T / 6.0
        F = ls.to_vector(expEp @ ls.to_matrix(F))
    r = ls.update(F, Ep, p)
    assert r["plastic"].all() if branch == "plastic" else not r["plastic"].any()
    A = _central_differences(F, Ep, p, 1e-6)
    err = np.abs(A - r["A"]).max(axis=(1, 2)) / np.abs(r["A"]).max(axis=(1, 2))
    print(f"tangent vs central differences ({state}, {branch}): {err.max():.3e}")
    assert err.max() <= 2.5e-9


def test_major_symmetry_in_the_elastic_branch():
    N = 500
    # small strains from the natural state; stretches of 0.3 around a non-coaxial history under a yield stress nothing reaches
    for r in (ls.update(ls.random_F(N, seed=4, amp=5e-4), *ls.natural_state(N)),
              ls.update(ls.random_F(N, seed=4, amp=0.3), *ls.history_state(N, seed=2), s0=1e12)):
        assert not r["plastic"].any()
        A = r["A"]
        asym = np.abs(A - A.transpose(0, 2, 1)).max(axis=(1, 2)) / np.abs(A).max(axis=(1, 2))
        assert asym.max() <= 1e-14, asym.max()


def test_objectivity():
    N = 64
    F1, F2 = ls.two_increments(N, seed=8)
    Q = ls._rotation([0.3, -1.0, 0.5], 1.1)
    a = ls.reference_path([F1, F2])
    b = ls.reference_path([ls.to_vector(Q @ ls.to_matrix(F1)), ls.to_vector(Q @ ls.to_matrix(F2))])
    for ra, rb in zip(a, b):
        want = ls.to_vector(Q @ ls.to_matrix(ra["P"]))
        got = dict(rb, P=ls.to_vector(Q.T @ ls.to_matrix(rb["P"])), A=ra["A"])     # the state is a function of C = F^T F alone
        e = ls.scaled_errors(got, ra)
        assert np.abs(rb["P"] - want).max() <= 1e-12 * max(np.abs(want).max(), ls.PRM["s0"])
        assert max(e["P"], e["eel"], e["Ep"], e["p"]) <= 1e-12, e
        assert np.array_equal(ra["plastic"], rb["plastic"])


def test_identity_is_stress_free_with_the_isotropic_elastic_tangent():
    r = ls.update(EYE9, *ls.natural_state(1))
    assert not r["P"].any() and not r["eel"].any() and not r["Ep"].any() and r["p"][0] == 0.0 and not r["plastic"][0]
    E, nu = ls.PRM["E"], ls.PRM["nu"]
    lam, mu = E * nu / (1 + nu) / (1 - 2 * nu), E / 2 / (1 + nu)
    want = np.zeros((9, 9))
    for row in range(9):
        i, J = int(ls.TI[row]), int(ls.TJ[row])
        for col in range(9):
            k, L = int(ls.TI[col]), int(ls.TJ[col])
            want[row, col] = lam * float(i == J and k == L) + mu * (float(i == k and J == L) + float(i == L and J == k))
    assert np.abs(r["A"][0] - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()


def test_inverted_and_non_finite_points_give_nan():
    F9 = np.array([[1.0, 1, -1, 0, 0, 0, 0, 0, 0], [1.0, 1, 0, 0, 0, 0, 0, 0, 0], [np.nan, 1, 1, 0, 0, 0, 0, 0, 0]])
    r = ls.update(F9, *ls.natural_state(3))
    for k in ("P", "A", "eel", "Ep", "p"):
        assert np.isnan(r[k]).all(), k
    assert not r["plastic"].any()


# ---- the seeded inputs of the GPU suite: the kink cap and the plastic share, by the reference alone ------------------------------
def _within_rules(r, what, share=True):
    kink = float(np.mean(r["skip"]))
    assert kink <= ls.KINK_CAP, (what, kink)
    if share:
        s = float(np.mean(r["plastic"]))
        assert ls.SHARE[0] <= s <= ls.SHARE[1], (what, s)
    return kink


@pytest.mark.parametrize("N,seed", [(N, N) for N in PARITY_SIZES] + [(257, 12), (100_003, 4), (41 * 4, 31), (3001 * 8, 31)])
def test_parity_inputs_stay_within_the_kink_cap_and_the_share(N, seed):
    """Every seeded pair of increments of test_gpu_log_strain.py: parity, protocol, routes, field maps."""
    for k, r in enumerate(ls.reference_path(ls.two_increments(N, seed=seed))):
        # the spliced-in special rows are no random batch: the share is that of the rows behind them
        _within_rules(r, (N, k), share=False)
        if N >= 1000:
            rest = {q: v[11:] for q, v in r.items()}
            _within_rules(rest, (N, k))


def test_tile_loop_inputs_stay_within_the_kink_cap_and_the_share_in_every_pass():
    N = tc.size_for(CU)
    F1, F2 = ls.two_increments(N, seed=77)
    Ep, p = ls.natural_state(N)
    for k, F in enumerate((F1, F2)):
        r = ls.branch(F, Ep, p)
        assert np.mean(r["skip"]) <= ls.KINK_CAP
        shares = tc.share_per_pass(r["plastic"], CU)
        print(f"log-strain tile loop, increment {k}: plastic share per pass {[round(s, 3) for s in shares]}")
        assert len(shares) == 4 and all(ls.SHARE[0] <= s <= ls.SHARE[1] for s in shares), shares
        Ep, p = r["Ep"], r["p"]
    # the cheap branch function is the update's
    idx = tc.reference_sample(N, CU)[::50]
    full = ls.reference_path([F1, F2], idx)[1]
    assert np.array_equal(full["plastic"], r["plastic"][idx]) and np.array_equal(full["Ep"], r["Ep"][idx])


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_behaviour_descriptor():
    b = jm.LogarithmicStrainPlasticity(250e6, 1e6)
    assert b.law == _lib.LAW_LOG_STRAIN_J2 == 19 and b.params() == [210e9, 0.3, 250e6, 1e6]
    assert isinstance(b, jm.FiniteStrainBehavior) and (b.gradient_name, b.flux_name) == ("DeformationGradient", "FirstPiolaKirchhoffStress")
    assert b.flat_properties() == {"E": 210e9, "nu": 0.3, "s0": 250e6, "H0": 1e6}
    assert jm.LogarithmicStrainPlasticity(s0=1.0, H0=0.0, E=10.0, nu=0.25).params() == [10.0, 0.25, 1.0, 0.0]
    d = jm.LogarithmicStrainPlasticity.from_mfront_properties({"YieldStrength": 250e6, "HardeningSlope": 1e6})   # the demo's call
    assert d.params() == b.params()
    assert jm.LogarithmicStrainPlasticity.from_mfront_properties({"YieldStress": 3.0, "HardeningSlope": 2.0}).params() == [210e9, 0.3, 3.0, 2.0]
    with pytest.raises(ValueError, match="unknown"):
        jm.LogarithmicStrainPlasticity.from_mfront_properties({"YieldStrength": 1.0, "HardeningSlope": 1.0, "YoungModulus": 1.0})
    for props in ({"YieldStrength": 1.0}, {"HardeningSlope": 1.0}, {}):
        with pytest.raises(ValueError, match="missing"):
            jm.LogarithmicStrainPlasticity.from_mfront_properties(props)
    for bad in (dict(s0=0.0, H0=1.0), dict(s0=1.0, H0=-1.0), dict(s0=1.0, H0=1.0, E=0.0), dict(s0=1.0, H0=1.0, nu=0.5),
                dict(s0=1.0, H0=1.0, nu=-1.0), dict(s0=float("nan"), H0=1.0), dict(s0=1.0, H0=float("inf"))):
        with pytest.raises(ValueError, match="logarithmic-strain plasticity"):
            jm.LogarithmicStrainPlasticity(**bad)


def test_law_table_row():
    i = _lib.law_info(_lib.LAW_LOG_STRAIN_J2)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (9, 9, 4, 2, 7, 952)
    assert [i.isv_name[f] for f in range(2)] == [b"ElasticStrain", b"EquivalentPlasticStrain"] and [i.isv_dim[f] for f in range(2)] == [6, 1]
    assert 72 + 72 + 648 + 56 + 104 == 952
    b = _lib.law_blocks(_lib.LAW_LOG_STRAIN_J2)
    assert (b.n_external, b.n_blocks, b.tangent_width) == (0, 1, 81)
    for law in (18, 20):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
    assert _lib.load().dxm_abi_version() == 6


def test_create_without_a_gpu_fails_loudly_for_the_new_law_too():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    prm = (C.c_double * 4)(210e9, 0.3, 250e6, 1e6)
    assert not lib.dxm_create(_lib.LAW_LOG_STRAIN_J2, prm, 4, 8, 0)
    assert b"no usable HIP device" in lib.dxm_last_error()


@pytest.fixture
def fake(monkeypatch):
    from fake_dxmat_log_strain import FakeDxmatLogStrain

    f = FakeDxmatLogStrain(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: f)
    return f


def test_material_over_the_test_double(fake):
    from dolfinx_materials_amd.conventions import hencky_strain
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    n = 37
    m = JAXMaterial(jm.LogarithmicStrainPlasticity(**{k: ls.PRM[k] for k in ("s0", "H0")}), lazy_isv=False)
    assert m.gradients == {"DeformationGradient": 9} and m.fluxes == {"FirstPiolaKirchhoffStress": 9}
    assert m.internal_state_variables == {"ElasticStrain": 6, "EquivalentPlasticStrain": 1}
    assert m.tangent_blocks == {("FirstPiolaKirchhoffStress", "DeformationGradient"): (9, 9)} and m.tangent_size == 81
    assert m.algorithmic_bytes_per_point == 952 and m.name == "LogarithmicStrainPlasticity" and m.rotation_matrix is None
    m.set_data_manager(n)
    s0 = m.get_initial_state_dict()
    assert np.array_equal(s0["DeformationGradient"], np.tile(EYE9, (n, 1))) and not s0["ElasticStrain"].any() and not s0["EquivalentPlasticStrain"].any()
    # protocol order: k updates from one initial state, the last one counts; advance; the next starts from what it left
    F1, F2 = ls.two_increments(n, seed=5)
    ref = ls.reference_path([F1, F2])
    for F in (F2, F1):
        P, isv, A = m.integrate(F)
    assert np.array_equal(np.array(P), ref[0]["P"]) and np.array_equal(np.array(A).reshape(n, 9, 9), ref[0]["A"])
    assert np.array_equal(np.array(isv)[:, :6], ref[0]["eel"]) and np.array_equal(np.array(isv)[:, 6], ref[0]["p"])
    assert A.shape == (n, 9, 9) and m.last_stats["n_plastic"] == int(ref[0]["plastic"].sum())
    assert set(m.get_final_state_dict()) == {"DeformationGradient", "FirstPiolaKirchhoffStress", "ElasticStrain", "EquivalentPlasticStrain"}
    assert not np.array(m.get_initial_state_dict()["ElasticStrain"]).any()
    m.data_manager.update()
    assert np.array_equal(np.array(m.get_initial_state_dict()["ElasticStrain"]), ref[0]["eel"])
    P2, isv2, A2 = m.integrate(F2)
    assert np.array_equal(np.array(P2), ref[1]["P"]) and np.array_equal(np.array(A2).reshape(n, 9, 9), ref[1]["A"])
    assert np.array_equal(np.array(isv2)[:, 6], ref[1]["p"])
    m.data_manager.revert()
    assert np.array_equal(np.array(m.get_final_state_dict()["EquivalentPlasticStrain"])[:, 0], ref[0]["p"])
    # the hidden field is rebuilt when the state is set: Ep = hencky(F) - ElasticStrain, from whichever of the two is given
    h = m._parts[0][0]
    hidden = lambda: fake._h(h).state[0]["PlasticStrain"]   # noqa: E731
    assert np.array_equal(hidden(), ref[0]["Ep"])
    fake.state_sets.clear()
    m.set_initial_state_dict({"DeformationGradient": F1, "ElasticStrain": ref[0]["eel"], "EquivalentPlasticStrain": ref[0]["p"]})
    assert (_lib.S0, 2) in fake.state_sets
    assert np.abs(hidden() - ref[0]["Ep"]).max() <= 1e-15 and np.array_equal(hidden(), hencky_strain(F1) - ref[0]["eel"])
    m.set_initial_state_dict({"ElasticStrain": 0.5 * ref[0]["eel"]})               # F_n stays
    assert np.array_equal(hidden(), hencky_strain(F1) - 0.5 * ref[0]["eel"])
    m.set_initial_state_dict({"DeformationGradient": F2})                            # ElasticStrain_n stays
    assert np.array_equal(hidden(), hencky_strain(F2) - 0.5 * ref[0]["eel"])
    fake.state_sets.clear()
    m.set_initial_state_dict({"EquivalentPlasticStrain": ref[0]["p"]})               # neither: the hidden field stays
    assert fake.state_sets == [(_lib.S0, 1)]
    # explicit state in, explicit state out: the update of the second increment from the first one's state
    Ct, new = m.batched_constitutive_update(F2, {"DeformationGradient": F1, "ElasticStrain": ref[0]["eel"], "EquivalentPlasticStrain": ref[0]["p"]})
    got = dict(P=new["FirstPiolaKirchhoffStress"], A=np.asarray(Ct), eel=new["ElasticStrain"], p=new["EquivalentPlasticStrain"][:, 0], Ep=ref[1]["Ep"])
    assert max(ls.scaled_errors(got, ref[1]).values()) <= 1e-12          # (Ep_n went through hencky(F1) - eel: rounding, no more)
    # uniform property updates reach the handle; a refused value leaves descriptor and handle as they were
    m.update_material_property("s0", 300e6)
    assert fake.last_params == [210e9, 0.3, 300e6, 1e6] and m.material_properties["s0"] == 300e6
    with pytest.raises(_lib.DxmError, match="s0 must be"):
        m.update_material_property("s0", -1.0)
    assert m.behavior.s0 == 300e6 and m.material_properties["s0"] == 300e6
    with pytest.raises(ValueError, match="Unknown material property"):
        m.update_material_property("sig0", 1.0)
    with pytest.raises(NotImplementedError, match="varies from point to point"):
        m.update_material_property("H0", np.linspace(1.0, 2.0, n))
    m.close()


def test_hencky_strain_of_the_python_layer():
    from dolfinx_materials_amd.conventions import hencky_strain

    F = ls.spliced(40, seed=3, amp=0.3)
    assert np.abs(hencky_strain(F) - ls.hencky(F)[0]).max() <= 1e-15
    bad = np.array([[0.0] * 9, [1.0, 1, -1, 0, 0, 0, 0, 0, 0], [np.nan] * 9])
    assert not hencky_strain(bad).any()      # no deformation gradient: counts as F = I


def test_refusals(fake):
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    b = jm.LogarithmicStrainPlasticity(250e6, 1e6)
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            JAXMaterial(b, tangent_layout=layout)
    m = JAXMaterial(b, property_fields=True)
    m.set_data_manager(4)
    with pytest.raises(NotImplementedError, match="logarithmic-strain plasticity"):
        m.update_material_property("s0", np.array([1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(AttributeError, match="isotropic"):
        m.rotation_matrix = np.eye(3)
    # the C ABI's own words for the two things the kernel does not do
    assert fake.dxm_set_tangent_layout(m._parts[0][0], 1) < 0 and b"no packed tangent record" in fake.dxm_last_error()
    assert fake.dxm_integrate_displacement(m._parts[0][0], None, None, 0.0, None, None, None, None) < 0
    assert b"no fused displacement-gradient form" in fake.dxm_last_error()
    m.close()


def test_refusal_texts_of_the_library_row():
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "dxmat.hip")).read()
    row = src[src.index("constexpr LawDesc law_log_strain_j2()"):]
    row = row[:row.index("\n}\n")]
    for field in ("set_refusal", "launch_refusal", "no_fused", "no_frame", "no_fields", "stock_only"):
        assert f"d.{field} = " in row, field
    assert "d.set_layouts = d.launch_layouts = L_FULL;" in row and "d.alg_bytes = 952;" in row and "LS_BLOCKS_PER_CU" in row
