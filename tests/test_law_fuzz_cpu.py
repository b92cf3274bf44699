"""CPU: what keeps ``test_gpu_fuzz_laws.py`` honest.  Over the parameter ranges and inputs of ``law_fuzz.py`` -- for every seed the GPU
sweep runs -- each law's float64 restatement converges at every point, the share of points the sweep may skip stays under its cap,
and the restatement agrees with its high-precision version on a sample of ``law_fuzz.MP_SAMPLE`` points per seed:
``hosford_ref.update_mp`` (50 digits), ``ogden_ref.closed_form_mp`` (60 digits), and for Ramberg-Osgood the scalar equation re-solved
in mpmath (``law_fuzz.ramberg_osgood_mp``).  The GPU bounds are stored in ``tests/golden/law_fuzz_bounds.npz``
(``golden/make_law_fuzz_bounds.py``): 8 x the largest such deviation, never less than the bound of the law's fixed-parameter tests.
The deviations are re-derived here and must still be covered.

Final ranges: those of ``law_fuzz.py``'s docstring, none narrowed -- the largest deviations measured are 8e-15 / 1.2e-14 (Hosford
state / tangent), 3.3e-14 (Ogden, against a bound of 3.2e-12) and 1.1e-15 / 6e-16 (Ramberg-Osgood stress / tangent, against 1e-12 and
1e-11), so every existing bound holds over the whole range with more than an order of magnitude to spare and all five GPU bounds are
the existing ones.  Hosford exponents strictly between 2 and 3 are not drawn; the last test says why."""
import os

import numpy as np
import pytest

import hosford_ref as hr
import law_fuzz as lf
import ogden_ref as og
import ramberg_osgood_ref as ro

BOUNDS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "law_fuzz_bounds.npz"))
N = lf.N_POINTS


def test_the_stored_bounds_are_8_x_the_stored_deviations_floored_at_the_existing_bounds():
    from test_ogden_cpu import E0

    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hosford_degenerate.npz"))
    floors = dict(hosford_state=float(gold["bound_state"]), hosford_tangent=float(gold["bound_tangent"]), ogden=min(16 * E0, 1e-11),
                  ro_stress=1e-12, ro_tangent=1e-11)      # test_gpu_ogden.BOUND; test_gpu_ramberg_osgood.check_against_ref
    seeds = dict(hosford_state=lf.HOSFORD_SEEDS, hosford_tangent=lf.HOSFORD_SEEDS, ogden=lf.OGDEN_SEEDS, ro_stress=lf.RO_SEEDS, ro_tangent=lf.RO_SEEDS)
    for k, floor in floors.items():
        assert float(BOUNDS[f"floor_{k}"]) == floor, k
        assert len(BOUNDS[f"dev_{k}"]) == len(seeds[k]), k
        assert float(BOUNDS[f"bound_{k}"]) == max(8 * BOUNDS[f"dev_{k}"].max(), floor), k
        assert BOUNDS[f"dev_{k}"].max() < 1e-9, k          # far from a conditioning defect


def test_the_draws_cover_the_ranges():
    hos = [lf.draw_hosford(s) for s in lf.HOSFORD_SEEDS]
    assert {p[4] for p in hos} == set(lf.HOSFORD_EXPONENTS) and not any(2.0 < p[4] < 3.0 for p in hos)
    assert [p[3] == 0.0 for p in hos] == [s % 3 == 0 for s in lf.HOSFORD_SEEDS]
    assert min(p[1] for p in hos) == 0.0 and max(p[1] for p in hos) == 0.49
    assert all(1e3 <= p[0] <= 10 ** 5.5 and 1e-4 <= p[2] / p[0] <= 1e-2 and 0.0 <= p[3] <= 0.5 * p[0] for p in hos)
    assert max(p[3] / p[0] for p in hos) > 0.25               # H ~ E is drawn, not only allowed
    ogd = [lf.draw_ogden(s) for s in lf.OGDEN_SEEDS]
    assert all(1.0 <= abs(p["alpha"]) <= 30.0 and 1e2 <= p["mu"] <= 1e5 and 10 ** 0.5 <= p["K"] / p["mu"] <= 10 ** 3.5 for p in ogd)
    assert min(p["alpha"] for p in ogd) < -10.0 and max(p["alpha"] for p in ogd) > 10.0 and min(abs(p["alpha"]) for p in ogd) < 2.0
    assert max(lf.OGDEN_AMPS) == 2.0
    rmo = [lf.draw_ramberg_osgood(s) for s in lf.RO_SEEDS]
    assert {p[4] for p in rmo} == set(lf.RO_EXPONENTS)
    assert all(1e3 <= p[0] <= 10 ** 5.5 and 0.0 <= p[1] <= 0.49 and 1e-4 <= p[2] / p[0] <= 1e-2 and 1e-2 <= p[3] <= 10.0 for p in rmo)
    assert min(p[1] for p in rmo) == 0.0 and max(p[1] for p in rmo) == 0.49


def test_the_strain_family_at_scale_1_is_the_one_the_fixed_parameter_tests_always_ran():
    eps = lf.ramberg_osgood_strains(600, seed=2)
    assert np.array_equal(eps, lf.ramberg_osgood_strains(600, seed=2, scale=1.0))
    big = lf.ramberg_osgood_strains(600, seed=2, scale=2.0)
    near = (big == eps).all(axis=1) & eps.any(axis=1)          # the rows at the absolute threshold e_eps are not scaled
    assert near.any() and (np.sqrt(2.0 / 3.0) * np.linalg.norm(eps[near], axis=1) < 2.1e-12).all()
    assert np.array_equal(big[~near], 2.0 * eps[~near])


@pytest.mark.parametrize("seed", lf.HOSFORD_SEEDS)
def test_hosford_reference_over_the_history(seed):
    prm = lf.draw_hosford(seed)
    E, nu, R0, H, a = prm
    hist = lf.hosford_history(seed, N, prm)
    assert len(hist["ref"]) == lf.HOSFORD_INCREMENTS == 4
    for inc, r in enumerate(hist["ref"]):
        assert r["converged"].all() and r["iters"].max() <= 8, (prm, inc, int(r["iters"].max()))
        assert np.isfinite(r["Ct"]).all() and np.isfinite(r["sig"]).all(), (prm, inc)
        assert hist["skip"][inc].mean() <= lf.KINK_CAP, (prm, inc, int(hist["skip"][inc].sum()))
        assert hist["overshoot"][inc] <= hr.max_overshoot(a) * (1 + 1e-9), (prm, inc)
        assert r["plastic"].sum() >= N // 10, (prm, inc)                      # every increment yields somewhere
    r1, r2 = hist["ref"][0], hist["ref"][1]
    unloaded = r1["plastic"] & ~r2["plastic"]
    assert unloaded.sum() > 0.2 * r1["plastic"].sum(), prm                    # increment 2 unloads into the elastic domain ...
    s1, s2 = r1["sig"][:, :3] - r1["sig"][:, :3].mean(axis=1, keepdims=True), r2["sig"][:, :3] - r2["sig"][:, :3].mean(axis=1, keepdims=True)
    reyield = r1["plastic"] & r2["plastic"] & ((s1 * s2).sum(axis=1) + (r1["sig"][:, 3:] * r2["sig"][:, 3:]).sum(axis=1) < 0)
    assert reyield.sum() > 0.05 * r1["plastic"].sum(), prm                    # ... and re-yields on the other side
    assert (hist["ref"][3]["p"] > hist["ref"][0]["p"]).sum() > N // 10, prm   # plastic flow after the first increment
    ds, dc = lf.hosford_deviation(seed)
    print(f"hosford seed {seed} {prm}: restatement against 50 digits: state {ds:.2e} tangent {dc:.2e}")
    assert 8 * ds <= float(BOUNDS["bound_hosford_state"]) and 8 * dc <= float(BOUNDS["bound_hosford_tangent"]), (prm, ds, dc)


@pytest.mark.parametrize("seed", lf.OGDEN_SEEDS)
def test_ogden_reference_over_the_stretches(seed):
    prm = lf.draw_ogden(seed)
    amp = lf.OGDEN_AMPS[seed % len(lf.OGDEN_AMPS)]
    F = lf.ogden_F(seed, N, amp)
    Fm = og.to_matrix(F)
    assert (np.linalg.det(Fm) > 0.0).all()
    lam = np.sqrt(np.linalg.eigvalsh(np.einsum("nki,nkj->nij", Fm, Fm)))
    assert lam.min() >= 1 / amp * (1 - 1e-6) and lam.max() <= amp * (1 + 1e-6) and lam.max() > 0.9 * amp, (amp, lam.min(), lam.max())
    assert (np.abs(Fm - Fm.transpose(0, 2, 1)).max(axis=(1, 2)) > 0.05).mean() > 0.5                 # rotated, not symmetric stretches
    P, A, isv = og.closed_form(F, **prm)
    assert np.isfinite(P).all() and np.isfinite(A).all() and np.isfinite(isv).all(), prm
    series, quotient = lf.ogden_paths(F, prm["alpha"])
    assert series.mean() >= 0.05 and quotient.mean() >= 0.05, (prm, series.mean(), quotient.mean())
    dev = lf.ogden_deviation(seed)
    print(f"ogden seed {seed} {prm} amp {amp}: closed form against 60 digits {dev:.2e}")
    assert 8 * dev <= float(BOUNDS["bound_ogden"]), (prm, dev)


@pytest.mark.parametrize("seed", lf.RO_SEEDS)
def test_ramberg_osgood_reference_over_the_parameters(seed):
    prm, eps = lf.ramberg_osgood_inputs(seed, N)
    r = ro.update(eps, *prm)
    assert r["converged"].all() and r["iters"].max() <= 10, (prm, int(r["iters"].max()))
    assert np.isfinite(r["sig"]).all() and np.isfinite(r["Ct_mfront"]).all(), prm
    assert 0.3 * N < r["newton"].sum() < 0.7 * N, prm
    knee = r["sig_e"] / prm[2]
    assert (knee[r["newton"]] < 0.1).any() and (knee > 1.0).any(), prm                           # both ends of the curve
    ds, dc = lf.ramberg_osgood_deviation(seed)
    print(f"ramberg-osgood seed {seed} {prm}: restatement against 50 digits: stress {ds:.2e} tangent {dc:.2e}")
    assert 8 * ds <= float(BOUNDS["bound_ro_stress"]) and 8 * dc <= float(BOUNDS["bound_ro_tangent"]), (prm, ds, dc)


def test_hosford_tangent_between_exponents_2_and_3():
    """Why the sweep draws no exponent strictly between 2 and 3.  There dn/dsigma carries |s_i - s_j|^(a-2): the tangent is bounded
    and continuous where two principal stresses coincide (uniaxial states), but only Hoelder continuous with exponent a - 2.  Measured
    at a = 2.5 against the derivative formulas evaluated at the 50-digit solution (``update_mp(tangent="analytic")``):

    * a generic point: restatement, analytic tangent and central differences of either step agree (1e-15);
    * exactly uniaxial: the RESTATEMENT is right (2e-16); the 50-digit central differences are off by O(h^(a-2)) -- 2.9e-11 with the
      relative step 1e-20, 2.9e-7 with 1e-12;
    * a relative eigenvalue gap of 1e-12 next to it: the DIFFERENCES (step 1e-20) are right; the float64 restatement is off by 7.5e-11,
      the rounding of the gap (1e-4 of it) times the tangent's slope 0.5 gap^(-1/2): no float64 evaluation can do better, so no 1e-12
      tangent bound can hold there, while the stress agrees to 4e-16.

    The same three points at a = 6 agree throughout."""
    P = hr.PROPS
    fig = {}
    for a in (2.5, 6.0):
        for cls in ("generic", "uniaxial", "uniaxial_near"):
            eps, ep, p = hr.make_inputs(cls, 1, a, seed=5)
            r = hr.update(eps, ep, p, **P, a=a)
            an = hr.update_mp(eps[0], ep[0], p[0], **P, a=a, tangent="analytic")
            sc = np.abs(an["Ct"]).max()
            fd = {h: hr.update_mp(eps[0], ep[0], p[0], **P, a=a, rel_step=h)["Ct"] for h in ((1e-20, 1e-12) if a == 2.5 else (1e-20,))}
            fig[a, cls] = dict(ref=np.abs(r["Ct"][0] - an["Ct"]).max() / sc, sig=np.abs(r["sig"][0] - an["sig"]).max() / P["R0"],
                               **{f"fd{h:g}": np.abs(c - an["Ct"]).max() / sc for h, c in fd.items()})
            assert r["plastic"][0] and fig[a, cls]["sig"] < 1e-14, (a, cls, fig[a, cls])
    print(fig)
    for cls in ("generic", "uniaxial", "uniaxial_near"):
        assert fig[6.0, cls]["ref"] < 1e-13 and fig[6.0, cls]["fd1e-20"] < 1e-13, fig[6.0, cls]
    g, u, n = fig[2.5, "generic"], fig[2.5, "uniaxial"], fig[2.5, "uniaxial_near"]
    assert g["ref"] < 1e-13 and g["fd1e-20"] < 1e-13 and g["fd1e-12"] < 1e-13, g
    assert u["ref"] < 1e-13 and 1e-12 < u["fd1e-20"] < 1e-9, u
    assert 0.3e4 < u["fd1e-12"] / u["fd1e-20"] < 3e4, u                  # (1e8)^(a-2): the error of the differences goes like h^(a-2)
    assert n["fd1e-20"] < 1e-13 and 1e-12 < n["ref"] < 1e-8, n           # at most eps^(a-2) = 1e-8
