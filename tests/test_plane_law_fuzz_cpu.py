"""CPU: what keeps ``test_gpu_fuzz_plane_laws.py`` honest.  Over the parameter draws of ``law_fuzz.py`` and the plane inputs of
``plane_law_fuzz.py`` -- for every seed the GPU sweep runs -- the definitions of the two plane-strain laws (``hosford_plane_ref.update``,
``ogden_plane_ref.restricted_closed_form``) converge and stay finite at every point, the inputs hold every branch of the two kernels
that the sweep is there to reach, and the definitions agree with their high-precision versions on ``law_fuzz.MP_SAMPLE`` points per seed.
The GPU bounds are stored in ``tests/golden/plane_law_fuzz_bounds.npz`` (``golden/make_plane_law_fuzz_bounds.py``): 8 x the largest such
deviation, never less than the bound of the law's fixed-parameter GPU tests.  The deviations are re-derived here.

Measured: 6.5e-15 / 1.6e-14 (Hosford state / tangent) and 7.0e-15 (Ogden), so all three bounds are the existing ones (1e-12, 1e-12,
3.2e-12).  The Hosford ranges are those of ``law_fuzz.py``, none narrowed; the Ogden rows are narrowed by the conditioning of the
pressure term, ``plane_law_fuzz.plane_ogden_F`` says how and why.

The branches of ``hosford_plane.hip`` and ``ogden_plane.hip`` asserted present (a kernel wrong in one of them meets rows here):

* the closed-form rotation at exactly 45 degrees (t_xx == t_yy to the bit, with shear): increment 2, the rows ``shear45``, every seed;
  at zero shear: increment 1, classes ``inplane_equal`` (d = 0: the guarded division), ``axis_aligned`` and every other row of
  ``zz_equal`` (d != 0), every seed;
* the one divided difference of law 40 in its series form (classes ``inplane_equal``, ``near``), its quotient form (``generic``) and its
  sum form for differences of opposite sign, on yielding rows of every seed; of law 38 in series and quotient form, every seed;
* H = 0 in ``mu2 * nz + H``: seeds 0, 3, 6, 9, with yielding rows in all four increments;
* the odd exponent a = 3 (seeds 1, 9) next to the even ones and a = 2, with differences of either sign under the signed powers;
* negative alpha: seeds 1, 3, 5, 7 of ``draw_ogden``."""
import os

import numpy as np
import pytest

import hosford_plane_ref as hp
import hosford_ref as hr
import ogden_plane_ref as op
import ogden_ref as og
import plane_law_fuzz as pf

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS = np.load(os.path.join(HERE, "golden", "plane_law_fuzz_bounds.npz"))
N = pf.N_POINTS
PLASTIC_CLASS = dict(generic=True, elastic=False, below=False, above=True, inplane_equal=True, zz_equal=True, near=True, axis_aligned=True,
                     volumetric=False, zero=False)


def test_the_stored_bounds_are_8_x_the_stored_deviations_floored_at_the_existing_bounds():
    from test_ogden_cpu import E0

    assert pf.OGDEN_E0 == E0 and pf.OGDEN_CONDITION_CAP == E0 / (4 * np.finfo(float).eps)
    gold = np.load(os.path.join(HERE, "golden", "hosford_plane.npz"))
    floors = dict(hosford_state=float(gold["bound_state"]), hosford_tangent=float(gold["bound_tangent"]), ogden=min(16 * E0, 1e-11))   # test_gpu_ogden.BOUND
    seeds = dict(hosford_state=pf.HOSFORD_SEEDS, hosford_tangent=pf.HOSFORD_SEEDS, ogden=pf.OGDEN_SEEDS)
    assert sorted(BOUNDS.files) == sorted(f"{w}_{k}" for w in ("dev", "floor", "bound") for k in floors)
    for k, floor in floors.items():
        assert float(BOUNDS[f"floor_{k}"]) == floor, k
        assert len(BOUNDS[f"dev_{k}"]) == len(seeds[k]), k
        assert float(BOUNDS[f"bound_{k}"]) == max(8 * BOUNDS[f"dev_{k}"].max(), floor), k
        assert BOUNDS[f"dev_{k}"].max() < 1e-9, k          # far from a conditioning defect
    for s in (pf.HOSFORD_SEEDS[1], pf.HOSFORD_SEEDS[-1]):
        assert pf.plane_hosford_deviation(s) == (float(BOUNDS["dev_hosford_state"][s]), float(BOUNDS["dev_hosford_tangent"][s])), s
    for s in (pf.OGDEN_SEEDS[0], pf.OGDEN_SEEDS[-1]):
        assert pf.plane_ogden_deviation(s) == float(BOUNDS["dev_ogden"][s]), s


def test_the_draws_cover_the_ranges():
    hos = [pf.draw_hosford(s) for s in pf.HOSFORD_SEEDS]
    assert {p[4] for p in hos} == {2.0, 3.0, 4.0, 6.0, 8.0, 10.0, 14.0, 20.0}                   # a = 3, 8 and 14 among them
    assert [s for s in pf.HOSFORD_SEEDS if hos[s][4] % 2.0 == 1.0] == [1, 9]                    # the odd exponent
    assert [s for s in pf.HOSFORD_SEEDS if hos[s][3] == 0.0] == [0, 3, 6, 9]                    # H = 0
    assert max(p[3] / p[0] for p in hos) > 0.25 and hos[5][4] == 10.0 and hos[5][3] / hos[5][0] > 0.25    # H ~ E, at a = 10
    assert min(p[1] for p in hos) == 0.0 and max(p[1] for p in hos) == 0.49
    assert min(p[2] / p[0] for p in hos) < 1e-3 and max(p[2] / p[0] for p in hos) > 5e-3      # R0 / E on either side of 2.9e-3
    ogd = [pf.draw_ogden(s) for s in pf.OGDEN_SEEDS]
    assert [s for s in pf.OGDEN_SEEDS if ogd[s]["alpha"] < 0.0] == [1, 3, 5, 7]
    for sign in (1.0, -1.0):
        mag = [abs(p["alpha"]) for p in ogd if p["alpha"] * sign > 0.0]
        assert min(mag) < 5.0 and max(mag) > 15.0, (sign, mag)
    assert min(abs(p["alpha"]) for p in ogd) < 1.5 and max(abs(p["alpha"]) for p in ogd) > 15.0
    ratio = [p["K"] / p["mu"] for p in ogd]
    assert max(ratio) / min(ratio) >= 100.0
    assert max(pf.OGDEN_AMPS) == 2.0 and {pf.plane_ogden_amp(s) for s in pf.OGDEN_SEEDS} == set(pf.OGDEN_AMPS)


def _deviator(v4):
    return v4 - v4[:, :3].mean(axis=1, keepdims=True) * np.array([1.0, 1.0, 1.0, 0.0])


@pytest.mark.parametrize("seed", pf.HOSFORD_SEEDS)
def test_plane_hosford_reference_over_the_history(seed):
    prm = pf.draw_hosford(seed)
    E, nu, R0, H, a = prm
    hist = pf.plane_hosford_history(seed, N, prm)
    assert len(hist["ref"]) == len(hist["eps"]) == pf.HOSFORD_INCREMENTS == 4
    assert hist["eps"][0].shape == (N, 4) and hist["ep0"].shape == (N, 4) and hist["p0"].shape == (N,)
    assert not any(x.flags.writeable for x in hist["eps"]) and not hist["ref"][0]["sig"].flags.writeable
    assert pf.plane_hosford_history(seed, N, list(prm)) is hist                                     # computed once
    for inc, r in enumerate(hist["ref"]):
        tag = (prm, inc)
        assert r["converged"].all() and r["dropped"] == 0.0 and r["iters"].max() <= 8, (tag, int(r["iters"].max()))
        assert np.isfinite(r["Ct"]).all() and np.isfinite(r["sig"]).all(), tag
        assert hist["skip"][inc].mean() <= pf.KINK_CAP and hist["skip"][inc].sum() == 0, (tag, int(hist["skip"][inc].sum()))
        assert hist["overshoot"][inc] <= hr.max_overshoot(a) * (1 + 1e-9), tag
        assert r["plastic"].mean() >= 0.1 and (~r["plastic"]).mean() >= 0.1, (tag, r["plastic"].mean())
        ser, quo, opp = pf.plane_hosford_paths(r["sig"], a)
        pl = r["plastic"]
        print(f"plane hosford seed {seed} increment {inc + 1}: plastic {pl.mean():.2f} overshoot {hist['overshoot'][inc]:.3f} of {hr.max_overshoot(a)} "
              f"divided difference on yielding rows: series {int((ser & pl).sum())} quotient {int((quo & pl).sum())} opposite signs {int((opp & pl).sum())}")
        assert not (ser & quo).any() and not (ser & opp).any() and not (quo & opp).any() and (ser | quo | opp)[pl].all(), tag
        assert (quo & pl).sum() >= 100 and (opp & pl).sum() >= 100, tag
        if inc < 2:
            assert (ser & pl).sum() >= 100, tag
    # increment 1: every class, each on the side it is built for, with the property that names it
    r1, r2 = hist["ref"][0], hist["ref"][1]
    cls = pf.plane_hosford_classes(seed, N)
    d, t01 = pf.plane_hosford_rotation(hist, 0)
    e1 = hist["eps"][0] - hist["ep0"]
    for k, name in enumerate(hp.CLASSES):
        rows = cls == k
        assert rows.sum() >= N // len(hp.CLASSES) and (r1["plastic"][rows] == PLASTIC_CLASS[name]).all(), (prm, name)
    ser, quo, opp = pf.plane_hosford_paths(r1["sig"], a)
    c = {name: cls == k for k, name in enumerate(hp.CLASSES)}
    assert (d[c["inplane_equal"]] == 0.0).all() and (t01[c["inplane_equal"]] == 0.0).all()           # zero shear, the guarded division
    assert (d[c["axis_aligned"]] != 0.0).all() and (t01[c["axis_aligned"]] == 0.0).all()             # zero shear, distinct values
    assert ((t01 == 0.0) & (e1[:, 1] == e1[:, 2]) & c["zz_equal"]).sum() >= 0.4 * c["zz_equal"].sum()
    assert (t01[c["generic"]] != 0.0).all() and (t01[c["near"]] != 0.0).any()
    for name in ("inplane_equal", "zz_equal"):                                                       # either sign of the repeated pair
        assert (e1[c[name], 2] > e1[c[name], 0]).any() and (e1[c[name], 2] < e1[c[name], 0]).any(), (prm, name)
    assert ser[c["inplane_equal"]].all() and ser[c["near"]].mean() > 0.9, prm
    assert (quo | opp)[c["generic"]].mean() > 0.8 and quo[c["generic"]].sum() >= 50 and opp[c["generic"]].sum() >= 50, prm
    assert np.array_equal(np.flatnonzero(c["zero"]), np.flatnonzero(~hist["eps"][0].any(axis=1)))     # the class layout is mixed_inputs'
    # increment 2: unloading, re-yielding with the deviator reversed, and the rotation at exactly 45 degrees
    unloaded = r1["plastic"] & ~r2["plastic"]
    reyield = r1["plastic"] & r2["plastic"] & ((_deviator(r1["sig"]) * _deviator(r2["sig"])).sum(axis=1) < 0.0)
    d, t01 = pf.plane_hosford_rotation(hist, 1)
    at45 = (d == 0.0) & (t01 != 0.0)
    print(f"plane hosford seed {seed}: increment 2 unloads {int(unloaded.sum())} points, yields {int(reyield.sum())} again reversed, "
          f"{int((at45 & r2['plastic']).sum())} yielding points with the in-plane axes at exactly 45 degrees")
    assert unloaded.mean() >= 0.01 and reyield.mean() >= 0.01, (prm, unloaded.mean(), reyield.mean())
    assert at45[hist["shear45"]].all() and (hist["shear45"] & r2["plastic"]).sum() >= 50, (prm, int(at45.sum()))
    assert (hist["ref"][3]["p"] > hist["ref"][0]["p"]).sum() > N // 10, prm                          # plastic flow after the first increment
    for inc in (2, 3):                                                                               # non-proportional: off the old direction
        s0, s1 = _deviator(hist["ref"][inc - 1]["sig"]), _deviator(hist["ref"][inc]["sig"])
        cosine = (s0 * s1).sum(axis=1) / np.maximum(np.linalg.norm(s0, axis=1) * np.linalg.norm(s1, axis=1), 1e-300)
        assert (cosine[hist["ref"][inc]["plastic"]] < 0.99).mean() > 0.5, (prm, inc)
    ds, dc = pf.plane_hosford_deviation(seed)
    print(f"plane hosford seed {seed} {prm}: definition against 50 digits: state {ds:.2e} tangent {dc:.2e}")
    assert ds <= 1.0 * float(BOUNDS["dev_hosford_state"][seed]) and dc <= 1.0 * float(BOUNDS["dev_hosford_tangent"][seed]), (prm, ds, dc)
    assert 8 * ds <= float(BOUNDS["bound_hosford_state"]) and 8 * dc <= float(BOUNDS["bound_hosford_tangent"]), (prm, ds, dc)


@pytest.mark.parametrize("seed", pf.OGDEN_SEEDS)
def test_plane_ogden_reference_over_the_stretches(seed):
    from test_ogden_cpu import E0

    prm = pf.draw_ogden(seed)
    amp = pf.plane_ogden_amp(seed)
    F = pf.plane_ogden_F(seed, N, amp)
    assert F.shape == (N, 5) and not F.flags.writeable and pf.plane_ogden_F(seed, N, amp) is F
    Fm = og.to_matrix(op.embed(F))
    assert (np.linalg.det(Fm) > 0.0).all()
    c = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", Fm, Fm))
    lam = np.sqrt(c)
    assert lam.min() >= 1 / amp * (1 - 1e-6) and lam.max() <= amp * (1 + 1e-6) and lam.max() > 0.9 * amp, (amp, lam.min(), lam.max())
    k = pf.plane_ogden_kinds(seed, N)
    assert (np.abs(F[~k["aligned"], 3] - F[~k["aligned"], 4]) > 0.05).mean() > 0.8                    # rotated, not symmetric stretches
    assert not F[k["aligned"], 3:].any()
    want = op.restricted_closed_form(F, **prm)
    assert all(np.isfinite(x).all() for x in want), prm
    e = op.errors(op.plane_closed_form(F, **prm), want)
    cond = pf.plane_ogden_conditioning(F, want[0], prm["K"])
    series, quotient = pf.plane_ogden_paths(F, prm["alpha"])
    print(f"plane ogden seed {seed} {prm} amp {amp}: the two restatements P {e[0]:.2e} A {e[1]:.2e} PK2Stress {e[2]:.2e} (E0 {E0:.0e}); "
          f"series rows {series.mean():.2f}; K J / |P| up to {cond.max():.0f} (cap {pf.OGDEN_CONDITION_CAP:.0f}), {pf.plane_ogden_redrawn(seed, N, amp)} rows drawn again")
    assert max(e) <= E0, (prm, e)
    assert cond.max() <= pf.OGDEN_CONDITION_CAP and pf.plane_ogden_redrawn(seed, N, amp) <= 0.02 * N, prm
    assert series.mean() >= 0.05 and quotient.mean() >= 0.05, (prm, series.mean(), quotient.mean())
    # the nearly repeated rows: every gap, aligned and rotated, with the gap they were built for
    assert 0.2 < k["inplane"].mean() < 0.3 and 0.09 < k["to_c2"].mean() < 0.16 and 0.4 < k["aligned"][k["inplane"] | k["to_c2"]].mean() < 0.6
    c2 = F[:, 2] ** 2
    inpl = np.stack(pf.plane_ogden_inplane_pair(F)[::-1], axis=1)                                     # the in-plane pair, ascending
    assert np.abs(np.sort(np.concatenate([inpl, c2[:, None]], axis=1), axis=1) / c - 1.0).max() < 1e-12
    for gap in og.GAPS:
        for aligned in (True, False):
            rows = k["inplane"] & (k["gap"] == gap) & (k["aligned"] == aligned)
            assert rows.sum() >= 20, (prm, gap, aligned)
            got = inpl[rows, 1] / inpl[rows, 0] - 1.0
            assert np.abs(got - gap).max() <= 1e-14 + 1e-6 * gap, (prm, gap, aligned, got)
            if aligned and gap == 0.0:
                assert np.array_equal(F[rows, 0], F[rows, 1])
            if gap <= 1e-4:
                assert series[rows].all()
            rows = k["to_c2"] & (k["gap"] == gap) & (k["aligned"] == aligned)
            assert rows.sum() >= 8, (prm, gap, aligned)
            assert (np.abs(c2[rows, None] / inpl[rows] - 1.0 - gap).min(axis=1) <= 1e-14 + 1e-6 * gap).all(), (prm, gap, aligned)
    dev = pf.plane_ogden_deviation(seed)
    print(f"plane ogden seed {seed}: definition against 60 digits {dev:.2e}")
    assert dev <= 1.0 * float(BOUNDS["dev_ogden"][seed]) and 8 * dev <= float(BOUNDS["bound_ogden"]), (prm, dev)
    rows = pf.plane_ogden_sample(seed, N, series)
    assert len(rows) == pf.MP_SAMPLE and series[rows].sum() == pf.MP_SAMPLE // 2
