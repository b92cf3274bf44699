"""CPU: plane-stress J2 plasticity with isotropic hardening (laws 30 and 31) over parameters and histories, without a GPU: the numpy
restatement ``plane_stress_j2_ref`` against the 50-digit sweep fixture ``golden/plane_stress_j2_sweep.npz`` (built in the nested
form) draw by draw and increment by increment, the figures the GPU bounds come from, the rules of the seeded inputs, the rows
with a closed form, the bracket under softening parameters, the counted point without a bracket, and the tangent against central
differences of the 50-digit stress."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import plane_stress_j2_cases as cs
import plane_stress_j2_ref as pj

DRAWS = [(law, k) for law in cs.LAWS for k in range(cs.N_DRAWS)]
HISTORIES = [(law, k) for law in cs.LAWS for k in cs.HISTORY_DRAWS[law]]
IDS = lambda lk: cs.tag(*lk)      # noqa: E731


@functools.lru_cache(maxsize=None)
def fixture():
    return cs.load_fixture()


def deviation(prm, r, want):
    """(stress in sig0, tangent in E, p and epsp in sig0 / E)"""
    s, Em = prm[2], prm[0]
    return np.array([np.abs(r["stress"] - want["stress"]).max() / s, np.abs(r["tangent"] - want["tangent"]).max() / Em,
                     max(np.abs(r["p"] - want["p"]).max(), np.abs(r["epsp"] - want["epsp"]).max()) / (s / Em)])


@functools.lru_cache(maxsize=None)
def restated_draw(law, k):
    d = cs.fixture_draw(fixture(), law, k)
    r = pj.update(law, d["eps"], d["epsp_n"], d["p_n"], d["prm"])
    return d, r, deviation(d["prm"], r, d)


@functools.lru_cache(maxsize=None)
def restated_history(law, k):
    """the restatement carries its own state, as the kernel does"""
    prm, incs = cs.fixture_history(fixture(), law, k)
    n = len(incs[0]["eps"])
    ep, p, out = np.zeros((n, 3)), np.zeros(n), []
    for inc in incs:
        r = pj.update(law, inc["eps"], ep, p, prm)
        out.append((r, deviation(prm, r, inc), (ep, p)))
        ep, p = r["epsp"], r["p"]
    return prm, incs, out


def healthy(tag, r, want):
    """what every draw and increment must show at the default cap"""
    assert np.array_equal(r["plastic"], want["plastic"]), tag
    st = pj.stats(r)
    assert st["n_not_converged"] == 0 and st["n_nan"] == 0, (tag, st)
    ct = r["tangent"].reshape(-1, 3, 3)
    assert np.array_equal(ct, np.swapaxes(ct, 1, 2))


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_generator_says():
    fx = fixture()
    meta = json.loads(str(fx["meta"]))
    assert meta["dps"] == 50 and meta["off_surface"] == cs.OFF
    assert [(m["law"], m["draw"]) for m in meta["draws"]] == DRAWS and [(m["law"], m["draw"]) for m in meta["histories"]] == HISTORIES
    largest = max(os.path.getsize(os.path.join(os.path.dirname(cs.GOLDEN), f)) for f in os.listdir(os.path.dirname(cs.GOLDEN))
                  if f != os.path.basename(cs.GOLDEN))
    assert os.path.getsize(cs.GOLDEN) <= largest


@pytest.mark.parametrize("lk", DRAWS, ids=IDS)
def test_the_restatement_against_the_fixture_draw_by_draw_and_the_rules_of_its_inputs(lk):
    law, k = lk
    d, r, dev = restated_draw(law, k)
    prm = cs.draw(law, k)
    eps, ep, p, far = cs.points(law, k)
    # the fixture holds the seeded inputs
    assert np.array_equal(d["prm"], prm) and np.array_equal(d["eps"], eps) and np.array_equal(d["epsp_n"], ep) and np.array_equal(d["p_n"], p)
    assert len(eps) == cs.N_STATE + cs.N_OVER and cs.off_surface(law, prm, eps, ep, p).all()
    share = d["plastic"].mean()
    over = r["overshoot"]
    top = cs.OVER_SOFT if cs.softening(law, k) else cs.OVER_HARD
    print(f"{cs.tag(law, k)} prm {prm}: yielded {share:.2f}, overshoot up to {over.max():.4g}, iterations of the yielded points: "
          f"max {r['iters'].max()} mean {r['iters'][r['plastic']].mean():.2f}; stress {dev[0]:.3e} tangent {dev[1]:.3e} state {dev[2]:.3e}")
    assert 0.3 <= share <= 0.8
    assert over[far].max() >= 0.999 * top and over.max() <= 1.001 * top and 0 < p.max() <= cs.P_OLD * prm[2] / prm[0]
    healthy(cs.tag(law, k), r, d)
    assert 2 <= r["iters"].max() < pj.MAXIT
    assert (dev <= np.array(cs.MEASURED_SWEEP[law])).all(), (dev, cs.MEASURED_SWEEP[law])
    # an elastic point keeps its bits
    el = ~d["plastic"]
    assert np.array_equal(r["p"][el], p[el]) and np.array_equal(r["epsp"][el], ep[el]) and (p[el] > 0).sum() >= 10


@pytest.mark.parametrize("lk", HISTORIES, ids=IDS)
def test_the_restatement_against_the_fixture_over_six_increments(lk):
    law, k = lk
    prm, incs, out = restated_history(law, k)
    seeded = cs.history(law, k)
    assert len(incs) == len(cs.HISTORY_SCHEDULE) == 6 and np.array_equal(prm, cs.draw(law, k))
    rested = 0
    for q, (inc, (r, dev, (ep, p))) in enumerate(zip(incs, out)):
        assert np.array_equal(inc["eps"], seeded[q]), (cs.tag(law, k), q)
        print(f"{cs.tag(law, k)} increment {q}: yielded {inc['plastic'].sum()} of {len(p)}, iterations max {r['iters'].max()}; "
              f"stress {dev[0]:.3e} tangent {dev[1]:.3e} state {dev[2]:.3e}")
        healthy((cs.tag(law, k), q), r, inc)
        assert (dev <= np.array(cs.MEASURED_SWEEP[law])).all(), (q, dev, cs.MEASURED_SWEEP[law])
        el = ~inc["plastic"]
        assert np.array_equal(r["p"][el], p[el]) and np.array_equal(r["epsp"][el], ep[el])
        rested += int((el & (p > 0)).sum())
        assert 5 <= inc["plastic"].sum() <= len(p) - 5
    assert rested >= 40            # "an elastic point keeps its bits" met states that are not zero
    # the schedule did what it says: the third increment unloads, the last exceeds the first peak
    assert incs[2]["plastic"].sum() < incs[1]["plastic"].sum() and (out[5][0]["p"] >= out[1][0]["p"]).all()


@pytest.mark.parametrize("law", cs.LAWS, ids=list(cs.NAME.values()))
def test_the_figures_the_gpu_bounds_come_from(law):
    worst = np.zeros(3)
    for k in range(cs.N_DRAWS):
        worst = np.maximum(worst, restated_draw(law, k)[2])
    for k in cs.HISTORY_DRAWS[law]:
        for _, dev, _ in restated_history(law, k)[2]:
            worst = np.maximum(worst, dev)
    rec = np.array(cs.MEASURED_SWEEP[law])
    print(cs.NAME[law], "restatement against the sweep fixture: stress %.3e  tangent %.3e  state %.3e" % tuple(worst), "recorded", cs.MEASURED_SWEEP[law])
    assert (worst <= rec).all() and (worst >= 0.5 * rec).all(), (worst, rec)
    assert all(b == max(16 * m, 2e-14) for b, m in zip(cs.gpu_bounds(law), cs.MEASURED_SWEEP[law]))


# ---- the softening draws ----------------------------------------------------------------------------------------------------------------
def residual(law, prm, t, p_n, dg):
    """g(dg) of the kernel's header, t = (ta, tb, tc) the trial in its basis"""
    c = pj.constants(prm[0], prm[1])
    R, _ = pj.hardening(law, prm)
    a, b = 1.0 / (1.0 + dg * c["ka"]), 1.0 / (1.0 + dg * c["CB"])
    seq = np.sqrt(0.5 * (t[0] * a) ** 2 + 1.5 * ((t[1] * b) ** 2 + (t[2] * b) ** 2))
    return seq - R(p_n + (2.0 / 3.0) * dg * seq)


def bracket(law, prm, eps, ep, p):
    """(t, f, floor, hi) of the yielded rows as the kernel forms them"""
    prm = [float(v) for v in prm]
    c = pj.constants(prm[0], prm[1])
    R, _ = pj.hardening(law, prm)
    ee = eps - ep
    t = np.array([c["CA"] * ((ee[:, 0] + ee[:, 1]) * pj.R2), c["CB"] * ((ee[:, 0] - ee[:, 1]) * pj.R2), c["CB"] * ee[:, 2]])
    seqt = np.sqrt(0.5 * t[0] ** 2 + 1.5 * (t[1] ** 2 + t[2] ** 2))
    Rn = R(p)
    if law == pj.J2_VOCE:
        floor = np.minimum(Rn, prm[3])
    else:
        floor = Rn + min(prm[3], 0.0) * (2.0 / 3.0) * np.sqrt(0.5 * (t[0] / c["ka"]) ** 2 + 1.5 * ((t[1] / c["CB"]) ** 2 + (t[2] / c["CB"]) ** 2))
    return t, seqt - Rn, floor, (seqt / floor - 1.0) / c["kmin"]


@pytest.mark.parametrize("law", cs.LAWS, ids=list(cs.NAME.values()))
def test_the_softening_draws_meet_the_generators_asserts_and_the_bracket_holds_the_root(law):
    for k in cs.SOFTENING:
        prm = cs.draw(law, k)
        R, dR = pj.hardening(law, prm)
        d, r, _ = restated_draw(law, k)
        sets = [(d["eps"], d["epsp_n"], d["p_n"], d)]
        if k in cs.HISTORY_DRAWS[law]:
            _, incs, out = restated_history(law, k)
            sets += [(inc["eps"], ep, p, inc) for inc, (_, _, (ep, p)) in zip(incs, out)]
        assert (dR(np.linspace(0.0, 40.0, 9) * prm[2] / prm[0]) < 0).all()           # it softens
        for eps, ep, p, want in sets:
            assert (R(want["p"]) >= cs.R_FLOOR * prm[2]).all() and R(want["p"]).min() < prm[2] * (1 - 1e-7)
            pl = want["plastic"]
            t, f, floor, hi = bracket(law, prm, eps[pl], ep[pl], p[pl])
            assert (floor > 0).all() and (f > 0).all()
            # g changes sign over [0, hi], is monotone on nine samples of it, and the 50-digit multiplier lies inside:
            # dg = 3/2 dp / seq of the returned state
            g = np.array([residual(law, prm, t, p[pl], hi * q / 8.0) for q in range(9)])
            assert (g[0] > 0).all() and (g[-1] <= 0).all() and (np.diff(g, axis=0) < 0).all()
            dg = 1.5 * (want["p"][pl] - p[pl]) / pj.seq_of(want["stress"][pl])
            assert (dg > 0).all() and (dg <= hi).all()
            # the bracket of R >= R_n, what the kernel had: it misses roots of these draws (H = -E / 70, Voce) or holds them all
            # (H = -1e-5 E at these overshoots)
            missed = int((dg > (f / R(p[pl])) / pj.constants(prm[0], prm[1])["kmin"]).sum())
            print(f"{cs.tag(law, k)}: {pl.sum()} yielded points, {missed} roots beyond the bracket of R >= R_n")


def test_a_point_without_a_bracket_is_counted_and_writes_its_start():
    """H = -E / 70 at overshoot 1e3: the bound of R over the step is negative, no bracket exists; the point is counted as not
    converged at its first residual, with finite outputs, and its neighbours are untouched.  Voce with sigu <= 0 likewise."""
    for law, prm in ((pj.J2_LINEAR, cs.draw(pj.J2_LINEAR, 10)), (pj.J2_VOCE, [70e3, 0.3, 500.0, -10.0, 100.0])):
        eps = pj.random_trials(prm, 8, seed=5, lo=2.0, hi=4.0)
        base = pj.update(law, eps, np.zeros_like(eps), np.zeros(8), prm)
        eps[3] *= 1e3 / base["overshoot"][3]
        r = pj.update(law, eps, np.zeros_like(eps), np.zeros(8), prm)
        assert bracket(law, prm, eps[3:4], np.zeros((1, 3)), np.zeros(1))[2][0] <= 0
        assert r["not_converged"].tolist() == [q == 3 for q in range(8)] if law == pj.J2_LINEAR else r["not_converged"].all()
        assert r["iters"][3] == 0 and r["plastic"][3] and pj.stats(r)["n_nan"] == 0 and r["multiplier"][3] > 0
        if law == pj.J2_LINEAR:
            keep = np.arange(8) != 3
            assert all(np.array_equal(r[q][keep], base[q][keep]) for q in ("stress", "tangent", "p", "epsp"))
            assert pj.stats(r)["n_not_converged"] == 1


# ---- rows with a closed form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", DRAWS, ids=IDS)
def test_special_rows_take_their_branch_and_follow_the_closed_forms(lk):
    """Bound: ``plane_stress_j2_cases.special_bounds`` -- 32 U |eps|_max E / (1 - |nu|) of stress and (1 + cond C) times that of state,
    from the conditioning of ``eps - C^-1 s`` (derived there).  The rows at R_n (1 -+ 1e-12) may take either branch: the two answers
    differ by 1e-12 sig0, which is added to their bound; nothing else is excluded."""
    law, k = lk
    prm = cs.draw(law, k)
    sp = cs.special_rows(law, prm, cs.softening(law, k))
    r = pj.update(law, sp["eps"], sp["epsp_n"], sp["p_n"], prm)
    bs, be = cs.special_bounds(prm, sp["eps"])
    assert len(sp["labels"]) == (11 if cs.softening(law, k) else 12)
    for i, label in enumerate(sp["labels"]):
        either = sp["plastic"][i] is None
        assert either or bool(r["plastic"][i]) == sp["plastic"][i], label
        slack = 2e-12 if either else 0.0
        es = np.abs(r["stress"][i] - sp["stress"][i]).max() / prm[2]
        ee = max(abs(r["p"][i] - sp["p"][i]), np.abs(r["epsp"][i] - sp["epsp"][i]).max()) / (prm[2] / prm[0])
        assert es <= bs[i] + slack and ee <= be[i] + slack, (cs.tag(law, k), label, es, bs[i], ee, be[i])
        assert not r["not_converged"][i], label
    # symmetry makes these exact zeros
    for i, label in enumerate(sp["labels"]):
        if label.startswith("equibiaxial"):
            assert r["stress"][i, 2] == 0.0 and r["epsp"][i, 2] == 0.0 and r["stress"][i, 0] == r["stress"][i, 1], label
        if label.startswith("pure shear"):
            assert not r["stress"][i, :2].any() and not r["epsp"][i, :2].any(), label
        if label == "zero strain":
            assert not r["stress"][i].any() and r["p"][i] == 0.0
    # the equibiaxial root sits at the upper end of the hardening bracket, (seq_tr / R_n - 1) / kmin with kmin = ka
    if prm[1] > -0.5 and not cs.softening(law, k):
        i = sp["labels"].index("equibiaxial")
        t, f, floor, hi = bracket(law, prm, sp["eps"][i:i + 1], sp["epsp_n"][i:i + 1], sp["p_n"][i:i + 1])
        R, _ = pj.hardening(law, prm)
        root = 1.5 * sp["p"][i] / R(sp["p"][i])
        if law == pj.J2_LINEAR and prm[3] == 0.0:
            assert abs(root / hi[0] - 1.0) <= 1e-12
        assert root <= hi[0] * (1 + 1e-12)


# ---- the tangent against central differences of the 50-digit stress --------------------------------------------------------------------
@pytest.mark.parametrize("law", cs.LAWS, ids=list(cs.NAME.values()))
def test_the_tangent_against_central_differences_of_the_50_digit_stress(law):
    """three yielded points per draw (the first two of the U(0, 2) R_n rows and the first of the far rows).  The step is 1e-12 of the
    strain's size: at 50 digits the quotient carries its truncation error only, of relative order 1e-24, so the restatement is
    held to what it deviates from the fixture's tangent by (MEASURED_SWEEP), plus 1e-15 E for the conversion of the quotient."""
    import mpmath as mp

    sys.path.insert(0, os.path.dirname(cs.GOLDEN))
    import make_plane_stress_j2 as gen

    worst = 0.0
    for k in range(cs.N_DRAWS):
        d, r, _ = restated_draw(law, k)
        prm = [float(v) for v in d["prm"]]
        pl = np.flatnonzero(d["plastic"])
        rows = list(pl[pl < cs.N_STATE][:2]) + list(pl[pl >= cs.N_STATE][:1])
        for i in rows:
            ep, p = [mp.mpf(float(v)) for v in d["epsp_n"][i]], mp.mpf(float(d["p_n"][i]))
            h = mp.mpf(10) ** -12 * mp.mpf(float(np.abs(d["eps"][i]).max()))
            fd = np.empty((3, 3))
            for c in range(3):
                e = [mp.mpf(float(v)) for v in d["eps"][i]]
                e[c] += h
                up = _mp_stress(gen, law, prm, e, ep, p)
                e[c] -= 2 * h
                dn = _mp_stress(gen, law, prm, e, ep, p)
                fd[:, c] = [float((a - b) / (2 * h)) for a, b in zip(up, dn)]
            err = np.abs(fd.reshape(9) - r["tangent"][i]).max() / prm[0]
            worst = max(worst, err)
            assert err <= cs.MEASURED_SWEEP[law][1] + 1e-15, (cs.tag(law, k), i, err)
            assert np.abs(fd.reshape(9) - d["tangent"][i]).max() / prm[0] <= 1e-15
    print(cs.NAME[law], "tangent against central differences of the 50-digit stress, in E:", worst)


def _mp_stress(gen, law, prm, e, ep, p):
    """``plane_stress_update`` rounds its strain to double on the way in: the shifted strain goes through its parts instead"""
    import mpmath as mp

    ep6 = [ep[0], ep[1], -(ep[0] + ep[1]), ep[2], mp.mpf(0), mp.mpf(0)]
    e6 = lambda z: [e[0], e[1], z, e[2], mp.mpf(0), mp.mpf(0)]      # noqa: E731
    szz = lambda z: gen.radial_return(law, prm, e6(z), ep6, p)[0][2]      # noqa: E731
    scale = sum(abs(v) for v in e) + sum(abs(v) for v in ep) + mp.mpf(10) ** -6
    z = mp.findroot(szz, (-4 * scale, 4 * scale), solver="illinois", tol=mp.mpf(10) ** -47, maxsteps=1000, verify=False)
    sig = gen.radial_return(law, prm, e6(z), ep6, p)[0]
    return [sig[0], sig[1], sig[3]]
