"""CPU: logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_J2) at finite stretches, over parameters and histories -- what
``test_gpu_log_strain_finite.py`` rests on, established by the references alone (``log_strain_cases``):

* the numpy restatement ``log_strain_ref.update`` against the eigen-free 100-digit values of ``golden/log_strain_finite.npz``, per
  stratum (one per ``amp`` and one for the special rows): the error floors ``FLOOR``, from which the GPU bounds follow,
  ``BOUNDS[s] = 16 FLOOR[s]`` (the margin of ``test_log_strain_cpu.py`` and ``test_gpu_ogden.py``; no clamp);
* the rules every batch of the GPU file obeys: plastic share, kink cap, and -- classified with the kernel's own Jacobi restated in
  numpy -- every form of every divided difference and every one of the three quotients the (0, 1, 2) call can be handed;
* that five cyclic sweeps leave nothing off the diagonal;
* the restatement's tangent against central differences of its own stress over the stretch family, for every draw;
* that the fixture comparison fails when the restatement is subtly wrong.

Measured (scaled as ``log_strain_ref.scaled_errors`` with the draw's own s0 and E), restatement against the fixture:

    stratum    PK1       tangent   ElasticStrain  p         PlasticStrain
    amp 1.1    1.06e-12  5.90e-13  9.29e-13       1.01e-15  1.83e-14
    amp 1.3    1.16e-12  7.27e-13  9.33e-13       2.88e-15  1.53e-15
    amp 2      1.37e-12  2.74e-12  1.30e-12       6.54e-14  6.82e-16
    amp 3      1.14e-11  1.23e-12  4.01e-12       1.54e-15  8.12e-16
    special    1.23e-13  2.91e-12  8.83e-14       1.24e-15  2.44e-14

These are above the E0 = 2e-13 of the degenerate set for a reason that no formulation in float64 escapes: the trial elastic strain
E(F) - Ep_n is of the size of the yield strain s0 / E (down to 1e-4 here) while E(F) and Ep_n are of order ln(amp) (up to 1.1), so
the rounding of the Hencky strain alone, eps ln(amp), is 1e-12 and more of what the stress is made of.

Jacobi (all families, 67 282 matrices): the largest off-diagonal entry left after five sweeps is 1.53e-19 of the largest eigenvalue
(4.34e-19 after four: the fifth sweep is the one that confirms), the eigenvalues are within 1.55e-15 (relative to the largest) of
``numpy.linalg.eigvalsh``, V^T V - 1 within 1.78e-15 and V c V^T - C within 1.89e-15: rounding, no more.

Tangent against central differences: at most 0.67 of the reasoned bound (draw 9, amp 3: 1.5e-8), see the test."""
import numpy as np
import pytest

import log_strain_cases as lc
import log_strain_ref as ls

FLOOR = {"amp 1.1": 1.2e-12, "amp 1.3": 1.2e-12, "amp 2": 3e-12, "amp 3": 1.2e-11, "special": 3e-12}   # the table above, rounded up
BOUNDS = {s: 16.0 * v for s, v in FLOOR.items()}
HISTORY_STRATUM = "amp 2"       # the histories reach stretches of at most 2
JACOBI_OFF = 2e-19              # see the module docstring; asserted by test_five_sweeps_suffice
JACOBI_EIG = 2.5e-15
MIN_PER_QUOTIENT = 100
EPS = np.finfo(np.float64).eps


def stratum_of(amp):
    return f"amp {amp:g}"


def batch_seed(k):
    """The seed of draw k's batch in the GPU file (chosen so that the rules below hold)."""
    return 0


def batch_of(k):
    amp = lc.AMPS[k % len(lc.AMPS)]
    return amp, lc.stretch_case(k, lc.N_BATCH, amp, batch_seed(k))


@pytest.fixture(scope="module")
def fx():
    return lc.load_fixture()


def restated(fx, rows):
    """``ls.update`` on the fixture's rows ``rows`` (a mask within one draw)."""
    k = int(fx["draw"][rows][0])
    assert (fx["draw"][rows] == k).all()
    prm = lc.draw(k)
    return prm, ls.update(fx["F"][rows], fx["Ep_n"][rows], fx["p_n"][rows], **prm)


def floor_figures(fx):
    """{stratum: {quantity: worst scaled error of the restatement against the fixture}}"""
    out = {}
    for name, mask in lc.strata(fx).items():
        worst = {}
        for k in np.unique(fx["draw"][mask]):
            rows = mask & (fx["draw"] == k)
            prm, r = restated(fx, rows)
            assert np.array_equal(r["plastic"], fx["plastic"][rows]) and not r["skip"].any(), (name, k)
            e = ls.scaled_errors(r, {q: fx[q][rows] for q in ("P", "A", "eel", "p", "Ep")}, s0=prm["s0"], E=prm["E"])
            worst = {q: max(v, worst.get(q, 0.0)) for q, v in e.items()}
        out[name] = worst
    return out


def test_error_floor_per_stratum(fx):
    figs = floor_figures(fx)
    for name, e in figs.items():
        print(f"log-strain finite floor, {name:8s}: " + " ".join(f"{q} {v:.2e}" for q, v in e.items()) + f" (FLOOR {FLOOR[name]:.1e})")
    for name, e in figs.items():
        assert max(e.values()) <= FLOOR[name], (name, e)
        assert max(e.values()) >= FLOOR[name] / 4.0, (name, e)      # the constant is the measured figure rounded up, no more


def test_fixture_is_the_generators_set(fx):
    F, Ep_n, p_n, params, dr, amp, labels = lc.fixture_points()
    assert len(F) == 144 == len(fx["F"]) and labels == fx["labels"]
    for key, want in (("F", F), ("Ep_n", Ep_n), ("p_n", p_n), ("params", params), ("draw", dr), ("amp", amp)):
        assert np.array_equal(fx[key], want), key
    for k in range(lc.N_DRAWS):
        assert np.array_equal(fx["params"][fx["draw"] == k][0], [lc.draw(k)[q] for q in ("E", "nu", "s0", "H0")])
        for a in lc.AMPS:
            pl = fx["plastic"][(fx["draw"] == k) & (fx["amp"] == a)]
            assert len(pl) == lc.FIXTURE_PER_AMP and pl.any() and not pl.all(), (k, a)       # both branches
    sp = fx["amp"] == 0.0
    assert sp.sum() == len(lc.FIXTURE_SPECIAL) == 24 and fx["plastic"][sp].any() and not fx["plastic"][sp].all()
    assert np.isfinite(fx["A"]).all() and np.isfinite(fx["P"]).all()
    # none of them is in the degenerate fixture already
    old = ls.load_golden()[0]
    assert not any((np.abs(old - row).max(axis=1) == 0.0).any() for row in fx["F"])
    # the (0, 1, 2) call is handed each of its three quotients, and takes its Taylor form, within the fixture
    f = lc.classify(fx["F"])["f"]
    assert all((f == q).sum() >= 10 for q in (0, 1, 2)) and (f == -1).sum() >= 5, np.bincount(f + 1)


def test_parameter_draws():
    d = [lc.draw(k) for k in range(lc.N_DRAWS)]
    assert d[0] == ls.PRM
    assert [x["nu"] for x in d if x["nu"] in (0.0, 0.49, -0.3)] == [0.49, 0.0, -0.3]
    assert all(-0.3 <= x["nu"] <= 0.49 and 1e3 <= x["E"] <= 10 ** 11.5 and 1e-4 <= x["s0"] / x["E"] <= 10 ** -1.5 for x in d)
    assert [k for k, x in enumerate(d) if x["H0"] == 0.0] == [3, 6, 9] and d[5]["H0"] == 10.0 * d[5]["E"]
    assert all(0.0 < x["H0"] <= 0.5 * x["E"] for k, x in enumerate(d) if k not in (0, 3, 5, 6, 9))
    assert set(lc.HISTORY_DRAWS) == {0, 3, 5}


# ---- input rules: by the references alone, for every batch the GPU file uses ------------------------------------------------------
def _within_rules(b, what):
    kink = float(np.mean(b["skip"]))
    share = float(np.mean(b["plastic"]))
    assert kink <= ls.KINK_CAP, (what, kink)
    assert ls.SHARE[0] <= share <= ls.SHARE[1], (what, share)
    return share


def _branch_rules(F9, what, mixed):
    cl = lc.classify(F9)
    far, tf, f = cl["gamma_far"], cl["theta_far"], cl["f"]
    counts = [int((f == q).sum()) for q in (0, 1, 2)]
    print(f"{what}: quotient form of the seven gamma calls {far.sum(axis=0)}, of the three theta calls {tf.sum(axis=0)}, "
          f"f0 / f1 / f2 {counts}, Taylor form of the (0, 1, 2) call {(f == -1).sum()}, of {len(F9)}")
    if mixed:
        assert min(counts) >= MIN_PER_QUOTIENT, (what, counts)
        assert far.any(axis=0).all() and (~far).any(axis=0).all(), (what, far.sum(axis=0))
        assert tf.any(axis=0).all() and (~tf).any(axis=0).all(), (what, tf.sum(axis=0))
    return cl


@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_batches_stay_within_the_rules(k):
    amp, (F, Ep, p) = batch_of(k)
    b = ls.branch(F, Ep, p, **lc.draw(k))
    share = _within_rules(b, (k, amp))
    print(f"draw {k} amp {amp:g}: plastic share {share:.3f}, {int(b['skip'].sum())} in the kink band")
    _branch_rules(F, f"draw {k} amp {amp:g}", mixed=amp >= 1.3)
    # the construction does what it says: seq_trial / R_n is uniform on (0, 2), the volume change is of the size of the yield strain
    prm = lc.draw(k)
    u = b["f_trial"] / (prm["s0"] + prm["H0"] * p) + 1.0
    assert 0.0 <= u.min() < 0.01 and 1.99 < u.max() <= 2.0 + 1e-9
    lnJ = np.log(np.linalg.det(ls.to_matrix(F)))
    assert np.abs(lnJ).max() <= 3.0 * prm["s0"] / prm["E"] * (1.0 + 1e-9) + 1e-15
    lam = np.sqrt(np.linalg.eigvalsh(np.einsum("nki,nkj->nij", ls.to_matrix(F), ls.to_matrix(F))))
    assert lam.max() <= amp ** (4.0 / 3.0) * 1.001 and lam.max() >= 0.95 * amp


def test_mixed_batch_stays_within_the_rules():
    F, Ep, p, special = lc.mixed_prm_batch()
    assert len(F) == lc.N_BATCH and special[[0, 63, 64, lc.N_BATCH - 3, lc.N_BATCH - 1]].all() and special.sum() == 168
    b = ls.branch(F, Ep, p)
    _within_rules({q: b[q][~special] for q in ("skip", "plastic")}, "mixed")
    assert not b["skip"][special].any()
    sp = b["plastic"][special]
    assert sp.any() and not sp.all()
    _branch_rules(F[~special], "mixed, random rows", mixed=True)
    # the special rows alone hand the (0, 1, 2) call each of its quotients and both forms of every call
    cl = _branch_rules(F[special], "mixed, special rows", mixed=False)
    assert all((cl["f"] == q).sum() >= 10 for q in (0, 1, 2))
    assert cl["gamma_far"].any(axis=0).all() and (~cl["gamma_far"]).any(axis=0).all()
    assert cl["theta_far"].any(axis=0).all() and (~cl["theta_far"]).any(axis=0).all()


def test_special_rows():
    F9, labels = lc.special_F()
    assert len(labels) == len(set(labels)) == 84 and all(lab in labels for lab, _ in lc.FIXTURE_SPECIAL)
    F = ls.to_matrix(F9)
    assert (np.linalg.det(F) > 0.0).all()
    C = np.einsum("nki,nkj->nij", F, F)
    c, V, off = lc.jacobi_np(C)
    at = labels.index
    # axis-aligned rows: every rotation is the no-op, the eigenvalues stay where they were written
    for lab in ("diagonal", "exact pair 01", "exact pair 02", "exact pair 12", "near pair 12", "3 identity"):
        k = at(lab)
        assert np.array_equal(c[k], np.diag(C[k])) and np.array_equal(V[k], np.eye(3)) and off[k] == 0.0, lab
    for i, j in ((0, 1), (0, 2), (1, 2)):
        k = at(f"exact pair {i}{j}")
        assert c[k, i] == c[k, j] and np.isclose(c[k].max() / c[k].min(), 2.0)
        k = at(f"near pair {i}{j}")
        assert 0.5e-7 < abs(c[k, i] / c[k, j] - 1.0) < 2e-7
    # the cyclic permutations deliver the same eigenvalues in another order
    for lab in ("diagonal", "near pair 01", "theta pair at switch +1"):
        k0, k1, k2 = at(lab), at(lab + " perm 1"), at(lab + " perm 2")
        assert np.array_equal(np.sort(c[k0]), np.sort(c[k1])) and np.array_equal(np.sort(c[k0]), np.sort(c[k2]))
        assert not np.array_equal(c[k0], c[k1]) and not np.array_equal(c[k1], c[k2]) and not np.array_equal(c[k0], c[k2])
    # both sides of either switch, as labelled
    cl = lc.classify(F9)
    for tag in ("", " rotated", " perm 1", " rotated perm 2"):
        assert not cl["gamma_far"][at("triple at switch -1" + tag), 6] and cl["gamma_far"][at("triple at switch +1" + tag), 6]
        assert cl["theta_far"][at("theta pair at switch +1" + tag)].sum() == 3
        assert cl["theta_far"][at("theta pair at switch -1" + tag)].sum() == 2
    # the history puts even rows past yield and odd rows inside, from p_n = 0.1
    Ep, p = lc.special_state(F9, ls.PRM)
    b = ls.branch(F9, Ep, p)
    assert np.array_equal(b["plastic"], np.arange(84) % 2 == 0) and not b["skip"].any()


@pytest.mark.parametrize("k", lc.HISTORY_DRAWS)
def test_histories_stay_within_the_rules(k):
    h = lc.history(k)
    prm = lc.draw(k)
    assert len(h["F"]) == len(lc.HISTORY_SCHEDULE) == 6
    shares = [_within_rules(r, (k, inc)) for inc, r in enumerate(h["ref"])]
    out = h["out"]
    assert all((out[i] <= out[i + 1]).all() for i in range(5)) and out[-1].mean() <= ls.KINK_CAP       # cumulative
    Epn = np.linalg.norm(h["ref"][-1]["Ep"], axis=1)
    lam = [np.sqrt(np.linalg.eigvalsh(np.einsum("nki,nkj->nij", ls.to_matrix(F), ls.to_matrix(F)))) for F in h["F"]]
    print(f"history draw {k}: plastic share per increment {[round(s, 3) for s in shares]}, largest |Ep| {Epn.max():.3f}, p {h['ref'][-1]['p'].max():.3f}, "
          f"stretches {min(x.min() for x in lam):.3f} .. {max(x.max() for x in lam):.3f}")
    assert max(x.max() for x in lam) <= 2.0 * 1.001 and min(x.min() for x in lam) >= 0.5 / 1.001
    assert lam[-1].max() > 1.9
    # points that yield on one side and again on the other: the plastic strain turns round
    rev = h["ref"][1]["plastic"] & h["ref"][4]["plastic"]
    assert rev.mean() > 0.2
    if prm["H0"] <= prm["E"]:
        assert Epn.max() > 0.3 and h["ref"][-1]["p"].max() > 1.0       # a plastic strain of order one
    # the plastic strain is coaxial with nothing: its commutator with C in the last increment
    F = ls.to_matrix(h["F"][-1])
    C = np.einsum("nki,nkj->nij", F, F)
    from oracle import constitutive_np as onp
    Ept = onp.mandel_to_tensor(h["ref"][-2]["Ep"])
    comm = np.abs(C @ Ept - Ept @ C).max(axis=(1, 2)) / (np.abs(C).max(axis=(1, 2)) * np.abs(Ept).max(axis=(1, 2)) + 1e-300)
    assert np.median(comm) > 0.01
    _branch_rules(np.vstack(h["F"]), f"history draw {k}", mixed=True)


# ---- five sweeps suffice ----------------------------------------------------------------------------------------------------------
def test_five_sweeps_suffice():
    Fs = [batch_of(k)[1][0] for k in range(lc.N_DRAWS)] + [lc.mixed_prm_batch()[0], lc.special_F()[0], ls.degenerate_F()[0]]
    Fs += [np.vstack(lc.history(k)["F"]) for k in lc.HISTORY_DRAWS] + [ls.random_F(4099, seed=1)]
    F = ls.to_matrix(np.vstack(Fs))
    C = np.einsum("nki,nkj->nij", F, F)
    c, V, off = lc.jacobi_np(C)
    w = np.linalg.eigvalsh(C)
    dev = np.abs(np.sort(c, axis=1) - w).max(axis=1) / w.max(axis=1)
    orth = np.abs(np.einsum("nki,nkj->nij", V, V) - np.eye(3)).max(axis=(1, 2))
    rec = np.abs(np.einsum("nia,na,nja->nij", V, c, V) - C).max(axis=(1, 2)) / w.max(axis=1)
    off4 = lc.jacobi_np(C, sweeps=4)[2]
    print(f"Jacobi over {len(C)} matrices: off-diagonal left after five sweeps {off.max():.2e} (after four {off4.max():.2e}), eigenvalues vs eigvalsh "
          f"{dev.max():.2e}, V^T V - 1 {orth.max():.2e}, V c V^T - C {rec.max():.2e}")
    assert off.max() <= JACOBI_OFF
    assert dev.max() <= JACOBI_EIG and orth.max() <= JACOBI_EIG and rec.max() <= JACOBI_EIG


# ---- the tangent against central differences --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_tangent_matches_central_differences_of_the_stress(k):
    """The step is reasoned as in ``test_log_strain_cpu.py`` -- rounding eps |stress error| / h against truncation h^2 |A'''| / 6 -- but
    here the trial elastic strain is of the size of the yield strain ey = R_n / E, not of the stretch: the plastic moduli (beta = dp /
    seq, n x n) vary over ey, so |A'''| ~ |A| / ey^2, while the stress carries the rounding of the Hencky strain, eps L |A| with
    L = 1/2 + ln(amp): the eigenvalues of C are rounded relative to themselves, which is eps / 2 in their logarithm however small that
    is, and the logarithm relative to itself.  With x = h / ey the two are eps L / (x ey) and x^2 / 6: smallest at
    x = (3 eps L / ey)^(1/3), where their sum is 1.04 q, q = (eps L / ey)^(2/3).  The bound is 16 q per point (the margin the floors above get), and not below the
    2.5e-9 of the existing test.  Points whose branch differs between the centre and any of the 18 displaced evaluations are left
    out (the difference quotient straddles the kink there); they are few."""
    prm = lc.draw(k)
    N = 120
    worst, kept, total = 0.0, 0, 0
    for amp in lc.AMPS:
        F, Ep, p = lc.stretch_case(k, N, amp, seed=2)
        r = ls.update(F, Ep, p, **prm)
        ey = np.minimum((prm["s0"] + prm["H0"] * p) / prm["E"], 1.0)
        L = 0.5 + np.log(amp)
        h = ey * (3.0 * EPS * L / ey) ** (1.0 / 3.0)
        tol = np.maximum(16.0 * (EPS * L / ey) ** (2.0 / 3.0), 2.5e-9)
        A = np.empty((N, 9, 9))
        same = np.ones(N, dtype=bool)
        for col in range(9):
            Fp, Fm = F.copy(), F.copy()
            Fp[:, col] += h
            Fm[:, col] -= h
            rp, rm = ls.update(Fp, Ep, p, **prm), ls.update(Fm, Ep, p, **prm)
            A[:, :, col] = (rp["P"] - rm["P"]) / (Fp[:, col] - Fm[:, col])[:, None]
            same &= (rp["plastic"] == r["plastic"]) & (rm["plastic"] == r["plastic"])
        err = np.abs(A - r["A"]).max(axis=(1, 2)) / np.abs(r["A"]).max(axis=(1, 2))
        rel = (err / tol)[same]
        print(f"draw {k} amp {amp:g}: tangent vs central differences {err[same].max():.2e}, {rel.max():.3f} of the bound ({same.sum()} of {N} points)")
        worst, kept, total = max(worst, rel.max()), kept + int(same.sum()), total + N
        assert r["plastic"][same].any() and not r["plastic"][same].all()
    assert kept >= 0.9 * total
    assert worst <= 1.0


# ---- the comparison with the fixture can fail --------------------------------------------------------------------------------------
def _wrong_pairing(ca, ck, cb):
    """``ls.gamma`` with its quotient taken over the wrong gap: (ln[hi, mid] - ln[mid, lo]) / (hi - mid)."""
    ca, ck, cb = (np.asarray(x, dtype=np.float64) for x in np.broadcast_arrays(ca, ck, cb))
    right = _GAMMA(ca, ck, cb)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sort(np.stack([ca, ck, cb]), axis=0)
        lo, mid, hi = s[0], s[1], s[2]
        wrong = (ls.theta(hi, mid) - ls.theta(mid, lo)) / (hi - mid)
        m = (ca + ck + cb) / 3.0
        small = np.abs(np.stack([ca, ck, cb]) - m).max(axis=0) / m <= ls.GAMMA_SWITCH
    distinct = (lo < mid) & (mid < hi)
    return np.where(distinct & ~small, wrong, right)


_GAMMA = ls.gamma


def test_a_wrong_quotient_fails_the_fixture(fx, monkeypatch):
    """Only the (0, 1, 2) call has three distinct arguments: a restatement that is wrong there alone (one entry of G^) misses every
    stratum's floor at the points that take the quotient, in the tangent and nowhere else."""
    monkeypatch.setattr(ls, "gamma", _wrong_pairing)
    figs = floor_figures(fx)
    for name, e in figs.items():
        print(f"with the wrong quotient, {name}: " + " ".join(f"{q} {v:.2e}" for q, v in e.items()))
        assert e["A"] > 1e3 * BOUNDS[name], (name, e)
        assert max(e["P"], e["eel"], e["p"], e["Ep"]) <= FLOOR[name]


def test_a_dropped_term_of_G_fails_the_fixture(fx, monkeypatch):
    """The restatement without the d_il M_jik term of G^ (its last einsum)."""
    real = np.einsum

    def einsum(spec, *ops, **kw):
        out = real(spec, *ops, **kw)
        return 0.0 * out if spec == "il,njik->nijkl" else out

    monkeypatch.setattr(ls.np, "einsum", einsum)
    figs = floor_figures(fx)
    monkeypatch.undo()
    for name, e in figs.items():
        assert e["A"] > 1e3 * BOUNDS[name], (name, e)
