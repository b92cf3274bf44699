"""Inputs of the parameter-space sweep of the two plane-strain kernels that are not their 3-D law with fewer columns: plane-strain
Hosford (law 40, ``hosford_plane.hip``) and plane-strain Ogden (law 38, ``ogden_plane.hip``).  Shared by
``test_plane_law_fuzz_cpu.py`` (which pins the references and these inputs), ``test_gpu_fuzz_plane_laws.py`` (which holds the kernels to
them) and ``golden/make_plane_law_fuzz_bounds.py`` (which measures the bounds).  TEST INFRASTRUCTURE ONLY.

The material constants are the draws of ``law_fuzz.py`` (``draw_hosford``, ``draw_ogden``: its docstring states the ranges), the
sizes, seeds, amplitudes and the kink rule are its too; what is new here are the 4-wide histories and the 5-wide deformation
gradients, both built in the plane so that every row has its property exactly."""
import functools

import numpy as np

import hosford_plane_ref as hp
import hosford_ref as hr
import ogden_plane_ref as op
import ogden_ref as og
from dolfinx_materials_amd.conventions import embed_plane_strain
from law_fuzz import (HOSFORD_INCREMENTS, HOSFORD_SEEDS, KINK, KINK_CAP, MP_SAMPLE, N_POINTS, OGDEN_AMPS, OGDEN_SEEDS,  # noqa: F401
                      draw_hosford, draw_ogden, hosford_sample, sample_rows)
from log_strain_plane_ref import rot_z

SERIES_SWITCH = 0.1       # max(|m h|, |h|) <= 0.1: the series form of a divided difference (hyperelastic.hip, hosford.hip)
OGDEN_E0 = 2e-13          # test_ogden_cpu.E0 (asserted equal by test_plane_law_fuzz_cpu.py)
OGDEN_CONDITION_CAP = OGDEN_E0 / (4.0 * np.finfo(np.float64).eps)      # K J / |P| of a row: see plane_ogden_F


# ---- Hosford -------------------------------------------------------------------------------------------------------------------
def _seq4(v4, a):
    """seq of (n, 4) plane stresses, on the embedding."""
    return hr.flow(embed_plane_strain(v4), a)[0]


def _unit_plane_deviatoric(rng, n, mu, a):
    """Random deviatoric PLANE strain directions d (n, 4) with seq(2 mu d) = 1 on the embedding: three principal values, the third
    along z, the other two turned by an in-plane angle."""
    pr = rng.standard_normal((n, 3))
    pr -= pr.mean(axis=1, keepdims=True)
    d = hp.plane_vector(pr[:, 0], pr[:, 1], pr[:, 2], rng.uniform(0.0, np.pi, n))
    return d / _seq4(2 * mu * d, a)[:, None]


def _unit_pure_shear(rng, n, mu, a):
    """Deviatoric plane directions [m, m, -2 m, sqrt(2) h] with seq(2 mu d) = 1: d_xx == d_yy to the bit and a shear, so the
    principal axes of the in-plane block sit at exactly 45 degrees."""
    m, h = rng.standard_normal(n), rng.standard_normal(n)
    h = np.where(np.abs(h) < 0.05, 0.05, h)
    d = np.stack([m, m, -2.0 * m, hp.SQ2 * h], axis=1)
    d = d / _seq4(2 * mu * d, a)[:, None]
    assert np.array_equal(d[:, 0], d[:, 1]) and (d[:, 3] != 0.0).all()
    return d


def plane_hosford_history(seed, n, params):
    """Four increments of n points, 4 wide ``[xx, yy, zz, sqrt(2) xy]``, from a non-trivial state: the plane analogue of
    ``law_fuzz.hosford_history``.  Returns a dict: ``ep0`` (n, 4), ``p0`` (n,), ``eps`` (four (n, 4) total strains), ``ref`` (the four
    results of ``hosford_plane_ref.update``, each from the state the one before left), ``skip`` (four (n,) bool: within KINK R0 of the
    yield kink), ``overshoot`` (four floats: the largest seq_trial / R).

    Increment 1: ``hosford_plane_ref.mixed_inputs`` at the draw's constants, every input class of ``hosford_plane_ref.CLASSES``.
    Increment 2: a step against the current deviatoric stress that leaves seq_trial = |t| R, t in U(-0.8, 0.9 max_overshoot): most
    points unload into the elastic domain, those with t > 1 yield again on the opposite side.  Rows that carry no deviatoric stress
    (the classes ``zero`` and ``volumetric``: their strain and state have xx == yy to the bit and no plastic strain) step along a
    random plane direction instead -- every other one of them along a pure in-plane shear ``[m, m, -2 m, sqrt(2) h]``, which leaves
    the trial deviator with t_xx == t_yy EXACTLY and a shear: the one place where the kernel's closed-form rotation is at 45 degrees
    to the bit (``shear45`` (n,) bool marks these rows).  Increments 3 and 4: a random plane deviatoric direction (three principal
    values and an in-plane angle, ``hosford_plane_ref.plane_vector``) of size U(0, 0.95 (max_overshoot - 1)) R / (2 mu) and a
    volumetric strain of +-R0 / E.  seq is a norm, so from a state with seq <= R the next trial state has seq_trial <= max_overshoot
    R: every step stays inside the stated convergence domain of the local Newton, which is asserted."""
    return _plane_hosford_history(seed, n, tuple(params))


@functools.lru_cache(maxsize=None)
def _plane_hosford_history(seed, n, params):
    E, nu, R0, H, a = params
    mu = hr.lame(E, nu)[1]
    mo = hr.max_overshoot(a)
    rng = np.random.default_rng(7500 + seed)
    eps, ep, p = hp.mixed_inputs(n, a, seed=7100 + seed, E=E, nu=nu, R0=R0, H=H)
    out = dict(ep0=ep, p0=p, eps=[], ref=[], skip=[], overshoot=[], shear45=np.zeros(n, dtype=bool))
    for inc in range(HOSFORD_INCREMENTS):
        if inc > 0:
            last = out["ref"][-1]
            R = R0 + H * last["p"]
            s = last["sig"].copy()
            s[:, :3] -= s[:, :3].mean(axis=1, keepdims=True)
            seq = _seq4(last["sig"], a)
            rnd = _unit_plane_deviatoric(rng, n, mu, a)
            if inc == 1:
                t = rng.uniform(-0.8, 0.9 * mo, n)
                has = seq > 1e-6 * R
                free = ~has & (eps[:, 0] == eps[:, 1]) & (eps[:, 3] == 0.0) & ~last["ep"].any(axis=1)
                pure = free & (np.cumsum(free) % 2 == 1)
                rnd = np.where(pure[:, None], _unit_pure_shear(rng, n, mu, a), rnd)
                out["shear45"] = pure
                back = -s / np.where(has, seq, 1.0)[:, None] / (2 * mu)           # seq(2 mu back) = 1
                step = np.where(has[:, None], back * (seq + t * R)[:, None], rnd * (np.abs(t) * R)[:, None])
            else:
                step = rnd * (rng.uniform(0.0, 0.95 * (mo - 1.0), n) * R)[:, None]
                step[:, :3] += (rng.choice([-1.0, 1.0], n) * R0 / E)[:, None]
            eps = eps + step
            ep, p = last["ep"], last["p"]
        r = hp.update(eps, ep, p, E, nu, R0, H, a)
        over = float(((r["f_trial"] + R0 + H * p) / (R0 + H * p)).max())
        assert over <= mo * (1.0 + 1e-9), (seed, inc, over, mo)
        out["eps"].append(eps)
        out["ref"].append(r)
        out["skip"].append(np.abs(r["f_trial"]) <= KINK * R0)
        out["overshoot"].append(over)
    for v in out["eps"] + [out["ep0"], out["p0"], out["shear45"]] + [x for r in out["ref"] for x in r.values() if isinstance(x, np.ndarray)]:
        v.setflags(write=False)          # shared between tests: computed once, left unchanged
    return out


def plane_hosford_classes(seed, n):
    """(n,) the index into ``hosford_plane_ref.CLASSES`` of every row of increment 1: ``mixed_inputs`` lays the classes out one after the
    other and permutes the rows; this is that layout under that permutation."""
    m = len(hp.CLASSES)
    labels = np.concatenate([np.full((n + m - 1 - k) // m, k) for k in range(m)])
    return labels[np.random.default_rng(7100 + seed + 999).permutation(n)]


def plane_hosford_state_before(hist, inc):
    """(ep, p) increment ``inc`` (0-based) starts from."""
    return (hist["ep0"], hist["p0"]) if inc == 0 else (hist["ref"][inc - 1]["ep"], hist["ref"][inc - 1]["p"])


def plane_hosford_rotation(hist, inc):
    """What the kernel's closed-form rotation sees in increment ``inc``: (d, t01) of the trial elastic strain e = eps - ep_n, d =
    e_yy - e_xx and t01 = e_xy (both up to the factor 2 mu).  d == 0 and t01 != 0: 45 degrees; t01 == 0: zero shear, no rotation."""
    e = hist["eps"][inc] - plane_hosford_state_before(hist, inc)[0]
    return e[:, 1] - e[:, 0], e[:, 3] / hp.SQ2


def plane_hosford_paths(sig4, a):
    """Per row, which form of the ONE divided difference law 40 keeps would evaluate at the stress ``sig4`` (n, 4): (series, quotient,
    opposite) bool.  With q0, q1 the in-plane principal deviatoric stresses and q2 = s_zz, the difference is taken over x3 = q0 - q2
    and x2 = q1 - q2: of opposite sign (q2 between the in-plane pair) the sum form, of one sign the series where
    max(|m h|, |h|) <= 0.1, m = a - 1, h = (ln |x3| - ln |x2|) / 2, and the plain quotient otherwise.  Rows without a deviator are in
    none of the three."""
    s = np.array(sig4, dtype=np.float64)
    s[:, :3] -= s[:, :3].mean(axis=1, keepdims=True)
    mean, half = 0.5 * (s[:, 0] + s[:, 1]), np.hypot(0.5 * (s[:, 0] - s[:, 1]), s[:, 3] / hp.SQ2)
    x3, x2 = (mean + half) - s[:, 2], (mean - half) - s[:, 2]
    some = (np.abs(x3) > 0.0) | (np.abs(x2) > 0.0)
    same = x3 * x2 > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        h = 0.5 * (np.log(np.abs(x3)) - np.log(np.abs(x2)))
    near = np.maximum(np.abs((a - 1.0) * h), np.abs(h)) <= SERIES_SWITCH
    return some & same & near, some & same & ~near, some & ~same


def plane_hosford_deviation(seed, n=N_POINTS):
    """(state, tangent): the largest deviation (``hosford_plane_ref.errors``) of ``hosford_plane_ref.update`` from ``update_mp`` over the
    seed's sample of MP_SAMPLE (increment, point) pairs; the plastic flag has to agree."""
    prm = draw_hosford(seed)
    E, nu, R0, H, a = prm
    hist = plane_hosford_history(seed, n, prm)
    dev_s = dev_c = 0.0
    for inc, k in hosford_sample(seed, n):
        r = hist["ref"][inc]
        ep, p = plane_hosford_state_before(hist, inc)
        if hist["skip"][inc][k]:
            continue
        m = hp.update_mp(hist["eps"][inc][k], ep[k], p[k], E, nu, R0, H, a)
        assert m["plastic"] == bool(r["plastic"][k]), (prm, inc, k)
        es, ec = hp.errors({q: r[q][k:k + 1] for q in ("sig", "eel", "p", "Ct")}, {q: np.asarray(m[q])[None] for q in ("sig", "eel", "p", "Ct")}, E, R0)
        dev_s, dev_c = max(dev_s, es[0]), max(dev_c, ec[0])
    return float(dev_s), float(dev_c)


# ---- Ogden ---------------------------------------------------------------------------------------------------------------------
def plane_ogden_amp(seed):
    return OGDEN_AMPS[seed % len(OGDEN_AMPS)]


def plane_ogden_kinds(seed, n):
    """What ``plane_ogden_F`` made of every row: dict(inplane, to_c2, aligned (n,) bool, gap (n,))."""
    rng = np.random.default_rng(8500 + seed)
    kind = rng.integers(0, 8, n)
    gap = np.asarray(og.GAPS)[rng.integers(0, len(og.GAPS), n)]
    inplane, to_c2 = kind <= 1, kind == 2
    aligned = (inplane | to_c2) & (rng.integers(0, 2, n) == 0)
    return dict(inplane=inplane, to_c2=to_c2, aligned=aligned, gap=gap)


def _stretches(rng, n, amp, k):
    lam = np.exp(rng.uniform(-np.log(amp), np.log(amp), (n, 3)))
    rep = k["inplane"] | k["to_c2"]
    lam[rep] = np.minimum(lam[rep], amp / np.sqrt(1.0 + 2.0 * max(og.GAPS)))    # the gap stays inside [1 / amp, amp]
    lam[k["inplane"], 1] = lam[k["inplane"], 0] * np.sqrt(1.0 + k["gap"][k["inplane"]])
    lam[k["to_c2"], 2] = lam[k["to_c2"], 0] * np.sqrt(1.0 + k["gap"][k["to_c2"]])
    return lam


def plane_ogden_conditioning(F5, P, K):
    """K J / max |P| per row: how many times the rounding of J = det F (a relative error of the order of eps, whatever evaluates it)
    shows in the row's stress RELATIVE TO THE ROW, through the pressure K (J - 1) J."""
    F5 = np.asarray(F5, dtype=np.float64)
    J = F5[:, 2] * (F5[:, 0] * F5[:, 1] - F5[:, 3] * F5[:, 4])
    return K * J / np.abs(P).max(axis=1)


def plane_ogden_F(seed, n, amp):
    """(n, 5) rows ``[F00, F11, F22, F01, F10]`` of F = R_z U, det F > 0: U = Q_z diag(lam) Q_z^T with principal stretches log-uniform
    in [1 / amp, amp], the third along z; R_z and Q_z rotations about z by angles in U(0, 2 pi).  Three rows in eight have a nearly
    repeated pair of eigenvalues of C = F^T F at a relative gap from ``ogden_ref.GAPS``: a quarter of all rows the in-plane pair
    (c0, c0 (1 + gap)), an eighth c2 = c0 (1 + gap); every other one of those is axis-aligned with R = Q = I, where gap 0 is exact in
    floating point.

    NARROWED, by the draw's own constants (``draw_ogden(seed)``): a row whose stress nearly cancels while K is large -- J within
    1e-4 of 1 next to a small isochoric stress -- carries the rounding of J, K J eps, at K J / |P| times eps of the row's own size.
    That is the conditioning of the law in this error measure, not of a formulation: the two float64 restatements, whose J differ
    by an ulp, are then K J eps / |P| apart (measured: 2.7e-13 and 4.7e-13 on one row each of seeds 6 and 7, against
    ``test_ogden_cpu.E0`` = 2e-13; every other row of the eight seeds agrees to 1.5e-13).  Rows with
    ``K J / |P| > OGDEN_CONDITION_CAP`` = E0 / (4 eps) -- two formulations, each with up to 2 eps on J -- have their stretches drawn
    again, kind, gap and angles kept (``plane_ogden_redrawn`` counts them: 94 of the 32 792 rows of the eight seeds, 60 of them at seed 4 -- K / mu = 273 at stretches
    within 10 % of 1), after which the two restatements agree to 6.5e-14."""
    return _plane_ogden_F(seed, n, amp)[0]


def plane_ogden_redrawn(seed, n, amp):
    """How many rows of ``plane_ogden_F`` had their stretches drawn again."""
    return _plane_ogden_F(seed, n, amp)[1]


@functools.lru_cache(maxsize=None)
def _plane_ogden_F(seed, n, amp):
    k = plane_ogden_kinds(seed, n)
    prm = draw_ogden(seed)
    rng = np.random.default_rng(8600 + seed)
    lam = _stretches(rng, n, amp, k)
    tq, tr = rng.uniform(0.0, 2 * np.pi, n), rng.uniform(0.0, 2 * np.pi, n)
    Q, R = rot_z(tq), rot_z(tr)
    Q[k["aligned"]] = np.eye(3)
    R[k["aligned"]] = np.eye(3)
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(16):
        F = R @ np.einsum("nik,nk,njk->nij", Q, lam, Q)
        F5 = np.ascontiguousarray(np.stack([F[:, 0, 0], F[:, 1, 1], F[:, 2, 2], F[:, 0, 1], F[:, 1, 0]], axis=1))
        bad = plane_ogden_conditioning(F5, op.restricted_closed_form(F5, **prm)[0], prm["K"]) > OGDEN_CONDITION_CAP
        if not bad.any():
            break
        redrawn |= bad
        lam[bad] = _stretches(rng, n, amp, k)[bad]
    assert not bad.any()
    assert (np.linalg.det(F) > 0.0).all()
    assert not F[:, :2, 2].any() and not F[:, 2, :2].any()        # a plane deformation gradient: nothing for the 5 columns to drop
    F5.setflags(write=False)
    return F5, int(redrawn.sum())


def plane_ogden_inplane_pair(F5):
    """(c0, c1), c0 >= c1: the eigenvalues of the 2 x 2 block of C = F^T F, the smaller one from c0 c1 = (det of the block)^2, without
    the cancellation of mean - half."""
    F5 = np.asarray(F5, dtype=np.float64)
    app, aqq = F5[:, 0] ** 2 + F5[:, 4] ** 2, F5[:, 1] ** 2 + F5[:, 3] ** 2
    apq = F5[:, 0] * F5[:, 3] + F5[:, 4] * F5[:, 1]
    c0 = 0.5 * (app + aqq) + np.hypot(0.5 * (app - aqq), apq)
    return c0, (F5[:, 0] * F5[:, 1] - F5[:, 3] * F5[:, 4]) ** 2 / c0


def plane_ogden_paths(F5, alpha):
    """(series, quotient): (n,) bool, the side of the switch ``max(|m h|, |h|) <= 0.1``, m = alpha / 2 - 1, h = (ln c0 - ln c1) / 2, on
    which the in-plane pair (c0, c1) of eigenvalues of the 2 x 2 block of C sits: the one divided difference ``ogden_plane.hip``
    evaluates, with the switch it copies from ``hyperelastic.hip``."""
    c0, c1 = plane_ogden_inplane_pair(F5)
    h = 0.5 * (np.log(c0) - np.log(c1))
    ser = np.maximum(np.abs((alpha / 2.0 - 1.0) * h), np.abs(h)) <= SERIES_SWITCH
    return ser, ~ser


def plane_ogden_mp(F5_row, alpha, mu, K):
    """(P (5), A (5, 5), PK2Stress (4)) of ONE row: ``ogden_ref.closed_form_mp`` on the embedded F, restricted with ``IDX``."""
    P9, A99, isv6 = og.closed_form_mp(op.embed(F5_row)[0], alpha, mu, K)
    idx = list(op.IDX)
    return P9[idx], A99[idx][:, idx], isv6[:4]


def plane_ogden_sample(seed, n, series):
    """MP_SAMPLE rows: half of them from the series side of the switch, half from the quotient side."""
    return np.union1d(sample_rows(seed, n, series)[: MP_SAMPLE // 2], sample_rows(seed + 100, n, ~series)[: MP_SAMPLE - MP_SAMPLE // 2])


def plane_ogden_deviation(seed, n=N_POINTS):
    """The largest deviation (P, A, PK2Stress; ``ogden_plane_ref.errors``) of ``ogden_plane_ref.restricted_closed_form`` from the
    60-digit closed form on the embedded F over the seed's sample."""
    prm = draw_ogden(seed)
    F = plane_ogden_F(seed, n, plane_ogden_amp(seed))
    rows = plane_ogden_sample(seed, n, plane_ogden_paths(F, prm["alpha"])[0])
    got = op.restricted_closed_form(F[rows], **prm)
    want = tuple(np.array(x) for x in zip(*(plane_ogden_mp(F[k], **prm) for k in rows)))
    return float(max(op.errors(got, want)))
