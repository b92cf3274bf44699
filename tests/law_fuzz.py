"""Random material constants and inputs for the parameter-space sweeps of the Hosford, Ogden and Ramberg-Osgood laws: shared by
``test_law_fuzz_cpu.py`` (which pins the references over these ranges), ``test_gpu_fuzz_laws.py`` (which holds the kernels to them)
and ``golden/make_law_fuzz_bounds.py`` (which measures the bounds).  TEST INFRASTRUCTURE ONLY.

Ranges (the same elastic ranges as ``test_gpu_fuzz.py``):

* Hosford: E = 10^U(3, 5.5), nu in [0, 0.49] (two draws in five sit on the ends), R0 / E = 10^U(-4, -2), H = 0 for every third draw
  and U(0, 0.5) E otherwise, a cycling through ``HOSFORD_EXPONENTS`` (exponents strictly between 2 and 3 are left out: the tangent
  is ill-conditioned there, ``test_law_fuzz_cpu.py::test_hosford_tangent_between_exponents_2_and_3``);
* Ogden: alpha = +-exp(U(ln 1, ln 30)), mu = 10^U(2, 5), K / mu = 10^U(0.5, 3.5), F = R U with principal stretches log-uniform in
  [1 / amp, amp], amp cycling through ``OGDEN_AMPS`` (up to 2);
* Ramberg-Osgood: E and nu as above, sig0 / E = 10^U(-4, -2), alpha = 10^U(-2, 1), n cycling through ``RO_EXPONENTS``."""
import functools

import numpy as np

import hosford_ref as hr
import ogden_ref as og

N_POINTS = 4099                        # 64 full tiles of 64 and a ragged tail of 3
HOSFORD_SEEDS = tuple(range(10))
OGDEN_SEEDS = tuple(range(8))
RO_SEEDS = tuple(range(8))
HOSFORD_EXPONENTS = (2.0, 3.0, 4.0, 6.0, 8.0, 10.0, 14.0, 20.0)
HOSFORD_INCREMENTS = 4
KINK = 1e-9                            # |f_trial| <= KINK R0: either branch is right, the point is not compared
KINK_CAP = 1e-4                        # the share of such points an increment may have
OGDEN_AMPS = (1.1, 1.3, 1.6, 2.0)
RO_EXPONENTS = (1.0, 1.5, 5.0, 20.0, 100.0)
RO_FIXED_YIELD_STRAIN = 500.0 / 100e3  # sig0 / E of the fixed parameter set the strain family was written for
MP_SAMPLE = 10                         # points per seed compared with the high-precision versions


def _elastic(rng, seed):
    E = float(10 ** rng.uniform(3, 5.5))
    nu = float(rng.uniform(0.0, 0.49))
    return E, {1: 0.49, 2: 0.0}.get(seed % 5, nu)


# ---- Hosford -------------------------------------------------------------------------------------------------------------------
def draw_hosford(seed):
    """(E, nu, R0, H, a) of draw ``seed``."""
    rng = np.random.default_rng(3000 + seed)
    E, nu = _elastic(rng, seed)
    R0 = E * float(10 ** rng.uniform(-4, -2))
    H = float(rng.uniform(0.0, 0.5)) * E
    return E, nu, R0, (0.0 if seed % 3 == 0 else H), HOSFORD_EXPONENTS[seed % len(HOSFORD_EXPONENTS)]


def _unit_deviatoric(rng, n, mu, a):
    """Random deviatoric strain directions d (n, 6) with seq(2 mu d) = 1."""
    d = rng.standard_normal((n, 6))
    d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
    return d / hr.flow(2 * mu * d, a)[0][:, None]


def hosford_history(seed, n, params):
    """Four increments of n points from a non-trivial state.  Returns a dict: ``ep0`` (n, 6), ``p0`` (n,), ``eps`` (four (n, 6) total
    strains), ``ref`` (the four results of ``hosford_ref.update``, each from the state the one before left), ``skip`` (four (n,) bool:
    within KINK R0 of the yield kink), ``overshoot`` (four floats: the largest seq_trial / R).

    Increment 1: every input class of ``hosford_ref.CLASSES``.  Increment 2: a step against the current deviatoric stress that
    leaves seq_trial = |t| R, t in U(-0.8, 0.9 max_overshoot): most points unload into the elastic domain, those with t > 1 yield again
    on the opposite side.  Increments 3 and 4: a random deviatoric direction of size U(0, 0.95 (max_overshoot - 1)) R / (2 mu) and a
    volumetric strain of +-R0 / E.  seq is a norm, so from a state with seq <= R the next trial state has seq_trial <= max_overshoot R:
    every step stays inside the stated convergence domain of the local Newton, which is asserted."""
    return _hosford_history(seed, n, tuple(params))


@functools.lru_cache(maxsize=None)
def _hosford_history(seed, n, params):
    E, nu, R0, H, a = params
    mu = hr.lame(E, nu)[1]
    mo = hr.max_overshoot(a)
    rng = np.random.default_rng(3500 + seed)
    eps, ep, p = hr.mixed_inputs(n, a, seed=3100 + seed, E=E, nu=nu, R0=R0, H=H)
    out = dict(ep0=ep, p0=p, eps=[], ref=[], skip=[], overshoot=[])
    for inc in range(HOSFORD_INCREMENTS):
        if inc > 0:
            last = out["ref"][-1]
            R = R0 + H * last["p"]
            s = last["sig"].copy()
            s[:, :3] -= s[:, :3].mean(axis=1, keepdims=True)
            seq = hr.flow(last["sig"], a)[0]
            rnd = _unit_deviatoric(rng, n, mu, a)
            if inc == 1:
                t = rng.uniform(-0.8, 0.9 * mo, n)
                has = seq > 1e-6 * R
                back = -s / np.where(has, seq, 1.0)[:, None] / (2 * mu)           # seq(2 mu back) = 1
                step = np.where(has[:, None], back * (seq + t * R)[:, None], rnd * (np.abs(t) * R)[:, None])
            else:
                step = rnd * (rng.uniform(0.0, 0.95 * (mo - 1.0), n) * R)[:, None]
                step[:, :3] += (rng.choice([-1.0, 1.0], n) * R0 / E)[:, None]
            eps = eps + step
            ep, p = last["ep"], last["p"]
        r = hr.update(eps, ep, p, E, nu, R0, H, a)
        over = float(((r["f_trial"] + R0 + H * p) / (R0 + H * p)).max())
        assert over <= mo * (1.0 + 1e-9), (seed, inc, over, mo)
        out["eps"].append(eps)
        out["ref"].append(r)
        out["skip"].append(np.abs(r["f_trial"]) <= KINK * R0)
        out["overshoot"].append(over)
    for v in out["eps"] + [out["ep0"], out["p0"]] + [x for r in out["ref"] for x in r.values()]:
        v.setflags(write=False)          # shared between tests: computed once, left unchanged
    return out


def hosford_errors(got, ref, E, R0):
    """Per-row deviations (stress, elastic strain, p, tangent) with the row scaling of ``test_gpu_hosford.compare``."""
    n = ref["sig"].shape[0]
    sc = np.maximum(np.abs(ref["sig"]).max(axis=1), R0)
    es = np.abs(got["sig"] - ref["sig"]).max(axis=1) / sc
    ee = E * np.abs(got["eel"] - ref["eel"]).max(axis=1) / sc
    ep = E * np.abs(got["p"] - ref["p"]) / sc
    ct = np.abs(got["Ct"] - ref["Ct"]).reshape(n, 36).max(axis=1) / np.abs(ref["Ct"]).reshape(n, 36).max(axis=1)
    return es, ee, ep, ct


def hosford_sample(seed, n):
    """MP_SAMPLE (increment, point) pairs of a history."""
    rng = np.random.default_rng(3900 + seed)
    return [(int(rng.integers(0, HOSFORD_INCREMENTS)), int(rng.integers(0, n))) for _ in range(MP_SAMPLE)]


# ---- Ogden ---------------------------------------------------------------------------------------------------------------------
def draw_ogden(seed):
    """dict(alpha, mu, K) of draw ``seed``; the sign of alpha alternates."""
    rng = np.random.default_rng(4000 + seed)
    alpha = float(np.exp(rng.uniform(0.0, np.log(30.0)))) * (1.0 if seed % 2 == 0 else -1.0)
    mu = float(10 ** rng.uniform(2, 5))
    return dict(alpha=alpha, mu=mu, K=mu * float(10 ** rng.uniform(0.5, 3.5)))


def _proper_rotations(rng, n):
    Q = hr._rotations(rng, n)
    return Q * np.sign(np.linalg.det(Q))[:, None, None]


def ogden_F(seed, n, amp):
    """(n, 9) deformation gradients F = R U, det F > 0: U with principal stretches log-uniform in [1 / amp, amp] on random axes, R a
    random rotation.  Three rows in eight have repeated eigenvalues of C = F^T F up to a relative gap from ``ogden_ref.GAPS``: a
    quarter two-fold (c1, c2, c2 (1 + gap)), an eighth three-fold (c, c (1 + gap), c (1 + 2 gap)); every other one of those is
    axis-aligned with R = I, where gap 0 is exact in floating point."""
    rng = np.random.default_rng(4500 + seed)
    lam = np.exp(rng.uniform(-np.log(amp), np.log(amp), (n, 3)))
    kind = rng.integers(0, 8, n)
    gap = np.asarray(og.GAPS)[rng.integers(0, len(og.GAPS), n)]
    two, three = kind <= 1, kind == 2
    lam[two | three] = np.minimum(lam[two | three], amp / np.sqrt(1.0 + 2.0 * max(og.GAPS)))    # the gap stays inside [1 / amp, amp]
    lam[two, 2] = lam[two, 1] * np.sqrt(1.0 + gap[two])
    lam[three, 1] = lam[three, 0] * np.sqrt(1.0 + gap[three])
    lam[three, 2] = lam[three, 0] * np.sqrt(1.0 + 2.0 * gap[three])
    Q, R = _proper_rotations(rng, n), _proper_rotations(rng, n)
    aligned = (two | three) & (rng.integers(0, 2, n) == 0)
    Q[aligned] = np.eye(3)
    R[aligned] = np.eye(3)
    F = R @ np.einsum("nik,nk,njk->nij", Q, lam, Q)
    assert (np.linalg.det(F) > 0.0).all()
    return og.to_vector(F)


def ogden_paths(F9, alpha):
    """(series, quotient): (n,) bool, whether a row has a pair of eigenvalues on that side of the divided difference's switch
    ``max(|m h|, |h|) <= 0.1``, m = alpha / 2 - 1, h = (ln c_i - ln c_j) / 2."""
    F = og.to_matrix(F9)
    l = np.log(np.linalg.eigvalsh(np.einsum("nki,nkj->nij", F, F)))
    h = 0.5 * np.stack([l[:, 0] - l[:, 1], l[:, 0] - l[:, 2], l[:, 1] - l[:, 2]], axis=1)
    ser = np.maximum(np.abs((alpha / 2.0 - 1.0) * h), np.abs(h)) <= 0.1
    return ser.any(axis=1), (~ser).any(axis=1)


def ogden_errors(got, want):
    """Per-point deviations (P, A, PK2Stress) with the scaling of ``test_gpu_ogden.check``."""
    n = len(want[0])
    eP = og.row_errors(np.asarray(got[0])[:, None, :], want[0][:, None, :])[:, 0]
    eA = og.row_errors(np.asarray(got[1]).reshape(n, 9, 9), want[1]).max(axis=1)
    scale = np.maximum(np.abs(want[2]).max(axis=1), np.abs(want[0]).max(axis=1))
    scale = np.where(scale > 0.0, scale, 1.0)
    return eP, eA, np.abs(np.asarray(got[2]) - want[2]).max(axis=1) / scale


# ---- Ramberg-Osgood ------------------------------------------------------------------------------------------------------------
def draw_ramberg_osgood(seed):
    """(E, nu, sig0, alpha, n) of draw ``seed``, the argument order of ``ramberg_osgood_ref.update``."""
    rng = np.random.default_rng(5000 + seed)
    E, nu = _elastic(rng, seed)
    sig0 = E * float(10 ** rng.uniform(-4, -2))
    return E, nu, sig0, float(10 ** rng.uniform(-2, 1)), RO_EXPONENTS[seed % len(RO_EXPONENTS)]


def ramberg_osgood_strains(N, seed, scale=1.0):
    """eps_e log-uniform over scale x (1e-14 ... 3e-1) with a volumetric part, plus zero rows, purely volumetric rows and rows just
    below and above the threshold e_eps = 1e-12 (an absolute strain: not scaled).  ``scale`` = (sig0 / E) / RO_FIXED_YIELD_STRAIN
    keeps the family where it was relative to the knee of the curve."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((N, 6))
    d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
    d /= np.linalg.norm(d, axis=1, keepdims=True) * np.sqrt(2.0 / 3.0)
    ee = np.exp(rng.uniform(np.log(1e-14), np.log(3e-1), N))
    eps = d * (scale * ee)[:, None]
    eps[:, :3] += (scale * ee * rng.uniform(-1.0, 1.0, N))[:, None]
    k = rng.integers(0, 6, N)
    eps[k == 0] = 0.0                                         # zero rows
    vol = k == 1
    eps[vol] = 0.0
    eps[vol, :3] = scale * rng.uniform(-1e-2, 1e-2, vol.sum())[:, None]   # purely volumetric
    near = k == 2
    eps[near] = d[near] * rng.choice([0.5e-12, 0.9e-12, 1.1e-12, 2e-12], near.sum())[:, None]
    return eps


def ramberg_osgood_inputs(seed, n):
    prm = draw_ramberg_osgood(seed)
    return prm, ramberg_osgood_strains(n, 5500 + seed, scale=(prm[2] / prm[0]) / RO_FIXED_YIELD_STRAIN)


def ramberg_osgood_mp(eps6, E, nu, sig0, alpha, n, dps=50):
    """Stress (6) and the .mfront tangent (6, 6) of ONE strain in mpmath: the law reduces to the scalar equation
    ``x / (3 mu) + beta (x / sig0)^n = eps_e`` for the equivalent stress x (``ramberg_osgood_ref.update`` states the rest)."""
    import mpmath as mp

    import ramberg_osgood_ref as ro

    with mp.workdps(dps):
        E, nu, sig0, alpha, n = (mp.mpf(float(v)) for v in (E, nu, sig0, alpha, n))
        mu, K, beta = E / 2 / (1 + nu), E / (3 * (1 - 2 * nu)), alpha * sig0 / E
        e = [mp.mpf(float(v)) for v in eps6]
        tr = e[0] + e[1] + e[2]
        d = [e[i] - tr / 3 if i < 3 else e[i] for i in range(6)]
        eq = mp.sqrt(mp.mpf(2) / 3 * sum(v * v for v in d))
        one = [1, 1, 1, 0, 0, 0]
        P = [[(1 if i == j else 0) - mp.mpf(one[i] * one[j]) / 3 for j in range(6)] for i in range(6)]
        if eq < ro.E_EPS:
            sig = [K * tr * one[i] + 2 * mu * d[i] for i in range(6)]
            Ct = [[K * one[i] * one[j] + 2 * mu * P[i][j] for j in range(6)] for i in range(6)]
        else:
            f = lambda x: x / (3 * mu) + beta * (x / sig0) ** n - eq   # noqa: E731
            x0 = min(3 * mu * eq, sig0 * (eq / beta) ** (1 / n))
            x = mp.findroot(f, x0, tol=mp.mpf(10) ** (-2 * dps + 20), maxsteps=200)
            dse = 1 / max(1 / (3 * mu) + n * beta * (x / sig0) ** n / max(E * ro.E_EPS, x), ro.E_EPS / (3 * mu))
            ne = [2 * v / (3 * eq) for v in d]
            sig = [K * tr * one[i] + x * ne[i] for i in range(6)]
            Ct = [[K * one[i] * one[j] + dse * ne[i] * ne[j] + x / eq * (mp.mpf(2) / 3 * P[i][j] - ne[i] * ne[j]) for j in range(6)] for i in range(6)]
        return np.array([float(v) for v in sig]), np.array([[float(v) for v in row] for row in Ct])


def ramberg_osgood_errors(sig, ct, ref_sig, ref_ct):
    """Per-row deviations (stress, tangent) with the scaling of ``test_gpu_ramberg_osgood.check_against_ref``."""
    srow = np.maximum(np.abs(ref_sig).max(axis=1), 1e-300)
    cscale = np.abs(ref_ct).max(axis=(1, 2))
    return np.abs(sig - ref_sig).max(axis=1) / srow, np.abs(np.asarray(ct).reshape(-1, 6, 6) - ref_ct).max(axis=(1, 2)) / cscale


def sample_rows(seed, n, want=None):
    """MP_SAMPLE row indices, drawn from the rows ``want`` (bool) marks if given."""
    rng = np.random.default_rng(6000 + seed)
    pool = np.arange(n) if want is None else np.flatnonzero(want)
    return np.sort(rng.choice(pool, size=min(MP_SAMPLE, pool.size), replace=False))


# ---- deviation of each restatement from its high-precision version on the sample of one seed ---------------------------------------
def hosford_deviation(seed, n=N_POINTS):
    """(state, tangent): the largest deviation of ``hosford_ref.update`` from ``update_mp`` over the seed's sample."""
    prm = draw_hosford(seed)
    E, nu, R0, H, a = prm
    hist = hosford_history(seed, n, prm)
    dev_s = dev_c = 0.0
    for inc, k in hosford_sample(seed, n):
        r = hist["ref"][inc]
        ep, p = (hist["ep0"], hist["p0"]) if inc == 0 else (hist["ref"][inc - 1]["ep"], hist["ref"][inc - 1]["p"])
        m = hr.update_mp(hist["eps"][inc][k], ep[k], p[k], E, nu, R0, H, a)
        if hist["skip"][inc][k]:
            continue
        assert m["plastic"] == bool(r["plastic"][k]), (prm, inc, k)
        es, ee, epl, ct = hosford_errors({q: r[q][k:k + 1] for q in ("sig", "eel", "p", "Ct")}, {q: np.asarray(m[q])[None] for q in ("sig", "eel", "p", "Ct")}, E, R0)
        dev_s, dev_c = max(dev_s, es[0], ee[0], epl[0]), max(dev_c, ct[0])
    return float(dev_s), float(dev_c)


def ogden_deviation(seed, n=N_POINTS):
    """The largest deviation (P, A, PK2Stress) of ``ogden_ref.closed_form`` from ``closed_form_mp`` over the seed's sample: half of it
    from the rows with (nearly) repeated eigenvalues."""
    prm = draw_ogden(seed)
    F = ogden_F(seed, n, OGDEN_AMPS[seed % len(OGDEN_AMPS)])
    series = ogden_paths(F, prm["alpha"])[0]
    rows = np.union1d(sample_rows(seed, n, series)[: MP_SAMPLE // 2], sample_rows(seed + 100, n, ~series)[: MP_SAMPLE - MP_SAMPLE // 2])
    got = og.closed_form(F[rows], **prm)
    want = [np.array(x) for x in zip(*(og.closed_form_mp(F[k], **prm) for k in rows))]
    return float(max(e.max() for e in ogden_errors(got, want)))


def ramberg_osgood_deviation(seed, n=N_POINTS):
    """(stress, tangent): the largest deviation of ``ramberg_osgood_ref.update`` from :func:`ramberg_osgood_mp` over the seed's
    sample (rows that run the local Newton)."""
    import ramberg_osgood_ref as ro

    prm, eps = ramberg_osgood_inputs(seed, n)
    r = ro.update(eps, *prm)
    rows = sample_rows(seed, n, r["newton"])
    want = [ramberg_osgood_mp(eps[k], *prm) for k in rows]
    es, ec = ramberg_osgood_errors(r["sig"][rows], r["Ct_mfront"][rows], np.array([w[0] for w in want]), np.array([w[1] for w in want]))
    return float(es.max()), float(ec.max())
