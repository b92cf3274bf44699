"""Seeded parameters and inputs for the sweep of plane-stress J2 plasticity with isotropic hardening (DXM_LAW_PS_J2_LINEAR = 30,
DXM_LAW_PS_J2_VOCE = 31): shared by ``test_plane_stress_j2_sweep_cpu.py`` (which pins the restatement and the rules of the inputs
over them), ``test_gpu_plane_stress_j2_sweep.py`` (which holds ``plane_stress_j2_kernel`` to them) and
``golden/make_plane_stress_j2_sweep.py`` (the 50-digit values).  TEST INFRASTRUCTURE ONLY: nothing here touches a GPU.

* :func:`draw`: twelve parameter sets per law, the existing case first: E = 10^U(3, 11.5); nu = 0.4999, 0.49, 0, -0.5, -0.9 on
  draws 1 .. 5 and U(0, 0.45) otherwise; sig0 / E = 10^U(-4, -1.5).  Linear: H = 0 on draws 3, 6, 9, U(0, 0.5) E otherwise,
  10 E on draw 7 and 1e-6 on draw 8.  Voce: sigu / sig0 in (1, 10], b = 10^U(-3, 6), sigu = sig0 on draw 7.  Draws 10 and 11
  soften: H = -E / 70 and -1e-5 E; (sig0, sigu, b) = (500, 350, 100) s with E = 70e3 s at s = 1 and s = 1e5.
* :func:`points`: the one-increment inputs of a draw, from a drawn old state.
* :func:`history`: six increments from the virgin state, for three draws per law.
* :func:`special_rows`: inputs whose answer is known in closed form.

Strain, stress and ``epsp`` are ``[xx, yy, sqrt(2) xy]``; parameters are the lists the library takes, [E, nu, sig0, H] and
[E, nu, sig0, sigu, b]."""
import functools
import os

import numpy as np

import plane_stress_j2_ref as pj

LAWS = (pj.J2_LINEAR, pj.J2_VOCE)
NAME = {pj.J2_LINEAR: "linear", pj.J2_VOCE: "voce"}
N_DRAWS = 12
SOFTENING = (10, 11)
FORCED_NU = {1: 0.4999, 2: 0.49, 3: 0.0, 4: -0.5, 5: -0.9}
HISTORY_DRAWS = {pj.J2_LINEAR: (0, 3, 10), pj.J2_VOCE: (0, 7, 10)}      # the existing case, a perfectly plastic draw, a softening draw
N_STATE, N_OVER, N_HISTORY = 40, 30, 40
OFF = 1e-6                        # of sig0: the least distance of a trial from the surface
P_OLD = 10.0                      # p_n = U(0, 0.5) 20 sig0 / E
OVER_HARD, OVER_SOFT = 1e4, 12.0  # the far end of the log-uniform overshoots.  Softening: the issue's limit is 20; at p_n up to
#                                   10 sig0 / E an equibiaxial trial at overshoot o adds up to 2 (1 - nu) o sig0 / E to p, and
#                                   H = -E / 70 is to keep R >= 0.5 sig0: 12 leaves R >= (1 - (10 + 24) / 70) sig0 at nu = 0
R_FLOOR = 0.5                     # of sig0: what every returned state of a softening draw keeps
#: of the amplitude, along (v1, v2): grows, grows, unloads, reverses past yield on the other side, turns into a new in-plane
#: direction, reloads beyond the first peak
HISTORY_SCHEDULE = ((0.5, 0.0), (0.9, 0.0), (0.55, 0.0), (-0.8, 0.0), (-0.3, 0.9), (1.3, 0.4))
HISTORY_DRIVEN = 0.55             # share of the points that follow the schedule in an increment; the others rest inside the surface
AMP_HARD, AMP_SOFT = 8.0, 3.0     # the amplitude is log-uniform in [1.5, AMP] sig0 (of the elastic stress of the strain)
GOLDEN = os.path.join(os.path.dirname(pj.GOLDEN), "plane_stress_j2_sweep.npz")

# the largest deviation of the restatement from the 50-digit sweep fixture per law over every draw, history and increment: stress in
# sig0, tangent in E, p and epsp in sig0 / E, as tests/test_plane_stress_j2_sweep_cpu.py measures and pins it, rounded up to two
# digits.  The GPU tests allow the kernel 16 times as much and never less than 2e-14, the rule of plane_stress_j2_ref.gpu_bounds
# (linear: the H = 10 E draw at overshoot 1e4 sets stress and state -- R there is 1e4 sig0, 7e-11 is 7e-15 of it; Voce: the far
# overshoots set the state, as in plane_stress_j2_ref.MEASURED, and the stress stays near sigu, where nothing cancels)
MEASURED_SWEEP = {pj.J2_LINEAR: (6.9e-11, 4.6e-15, 8.2e-11), pj.J2_VOCE: (3.2e-15, 2.3e-14, 2.3e-11)}


def gpu_bounds(law):
    return tuple(max(16 * m, 2e-14) for m in MEASURED_SWEEP[law])


def draw(law, k):
    """the parameter list of draw ``k`` of ``law``"""
    if k == 0:
        return list(pj.CASES["linear_H5e3" if law == pj.J2_LINEAR else "voce"][1])
    rng = np.random.default_rng(3000 + 100 * law + k)
    E = float(10 ** rng.uniform(3, 11.5))
    nu = FORCED_NU.get(k, float(rng.uniform(0.0, 0.45)))
    sig0 = E * float(10 ** rng.uniform(-4, -1.5))
    h, ratio, b = float(rng.uniform(0.0, 0.5)), 1.0 + 9.0 * (1.0 - float(rng.uniform(0.0, 1.0))), float(10 ** rng.uniform(-3, 6))
    if law == pj.J2_LINEAR:
        H = h * E
        if k % 3 == 0:
            H = 0.0
        H = {7: 10.0 * E, 8: 1e-6, 10: -E / 70.0, 11: -1e-5 * E}.get(k, H)
        return [E, nu, sig0, H]
    if k in SOFTENING:
        s = 1.0 if k == 10 else 1e5
        return [70e3 * s, 0.3 if k == 10 else nu, 500.0 * s, 350.0 * s, 100.0]
    return [E, nu, sig0, sig0 if k == 7 else ratio * sig0, b]


def softening(law, k):
    return k in SOFTENING


def tag(law, k):
    return f"{NAME[law]}{k}"


def unit_directions(rng, n):
    """random in-plane stress directions of unit von Mises norm"""
    v = rng.normal(size=(n, 3))
    return v / pj.seq_of(v)[:, None]


def off_surface(law, prm, eps, epsp_n, p_n):
    """the trial of every row is at least OFF sig0 away from the surface (in double precision, as the generator decides it)"""
    R, _ = pj.hardening(law, prm)
    seq = pj.seq_of((np.asarray(eps) - epsp_n) @ pj.stiffness(prm[0], prm[1]).T)
    return np.abs(seq - R(np.asarray(p_n))) >= OFF * prm[2]


def _from_state(law, prm, rng, n, over):
    """``n`` rows from a drawn old state -- p_n = U(0, 0.5) 20 sig0 / E, epsp_n of that size in a random direction -- whose trial
    lies at ``over(rng, n)`` times R_n along a random in-plane direction; rows nearer the surface than OFF are drawn again"""
    E, nu, sig0 = prm[:3]
    R, _ = pj.hardening(law, prm)
    S = pj.compliance(E, nu)
    eps, ep, p = np.empty((n, 3)), np.empty((n, 3)), np.empty(n)
    todo = np.arange(n)
    while todo.size:
        m = todo.size
        pn = rng.uniform(0.0, 0.5, m) * 2.0 * P_OLD * sig0 / E
        epn = rng.normal(size=(m, 3))
        epn *= (pn / np.linalg.norm(epn, axis=1))[:, None]
        e = epn + (unit_directions(rng, m) * (over(rng, m) * R(pn))[:, None]) @ S.T
        eps[todo], ep[todo], p[todo] = e, epn, pn
        todo = todo[~off_surface(law, prm, e, epn, pn)]
    return eps, ep, p


@functools.lru_cache(maxsize=None)
def points(law, k):
    """(eps, epsp_n, p_n, far) of draw ``k``: N_STATE rows with the trial at U(0, 2) R_n, then N_OVER rows (``far``) at log-uniform
    overshoots from 0.1 to OVER_HARD (OVER_SOFT on a softening draw), both ends present"""
    prm = draw(law, k)
    rng = np.random.default_rng(5000 + 100 * law + k)
    top = OVER_SOFT if softening(law, k) else OVER_HARD

    def far(r, m):
        o = np.exp(r.uniform(np.log(0.1), np.log(top), m))
        if m == N_OVER:
            o[:2] = 1.0001, top
        return o

    a = _from_state(law, prm, rng, N_STATE, lambda r, m: r.uniform(0.0, 2.0, m))
    b = _from_state(law, prm, rng, N_OVER, far)
    eps, ep, p = (np.concatenate([x, y]) for x, y in zip(a, b))
    return eps, ep, p, np.arange(N_STATE + N_OVER) >= N_STATE


@functools.lru_cache(maxsize=None)
def history(law, k, n=N_HISTORY):
    """six (n, 3) strains from the virgin state under draw ``k`` (one of HISTORY_DRAWS).  A *driven* point (probability
    HISTORY_DRIVEN per increment) takes the strain ``S (amp sig0 (c1 v1 + c2 v2))`` of HISTORY_SCHEDULE, v1 and v2 its own two
    directions and amp its own amplitude; a *resting* point is put inside the surface, at U(0, 0.9) R_n from the plastic strain it
    carries, in a random direction.  The state that decides this is the restatement's (``pj.update``), carried along."""
    prm = draw(law, k)
    E, nu, sig0 = prm[:3]
    R, _ = pj.hardening(law, prm)
    S = pj.compliance(E, nu)
    rng = np.random.default_rng(7000 + 100 * law + k)
    v1, v2 = unit_directions(rng, n), unit_directions(rng, n)
    amp = np.exp(rng.uniform(np.log(1.5), np.log(AMP_SOFT if softening(law, k) else AMP_HARD), n)) * sig0
    ep, p, out = np.zeros((n, 3)), np.zeros(n), []
    for c1, c2 in HISTORY_SCHEDULE:
        eps, todo = np.empty((n, 3)), np.arange(n)
        while todo.size:
            m = todo.size
            driven = rng.random(m) < HISTORY_DRIVEN
            ed = ((c1 * v1[todo] + c2 * v2[todo]) * amp[todo, None]) @ S.T
            er = ep[todo] + (unit_directions(rng, m) * (rng.uniform(0.0, 0.9, m) * R(p[todo]))[:, None]) @ S.T
            eps[todo] = np.where(driven[:, None], ed, er)
            todo = todo[~off_surface(law, prm, eps[todo], ep[todo], p[todo])]
        r = pj.update(law, eps, ep, p, prm)
        ep, p = r["epsp"], r["p"]
        out.append(eps)
    return tuple(out)


# ---- rows with a closed form ----------------------------------------------------------------------------------------------------
SQ15 = np.sqrt(1.5)
#: name -> (stress direction d with seq(d) = 1, flow direction m: epsp = p m, so that sig = R(p) d)
MODES = {"uniaxial x": ((1.0, 0.0, 0.0), (1.0, -0.5, 0.0)), "uniaxial y": ((0.0, 1.0, 0.0), (-0.5, 1.0, 0.0)),
         "equibiaxial": ((1.0, 1.0, 0.0), (0.5, 0.5, 0.0)), "pure shear": ((0.0, 0.0, 1.0 / SQ15), (0.0, 0.0, SQ15))}


def special_rows(law, prm, soft=False):
    """dict(eps, epsp_n, p_n, labels, plastic (bool; None where either branch is accepted), stress, p, epsp) of rows whose answer
    needs no root-finder: prescribe the final p, then sig = R(p) d, epsp = p m and eps = C^-1 sig + epsp for the four MODES (the
    flow direction of a proportional path is that of the final stress, so the backward-Euler step is exact).  Per mode: from the
    virgin state to p = 1.5 sig0 / E; from the yielded state p_n = 2 sig0 / E (epsp_n = p_n m) to p = 3.5 sig0 / E; and, on a
    hardening draw, uniaxial x to the overshoot 1e6.  Then the zero strain, and uniaxial trials at R_n (1 -+ 1e-12)."""
    E, nu, sig0 = prm[:3]
    R, _ = pj.hardening(law, prm)
    unit = sig0 / E
    rows = []

    def strain(s):      # C^-1 s, written so that s_xx = s_yy gives eps_xx = eps_yy to the bit
        return np.array([(s[0] - nu * s[1]) / E, (s[1] - nu * s[0]) / E, (1.0 + nu) * s[2] / E])

    def add(label, d, m, p0, p1, plastic=True):
        d, m = np.array(d), np.array(m)
        sig = float(R(np.array(p1))) * d
        rows.append((label, strain(sig) + p1 * m, p0 * m, p0, plastic, sig, p1, p1 * m))

    for name, (d, m) in MODES.items():
        add(name, d, m, 0.0, 1.5 * unit)
        add(name + " from a yielded state", d, m, 2.0 * unit, 3.5 * unit)
    if not soft:
        add("uniaxial x at overshoot 1e6", *MODES["uniaxial x"], 0.0, 1e6 * unit)
    z = np.zeros(3)
    rows.append(("zero strain", z, z, 0.0, False, z, 0.0, z))
    for sgn in (-1.0, 1.0):
        sig = sig0 * (1.0 + sgn * 1e-12) * np.array(MODES["uniaxial x"][0])
        rows.append((f"trial at R_n (1 {sgn:+g}e-12)", strain(sig), z, 0.0, None, sig, 0.0, z))
    cols = list(zip(*rows))
    return dict(labels=list(cols[0]), eps=np.array(cols[1]), epsp_n=np.array(cols[2]), p_n=np.array(cols[3], dtype=float),
                plastic=list(cols[4]), stress=np.array(cols[5]), p=np.array(cols[6], dtype=float), epsp=np.array(cols[7]))


U = 2.0 ** -53


def special_bounds(prm, eps):
    """(stress in sig0, state in sig0 / E) per row: what a float64 evaluation of the closed form can guarantee.  The closed form
    hands the law the strain ``fl(C^-1 sig + epsp)``: a handful of roundings, each at most U of the largest term, so the strain is
    the exact one perturbed by at most 8 U |eps|_max.  The law maps a strain perturbation to stress through its tangent, in norm at
    most that of C, E / (1 - |nu|): 8 U |eps|_max E / (1 - |nu|) of stress.  The state is ``eps - C^-1 s``: the strain perturbation
    plus ``C^-1`` of the stress perturbation, that is (1 + cond C) times it, cond C = (1 + |nu|) / (1 - |nu|).  The update itself adds
    its own roundings on quantities of the same size (t = C (eps - epsp_n), the divisions of the return, eps - C^-1 s: some twenty
    operations, 24 U allowed), hence 32 U in all.  In units of sig0 and sig0 / E with scale = max(|eps|_max E / sig0, 1)."""
    E, nu, sig0 = prm[:3]
    scale = np.maximum(np.abs(eps).max(axis=1) * E / sig0, 1.0)
    stress = 32 * U * scale / (1.0 - abs(nu))
    return stress, stress * (1.0 + (1.0 + abs(nu)) / (1.0 - abs(nu)))


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def load_fixture(path=GOLDEN):
    return np.load(path, allow_pickle=False)


def fixture_draw(fx, law, k):
    """dict(prm, eps, epsp_n, p_n, stress, tangent (n, 9), p, epsp, plastic) of the one-increment points of a draw"""
    t = tag(law, k)
    out = {q: fx[f"{t}_{q}"] for q in ("prm", "eps", "epsp_n", "p_n", "stress", "p", "epsp", "plastic")}
    out["tangent"] = fx[f"{t}_tangent"][:, pj.SLOT]
    return out


def fixture_history(fx, law, k):
    """(prm, six dict(eps, stress, tangent (n, 9), p, epsp, plastic))"""
    t = tag(law, k)
    incs = []
    for q in range(len(HISTORY_SCHEDULE)):
        d = {x: fx[f"{t}_h{q}_{x}"] for x in ("eps", "stress", "p", "epsp", "plastic")}
        d["tangent"] = fx[f"{t}_h{q}_tangent"][:, pj.SLOT]
        incs.append(d)
    return fx[f"{t}_prm"], incs


def state_of(d):
    return np.concatenate([d["p"][:, None], d["epsp"]], axis=1)


# ---- the same draws through the plane-strain laws 27 and 28 ---------------------------------------------------------------------------
N_PLANE_STRAIN = 321


def plane_strain_increments(prm, n=N_PLANE_STRAIN, seed=20):
    """two (n, 4) strains ``[xx, yy, zz, sqrt(2) xy]`` from the virgin state: load, then beyond it in another direction.  The
    deviatoric part puts the trial at U(0, 3) sig0; the volume change is U(-1, 1) sig0 / K, so that the pressure stays of the size
    of sig0 at every nu (a free volume change at nu = 0.4999 would put 1667 E tr(eps) on top of a deviatoric stress of sig0, and
    the error scale of the stress would say nothing about the plastic part)."""
    E, nu, sig0 = prm[:3]
    mu, K = E / 2.0 / (1.0 + nu), E / 3.0 / (1.0 - 2.0 * nu)
    rng = np.random.default_rng(seed)

    def one():
        d = rng.standard_normal((n, 4))
        d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
        d *= (rng.uniform(0.0, 3.0, n) * sig0 / (2.0 * mu * np.sqrt(1.5)) / np.linalg.norm(d, axis=1))[:, None]
        d[:, :3] += (rng.uniform(-1.0, 1.0, n) * sig0 / K / 3.0)[:, None]
        return d

    a, b = one(), one()
    return [a, 1.3 * a + 0.6 * b]


def plane_strain_scales(prm):
    """(stress, tangent, strain) scales of the plane-strain comparison: those of ``test_gpu_plane_strain.py`` -- sig0, E, sig0 / E --
    with one change that is idle at its nu = 0.3: the stress scale is sig0 max(1, lambda / (2 mu)).  The stress is
    lambda tr(e) 1 + 2 mu e; the strains above have entries of sig0 / (2 mu) and a trace 2500 times smaller at nu = 0.4999, so
    tr(e) is known to ulp(sig0 / (2 mu)) only and ONE rounding of it moves the stress by lambda / (2 mu) ulp(sig0) = 2.8e-13 sig0:
    two correct evaluations that sum the trace in another order (the oracle and the restatement do) differ by a few of these,
    1.7e-12 sig0 measured.  lambda / (2 mu) = nu / (1 - 2 nu): 2500 at 0.4999, 24.5 at 0.49, below 1 up to nu = 0.25."""
    E, nu = prm[0], prm[1]
    return prm[2] * max(1.0, nu / (1.0 - 2.0 * nu)), E, prm[2] / E
