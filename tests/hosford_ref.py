"""Numpy restatement of the Hosford plasticity law with linear hardening (``DXM_LAW_HOSFORD_LINEAR``), written from the equations of
``include/dxmat.h`` / DESIGN.md and deliberately formulated differently from ``csrc/hosford.hip``:

* the kernel iterates on 3 principal deviatoric stresses + dp; :func:`update` runs a tensor-space Newton on the 7 unknowns
  (eps_el (6, Mandel), dp) and takes the tangent from the linearised system, ``Ct = D (J^-1)[:6, :6]``;
* the kernel treats repeated eigenvalues with a sinh series; here the divided difference of the flow direction is
  ``|y|^(m-1) expm1(m t) / expm1(t)``, ``t = log1p((|x| - |y|) / |y|)``.

:func:`update_mp` is the same update in ``mpmath`` (50 digits): the principal problem solved with ``findroot`` (numerical Jacobian, none
of the derivative formulas above), the tangent by central differences of that stress.  TEST INFRASTRUCTURE ONLY.

State convention of the engine: the strain handed in is the total strain, the state that drives the update is the plastic strain;
``eps_el = eps - eps_p``."""
import numpy as np

SQ2 = np.sqrt(2.0)
CLASSES = ("generic", "elastic", "below", "above", "uniaxial", "uniaxial_near", "volumetric", "zero")
EXPONENTS = (2.0, 4.0, 6.0, 10.0, 20.0)
PROPS = dict(E=70e3, nu=0.3, R0=200.0, H=10.0)   # the parameters the convergence domain was established with


def lame(E, nu):
    return E * nu / (1 + nu) / (1 - 2 * nu), E / 2 / (1 + nu)


def to_tensor(v):
    v = np.asarray(v)
    t = np.empty(v.shape[:-1] + (3, 3))
    t[..., 0, 0], t[..., 1, 1], t[..., 2, 2] = v[..., 0], v[..., 1], v[..., 2]
    t[..., 0, 1] = t[..., 1, 0] = v[..., 3] / SQ2
    t[..., 0, 2] = t[..., 2, 0] = v[..., 4] / SQ2
    t[..., 1, 2] = t[..., 2, 1] = v[..., 5] / SQ2
    return t


def to_mandel(t):
    return np.stack([t[..., 0, 0], t[..., 1, 1], t[..., 2, 2], SQ2 * t[..., 0, 1], SQ2 * t[..., 0, 2], SQ2 * t[..., 1, 2]], axis=-1)


def elastic_matrix(E, nu):
    lam, mu = lame(E, nu)
    D = 2 * mu * np.eye(6)
    D[:3, :3] += lam
    return D


def hosford_principal(s, a):
    """seq (N,), n = d seq / d s (N, 3), d n / d s (N, 3, 3) of principal stresses s (N, 3); powers of differences scaled by the
    largest one."""
    d = np.stack([s[:, 0] - s[:, 1], s[:, 1] - s[:, 2], s[:, 0] - s[:, 2]], axis=1)
    dmax = np.abs(d).max(axis=1)
    safe = np.where(dmax > 0, dmax, 1.0)
    x = d / safe[:, None]
    ax = np.abs(x)
    phi = 0.5 * (ax ** a).sum(axis=1)
    phi = np.where(dmax > 0, phi, 1.0)
    seq = dmax * phi ** (1.0 / a)
    r = ax / (phi ** (1.0 / a))[:, None]                    # |d_k| / seq
    g = 0.5 * np.sign(x) * r ** (a - 1.0)
    h = 0.5 * r ** (a - 2.0)
    B = np.array([[1.0, -1.0, 0.0], [0.0, 1.0, -1.0], [1.0, 0.0, -1.0]])
    n = g @ B
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = (a - 1.0) / seq[:, None, None] * (np.einsum("ki,nk,kj->nij", B, h, B) - n[:, :, None] * n[:, None, :])
    return seq, n, dn, d, x, r


def _dd_pow(x, y, m):
    """(sgn(x) |x|^m - sgn(y) |y|^m) / (x - y) elementwise, without cancellation (module docstring)."""
    ax, ay = np.abs(x), np.abs(y)
    big, small = np.maximum(ax, ay), np.minimum(ax, ay)
    same = x * y > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        opposite = (ax ** m + ay ** m) / (ax + ay)
        t = np.log1p((big - small) / small)
        tc = np.minimum(t, 0.5)
        ratio = np.where(tc > 0, np.expm1(m * tc) / np.expm1(tc), m)
        close = np.where(t <= 0.5, small ** (m - 1.0) * ratio, (big ** m - small ** m) / (big - small))   # far apart: the plain quotient
    out = np.where(same, close, opposite)
    return np.where((ax == 0) & (ay == 0), 0.0, out)


def flow(sig, a):
    """seq (N,), n (N, 6) and d n / d sigma (N, 6, 6) of Mandel stresses sig (N, 6)."""
    w, Q = np.linalg.eigh(to_tensor(sig))
    seq, n3, dn3, d, x, r = hosford_principal(w, a)
    N = sig.shape[0]
    Ev = np.stack([to_mandel(Q[:, :, i, None] * Q[:, None, :, i]) for i in range(3)], axis=1)            # (N, 3, 6)
    n = np.einsum("ni,nik->nk", n3, Ev)
    dn = np.einsum("nij,nik,njl->nkl", dn3, Ev, Ev)
    # (n_i - n_j) / (s_i - s_j) for the pairs (0,1), (1,2), (0,2): 2 g_k / d_k plus the divided difference over the two other differences
    m = a - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = 1.0 / seq                                                                              # r = |d| / seq: rho has units 1 / stress
        rs = np.stack([d[:, 0], d[:, 1], d[:, 2]], axis=1) * scale[:, None]                            # signed ratios
        own = np.abs(rs) ** (a - 2.0)
        dd = np.stack([_dd_pow(rs[:, 2], rs[:, 1], m), _dd_pow(rs[:, 2], rs[:, 0], m), _dd_pow(rs[:, 0], -rs[:, 1], m)], axis=1)
        rho = scale[:, None] * (own + 0.5 * dd)
    for k, (i, j) in enumerate(((0, 1), (1, 2), (0, 2))):
        Mij = to_mandel((Q[:, :, i, None] * Q[:, None, :, j] + Q[:, :, j, None] * Q[:, None, :, i]) / SQ2)
        dn += rho[:, k, None, None] * Mij[:, :, None] * Mij[:, None, :]
    return seq, n, dn


def _deviatoric_stress(e, mu):
    """2 mu dev(e): what the flow functions are evaluated on.  seq, n and dn/dsigma depend on the deviator alone; formed from the strain,
    it carries no rounding of the hydrostatic part, which at nu -> 0.5 is far larger (kappa tr / R0 ~ 1e3 stalls the iteration at its
    tolerance of 1e-14 R0 otherwise)."""
    d = e.copy()
    d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
    return 2 * mu * d


def update(eps, ep_n, p_n, E, nu, R0, H, a, maxit=25, rtol=1e-14):
    """One implicit update of N points.  Returns a dict: sig (N, 6), eel (N, 6), ep (N, 6), p (N,), Ct (N, 6, 6), plastic (N,) bool,
    iters (N,), converged (N,) bool, f_trial (N,)."""
    eps, ep_n, p_n = np.atleast_2d(eps).astype(float), np.atleast_2d(ep_n).astype(float), np.atleast_1d(p_n).astype(float)
    N = eps.shape[0]
    lam, mu = lame(E, nu)
    D = elastic_matrix(E, nu)
    e = eps - ep_n
    seq_tr = flow(_deviatoric_stress(e, mu), a)[0] if N else np.zeros(0)
    f_tr = seq_tr - (R0 + H * p_n)
    plastic = f_tr > 0
    eel, dp = e.copy(), np.zeros(N)
    Ct = np.broadcast_to(D, (N, 6, 6)).copy()
    iters = np.zeros(N, dtype=int)
    converged = np.ones(N, dtype=bool)
    idx = np.flatnonzero(plastic)
    if idx.size:
        et, pn = e[idx], p_n[idx]
        x_e, x_p = et.copy(), np.zeros(idx.size)
        tol = np.maximum(rtol * max(abs(R0), 2e-8 * mu), rtol * seq_tr[idx])
        it = np.zeros(idx.size, dtype=int)
        done = np.zeros(idx.size, dtype=bool)
        ok = np.zeros(idx.size, dtype=bool)
        Jinv = np.zeros((idx.size, 7, 7))
        while not done.all():
            act = np.flatnonzero(~done)
            seq, n, dn = flow(_deviatoric_stress(x_e[act], mu), a)
            r_e = x_e[act] - et[act] + x_p[act, None] * n
            r_p = seq - R0 - H * (pn[act] + x_p[act])
            J = np.zeros((act.size, 7, 7))
            J[:, :6, :6] = np.eye(6) + x_p[act, None, None] * (dn @ D)
            J[:, :6, 6] = n
            J[:, 6, :6] = (n @ D) / (2 * mu)
            J[:, 6, 6] = -H / (2 * mu)
            with np.errstate(all="ignore"):
                res = np.maximum(np.abs(2 * mu * r_e).max(axis=1), np.abs(r_p))
                good = res <= tol[act]
                bad = ~np.isfinite(res)
                stop = good | bad | (it[act] >= maxit)
                Ji = np.linalg.inv(np.where(np.isfinite(J), J, 0.0) + np.where(bad, 1.0, 0.0)[:, None, None] * np.eye(7))
            Jinv[act[stop]] = Ji[stop]
            ok[act[good]] = True
            done[act[stop]] = True
            go = ~stop
            step = np.einsum("nij,nj->ni", Ji[go], np.concatenate([r_e[go], (r_p[go] / (2 * mu))[:, None]], axis=1))
            x_e[act[go]] -= step[:, :6]
            x_p[act[go]] -= step[:, 6]
            it[act[go]] += 1
        eel[idx], dp[idx] = x_e, x_p
        Ct[idx] = np.einsum("ij,njk->nik", D, Jinv[:, :6, :6])
        iters[idx], converged[idx] = it, ok
    sig = eel @ D
    return dict(sig=sig, eel=eel, ep=eps - eel, p=p_n + dp, Ct=Ct, plastic=plastic, iters=iters, converged=converged, f_trial=f_tr)


# ---- 50-digit version ------------------------------------------------------------------------------------------------------------
def _mp_stress(mp, e6, pn, E, nu, R0, H, a, principal=False):
    """(sig (6), dp, f_trial) of one trial elastic strain e6 (list of mpf, Mandel); ``principal``: also (s, w, Q), the principal deviatoric
    stresses, the eigenvalues of the trial strain and their eigenvectors."""
    lam = E * nu / (1 + nu) / (1 - 2 * nu)
    mu = E / 2 / (1 + nu)
    r2 = mp.sqrt(2)
    T = mp.matrix([[e6[0], e6[3] / r2, e6[4] / r2], [e6[3] / r2, e6[1], e6[5] / r2], [e6[4] / r2, e6[5] / r2, e6[2]]])
    tr = e6[0] + e6[1] + e6[2]
    w, Q = mp.eigsy(T)
    t = [2 * mu * (w[i] - tr / 3) for i in range(3)]

    def seq_of(s):
        d = [abs(s[0] - s[1]), abs(s[1] - s[2]), abs(s[0] - s[2])]
        dm = max(d)
        if dm == 0:
            return mp.mpf(0)
        return dm * (sum((x / dm) ** a for x in d) / 2) ** (1 / a)

    def grad_of(s):
        q = seq_of(s)
        d = [s[0] - s[1], s[1] - s[2], s[0] - s[2]]
        g = [mp.sign(x) * (abs(x) / q) ** (a - 1) / 2 for x in d]
        return [g[0] + g[2], g[1] - g[0], -g[1] - g[2]]

    f = seq_of(t) - (R0 + H * pn)
    if f <= 0:
        s, dp = t, mp.mpf(0)
    else:
        def F(s0, s1, s2, dp):
            s_ = [s0, s1, s2]
            n = grad_of(s_)
            return [(s_[i] - t[i]) / (2 * mu) + dp * n[i] for i in range(3)] + [(seq_of(s_) - R0 - H * (pn + dp)) / (2 * mu)]
        x = mp.findroot(F, (t[0], t[1], t[2], mp.mpf(0)), tol=mp.mpf(10) ** (-80), maxsteps=60)
        s, dp = [x[0], x[1], x[2]], x[3]
    kap = lam + 2 * mu / 3
    S = mp.zeros(3, 3)
    for i in range(3):
        S += (s[i] + kap * tr) * (Q[:, i] * Q[:, i].T)
    sig = [S[0, 0], S[1, 1], S[2, 2], r2 * S[0, 1], r2 * S[0, 2], r2 * S[1, 2]]
    return (sig, dp, f, s, w, Q) if principal else (sig, dp, f)


def _mp_tangent_analytic(mp, e6, pn, E, nu, R0, H, a):
    """The consistent tangent (6 x 6 mpmath matrix) from the derivative formulas, evaluated at the 50-digit solution -- no differences:
    principal block lambda 1x1 + 2 mu A^-1 - 4 mu^2 z z^T / (2 mu n.z + H), A = I + 2 mu dp dn/ds, z = A^-1 n; shear moduli
    (s_i - s_j) / (2 mu (w_i - w_j)) 2 mu, at exactly repeated trial eigenvalues their limit 2 mu / (1 + 2 mu dp (dn_ii - dn_ij))."""
    lam = E * nu / (1 + nu) / (1 - 2 * nu)
    mu = E / 2 / (1 + nu)
    sig, dp, f, s, w, Q = _mp_stress(mp, e6, pn, E, nu, R0, H, a, principal=True)
    one = mp.matrix([1, 1, 1])
    if f <= 0:
        P, th = lam * one * one.T + 2 * mu * mp.eye(3), {k: 2 * mu for k in ((0, 1), (0, 2), (1, 2))}
    else:
        d = [s[0] - s[1], s[1] - s[2], s[0] - s[2]]
        dm = max(abs(x) for x in d)
        q = dm * (sum((abs(x) / dm) ** a for x in d) / 2) ** (1 / a)
        r = [abs(x) / q for x in d]
        g = mp.matrix([mp.sign(x) * y ** (a - 1) / 2 for x, y in zip(d, r)])
        h = mp.diag([(y ** (a - 2) if y > 0 else mp.mpf(1 if a == 2 else 0)) / 2 for y in r])
        B = mp.matrix([[1, -1, 0], [0, 1, -1], [1, 0, -1]])
        n = B.T * g
        dn = (a - 1) / q * (B.T * h * B - n * n.T)
        Ai = (mp.eye(3) + 2 * mu * dp * dn) ** -1
        z = Ai * n
        P = lam * one * one.T + 2 * mu * Ai - 4 * mu * mu * z * z.T / (2 * mu * (n.T * z)[0] + H)
        th = {(i, j): (s[i] - s[j]) / (w[i] - w[j]) if w[i] != w[j] else 2 * mu / (1 + 2 * mu * dp * (dn[i, i] - dn[i, j])) for i, j in ((0, 1), (0, 2), (1, 2))}
    r2 = mp.sqrt(2)
    mandel = lambda T: mp.matrix([T[0, 0], T[1, 1], T[2, 2], r2 * T[0, 1], r2 * T[0, 2], r2 * T[1, 2]])   # noqa: E731
    Ev = [mandel(Q[:, i] * Q[:, i].T) for i in range(3)]
    Ct = mp.zeros(6, 6)
    for i in range(3):
        for j in range(3):
            Ct += P[i, j] * Ev[i] * Ev[j].T
    for (i, j), t in th.items():
        M = mandel((Q[:, i] * Q[:, j].T + Q[:, j] * Q[:, i].T) / r2)
        Ct += t * M * M.T
    return Ct


def update_mp(eps, ep_n, p_n, E, nu, R0, H, a, tangent=True, dps=50, rel_step=1e-20):
    """The update of ONE point in 50-digit arithmetic; returns float64 arrays sig (6), eel (6), p, Ct (6, 6) and plastic.  ``tangent``:
    True for central differences of the 50-digit stress with the relative step ``rel_step``, "analytic" for the derivative formulas
    evaluated at the 50-digit solution (:func:`_mp_tangent_analytic`).

    Where the differences stop being trusted: for an exponent 2 < a < 3 at a trial state with exactly repeated eigenvalues (uniaxial
    loading).  The tangent is continuous there but only Hoelder continuous -- dn/ds carries |s_i - s_j|^(a-2) -- so a central
    difference of step h is off by O(h^(a-2)): at a = 2.5, 3e-11 of the tangent with the default step and 3e-7 with 1e-12, while
    ``update`` agrees with the analytic 50-digit tangent to 1e-15.  Next to such a state (a relative gap of 1e-12) it is the other way
    round: the differences are exact, and every float64 evaluation, ``update`` included, is off by about (a - 2) gap^(a-3) x the
    rounding of the gap, 7e-11 there (``test_law_fuzz_cpu.py::test_hosford_tangent_between_exponents_2_and_3``).  For a = 2 and a >= 3 the
    default step is good to better than 1e-14 everywhere."""
    import mpmath

    mp = mpmath.mp
    old = mp.dps
    mp.dps = dps
    try:
        E, nu, R0, H, a = (mp.mpf(float(v)) for v in (E, nu, R0, H, a))
        e = [mp.mpf(float(x)) - mp.mpf(float(y)) for x, y in zip(eps, ep_n)]
        pn = mp.mpf(float(p_n))
        sig, dp, f = _mp_stress(mp, e, pn, E, nu, R0, H, a)
        lam = E * nu / (1 + nu) / (1 - 2 * nu)
        mu = E / 2 / (1 + nu)
        trs = sig[0] + sig[1] + sig[2]
        eel = [(sig[i] - trs / 3) / (2 * mu) + trs / (3 * (3 * lam + 2 * mu)) if i < 3 else sig[i] / (2 * mu) for i in range(6)]
        Ct = np.zeros((6, 6))
        if tangent == "analytic":
            Cm = _mp_tangent_analytic(mp, e, pn, E, nu, R0, H, a)
            Ct = np.array([[float(Cm[i, j]) for j in range(6)] for i in range(6)])
        elif tangent:
            scale = max(abs(x) for x in e) or mp.mpf(1)
            hstep = scale * mp.mpf(float(rel_step))
            for j in range(6):
                ep_, em_ = list(e), list(e)
                ep_[j] += hstep
                em_[j] -= hstep
                sp = _mp_stress(mp, ep_, pn, E, nu, R0, H, a)[0]
                sm = _mp_stress(mp, em_, pn, E, nu, R0, H, a)[0]
                for i in range(6):
                    Ct[i, j] = float((sp[i] - sm[i]) / (2 * hstep))
        return dict(sig=np.array([float(x) for x in sig]), eel=np.array([float(x) for x in eel]), p=float(pn + dp), Ct=Ct, plastic=bool(f > 0))
    finally:
        mp.dps = old


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def max_overshoot(a):
    """The tested convergence domain of plain Newton from the trial state: seq_trial / R <= 3 for a <= 10, <= 1.5 for a = 20."""
    return 3.0 if a <= 10.0 else 1.5


def _rotations(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    return q * np.sign(np.einsum("nii->ni", r))[:, None, :]


def make_inputs(cls, n, a, seed, E=PROPS["E"], nu=PROPS["nu"], R0=PROPS["R0"], H=PROPS["H"], trivial_state=False):
    """(eps (n, 6), ep_n (n, 6), p_n (n,)) of one input class: the trial elastic strain eps - ep_n has the class's property."""
    rng = np.random.default_rng(seed)
    lam, mu = lame(E, nu)
    if cls == "zero":
        return np.zeros((n, 6)), np.zeros((n, 6)), np.zeros(n)
    p_n = np.zeros(n) if trivial_state else rng.uniform(0.0, 0.02, n)
    ep_n = np.zeros((n, 6))
    if not trivial_state:
        d = to_tensor(rng.standard_normal((n, 6)))
        d -= np.einsum("nii->n", d)[:, None, None] / 3 * np.eye(3)
        ep_n = to_mandel(d) * 1e-3
    R = R0 + H * p_n
    vol = rng.uniform(-1e-3, 1e-3, n)
    if cls == "volumetric":
        e = np.zeros((n, 6))
        e[:, :3] = vol[:, None]
        return ep_n + e, ep_n, p_n
    if cls in ("uniaxial", "uniaxial_near"):
        pr = np.tile(np.array([2.0, -1.0, -1.0]), (n, 1)) * rng.choice([-1.0, 1.0], n)[:, None]
        if cls == "uniaxial_near":
            pr[:, 2] *= 1.0 + 1e-12
    else:
        pr = rng.standard_normal((n, 3))
        pr -= pr.mean(axis=1)[:, None]
    ratio = {"elastic": rng.uniform(0.1, 0.9, n), "below": np.full(n, 1 - 1e-6), "above": np.full(n, 1 + 1e-6)}.get(
        cls, rng.uniform(1.05, max_overshoot(a), n))
    seq = hosford_principal(2 * mu * pr, a)[0]
    pr = pr * (ratio * R / seq)[:, None]
    if cls == "uniaxial":     # axis-aligned: two trial eigenvalues are EXACTLY equal
        e = np.zeros((n, 6))
        ax = rng.integers(0, 3, n)
        for k in range(3):
            e[:, k] = np.where(ax == k, pr[:, 0], pr[:, 1])
        e[:, :3] += vol[:, None]
    else:
        Q = _rotations(rng, n)
        T = np.einsum("nik,nk,njk->nij", Q, pr + vol[:, None], Q)
        e = to_mandel(T)
    if cls == "uniaxial":
        # the state must not break the exact degeneracy of eps - ep_n: an axis-aligned old plastic strain with the same pair equal
        ep_n = np.zeros((n, 6)) if trivial_state else np.where(np.arange(6)[None, :] < 3, 0.0, 0.0) * ep_n
    return ep_n + e, ep_n, p_n


def mixed_inputs(n, a, seed, trivial_state=False, **props):
    """n points cycling through every class (what the GPU parity tests run); ``props``: E, nu, R0, H other than ``PROPS``."""
    per = [make_inputs(c, (n + len(CLASSES) - 1 - k) // len(CLASSES), a, seed + 17 * k, trivial_state=trivial_state, **props) for k, c in enumerate(CLASSES)]
    eps, ep, p = (np.concatenate([x[i] for x in per]) for i in range(3))
    perm = np.random.default_rng(seed + 999).permutation(eps.shape[0])
    return eps[perm], ep[perm], p[perm]
