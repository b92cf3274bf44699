"""A vectorised numpy restatement of the two plane-stress return mappings (DXM_LAW_PS_QUADRATIC = 23, DXM_LAW_PS_POLYGON = 24;
``csrc/plane_stress.hip``), operation by operation in the kernel's order (numpy rounds every operation, as the kernel's
``fp contract(off)`` does), and the constants ``dxmat.hip::launch_ps_*`` form on the host.  TEST INFRASTRUCTURE ONLY.

Strain and stress are ``[xx, yy, sqrt(2) xy]``; the state is the hidden plastic strain ``eps - C^-1 sigma`` (N, 3)."""
import json
import os

import numpy as np

QUADRATIC, POLYGON = 23, 24
MAX_PLANES = 4
R2 = 0.70710678118654752440
EPS = 2.220446049250313e-16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_stress.npz")
SLOT = (0, 1, 2, 1, 3, 4, 2, 4, 5)   # (row, column) of the row-major 3 x 3 -> slot of (D00, D01, D02, D11, D12, D22)


def stiffness(E, nu):
    """``cvxpy_materials.py:16-18``"""
    return (E / (1 - nu**2)) * np.array([[1.0, nu, 0.0], [nu, 1.0, 0.0], [0.0, 0.0, (1.0 - nu)]])


def compliance(E, nu):
    return np.array([[1.0, -nu, 0.0], [-nu, 1.0, 0.0], [0.0, 0.0, 1.0 + nu]]) / E


def q_matrix(q):
    return np.array([[1.0, -0.5, 0.0], [-0.5, 1.0, 0.0], [0.0, 0.0, q]])


def elastic_constants(E, nu):
    c0 = E / (1.0 - nu * nu)
    return dict(c11=c0, c12=c0 * nu, c33=c0 * (1.0 - nu), E=E, nu=nu, CA=E / (1.0 - nu), CB=E / (1.0 + nu))


def rankine_planes(ft, fc):
    return [(1.0, 0.0, ft), (0.0, 1.0, ft), (-1.0, 0.0, fc), (0.0, -1.0, fc)]


def l1rankine_planes(ft, fc):
    a, b = (1 / ft - 1 / fc) / 2, (1 / ft + 1 / fc) / 2
    return [(1.0, 1.0, ft), (-1.0, -1.0, fc), (a + b, a - b, 1.0), (a - b, a + b, 1.0)]


def polygon_params(E, nu, planes):
    """the 15 numbers of DXM_LAW_PS_POLYGON: the rows past M are zeros"""
    rows = [float(v) for r in planes for v in r]
    return [float(E), float(nu), float(len(planes))] + rows + [0.0] * (3 * MAX_PLANES - len(rows))


def planes_of(prm):
    M = int(prm[2])
    return [tuple(prm[3 + 3 * k: 6 + 3 * k]) for k in range(M)]


def check_polygon(prm):
    """what ``build_ps_polygon`` refuses, as a sentence; None: accepted"""
    E, nu, Mf = prm[0], prm[1], prm[2]
    if not all(np.isfinite(prm[:3])) or not E > 0 or not -1 < nu < 1:
        return "elastic constants"
    if Mf != int(Mf) or not 1 <= int(Mf) <= MAX_PLANES:
        return "the number of half-planes M must be an integer"
    rows = planes_of(prm)
    for k, (n1, n2, d) in enumerate(rows):
        if not all(np.isfinite((n1, n2, d))):
            return "must be finite"
        if not d > 0:
            return "d must be > 0"
        if n1 == 0 and n2 == 0:
            return "zero normal"
    for n1, n2, d in rows:
        if (n2, n1, d) not in rows:
            return "not symmetric under the exchange of the principal stresses"
    return None


def polygon_constants(prm):
    """``dxmat.hip::launch_ps_polygon``: per row (n1, n2, d, w1, w2, n.w, slack), and the admissible vertices"""
    c = elastic_constants(prm[0], prm[1])
    rows = planes_of(prm)
    rec = []
    for n1, n2, d in rows:
        w1 = c["c11"] * n1 + c["c12"] * n2
        w2 = c["c12"] * n1 + c["c11"] * n2
        rec.append((n1, n2, d, w1, w2, n1 * w1 + n2 * w2, (8.0 * EPS) * d))
    verts = []
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            ri, rj = rows[i], rows[j]
            det = ri[0] * rj[1] - ri[1] * rj[0]
            if det == 0.0:
                continue
            x, y = (ri[2] * rj[1] - rj[2] * ri[1]) / det, (ri[0] * rj[2] - rj[0] * ri[2]) / det
            adm = np.isfinite(x) and np.isfinite(y)
            for k, rk in enumerate(rows):
                if k != i and k != j:
                    adm = adm and ((rk[0] * x + rk[1] * y) - rk[2] <= (64.0 * EPS) * rk[2])
            if adm:
                verts.append((x, y))
    return c, rec, verts


def _out(n, c):
    ct = np.empty((n, 6))
    ct[:] = (c["c11"], c["c12"], 0.0, c["c11"], 0.0, c["c33"])
    return ct


def quadratic(eps, epn, prm, maxit=25, rtol=1e-14):
    """[E, nu, sig0, q, tangent]"""
    eps, epn = np.asarray(eps, dtype=np.float64).reshape(-1, 3), np.asarray(epn, dtype=np.float64).reshape(-1, 3)
    E, nu, sig0, QC, tangent = (float(v) for v in prm)
    c = elastic_constants(E, nu)
    CA, CB = c["CA"], c["CB"]
    tol, sig0sq = rtol * sig0, sig0 * sig0
    ka, kb, kc = 0.5 * CA, 1.5 * CB, QC * CB
    kmax = max(max(ka, kb), kc)
    n = len(eps)
    with np.errstate(all="ignore"):
        ee = eps - epn
        ta, tb, tc = CA * ((ee[:, 0] + ee[:, 1]) * R2), CB * ((ee[:, 0] - ee[:, 1]) * R2), CB * ee[:, 2]
        seq = np.sqrt((0.5 * (ta * ta) + 1.5 * (tb * tb)) + QC * (tc * tc))
        plastic = (seq > sig0) & (seq <= np.finfo(float).max)
        sa, sb, sc = ta.copy(), tb.copy(), tc.copy()
        lam = np.where(plastic, (seq / sig0 - 1.0) / kmax, 0.0)
        da, db, dc = np.ones(n), np.ones(n), np.ones(n)
        iters, notconv = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
        act = plastic.copy()
        while act.any():
            i = np.flatnonzero(act)
            l = lam[i]
            a_, b_, c_ = 1.0 / (1.0 + l * ka), 1.0 / (1.0 + l * kb), 1.0 / (1.0 + l * kc)
            xa, xb, xc = ta[i] * a_, tb[i] * b_, tc[i] * c_
            qa, qb, qc = 0.5 * (xa * xa), 1.5 * (xb * xb), QC * (xc * xc)
            S = (qa + qb) + qc
            conv = (np.sqrt(S) - sig0) <= tol
            stop = ~conv & (iters[i] >= maxit)
            notconv[i[stop]] = True
            l2 = l + (S - sig0sq) / (2.0 * ((qa * (ka * a_) + qb * (kb * b_)) + qc * (kc * c_)))
            # a converged point takes the step of its last residual and forms the stress at the new multiplier
            a2, b2, c2 = 1.0 / (1.0 + l2 * ka), 1.0 / (1.0 + l2 * kb), 1.0 / (1.0 + l2 * kc)
            fin = conv
            da[i] = np.where(fin, a2, a_); db[i] = np.where(fin, b2, b_); dc[i] = np.where(fin, c2, c_)
            sa[i] = np.where(fin, ta[i] * a2, xa); sb[i] = np.where(fin, tb[i] * b2, xb); sc[i] = np.where(fin, tc[i] * c2, xc)
            lam[i] = np.where(stop, l, l2)
            go = ~conv & ~stop
            iters[i[go]] += 1
            act[i[~go]] = False
        sig = np.stack([(sa + sb) * R2, (sa - sb) * R2, sc], axis=1)
        xa, xb, xc = sa / CA, sb / CB, sc / CB
        epo = np.where(plastic[:, None], np.stack([eps[:, 0] - (xa + xb) * R2, eps[:, 1] - (xa - xb) * R2, eps[:, 2] - xc], axis=1), epn)
        D = _out(n, c)
        if tangent:
            Aa, Ab, Ac = CA * da, CB * db, CB * dc
            na, nb, nc = 0.5 * sa, 1.5 * sb, QC * sc
            va, vb, vc = Aa * na, Ab * nb, Ac * nc
            den = (na * va + nb * vb) + nc * vc
            Taa, Tbb, Tcc = Aa - (va * va) / den, Ab - (vb * vb) / den, Ac - (vc * vc) / den
            Tab, Tac, Tbc = -((va * vb) / den), -((va * vc) / den), -((vb * vc) / den)
            h = 0.5 * (Taa + Tbb)
            Dp = np.stack([h + Tab, 0.5 * (Taa - Tbb), (Tac + Tbc) * R2, h - Tab, (Tac - Tbc) * R2, Tcc], axis=1)
            D = np.where(plastic[:, None], Dp, D)
    return dict(stress=sig, state=epo, tangent=D[:, SLOT], plastic=plastic, iters=iters, not_converged=notconv, multiplier=lam)


def polygon(eps, epn, prm):
    """[E, nu, M, (n1, n2, d) x 4]"""
    eps, epn = np.asarray(eps, dtype=np.float64).reshape(-1, 3), np.asarray(epn, dtype=np.float64).reshape(-1, 3)
    c, rec, verts = polygon_constants([float(v) for v in prm])
    E, nu, c11, c12, c33 = c["E"], c["nu"], c["c11"], c["c12"], c["c33"]
    n = len(eps)
    with np.errstate(all="ignore"):
        ee = eps - epn
        t0, t1, t2 = c11 * ee[:, 0] + c12 * ee[:, 1], c12 * ee[:, 0] + c11 * ee[:, 1], c33 * ee[:, 2]
        mean, dlt, tau = 0.5 * (t0 + t1), 0.5 * (t0 - t1), t2 * R2
        r = np.sqrt(dlt * dlt + tau * tau)
        pos = r > 0.0
        cs, sn = np.where(pos, dlt / np.where(pos, r, 1.0), 1.0), np.where(pos, tau / np.where(pos, r, 1.0), 0.0)
        p1, p2 = mean + r, mean - r
        over = np.zeros(n)
        for n1, n2, d, *_ in rec:
            ratio = (n1 * p1 + n2 * p2) / d
            over = np.where(ratio > over, ratio, over)
        plastic = (over > 1.0) & (over <= np.finfo(float).max)
        best = np.full(n, np.inf)
        b1, b2 = p1 / np.where(plastic, over, 1.0), p2 / np.where(plastic, over, 1.0)
        nu2 = 2.0 * nu

        def nearer(x, y, adm):
            nonlocal best, b1, b2
            dx, dy = x - p1, y - p2
            dist = (dx * dx + dy * dy) - (nu2 * dx) * dy
            take = adm & (dist < best)
            best, b1, b2 = np.where(take, dist, best), np.where(take, x, b1), np.where(take, y, b2)

        for k, (n1, n2, d, w1, w2, nw, _s) in enumerate(rec):
            step = ((n1 * p1 + n2 * p2) - d) / nw
            x, y = p1 - w1 * step, p2 - w2 * step
            adm = np.ones(n, dtype=bool)
            for j, (m1, m2, dj, _a, _b, _c, slack) in enumerate(rec):
                if j != k:
                    adm &= ((m1 * x + m2 * y) - dj <= slack)
            nearer(x, y, adm)
        for vx, vy in verts:
            nearer(np.full(n, vx), np.full(n, vy), np.ones(n, dtype=bool))
        sm, sr = 0.5 * (b1 + b2), 0.5 * (b1 - b2)
        sp = np.stack([sm + sr * cs, sm - sr * cs, (sr * sn) / R2], axis=1)
        sig = np.where(plastic[:, None], sp, np.stack([t0, t1, t2], axis=1))
        ep = np.stack([eps[:, 0] - (sp[:, 0] - nu * sp[:, 1]) / E, eps[:, 1] - (sp[:, 1] - nu * sp[:, 0]) / E,
                       eps[:, 2] - ((1.0 + nu) * sp[:, 2]) / E], axis=1)
        epo = np.where(plastic[:, None], ep, epn)
    z = np.zeros(n, dtype=np.int64)
    return dict(stress=sig, state=epo, tangent=_out(n, c)[:, SLOT], plastic=plastic, iters=z, not_converged=z.astype(bool),
                principal_trial=np.stack([p1, p2], axis=1), principal=np.stack([b1, b2], axis=1))


def update(law, eps, epn, prm, maxit=25, rtol=1e-14):
    return quadratic(eps, epn, prm, maxit, rtol) if law == QUADRATIC else polygon(eps, epn, prm)


def n_nan(r, tangent=False):
    bad = ~np.isfinite(r["stress"]).all(axis=1) | ~np.isfinite(r["state"]).all(axis=1)
    if tangent:
        bad |= ~np.isfinite(r["tangent"]).all(axis=1)
    return int(bad.sum())


def stats(r, tangent=False):
    return dict(n_plastic=int(r["plastic"].sum()), n_not_converged=int(r["not_converged"].sum()), n_nan=n_nan(r, tangent),
                max_local_iters=int(r["iters"].max()) if len(r["iters"]) else 0)


def scale(law, prm):
    """s*: sig0 / the largest d_k"""
    return float(prm[2]) if law == QUADRATIC else max(d for _, _, d in planes_of(prm))


# ---- the yield sets themselves, for the checks that need no reference ------------------------------------------------------------
def principal(sig):
    sig = np.asarray(sig, dtype=np.float64).reshape(-1, 3)
    m, d, t = 0.5 * (sig[:, 0] + sig[:, 1]), 0.5 * (sig[:, 0] - sig[:, 1]), sig[:, 2] * R2
    r = np.hypot(d, t)
    return m + r, m - r


def violation(law, sig, prm):
    """how far outside the set, in stress units (<= 0 inside)"""
    sig = np.asarray(sig, dtype=np.float64).reshape(-1, 3)
    if law == QUADRATIC:
        return np.sqrt(np.einsum("ni,ij,nj->n", sig, q_matrix(prm[3]), sig)) - prm[2]
    p1, p2 = principal(sig)
    return np.max([(n1 * p1 + n2 * p2 - d) / np.hypot(n1, n2) for n1, n2, d in planes_of(prm)], axis=0)


def sample_admissible(law, prm, count, rng):
    """stresses of the set: random directions, scaled onto the surface and then inwards by a random factor"""
    v = rng.normal(size=(count, 3))
    if law == QUADRATIC:
        onto = prm[2] / np.sqrt(np.einsum("ni,ij,nj->n", v, q_matrix(prm[3]), v))
    else:
        p1, p2 = principal(v)
        onto = 1.0 / np.max([(n1 * p1 + n2 * p2) / d for n1, n2, d in planes_of(prm)], axis=0)
    return v * (onto * rng.uniform(0.0, 1.0, count) ** 0.5)[:, None]


def random_trials(law, prm, n, seed, lo=0.2, hi=8.0):
    """strains (from a zero plastic strain) whose trial stress lies at lo ... hi times the yield surface (log-uniform), in random
    directions"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    factor = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    # every direction onto the surface first (the set is star-shaped about the origin)
    if law == QUADRATIC:
        a = prm[2] / np.sqrt(np.einsum("ni,ij,nj->n", v, q_matrix(prm[3]), v))
    else:
        p1, p2 = principal(v)
        a = 1.0 / np.max([(n1 * p1 + n2 * p2) / d for n1, n2, d in planes_of(prm)], axis=0)
    return (v * (a * factor)[:, None]) @ compliance(prm[0], prm[1]).T


def check_projection(law, prm, trial, stress, plastic, rng, samples=2000):
    """what characterises the closest point s of the trial t in the norm of C^-1, with no reference: s is in the set (to 1e-12 s*), and
    (t - s)^T C^-1 (tau - s) <= 0 (to 1e-12 |C^-1 (t - s)| |tau - s|) for every tau of the set, here ``samples`` sampled ones"""
    s = scale(law, prm)
    assert violation(law, stress, prm).max() <= 1e-12 * s
    assert np.abs(stress[~plastic] - trial[~plastic]).max(initial=0.0) <= 1e-12 * s      # (the caller's C eps rounds differently)
    tau = sample_admissible(law, prm, samples, rng)
    assert violation(law, tau, prm).max() <= 1e-12 * s
    d = (trial - stress) @ compliance(prm[0], prm[1]).T
    for i in np.flatnonzero(plastic):
        gap = tau - stress[i]
        assert ((gap @ d[i]) <= 1e-12 * np.linalg.norm(d[i]) * np.linalg.norm(gap, axis=1)).all(), i


# the largest deviation of this restatement from the 50-digit fixture over both increments (stress in s*, tangent in E, state in
# s* / E), as tests/test_plane_stress_cpu.py measures and pins it, rounded up to two digits: the far overshoots (1e4 sig0, 1e3 d) set
# them -- C (eps - epsp) cancels there.  The GPU tests allow the kernel 16 times as much, and never less than 2e-14: it orders its sums
# and its division and square-root sequences differently from numpy
MEASURED = {QUADRATIC: (5.2e-13, 3.5e-13, 2.1e-12), POLYGON: (1.3e-13, 1.1e-16, 1.3e-13)}


def gpu_bounds(law):
    return tuple(max(16 * m, 2e-14) for m in MEASURED[law])


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def load_kat():
    return np.load(GOLDEN, allow_pickle=False)


def kat_cases(kat):
    """(tag, law, prm, [eps of increment 1, 2], per increment dict(stress, tangent, state, plastic))"""
    meta = json.loads(str(kat["meta"]))
    for case in meta["cases"]:
        t = case["tag"]
        incs = [dict(stress=kat[f"{t}_stress{k}"], tangent=kat[f"{t}_tangent{k}"], state=kat[f"{t}_state{k}"], plastic=kat[f"{t}_plastic{k}"])
                for k in (1, 2)]
        yield t, case["law"], np.array(kat[f"{t}_prm"]), [kat[f"{t}_eps1"], kat[f"{t}_eps2"]], incs
