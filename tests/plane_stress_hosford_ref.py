"""A vectorised numpy restatement of plane-stress Hosford plasticity (DXM_LAW_PS_HOSFORD = 33; ``csrc/plane_stress_hosford.hip``),
operation by operation in the kernel's order (numpy rounds every operation, as the kernel's ``fp contract(off)`` does; ``pow``,
``sin``, ``cos`` and ``atan2`` are numpy's), and the constants ``dxmat.hip::launch_ps_hosford`` forms on the host.  TEST
INFRASTRUCTURE ONLY.

Strain and stress are ``[xx, yy, sqrt(2) xy]``; the state is the hidden plastic strain ``eps - C^-1 sigma`` (N, 3)."""
import json
import os

import numpy as np

LAW = 33
R2 = 0.70710678118654752440
HALF_PI = 1.57079632679489661923
EPS = 2.220446049250313e-16
A_MIN, A_MAX = 2.0, 100.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_stress_hosford.npz")
SLOT = (0, 1, 2, 1, 3, 4, 2, 4, 5)   # (row, column) of the row-major 3 x 3 -> slot of (D00, D01, D02, D11, D12, D22)


def stiffness(E, nu):
    """``cvxpy_materials.py:16-18``"""
    return (E / (1 - nu**2)) * np.array([[1.0, nu, 0.0], [nu, 1.0, 0.0], [0.0, 0.0, (1.0 - nu)]])


def compliance(E, nu):
    return np.array([[1.0, -nu, 0.0], [-nu, 1.0, 0.0], [0.0, 0.0, 1.0 + nu]]) / E


def constants(prm, rtol=1e-14):
    """``dxmat.hip::launch_ps_hosford`` and ``build_ps_hosford``"""
    E, nu, sig0, a, tangent = (float(v) for v in prm)
    c0 = E / (1.0 - nu * nu)
    return dict(c11=c0, c12=c0 * nu, c33=c0 * (1.0 - nu), E=E, nu=nu, sqA=np.sqrt(E / (1.0 - nu)), sqB=np.sqrt(E / (1.0 + nu)), sig0=sig0,
                a=a, am1=a - 1.0, am2=a - 2.0, inva=1.0 / a, tol=max(rtol, 2.0 ** -49), CB=E / (1.0 + nu), tangent=int(tangent),
                klo=np.power(0.5, 1.0 / a) * (1.0 - 4.0 * EPS), khi=np.power(1.5, 1.0 / a) * (1.0 + 4.0 * EPS))


def _evaluate(th, sx, Tx, Ty, k):
    c, s = np.cos(th), np.sin(th)
    Ad, Bd = sx * (c * k["sqA"]), s * k["sqB"]
    d1, d2 = (Ad + Bd) * R2, (Ad - Bd) * R2
    d3 = (2.0 * Bd) * R2
    Ap, Bp = -(sx * (s * k["sqA"])), c * k["sqB"]
    e1, e2 = (Ap + Bp) * R2, (Ap - Bp) * R2
    e3 = (2.0 * Bp) * R2
    a1, a2, a3 = np.abs(d1), np.abs(d2), np.abs(d3)
    m = np.maximum(np.maximum(a1, a2), a3)
    r1, r2, r3 = a1 / m, a2 / m, a3 / m
    u1, u2, u3 = np.power(r1, k["am2"]), np.power(r2, k["am2"]), np.power(r3, k["am2"])
    v1, v2, v3 = u1 * r1, u2 * r2, u3 * r3
    S0 = (v1 * r1 + v2 * r2) + v3 * r3
    N = (np.copysign(v1, d1) * e1 + np.copysign(v2, d2) * e2) + np.copysign(v3, d3) * e3
    L = N / (m * S0)
    K2 = ((u1 * (e1 * e1) + u2 * (e2 * e2)) + u3 * (e3 * e3)) / ((m * m) * S0)
    Lp = (k["am1"] * K2 - 1.0) - k["a"] * (L * L)
    kap = np.power(0.5 * S0, k["inva"])
    rho = k["sig0"] / (m * kap)
    Tu, Tp = Tx * c + Ty * s, Ty * c - Tx * s
    gap = Tu - rho
    g = L * gap - Tp
    dg = (Lp * gap + L * (Tp + rho * L)) + Tu
    return dict(d1=d1, d2=d2, d3=d3, m=m, u1=u1, u2=u2, u3=u3, v1=v1, v2=v2, S0=S0, kap=kap, rho=rho, g=g, dg=dg)


def update(eps, epn, prm, maxit=25, rtol=1e-14):
    """[E, nu, sig0, a, tangent]"""
    eps, epn = np.asarray(eps, dtype=np.float64).reshape(-1, 3), np.asarray(epn, dtype=np.float64).reshape(-1, 3)
    k = constants(prm, rtol)
    E, nu, c11, c12, c33, sig0 = k["E"], k["nu"], k["c11"], k["c12"], k["c33"], k["sig0"]
    n = len(eps)
    with np.errstate(all="ignore"):
        ee = eps - epn
        t0, t1, t2 = c11 * ee[:, 0] + c12 * ee[:, 1], c12 * ee[:, 0] + c11 * ee[:, 1], c33 * ee[:, 2]
        mean, dlt, tau = 0.5 * (t0 + t1), 0.5 * (t0 - t1), t2 * R2
        r = np.sqrt(dlt * dlt + tau * tau)
        pos = r > 0.0
        cs, sn = np.where(pos, dlt / np.where(pos, r, 1.0), 1.0), np.where(pos, tau / np.where(pos, r, 1.0), 0.0)
        p1, p2 = mean + r, mean - r
        a1, a2, a3 = np.abs(p1), np.abs(p2), 2.0 * r
        m = np.maximum(np.maximum(a1, a2), a3)
        r1, r2, r3 = a1 / m, a2 / m, a3 / m
        w1, w2, w3 = (np.power(r1, k["am2"]) * r1) * r1, (np.power(r2, k["am2"]) * r2) * r2, (np.power(r3, k["am2"]) * r3) * r3
        phi_tr = m * np.power(0.5 * ((w1 + w2) + w3), k["inva"])
        # the bounds of phi decide where they can; the powers decide the rest (the kernel forms them only there)
        sure = (m * k["klo"] > sig0) & (m <= np.finfo(float).max)
        open_ = ~sure & ~(m * k["khi"] <= sig0)
        plastic = sure | (open_ & (phi_tr > sig0) & (phi_tr <= np.finfo(float).max))
        assert np.array_equal(plastic, (phi_tr > sig0) & (phi_tr <= np.finfo(float).max))

        sig = np.stack([t0, t1, t2], axis=1)
        epo = epn.copy()
        D = np.empty((n, 6))
        D[:] = (c11, c12, 0.0, c11, 0.0, c33)
        iters, notconv = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
        theta = np.zeros(n)
        i = np.flatnonzero(plastic)
        if len(i):
            p1, p2, r, cs, sn = p1[i], p2[i], r[i], cs[i], sn[i]
            x, Ty = ((p1 + p2) * R2) / k["sqA"], ((2.0 * r) * R2) / k["sqB"]
            Tx, sx = np.abs(x), np.copysign(1.0, x)
            np_ = len(i)
            lo, hi, th = np.zeros(np_), np.full(np_, HALF_PI), np.arctan2(Ty, Tx)
            dx, dxold = np.full(np_, HALF_PI), np.full(np_, HALF_PI)
            it, nc = np.zeros(np_, dtype=np.int64), np.zeros(np_, dtype=bool)
            act = np.ones(np_, dtype=bool)
            while act.any():
                j = np.flatnonzero(act)
                ev = _evaluate(th[j], sx[j], Tx[j], Ty[j], k)
                g, dg = ev["g"], ev["dg"]
                done = ((it[j] > 0) & (np.abs(dx[j]) <= k["tol"])) | (g == 0.0)
                cap = ~done & (it[j] >= maxit)
                nc[j[cap]] = True
                go = ~done & ~cap
                lo[j] = np.where(go & (g < 0.0), th[j], lo[j])
                hi[j] = np.where(go & ~(g < 0.0), th[j], hi[j])
                newton = th[j] - g / dg
                use = ((newton >= lo[j]) & (newton <= hi[j])) & (np.abs(2.0 * g) <= np.abs(dxold[j] * dg))
                thn = np.where(use, newton, 0.5 * (lo[j] + hi[j]))
                dxold[j] = np.where(go, dx[j], dxold[j])
                dx[j] = np.where(go, thn - th[j], dx[j])
                th[j] = np.where(go, thn, th[j])
                it[j] += go
                act[j[~go]] = False
            ev = _evaluate(th, sx, Tx, Ty, k)   # the evaluation the kernel leaves its loop with
            iters[i], notconv[i], theta[i] = it, nc, th
            rho, d1, d2 = ev["rho"], ev["d1"], ev["d2"]
            b1, b2, b3 = rho * d1, rho * d2, rho * ev["d3"]
            sm, sr = 0.5 * (b1 + b2), 0.5 * b3
            sp = np.stack([sm + sr * cs, sm - sr * cs, (sr * sn) / R2], axis=1)
            sig[i] = sp
            epo[i] = np.stack([eps[i, 0] - (sp[:, 0] - nu * sp[:, 1]) / E, eps[i, 1] - (sp[:, 1] - nu * sp[:, 0]) / E,
                               eps[i, 2] - ((1.0 + nu) * sp[:, 2]) / E], axis=1)
            if k["tangent"]:
                S0, kap, mm, d3 = ev["S0"], ev["kap"], ev["m"], ev["d3"]
                u1, u2, u3, v1, v2 = ev["u1"], ev["u2"], ev["u3"], ev["v1"], ev["v2"]
                am1 = k["am1"]
                hs = 0.5 * S0
                k1, k2 = kap / hs, (kap * kap) / hs
                r3 = np.abs(d3) / mm
                w1, w2 = 0.5 * (np.copysign(v1, d1) * k1), 0.5 * (np.copysign(v2, d2) * k1)
                w3 = 0.5 * (np.copysign(u3 * r3, d3) * k1)
                hf = am1 / (2.0 * sig0)
                h1, h2, h3 = hf * (u1 * k2), hf * (u2 * k2), hf * (u3 * k2)
                n1, n2 = w1 + w3, w2 - w3
                af = am1 / sig0
                H11, H22, H12 = (h1 + h3) - af * (n1 * n1), (h2 + h3) - af * (n2 * n2), -h3 - af * (n1 * n2)
                q1, q2 = c11 * n1 + c12 * n2, c12 * n1 + c11 * n2
                lam = ((p1 - b1) * n1 + (p2 - b2) * n2) / (n1 * q1 + n2 * q2)
                M11, M22, M12 = 1.0 / E + lam * H11, 1.0 / E + lam * H22, lam * H12 - nu / E
                det = M11 * M22 - M12 * M12
                A11, A22, A12 = M22 / det, M11 / det, -(M12 / det)
                z1, z2 = A11 * n1 + A12 * n2, A12 * n1 + A22 * n2
                den = n1 * z1 + n2 * z2
                D11, D22, D12 = A11 - (z1 * z1) / den, A22 - (z2 * z2) / den, A12 - (z1 * z2) / den
                gam = 0.25 * ((D11 + D22) - 2.0 * D12)
                alp, bet = 0.25 * ((D11 + D22) + 2.0 * D12), 0.25 * (D11 - D22)
                rp = r > 0.0
                c_, s_ = np.cos(th), np.sin(th)
                aA, Bd, Bp = c_ * k["sqA"], s_ * k["sqB"], c_ * k["sqB"]
                tot = aA + Bd
                dl = (2.0 * Bd) / tot
                qs = np.ones_like(dl)
                for kk in range(8, 0, -1):
                    qs = 1.0 - (((am1 - float(kk)) * dl) / float(kk + 1)) * qs
                small = am1 * dl < 0.05
                q = np.where(small, am1 * qs, (1.0 - np.minimum(v1, v2)) / np.where(small, 1.0, dl))
                ks = (2.0 * k["sqB"]) / tot
                Ns = (Bp * (q * ks) - k["sqA"] * (v1 + v2)) * R2 + (u3 * ks) * ((2.0 * Bp) * R2)
                Ls = Ns / (mm * S0)
                near = k["CB"] * ((rho * c_) / (Ls * ((Tx * c_ + Ty * s_) - rho) + Tx))
                far = k["CB"] * (b3 / np.where(rp, 2.0 * r, 1.0))
                G = np.where(rp, np.where(dl < 0.5, near, far), 2.0 * gam)
                cc, ss, sc = cs * cs, sn * sn, sn * cs
                gs = 0.5 * (G * ss)
                D[i] = np.stack([((alp + 2.0 * (bet * cs)) + gam * cc) + gs,
                                 (alp - gam * cc) - gs,
                                 ((bet * sn + gam * sc) / R2) - (G * sc) * R2,
                                 ((alp - 2.0 * (bet * cs)) + gam * cc) + gs,
                                 ((bet * sn - gam * sc) / R2) + (G * sc) * R2,
                                 2.0 * (gam * ss) + G * cc], axis=1)
    return dict(stress=sig, state=epo, tangent=D[:, SLOT], plastic=plastic, iters=iters, not_converged=notconv, theta=theta)


def n_nan(r, tangent=False):
    bad = ~np.isfinite(r["stress"]).all(axis=1) | ~np.isfinite(r["state"]).all(axis=1)
    if tangent:
        bad |= ~np.isfinite(r["tangent"]).all(axis=1)
    return int(bad.sum())


def stats(r, tangent=False):
    return dict(n_plastic=int(r["plastic"].sum()), n_not_converged=int(r["not_converged"].sum()), n_nan=n_nan(r, tangent),
                max_local_iters=int(r["iters"].max()) if len(r["iters"]) else 0)


# ---- the yield set itself, for the checks that need no reference -----------------------------------------------------------------
def principal(sig):
    sig = np.asarray(sig, dtype=np.float64).reshape(-1, 3)
    m, d, t = 0.5 * (sig[:, 0] + sig[:, 1]), 0.5 * (sig[:, 0] - sig[:, 1]), sig[:, 2] * R2
    r = np.hypot(d, t)
    return m + r, m - r


def phi(sig, a):
    p1, p2 = principal(sig)
    v = np.abs(np.stack([p1, p2, p1 - p2], axis=1))
    m = v.max(axis=1)
    m1 = np.where(m > 0, m, 1.0)
    return m * (0.5 * ((v / m1[:, None]) ** a).sum(axis=1)) ** (1.0 / a)


def sample_admissible(prm, count, rng):
    """stresses of the set: random directions, scaled onto the surface and then inwards by a random factor"""
    v = rng.normal(size=(count, 3))
    onto = prm[2] / phi(v, prm[3])
    return v * (onto * rng.uniform(0.0, 1.0, count) ** 0.5)[:, None]


def check_projection(prm, trial, stress, plastic, rng, samples=2000):
    """what characterises the closest point s of the trial t in the norm of C^-1, with no reference: s is in the set (to 1e-12 sig0),
    and (t - s)^T C^-1 (tau - s) <= 0 (to 1e-12 |C^-1 (t - s)| |tau - s|) for every tau of the set, here ``samples`` sampled ones"""
    s = prm[2]
    assert (phi(stress, prm[3]) - s).max() <= 1e-12 * s
    assert np.abs(stress[~plastic] - trial[~plastic]).max(initial=0.0) <= 1e-12 * s
    tau = sample_admissible(prm, samples, rng)
    assert (phi(tau, prm[3]) - s).max() <= 1e-12 * s
    d = (trial - stress) @ compliance(prm[0], prm[1]).T
    for i in np.flatnonzero(plastic):
        gap = tau - stress[i]
        assert ((gap @ d[i]) <= 1e-12 * np.linalg.norm(d[i]) * np.linalg.norm(gap, axis=1)).all(), i


# The largest deviation of this restatement from the 50-digit fixture over both increments and every case (stress in sig0, tangent in
# E, state in sig0 / E), per tangent mode, as tests/test_plane_stress_hosford_cpu.py measures and pins it, rounded up to two digits.
# The GPU tests allow the kernel 16 times as much, and never less than 2e-14.
MEASURED = {0: (1.6e-15, 0.0, 6.5e-14), 1: (1.6e-15, 2.4e-14, 6.5e-14)}


def gpu_bounds(tangent):
    return tuple(max(16 * m, 2e-14) for m in MEASURED[int(tangent)])


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def load_kat():
    return np.load(GOLDEN, allow_pickle=False)


def kat_cases(kat):
    """(tag, prm with tangent = 0, [eps of increment 1, 2], per increment dict(stress, tangent, state, plastic)); ``tangent`` is the
    algorithmic one (the tangent = 0 law hands back C)"""
    meta = json.loads(str(kat["meta"]))
    for case in meta["cases"]:
        t = case["tag"]
        incs = [dict(stress=kat[f"{t}_stress{k}"], tangent=kat[f"{t}_tangent{k}"], state=kat[f"{t}_state{k}"], plastic=kat[f"{t}_plastic{k}"])
                for k in (1, 2)]
        yield t, np.array(kat[f"{t}_prm"]), [kat[f"{t}_eps1"], kat[f"{t}_eps2"]], incs
