"""A vectorised numpy restatement of plane-stress J2 plasticity with isotropic hardening (DXM_LAW_PS_J2_LINEAR = 30,
DXM_LAW_PS_J2_VOCE = 31; ``csrc/plane_stress_j2.hip``), operation by operation in the kernel's order (numpy rounds every operation, as
the kernel's ``fp contract(off)`` does), and the constants ``dxmat.hip::launch_plane_stress_j2`` forms on the host.  TEST
INFRASTRUCTURE ONLY.  The hardening law is evaluated with plain operations: the kernel calls ``small_strain.hpp::hardening_R``, whose
linear ``sig0 + H p`` is one FMA and whose ``exp`` is the device's, so the two differ by roundings of ``R``.

Strain, stress and ``epsp`` are ``[xx, yy, sqrt(2) xy]``; the state is ``p`` (N,) and ``epsp`` (N, 3)."""
import json
import os

import numpy as np

J2_LINEAR, J2_VOCE = 30, 31
R2 = 0.70710678118654752440
TWO3 = 2.0 / 3.0
DBL_MAX = np.finfo(float).max
MAXIT, RTOL = 25, 1e-14
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_stress_j2.npz")
SLOT = (0, 1, 2, 1, 3, 4, 2, 4, 5)   # (row, column) of the row-major 3 x 3 -> slot of (D00, D01, D02, D11, D12, D22)


def constants(E, nu):
    """``PsJ2Params`` and the entries of ``LawParams`` the kernel reads"""
    c0 = E / (1.0 - nu * nu)
    CA, CB = E / (1.0 - nu), E / (1.0 + nu)
    ka = CA / 3.0
    return dict(c11=c0, c12=c0 * nu, c33=c0 * (1.0 - nu), CA=CA, CB=CB, ka=ka, kmax=max(ka, CB), kmin=min(ka, CB), mu=E / 2 / (1 + nu))


def stiffness(E, nu):
    return (E / (1 - nu**2)) * np.array([[1.0, nu, 0.0], [nu, 1.0, 0.0], [0.0, 0.0, (1.0 - nu)]])


def compliance(E, nu):
    return np.array([[1.0, -nu, 0.0], [-nu, 1.0, 0.0], [0.0, 0.0, 1.0 + nu]]) / E


def hardening(law, prm):
    """(R, dR) of the law's parameters [E, nu, sig0, H] / [E, nu, sig0, sigu, b]"""
    if law == J2_LINEAR:
        sig0, H = prm[2], prm[3]
        return (lambda p: sig0 + H * p), (lambda p: np.full_like(p, H))
    sig0, sigu, b = prm[2], prm[3], prm[4]
    return (lambda p: sig0 + (sigu - sig0) * (1.0 - np.exp(-b * p))), (lambda p: ((sigu - sig0) * b) * np.exp(-b * p))


def seq_of(sig):
    """von Mises of a plane-stress state in the three components"""
    sig = np.asarray(sig, dtype=np.float64).reshape(-1, 3)
    return np.sqrt((sig[:, 0] ** 2 + sig[:, 1] ** 2 - sig[:, 0] * sig[:, 1]) + 1.5 * sig[:, 2] ** 2)


def update(law, eps, epsp_n, p_n, prm, maxit=MAXIT, rtol=RTOL):
    """One increment of ``n`` points.  Returns dict(stress (n, 3), tangent (n, 9), p (n,), epsp (n, 3), plastic, iters, not_converged,
    multiplier, overshoot)."""
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, 3)
    n = len(eps)
    epn = np.array(epsp_n, dtype=np.float64).reshape(n, 3)
    p_n = np.array(p_n, dtype=np.float64).reshape(n)
    prm = [float(v) for v in prm]
    c = constants(prm[0], prm[1])
    CA, CB, ka, kmax, kmin = c["CA"], c["CB"], c["ka"], c["kmax"], c["kmin"]
    R, dR = hardening(law, prm)
    tol = rtol * max(abs(prm[2]), 2e-8 * c["mu"])
    with np.errstate(all="ignore"):
        ee = eps - epn
        ta, tb, tc = CA * ((ee[:, 0] + ee[:, 1]) * R2), CB * ((ee[:, 0] - ee[:, 1]) * R2), CB * ee[:, 2]
        seqt = np.sqrt((0.5 * (ta * ta) + 1.5 * (tb * tb)) + 1.5 * (tc * tc))
        Rn = R(p_n)
        plastic = (seqt > Rn) & (seqt <= DBL_MAX)
        sa, sb, sc = ta.copy(), tb.copy(), tc.copy()
        p_new, epo = p_n.copy(), epn.copy()
        D = np.empty((n, 6))
        D[:] = (c["c11"], c["c12"], 0.0, c["c11"], 0.0, c["c33"])
        iters, notconv, mult = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n)
        i = np.flatnonzero(plastic)
        if i.size:
            ta_, tb_, tc_, sq, rn, pn = ta[i], tb[i], tc[i], seqt[i], Rn[i], p_n[i]
            tolp = np.maximum(tol, rtol * sq)
            f = sq - rn
            cc = (TWO3 * np.maximum(dR(pn), 0.0)) * sq
            B = cc + rn * kmax
            dg = (2.0 * f) / (B + np.sqrt(B * B + (4.0 * (cc * kmax)) * f))
            if law == J2_VOCE:
                cap = np.maximum(prm[3], rn)
                dg = np.maximum(dg, (sq / cap - 1.0) / kmax)
            dg = np.where((dg >= 0.0) & (dg <= DBL_MAX), dg, 0.0)
            # the lower bound of R over the step; no positive bound: no bracket, the point is counted at its first residual
            floor = rn
            if law == J2_VOCE:
                floor = np.minimum(rn, prm[3])
            elif prm[3] < 0.0:
                ua, ub, uc = ta_ / ka, tb_ / CB, tc_ / CB
                floor = rn + prm[3] * (TWO3 * np.sqrt(0.5 * (ua * ua) + 1.5 * (ub * ub + uc * uc)))
            cap = np.where(floor > 0.0, maxit, 0)
            lo, hi = np.zeros(i.size), (sq / floor - 1.0) / kmin
            m = i.size
            da, db, S, seq, pp = np.ones(m), np.ones(m), np.zeros(m), np.zeros(m), pn.copy()
            xa, xb, xc = ta_.copy(), tb_.copy(), tc_.copy()
            it, nc = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=bool)
            live = np.ones(m, dtype=bool)
            while live.any():
                j = np.flatnonzero(live)
                g_ = dg[j]
                a_, b_ = 1.0 / (1.0 + g_ * ka), 1.0 / (1.0 + g_ * CB)
                ya, yb, yc = ta_[j] * a_, tb_[j] * b_, tc_[j] * b_
                qa, qb, qc = 0.5 * (ya * ya), 1.5 * (yb * yb), 1.5 * (yc * yc)
                S_ = (qa + qb) + qc
                sq_ = np.sqrt(S_)
                pp_ = pn[j] + (TWO3 * g_) * sq_
                g = sq_ - R(pp_)
                conv = np.abs(g) <= tolp[j]
                stop = ~conv & (it[j] >= cap[j])
                dseq = -((qa * (ka * a_) + (qb + qc) * (CB * b_)) / sq_)
                gp = dseq - (TWO3 * dR(pp_)) * (sq_ + g_ * dseq)
                dgn = g_ - g / gp
                # a converged point takes the step of its last residual, unsafeguarded, and forms stress and p at the new multiplier
                a2, b2 = 1.0 / (1.0 + dgn * ka), 1.0 / (1.0 + dgn * CB)
                za, zb, zc = ta_[j] * a2, tb_[j] * b2, tc_[j] * b2
                S2 = (0.5 * (za * za) + 1.5 * (zb * zb)) + 1.5 * (zc * zc)
                sq2 = np.sqrt(S2)
                pp2 = pn[j] + (TWO3 * dgn) * sq2
                da[j], db[j] = np.where(conv, a2, a_), np.where(conv, b2, b_)
                xa[j], xb[j], xc[j] = np.where(conv, za, ya), np.where(conv, zb, yb), np.where(conv, zc, yc)
                S[j], seq[j], pp[j] = np.where(conv, S2, S_), np.where(conv, sq2, sq_), np.where(conv, pp2, pp_)
                go = ~conv & ~stop
                lo[j] = np.where(go & (g > 0.0), g_, lo[j])
                hi[j] = np.where(go & ~(g > 0.0), g_, hi[j])
                safe = np.where((dgn > lo[j]) & (dgn < hi[j]), dgn, 0.5 * (lo[j] + hi[j]))
                dg[j] = np.where(conv, dgn, np.where(stop, g_, safe))
                nc[j[stop]] = True
                it[j[go]] += 1
                live[j[~go]] = False
            iters[i], notconv[i], mult[i] = it, nc, dg
            sa[i], sb[i], sc[i] = xa, xb, xc
            p_new[i] = pp
            ua, ub, uc = xa / CA, xb / CB, xc / CB
            e_ = eps[i]
            epo[i] = np.stack([e_[:, 0] - (ua + ub) * R2, e_[:, 1] - (ua - ub) * R2, e_[:, 2] - uc], axis=1)
            dRf = dR(pp)
            theta = 1.0 - (TWO3 * dRf) * dg
            Aa, Ab = CA * da, CB * db
            na, nb, nc_ = 0.5 * xa, 1.5 * xb, 1.5 * xc
            va, vb, vc = Aa * na, Ab * nb, Ab * nc_
            den = ((na * va + nb * vb) + nc_ * vc) + (dRf * S) / theta
            Taa, Tbb, Tcc = Aa - (va * va) / den, Ab - (vb * vb) / den, Ab - (vc * vc) / den
            Tab, Tac, Tbc = -((va * vb) / den), -((va * vc) / den), -((vb * vc) / den)
            h = 0.5 * (Taa + Tbb)
            D[i] = np.stack([h + Tab, 0.5 * (Taa - Tbb), (Tac + Tbc) * R2, h - Tab, (Tac - Tbc) * R2, Tcc], axis=1)
        sig = np.stack([(sa + sb) * R2, (sa - sb) * R2, sc], axis=1)
        overshoot = seqt / Rn
    return dict(stress=sig, tangent=D[:, SLOT], p=p_new, epsp=epo, plastic=plastic, iters=iters, not_converged=notconv, multiplier=mult,
                overshoot=overshoot)


def stats(r):
    """dxm_stats of one launch"""
    bad = ~np.isfinite(r["stress"]).all(axis=1) | ~np.isfinite(r["tangent"]).all(axis=1) | ~np.isfinite(r["p"]) | ~np.isfinite(r["epsp"]).all(axis=1)
    return dict(n_plastic=int(r["plastic"].sum()), n_not_converged=int(r["not_converged"].sum()), n_nan=int(bad.sum()),
                max_local_iters=int(r["iters"].max()) if len(r["iters"]) else 0)


def axial_strain(E, nu, stress, epsp):
    """eps_zz of the plane-stress state: the elastic part from sig_zz = 0, the plastic part from the trace-free flow"""
    stress, epsp = np.asarray(stress).reshape(-1, 3), np.asarray(epsp).reshape(-1, 3)
    return -nu / E * (stress[:, 0] + stress[:, 1]) - (epsp[:, 0] + epsp[:, 1])


# ---- the inputs the CPU and the GPU tests share --------------------------------------------------------------------------------------
E, NU, SIG0 = 70e3, 0.3, 250.0
#: linear hardening with H in {0, 5e3, E}; Voce with the constants of the reference's plane-stress demo
CASES = {"linear_H0": (J2_LINEAR, [E, NU, SIG0, 0.0]), "linear_H5e3": (J2_LINEAR, [E, NU, SIG0, 5e3]), "linear_HE": (J2_LINEAR, [E, NU, SIG0, E]),
         "voce": (J2_VOCE, [E, NU, 350.0, 500.0, 1e3])}


def random_trials(prm, n, seed, lo=0.2, hi=8.0):
    """strains (from the virgin state) whose trial stress lies at lo ... hi times the initial yield surface (log-uniform), in random
    directions"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    factor = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return (v * (prm[2] / seq_of(v) * factor)[:, None]) @ compliance(prm[0], prm[1]).T


def increments(prm, n, seed=30):
    """three increments with an unloading: load, unload to 40 % of it plus a small new direction, reload beyond"""
    a = random_trials(prm, n, seed, 0.2, 4.0)
    b = random_trials(prm, n, seed + 1, 0.2, 4.0)
    return [a, 0.4 * a + 0.05 * b, 1.3 * a + 0.6 * b]


# the largest deviation of this restatement from the 50-digit fixture over both increments and all cases of a law (stress in sig0,
# tangent in E, p and epsp in sig0 / E), as tests/test_plane_stress_j2_cpu.py measures and pins it, rounded up to two digits: the far
# overshoots (1e4 sig0) set them -- C (eps - epsp) cancels there.  The GPU tests allow the kernel 16 times as much, and never less than
# 2e-14: it orders its division and square-root sequences differently from numpy, and evaluates R with its own exp and one FMA
MEASURED = {J2_LINEAR: (1.3e-12, 1.1e-14, 2.0e-12), J2_VOCE: (4.8e-13, 2.4e-13, 4.3e-12)}


def gpu_bounds(law):
    return tuple(max(16 * m, 2e-14) for m in MEASURED[law])


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def load_kat():
    return np.load(GOLDEN, allow_pickle=False)


def kat_cases(kat):
    """(tag, law, prm, [eps of increment 1, 2], per increment dict(stress, tangent, p, epsp, plastic))"""
    meta = json.loads(str(kat["meta"]))
    for case in meta["cases"]:
        t = case["tag"]
        incs = [dict(stress=kat[f"{t}_stress{k}"], tangent=kat[f"{t}_tangent{k}"], p=kat[f"{t}_p{k}"], epsp=kat[f"{t}_epsp{k}"],
                     plastic=kat[f"{t}_plastic{k}"]) for k in (1, 2)]
        yield t, case["law"], np.array(kat[f"{t}_prm"]), [kat[f"{t}_eps1"], kat[f"{t}_eps2"]], incs
