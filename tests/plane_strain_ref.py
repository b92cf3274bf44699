"""The plane-strain forms of isotropic elasticity and J2 plasticity (DXM_LAW_PE_ELASTIC_ISO = 26, DXM_LAW_PE_J2_LINEAR = 27,
DXM_LAW_PE_J2_VOCE = 28) restated in numpy IN FOUR COMPONENTS ``[xx, yy, zz, sqrt(2) xy]``, following ``csrc/plane_strain.hip`` line
by line.  TEST INFRASTRUCTURE ONLY.  Deliberately no call into ``oracle``: the tests compare this text with the 6-wide oracle on the
embedded input, which means something only if the two are separate statements."""
import numpy as np

ELASTIC, J2_LINEAR, J2_VOCE = 26, 27, 28
ONE = np.array([1.0, 1.0, 1.0, 0.0])
MAXIT, RTOL = 25, 1e-14


def lame(E, nu):
    return E * nu / (1 + nu) / (1 - 2 * nu), E / 2 / (1 + nu)


def stiffness(E, nu):
    """the 4x4 block: lambda 1x1 + 2 mu I"""
    lam, mu = lame(E, nu)
    return lam * np.outer(ONE, ONE) + 2 * mu * np.eye(4)


def hardening(law, prm):
    """(R, dR) of the law's parameters [E, nu, sig0, H] / [E, nu, sig0, sigu, b]"""
    if law == J2_LINEAR:
        sig0, H = prm[2], prm[3]
        return (lambda p: sig0 + H * p), (lambda p: np.full_like(p, H))
    sig0, sigu, b = prm[2], prm[3], prm[4]
    return (lambda p: sig0 + (sigu - sig0) * (1.0 - np.exp(-b * p))), (lambda p: ((sigu - sig0) * b) * np.exp(-b * p))


def update(law, eps, epsp_n=None, p_n=None, prm=None, maxit=MAXIT, rtol=RTOL):
    """One increment of ``n`` points.  Returns dict(stress (n, 4), tangent (n, 16), p (n,), epsp (n, 4), plastic, iters,
    not_converged, f_trial, coef (n, 3), n (n, 4))."""
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, 4)
    N = len(eps)
    E, nu = prm[0], prm[1]
    lam, mu = lame(E, nu)
    mu2 = 2.0 * mu
    c1, c2, c3 = np.full(N, lam), np.full(N, mu2), np.zeros(N)
    wn = np.zeros(N)
    plastic, iters, notconv = np.zeros(N, dtype=bool), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
    f = np.full(N, -np.inf)
    if law == ELASTIC:
        e = eps.copy()
        p_new, ep = np.zeros(N), np.zeros((N, 4))
    else:
        ep = np.array(epsp_n, dtype=np.float64).reshape(N, 4)
        p_n = np.asarray(p_n, dtype=np.float64).reshape(N)
        p_new = p_n.copy()
        R, dR = hardening(law, prm)
        e = eps - ep
        with np.errstate(invalid="ignore", over="ignore"):
            third = ((e[:, 0] + e[:, 1]) + e[:, 2]) / 3.0
            se = mu2 * (e - third[:, None] * ONE)
            nrm2 = ((se[:, 0] * se[:, 0] + se[:, 1] * se[:, 1]) + se[:, 2] * se[:, 2]) + se[:, 3] * se[:, 3]   # the Mandel shear once
            seq = np.sqrt(1.5 * nrm2)
            f = seq - R(p_n)
            plastic = f > 0.0
        i = np.flatnonzero(plastic)
        if i.size:
            sq, pn = seq[i], p_n[i]
            if law == J2_LINEAR:
                dp = f[i] / (prm[3] + 3.0 * mu)
            else:
                sig0 = prm[2]
                tol = rtol * max(abs(sig0), 2e-8 * mu)
                tolp = np.maximum(tol, rtol * sq)
                dp = np.zeros(i.size)
                it = np.zeros(i.size, dtype=np.int64)
                live = np.ones(i.size, dtype=bool)
                nc = np.zeros(i.size, dtype=bool)
                for k in range(maxit + 1):
                    r = (sq - (3.0 * mu) * dp) - R(pn + dp)
                    live &= ~(np.abs(r) <= tolp)
                    if not live.any():
                        break
                    if k >= maxit:
                        nc |= live
                        break
                    dr = -(3.0 * mu) - dR(pn + dp)
                    dp = np.where(live, dp - r / dr, dp)
                    it += live
                iters[i], notconv[i] = it, nc
            iseq = 1.0 / sq
            beta = dp * iseq
            rho = 1.0 - (3.0 * mu) * beta
            with np.errstate(divide="ignore", invalid="ignore"):
                wn[i] = np.where(rho > 0.0, (1.5 * iseq) / rho, 0.0)
            if law != J2_LINEAR or prm[3] < 0.0:
                notconv[i] |= ~(rho > 0.0)
            gamma = 1.0 / (dR(pn + dp) + 3.0 * mu)
            mm = mu * mu
            c1[i] = lam + (2.0 * mm) * beta
            c2[i] = mu2 - (6.0 * mm) * beta
            c3[i] = (4.0 * mm) * (beta - gamma)
            p_new[i] = pn + dp
            dn = dp[:, None] * ((1.5 * se[i]) * iseq[:, None])
            ep[i] += dn
            e[i] -= dn
    ltr = lam * ((e[:, 0] + e[:, 1]) + e[:, 2])
    s = ltr[:, None] * ONE + mu2 * e
    third = ((s[:, 0] + s[:, 1]) + s[:, 2]) * (1.0 / 3.0)
    nn = (s - third[:, None] * ONE) * wn[:, None]
    Ct = (c1[:, None, None] * np.outer(ONE, ONE)[None] + c2[:, None, None] * np.eye(4)[None]) + c3[:, None, None] * (nn[:, :, None] * nn[:, None, :])
    return dict(stress=s, tangent=Ct.reshape(N, 16), p=p_new, epsp=ep, plastic=plastic, iters=iters, not_converged=notconv, f_trial=f,
                coef=np.stack([c1, c2, c3], axis=1), n=nn)


def stats(law, r):
    """dxm_stats of one launch"""
    bad = ~np.isfinite(r["stress"]).all(axis=1) | ~np.isfinite(r["tangent"]).all(axis=1)
    if law != ELASTIC:
        bad |= ~np.isfinite(r["p"]) | ~np.isfinite(r["epsp"]).all(axis=1)
    return dict(n_plastic=int(r["plastic"].sum()), n_not_converged=int(r["not_converged"].sum()), n_nan=int(bad.sum()),
                max_local_iters=int(r["iters"][r["plastic"]].max()) if r["plastic"].any() else 0)


# ---- the inputs the CPU and the GPU tests share ------------------------------------------------------------------------------------
E, NU, SIG0 = 70e3, 0.3, 250.0
#: linear hardening with H in {0, 5e3}; Voce with the constants of demos/jax/elastoplasticity/plane_elastoplasticity.py:60-73
CASES = {"linear_H0": (J2_LINEAR, [E, NU, SIG0, 0.0]), "linear_H5e3": (J2_LINEAR, [E, NU, SIG0, 5e3]),
         "voce": (J2_VOCE, [E, NU, 350.0, 500.0, 1e3])}
ELASTIC_CASE = (ELASTIC, [E, NU])
KINK = 1e-9      # points with |f_trial| <= KINK sig0 are left out of a comparison


def strains(n, sig0, Eprm, seed, zz=True):
    """fixed-seed random strains of magnitude up to 3 sig0 / E; ``zz``: eps_zz non-zero too (else the plane-strain caller's 0)"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 4))
    if not zz:
        d[:, 2] = 0.0
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * rng.uniform(0.0, 3.0, n)[:, None] * (sig0 / Eprm)


def increments(n, sig0, Eprm, seed=20, zz=True):
    """three increments with an unloading: load, unload to 40 % of it plus a small new direction, reload beyond"""
    a = strains(n, sig0, Eprm, seed, zz)
    b = strains(n, sig0, Eprm, seed + 1, zz)
    return [a, 0.4 * a + 0.05 * b, 1.3 * a + 0.6 * b]
