"""Float64 restatement of the finite-strain FCC single-crystal viscoplastic law (law id 21), vectorised over points, in the
reduced form the kernel uses: the twelve slip increments are the unknowns, ``Fe = F Fp_n^-1 A / det(A)^(1/3)``,
``A = I - sum dg_i mu_i``.  Same conventions and the same iteration as the kernel (start at ``dg = 0``; a step is halved while the
new ``max |fg|`` is not finite or larger than the old one, a halving counts as an iteration; stop at ``max |fg| <= rtol``, then one
more correction from the factorisation the tangent needs), so that iteration counts and failure flags compare too.  DESIGN.md,
section "Finite-strain single-crystal viscoplasticity", lists the equations.

9-vectors are in the order [11, 22, 33, 12, 21, 13, 31, 23, 32] (``TI`` / ``TJ``); the state lives in the material frame."""
import numpy as np

from single_crystal_ref import interaction_classes, systems

TI = (0, 1, 2, 0, 1, 0, 2, 1, 2)
TJ = (0, 1, 2, 1, 0, 2, 0, 2, 1)
NAMES = ("E", "nu", "G", "n", "K", "tau0", "Q", "b", "d", "C")
#: the constants law 14's behaviour file carries, with the self-hardening-only interaction matrix of the finite-strain file
MFRONT = dict(E=208000.0, nu=0.3, G=80000.0, n=10.0, K=25.0, tau0=66.62, Q=11.43, b=2.1, d=494.0, C=14363.0)
SELF_ONLY = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
FIELDS = (("PlasticSlip", 12), ("EquivalentViscoplasticSlip", 12), ("BackStrain", 12), ("PlasticPartOfTheDeformationGradient", 9))
I3 = np.eye(3)


def param_vector(props=None, interaction=SELF_ONLY):
    p = {**MFRONT, **(props or {})}
    return np.array([p[k] for k in NAMES] + list(interaction), dtype=np.float64)


def to_mat(v):
    """(..., 9) -> (..., 3, 3)"""
    v = np.asarray(v, dtype=np.float64)
    out = np.empty(v.shape[:-1] + (3, 3))
    for t in range(9):
        out[..., TI[t], TJ[t]] = v[..., t]
    return out


def to_vec(m):
    m = np.asarray(m, dtype=np.float64)
    return np.stack([m[..., TI[t], TJ[t]] for t in range(9)], axis=-1)


def schmid_full():
    """(12, 3, 3): mu_i = m_i x n_i of the unit slip direction and the unit plane normal, not symmetrised."""
    n, s, _ = systems()
    return np.array([np.outer(si, ni) / (np.sqrt(2.0) * np.sqrt(3.0)) for ni, si in zip(n, s)])


def cubic(p):
    """(c11, c12, 2 G) of the cubic stiffness of E, nu, G: the normal block is the inverse of the compliance block."""
    E, nu, G = p[:3]
    S = np.array([[1 / E, -nu / E, -nu / E], [-nu / E, 1 / E, -nu / E], [-nu / E, -nu / E, 1 / E]])
    A = np.linalg.inv(S)
    return A[0, 0], A[0, 1], 2.0 * G


def stiff(cub, E):
    """S = D : E for symmetric E (..., 3, 3)"""
    c11, c12, g2 = cub
    tr = E[..., 0, 0] + E[..., 1, 1] + E[..., 2, 2]
    S = g2 * E
    for i in range(3):
        S[..., i, i] = (c11 - c12) * E[..., i, i] + c12 * tr
    return S


def zero_state(n):
    Fp = np.zeros((n, 9))
    Fp[:, :3] = 1.0
    return {"g": np.zeros((n, 12)), "p": np.zeros((n, 12)), "a": np.zeros((n, 12)), "Fp": Fp}


def _sgn(x):
    return np.where(x > 0.0, 1.0, -1.0)   # 0 counts as -1, as in law 14


def _mm(a, b):
    return np.einsum("...ij,...jk->...ik", a, b)


def _T(a):
    return np.swapaxes(a, -1, -2)


def kinematics(dg, Fetr, Fpi, cub, mu):
    A = I3 - np.einsum("ni,ijk->njk", dg, mu)
    with np.errstate(all="ignore"):
        a3 = 1.0 / np.cbrt(np.linalg.det(A))
    Dp = A * a3[:, None, None]
    Fe = _mm(Fetr, Dp)
    Eel = 0.5 * (_mm(_T(Fe), Fe) - I3)
    S = stiff(cub, Eel)
    M = _mm(I3 + 2.0 * Eel, S)
    return dict(A=A, a3=a3, Dp=Dp, Fe=Fe, Eel=Eel, S=S, M=M, G=_mm(Fpi, Dp))


def directional(k, cub, c, dFe, dG):
    """(dM, dP) for the variations dFe of Fe and dG of G = Fp^-1"""
    dE = _mm(_T(k["Fe"]), dFe)
    dE = 0.5 * (dE + _T(dE))
    dS = stiff(cub, dE)
    dM = 2.0 * _mm(dE, k["S"]) + _mm(I3 + 2.0 * k["Eel"], dS)
    dP = _mm(_mm(dFe, k["S"]) + _mm(k["Fe"], dS), _T(k["G"])) + _mm(_mm(k["Fe"], k["S"]), _T(dG))
    return dM, c[:, None, None] * dP


def slip_variation(k, j, mu, Fetr, Fpi):
    """d(DeltaFp^-1) / d dg_j and the variations of Fe and G that follow"""
    with np.errstate(all="ignore"):
        Ainv = np.linalg.inv(k["A"])
    tr = np.einsum("nkl,lk->n", Ainv, mu[j])
    dDp = k["a3"][:, None, None] * (-mu[j][None] + tr[:, None, None] / 3.0 * k["A"])
    return _mm(Fetr, dDp), _mm(Fpi, dDp)


def f_variation(k, u):
    """variation of Fe for a unit variation of component u (TI / TJ) of the material-frame F"""
    dFe = np.zeros_like(k["G"])
    dFe[:, TI[u], :] = k["G"][:, TJ[u], :]
    return dFe


def tangent_at_fixed_slip(k, cub, c):
    """(N, 9, 9) dP/dF at fixed dg, both indices in the 9-vector order, material frame"""
    N = k["Fe"].shape[0]
    T = np.empty((N, 9, 9))
    for u in range(9):
        _, dP = directional(k, cub, c, f_variation(k, u), np.zeros_like(k["G"]))
        T[:, :, u] = to_vec(dP)
    return T


def rotate_tangent(Tm, R):
    """T[(iJ),(kL)] = R_ai R_bJ Tm[(ab),(cd)] R_ck R_dL"""
    N = Tm.shape[0]
    T4 = np.zeros((N, 3, 3, 3, 3))
    for t in range(9):
        for u in range(9):
            T4[:, TI[t], TJ[t], TI[u], TJ[u]] = Tm[:, t, u]
    T4 = np.einsum("nai,nbj,nabcd,nck,ndl->nijkl", R, R, T4, R, R)
    out = np.empty_like(Tm)
    for t in range(9):
        for u in range(9):
            out[:, t, u] = T4[:, TI[t], TJ[t], TI[u], TJ[u]]
    return out


def update(F, state, params, dt, R=None, rtol=1e-14, maxit=25):
    """One implicit step.  F (N, 9) global, state dict of (N, .) arrays g, p, a, Fp; R None, (3, 3) or (N, 3, 3).  Returns a dict:
    stress (N, 9) PK1, tangent (N, 9, 9), g, p, a, Fp, plastic, status (0 ok, 1 iteration cap), iters, halvings."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    N = F.shape[0]
    prm = np.asarray(params, dtype=np.float64)
    nn, K, tau0, Qc, b, d, C = prm[3:10]
    cub = cubic(prm)
    mu = schmid_full()
    QH = Qc * prm[10:16][interaction_classes()]
    Rb = None if R is None else np.ascontiguousarray(np.broadcast_to(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), (N, 3, 3)))
    Fm = to_mat(F)
    if Rb is not None:
        Fm = _mm(_mm(Rb, Fm), _T(Rb))
    g0, p0, a0 = state["g"], state["p"], state["a"]
    Fpn = to_mat(state["Fp"])
    with np.errstate(all="ignore"):
        Fpi = np.linalg.inv(Fpn)
        c = np.linalg.det(Fpn)
    Fetr = _mm(Fm, Fpi)

    def evaluate(dg, idx):
        k = kinematics(dg, Fetr[idx], Fpi[idx], cub, mu)
        adg = np.abs(dg)
        E = np.exp(-b * (p0[idx] + adg))
        tau = np.einsum("nkl,ikl->ni", k["M"], mu)
        r = tau0 + (1.0 - E) @ QH.T
        den = 1.0 / (1.0 + d * adg)
        da = (dg - d * a0[idx] * adg) * den
        y = tau - C * (a0[idx] + da)
        s = _sgn(y)
        f = np.maximum(np.abs(y) - r, 0.0)
        with np.errstate(all="ignore"):
            fk = np.where(f > 0.0, np.exp(nn * np.log(np.where(f > 0.0, f, 1.0) / K)), 0.0)
        fg = dg - dt * fk * s
        return k, E, s, f, fk, fg, den

    def system(k, idx, dg, E, s, f, fk, den):
        """J (m, 12, 12) and the right-hand sides d fg / dF (m, 12, 9)"""
        m = idx.size
        with np.errstate(all="ignore"):
            w = dt * np.where(f > 0.0, nn * fk / np.where(f > 0.0, f, 1.0), 0.0)
        dda = (1.0 - d * a0[idx] * _sgn(dg)) * den * den
        Tt = np.empty((m, 12, 12))
        for j in range(12):
            dFe, dG = slip_variation(k, j, mu, Fetr[idx], Fpi[idx])
            dM, _ = directional(k, cub, c[idx], dFe, dG)
            Tt[:, :, j] = np.einsum("nkl,ikl->ni", dM, mu)
        J = w[:, :, None] * (-Tt + s[:, :, None] * b * QH[None] * (E * _sgn(dg))[:, None, :])
        J[:, np.arange(12), np.arange(12)] += w * C * dda + 1.0
        rhs = np.empty((m, 12, 9))
        for u in range(9):
            dM, _ = directional(k, cub, c[idx], f_variation(k, u), np.zeros_like(k["G"]))
            rhs[:, :, u] = -w * np.einsum("nkl,ikl->ni", dM, mu)
        return J, rhs

    everyone = np.arange(N)
    k0, _, _, f_tr, _, _, _ = evaluate(np.zeros((N, 12)), everyone)
    plastic = (f_tr > 0.0).any(axis=1)
    tangent_m = tangent_at_fixed_slip(k0, cub, c)   # the elastic answer; yielded points overwrite theirs
    dg_all = np.zeros((N, 12))
    status = np.zeros(N, dtype=int)
    iters = np.zeros(N, dtype=int)
    halvings = np.zeros(N, dtype=int)
    idx = np.nonzero(plastic)[0]
    dg = np.zeros((idx.size, 12))
    step = np.zeros_like(dg)
    it = np.zeros(idx.size, dtype=int)
    old = np.full(idx.size, np.inf)
    while idx.size:
        k, E, s, f, fk, fg, den = evaluate(dg, idx)
        with np.errstate(all="ignore"):
            fmax = np.abs(fg).max(axis=1)
            bad = ~(fmax <= old)
        conv = ~(~(np.abs(fg) <= rtol)).any(axis=1)
        done = np.zeros(idx.size, dtype=bool)
        fail0 = bad & (it == 0)
        status[idx[fail0]] = 1
        done |= fail0
        halve = bad & (it > 0)
        step[halve] *= 0.5
        dg[halve] -= step[halve]
        it[halve] += 1
        halvings[idx[halve]] += 1
        capped = halve & (it >= maxit)
        status[idx[capped]] = 1
        done |= capped
        ok = ~bad
        if ok.any():
            sub = np.nonzero(ok)[0]
            ks = {key: v[sub] for key, v in k.items()}
            J, rhs = system(ks, idx[sub], dg[sub], E[sub], s[sub], f[sub], fk[sub], den[sub])
            sol = np.linalg.solve(J, np.concatenate([fg[sub][:, :, None], rhs], axis=2))
            delta, X = sol[:, :, 0], sol[:, :, 1:]
            old[sub] = fmax[sub]
            fin = conv[sub] | (it[sub] >= maxit)
            # the tangent of a finished point, at the iterate its convergence test saw
            if fin.any():
                fs = sub[fin]
                kf = {key: v[fin] for key, v in ks.items()}
                cf = c[idx[fs]]
                T = tangent_at_fixed_slip(kf, cub, cf)
                for j in range(12):
                    dFe, dG = slip_variation(kf, j, mu, Fetr[idx[fs]], Fpi[idx[fs]])
                    _, dP = directional(kf, cub, cf, dFe, dG)
                    T -= to_vec(dP)[:, :, None] * X[fin][:, j, None, :]
                good = conv[sub][fin]
                tangent_m[idx[fs[good]]] = T[good]
            step[sub] = -delta
            dg[sub] += step[sub]
            status[idx[sub[fin & ~conv[sub]]]] = 1
            done[sub[fin]] = True
            it[sub[~fin]] += 1
        dg_all[idx[done]] = dg[done]
        iters[idx[done]] = it[done]
        keep = ~done
        idx, dg, step, it, old = idx[keep], dg[keep], step[keep], it[keep], old[keep]

    moved = plastic & (status == 0)
    dg_all[~moved] = 0.0
    k = kinematics(dg_all, Fetr, Fpi, cub, mu)
    Pm = c[:, None, None] * _mm(_mm(k["Fe"], k["S"]), _T(k["G"]))
    with np.errstate(all="ignore"):
        Fp_new = _mm(np.linalg.inv(k["Dp"]), Fpn)
    adg = np.abs(dg_all)
    da = (dg_all - d * a0 * adg) / (1.0 + d * adg)
    m = moved[:, None]
    out = {"g": np.where(m, g0 + dg_all, g0), "p": np.where(m, p0 + adg, p0), "a": np.where(m, a0 + da, a0),
           "Fp": np.where(m, to_vec(Fp_new), state["Fp"])}
    if Rb is None:
        out["stress"], out["tangent"] = to_vec(Pm), tangent_m
    else:
        out["stress"] = to_vec(_mm(_mm(_T(Rb), Pm), Rb))
        out["tangent"] = rotate_tangent(tangent_m, Rb)
    out.update(plastic=plastic, status=status, iters=iters, halvings=halvings, dg=dg_all)
    return out


def next_state(out):
    return {k: out[k].copy() for k in ("g", "p", "a", "Fp")}


def derived(F, state, params, R=None):
    """MFront's other variables, functions of F and the state: ElasticStrain (N, 6) [11, 22, 33, 12, 13, 23] tensor components,
    the elastic part Fe (N, 9) and ResolvedShearStress (N, 12), all in the material frame."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    N = F.shape[0]
    prm = np.asarray(params, dtype=np.float64)
    Fm = to_mat(F)
    if R is not None:
        Rb = np.broadcast_to(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), (N, 3, 3))
        Fm = _mm(_mm(Rb, Fm), _T(Rb))
    Fe = _mm(Fm, np.linalg.inv(to_mat(state["Fp"])))
    Eel = 0.5 * (_mm(_T(Fe), Fe) - I3)
    M = _mm(I3 + 2.0 * Eel, stiff(cubic(prm), Eel))
    tau = np.einsum("nkl,ikl->ni", M, schmid_full())
    eel6 = np.stack([Eel[:, 0, 0], Eel[:, 1, 1], Eel[:, 2, 2], Eel[:, 0, 1], Eel[:, 0, 2], Eel[:, 1, 2]], axis=1)
    return {"ElasticStrain": eel6, "ElasticPartOfTheDeformationGradient": to_vec(Fe), "ResolvedShearStress": tau}
