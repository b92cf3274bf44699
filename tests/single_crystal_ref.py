"""Float64 restatement of the FCC single-crystal viscoplastic law (law id 14), vectorised over points, in the reduced form the
kernel uses: twelve slip increments as unknowns, ``eel = eel_tr - sum dg_i mu_i``.  Same conventions, same iteration (start at
``dg = 0``, MFront's ``f > 1.1 K`` guard with step halving, stop at ``max |fg| <= rtol``, then one more correction from the
factorisation the tangent needs), so that iteration counts and failure flags compare too.  DESIGN.md lists the equations."""
import numpy as np

SQ2 = np.sqrt(2.0)
PLANES = np.array([[1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1]])
DIRS = np.array([[0, 1, -1], [1, 0, -1], [1, -1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
SELF, COPLANAR, HIRTH, COLLINEAR, GLISSILE, LOMER = range(6)
#: the file's constants with YoungModulus1 = 208000 and the published copper interaction coefficients
MFRONT = dict(E1=208000.0, E2=208000.0, E3=208000.0, nu12=0.3, nu23=0.3, nu13=0.3, G12=80000.0, G23=80000.0, G13=80000.0,
              n=10.0, K=25.0, tau0=66.62, Q=11.43, b=2.1, d=494.0, C=14363.0)
INTERACTION = (1.0, 1.0, 0.6, 12.3, 1.6, 1.8)
NAMES = ("E1", "E2", "E3", "nu12", "nu23", "nu13", "G12", "G23", "G13", "n", "K", "tau0", "Q", "b", "d", "C")
FIELDS = (("ElasticStrain", 6), ("ViscoplasticSlip", 12), ("EquivalentViscoplasticSlip", 12), ("BackStrain", 12))


def param_vector(props=None, interaction=INTERACTION):
    p = {**MFRONT, **(props or {})}
    return np.array([p[k] for k in NAMES] + list(interaction), dtype=np.float64)


def systems():
    """(n, s, plane): integer normals and directions of the twelve systems, plane-major, and the plane of each."""
    n, s, pl = [], [], []
    for ip, p in enumerate(PLANES):
        for d in DIRS:
            if p @ d == 0:
                n.append(p); s.append(d); pl.append(ip)
    return np.array(n), np.array(s), np.array(pl)


def mandel(t):
    return np.array([t[0, 0], t[1, 1], t[2, 2], SQ2 * t[0, 1], SQ2 * t[0, 2], SQ2 * t[1, 2]])


def schmid():
    """(12, 6): mu_i = Mandel(sym(s_i x n_i)) of the unit vectors."""
    n, s, _ = systems()
    out = []
    for ni, si in zip(n, s):
        t = np.outer(si, ni) / (np.sqrt(2.0) * np.sqrt(3.0))
        out.append(mandel(0.5 * (t + t.T)))
    return np.array(out)


def interaction_classes():
    """(12, 12) integers: the class of every pair, decided from the geometry."""
    n, s, pl = systems()
    cls = np.zeros((12, 12), dtype=int)
    for i in range(12):
        for j in range(12):
            c = np.cross(n[i], n[j])
            if i == j:
                k = SELF
            elif pl[i] == pl[j]:
                k = COPLANAR
            elif not np.cross(s[i], s[j]).any():
                k = COLLINEAR
            elif s[i] @ s[j] == 0:
                k = HIRTH
            elif not np.cross(s[i], c).any() or not np.cross(s[j], c).any():
                k = GLISSILE
            else:
                k = LOMER
            cls[i, j] = k
    return cls


def stiffness(p):
    """6x6 Mandel stiffness in the material frame from the nine constants (the orthotropic law's)."""
    E1, E2, E3, nu12, nu23, nu13, G12, G23, G13 = p[:9]
    S = np.array([[1 / E1, -nu12 / E1, -nu13 / E1], [-nu12 / E1, 1 / E2, -nu23 / E2], [-nu13 / E1, -nu23 / E2, 1 / E3]])
    D = np.zeros((6, 6))
    D[:3, :3] = np.linalg.inv(S)
    D[3, 3], D[4, 4], D[5, 5] = 2 * G12, 2 * G13, 2 * G23
    return D


IJ = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def mandel_rotation(R):
    """(N, 6, 6): Q(R) with eps_m = Q eps; the rows of R are the material axes."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    Q = np.empty((R.shape[0], 6, 6))
    for I, (i, j) in enumerate(IJ):
        for K, (k, l) in enumerate(IJ):
            if I < 3 and K < 3:
                Q[:, I, K] = R[:, i, k] ** 2
            elif I < 3:
                Q[:, I, K] = SQ2 * R[:, i, k] * R[:, i, l]
            elif K < 3:
                Q[:, I, K] = SQ2 * R[:, i, k] * R[:, j, k]
            else:
                Q[:, I, K] = R[:, i, k] * R[:, j, l] + R[:, i, l] * R[:, j, k]
    return Q


def rot_z(angle):
    """A material turned by +angle about z: the rows are the material axes."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def zero_state(n):
    return {"g": np.zeros((n, 12)), "p": np.zeros((n, 12)), "a": np.zeros((n, 12)), "eel": np.zeros((n, 6))}


def _sgn(x):
    return np.where(x > 0.0, 1.0, -1.0)   # 0 counts as -1, as in the file


def update(eps, state, params, dt, R=None, rtol=1e-14, maxit=25):
    """One implicit step.  eps (N, 6) total strain (global), state dict of (N, .) arrays g, p, a, eel; R None or (N, 3, 3) /
    (3, 3).  Returns a dict: stress (N, 6), tangent (N, 6, 6), g, p, a, eel, plastic, status (0 ok, 1 iteration cap, 2 guard at
    dg = 0), iters, halvings."""
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, 6)
    N = eps.shape[0]
    prm = np.asarray(params, dtype=np.float64)
    nn, K, tau0, Qc, b, d, C = prm[9:16]
    h = prm[16:22]
    D = stiffness(prm)
    mu = schmid()
    B = mu @ D              # (12, 6): B_i = D mu_i (D symmetric)
    M = B @ mu.T            # (12, 12)
    QH = Qc * h[interaction_classes()]
    floor = 1e-12 * D[0, 0]
    if R is None:
        Q = None
        em = eps.copy()
    else:
        Rb = np.broadcast_to(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), (N, 3, 3))
        Q = mandel_rotation(Rb)
        em = np.einsum("nik,nk->ni", Q, eps)
    g0, p0, a0 = state["g"], state["p"], state["a"]
    et = em - g0 @ mu
    tau_tr = et @ B.T

    def evaluate(dg, idx):
        adg = np.abs(dg)
        E = np.exp(-b * (p0[idx] + adg))
        tau = tau_tr[idx] - dg @ M.T
        r = tau0 + (1.0 - E) @ QH.T
        den = 1.0 / (1.0 + d * adg)
        da = (dg - d * a0[idx] * adg) * den
        y = tau - C * (a0[idx] + da)
        s = _sgn(y)
        f = np.maximum(np.abs(y) - r, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            fk = np.where(f > 0.0, (f / K) ** nn, 0.0)
        fg = dg - dt * fk * s
        return E, s, f, fk, fg, den, da

    _, _, f_tr, _, _, _, _ = evaluate(np.zeros((N, 12)), np.arange(N))
    plastic = (f_tr > 0.0).any(axis=1)
    dg_all = np.zeros((N, 12))
    X_all = np.zeros((N, 12, 6))
    status = np.zeros(N, dtype=int)
    iters = np.zeros(N, dtype=int)
    halvings = np.zeros(N, dtype=int)
    idx = np.nonzero(plastic)[0]
    dg = np.zeros((idx.size, 12))
    step = np.zeros_like(dg)
    it = np.zeros(idx.size, dtype=int)
    while idx.size:
        E, s, f, fk, fg, den, da = evaluate(dg, idx)
        guard = (f > 1.1 * K).any(axis=1)
        conv = ~(~(np.abs(fg) <= rtol)).any(axis=1)
        w = dt * (nn * fk / np.maximum(f, floor))
        dda = (1.0 - d * a0[idx] * _sgn(dg)) * den * den
        J = w[:, :, None] * (M[None] + s[:, :, None] * b * QH[None] * (E * _sgn(dg))[:, None, :])
        J[:, np.arange(12), np.arange(12)] += w * C * dda + 1.0
        rhs = np.concatenate([fg[:, :, None], w[:, :, None] * B[None]], axis=2)
        sol = np.linalg.solve(J, rhs)
        delta, X = sol[:, :, 0], sol[:, :, 1:]
        done = np.zeros(idx.size, dtype=bool)
        fail0 = guard & (it == 0)
        status[idx[fail0]] = 2
        dg[fail0] = 0.0
        done |= fail0
        halve = guard & (it > 0)
        step[halve] *= 0.5
        dg[halve] -= step[halve]
        it[halve] += 1
        halvings[idx[halve]] += 1
        capped = halve & (it >= maxit)
        status[idx[capped]] = 1
        done |= capped
        ok = ~guard
        step[ok] = -delta[ok]
        dg[ok] += step[ok]
        fin = ok & (conv | (it >= maxit))
        status[idx[fin & ~conv]] = 1
        X_all[idx[fin]] = X[fin]
        done |= fin
        it[ok & ~fin] += 1
        dg_all[idx[done]] = dg[done]
        iters[idx[done]] = it[done]
        keep = ~done
        idx, dg, step, it = idx[keep], dg[keep], step[keep], it[keep]

    moved = plastic & (status != 2)
    eel = et - dg_all @ mu
    sm = eel @ D
    Ctm = D[None] - np.einsum("ia,nik->nak", B, X_all)
    adg = np.abs(dg_all)
    da = (dg_all - d * a0 * adg) / (1.0 + d * adg)
    m = moved[:, None]
    out = {"g": np.where(m, g0 + dg_all, g0), "p": np.where(m, p0 + adg, p0), "a": np.where(m, a0 + da, a0),
           "eel": np.where((status == 2)[:, None], state["eel"], eel)}
    if Q is None:
        out["stress"], out["tangent"] = sm, Ctm
    else:
        out["stress"] = np.einsum("nik,ni->nk", Q, sm)
        out["tangent"] = np.einsum("nri,nrs,nsk->nik", Q, Ctm, Q)
    out.update(plastic=plastic, status=status, iters=iters, halvings=halvings)
    return out


def next_state(out):
    return {k: out[k].copy() for k in ("g", "p", "a", "eel")}
