"""Writes ``plane_stress_hosford.npz``: plane-stress Hosford plasticity (DXM_LAW_PS_HOSFORD = 33) at 50 digits with mpmath, in a
form the kernel does not use.  Needs mpmath; the tests read the committed file only.

    python tests/golden/make_plane_stress_hosford.py

The kernel solves one bracketed root in a polar angle of the scaled principal plane.  Here the KKT system of the projection
    Cp^-1 (s - t) + lambda grad phi(s) = 0,   phi(s) = sig0          (s, t the principal stresses, Cp their stiffness)
is solved by ``findroot`` in (s_I, s_II, lambda), and a solution is accepted only if it is the global minimum: lambda > 0 and the
variational inequality (t - s)^T Cp^-1 (tau - s) <= 0 against 2000 points tau of the yield surface.  The tangent is ``mpmath.diff``
of that projection with respect to the strain, not the implicit formula.  Two increments; the second starts from the first one's
plastic strain as the file stores it (rounded to double)."""
import json
import os
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-6                     # every point at least this far (in sig0) from the yield surface
OVERSHOOTS = (1.0001, 1.01, 1.3, 3.0, 30.0, 1e3, 1e4)
NSURF = 2000


def phi(s1, s2, a):
    v = [abs(s1), abs(s2), abs(s1 - s2)]
    m = max(v)
    if m == 0:
        return mp.mpf(0)
    return m * (sum((x / m) ** a for x in v) / 2) ** (1 / mp.mpf(a))


def grad_phi(s1, s2, a):
    f = phi(s1, s2, a)
    w = [mp.sign(x) * (abs(x) / f) ** (a - 1) / 2 for x in (s1, s2, s1 - s2)]
    return w[0] + w[2], w[1] - w[2]


def surface(a, sig0):
    """NSURF points of the yield surface in the principal plane (doubles)"""
    ang = np.linspace(0.0, 2 * np.pi, NSURF, endpoint=False) + 0.001
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    v = np.abs(np.stack([d[:, 0], d[:, 1], d[:, 0] - d[:, 1]], axis=1))
    m = v.max(axis=1)
    f = m * (0.5 * ((v / m[:, None]) ** a).sum(axis=1)) ** (1.0 / a)
    return d * (sig0 / f)[:, None]


class Law:
    def __init__(self, E, nu, sig0, a):
        self.E, self.nu, self.sig0, self.a = (mp.mpf(v) for v in (E, nu, sig0, a))
        c0 = self.E / (1 - self.nu**2)
        self.c11, self.c12, self.c33 = c0, c0 * self.nu, c0 * (1 - self.nu)
        self.surf = surface(float(a), float(sig0))
        self.Cinv = np.array([[1.0, -float(nu)], [-float(nu), 1.0]]) / float(E)

    def principal_projection(self, t1, t2, guess, check):
        E, nu, a, sig0 = self.E, self.nu, self.a, self.sig0

        def kkt(s1, s2, lam):
            n1, n2 = grad_phi(s1, s2, a)
            return [((s1 - t1) - nu * (s2 - t2)) + E * lam * n1, ((s2 - t2) - nu * (s1 - t1)) + E * lam * n2, phi(s1, s2, a) / sig0 - 1]

        if guess is None:
            f = phi(t1, t2, a)
            g1, g2 = t1 * sig0 / f, t2 * sig0 / f
            n1, n2 = grad_phi(g1, g2, a)
            q1, q2 = self.c11 * n1 + self.c12 * n2, self.c12 * n1 + self.c11 * n2
            guess = (g1, g2, ((t1 - g1) * n1 + (t2 - g2) * n2) / (n1 * q1 + n2 * q2))
        sol = mp.findroot(kkt, guess, tol=mp.mpf(10) ** (-42), maxsteps=200)
        s1, s2, lam = sol[0], sol[1], sol[2]
        if check:
            assert lam > 0, (t1, t2, lam)
            assert abs(phi(s1, s2, a) / sig0 - 1) < mp.mpf(10) ** (-40)
            d = self.Cinv @ np.array([float(t1 - s1), float(t2 - s2)])
            gap = self.surf - np.array([float(s1), float(s2)])
            assert ((gap @ d) <= 1e-9 * np.linalg.norm(d) * np.linalg.norm(gap, axis=1)).all(), (t1, t2, s1, s2)
        return s1, s2, lam

    def project(self, eps, epn, guess=None, check=True):
        """(stress, yielded, (s_I, s_II, lambda))"""
        ee = [eps[k] - epn[k] for k in range(3)]
        t = [self.c11 * ee[0] + self.c12 * ee[1], self.c12 * ee[0] + self.c11 * ee[1], self.c33 * ee[2]]
        mean, dlt, tau = (t[0] + t[1]) / 2, (t[0] - t[1]) / 2, t[2] / mp.sqrt(2)
        r = mp.sqrt(dlt**2 + tau**2)
        p1, p2 = mean + r, mean - r
        f = phi(p1, p2, self.a)
        if check:
            assert abs(f / self.sig0 - 1) >= MARGIN, (eps, f)
        if f <= self.sig0:
            return t, False, None
        cs, sn = (dlt / r, tau / r) if r != 0 else (mp.mpf(1), mp.mpf(0))
        s1, s2, lam = self.principal_projection(p1, p2, guess, check)
        sm, sr = (s1 + s2) / 2, (s1 - s2) / 2
        return [sm + sr * cs, sm - sr * cs, sr * sn * mp.sqrt(2)], True, (s1, s2, lam)

    def point(self, eps, epn):
        """stress, plastic strain, tangent (mpmath.diff of the projection), yielded"""
        eps = [mp.mpf(float(v)) for v in eps]
        epn = [mp.mpf(float(v)) for v in epn]
        sig, pl, sol = self.project(eps, epn)
        if not pl:
            C = [[self.c11, self.c12, 0], [self.c12, self.c11, 0], [0, 0, self.c33]]
            return sig, epn, C, False
        E, nu = self.E, self.nu
        state = [eps[0] - (sig[0] - nu * sig[1]) / E, eps[1] - (sig[1] - nu * sig[0]) / E, eps[2] - (1 + nu) * sig[2] / E]
        D = [[None] * 3 for _ in range(3)]
        for j in range(3):
            memo = {}

            def column(x, j=j, memo=memo):
                key = mp.nstr(x, 80)
                if key not in memo:
                    e = list(eps)
                    e[j] = e[j] + x
                    memo[key] = self.project(e, epn, guess=sol, check=False)[0]
                return memo[key]

            for i in range(3):
                D[i][j] = mp.diff(lambda x, i=i: column(x)[i], 0)
        return sig, state, D, True


def rotate(p1, p2, ang):
    """the stress [xx, yy, sqrt(2) xy] with principal values p1, p2, the first axis at ``ang``"""
    m, d = 0.5 * (p1 + p2), 0.5 * (p1 - p2)
    return np.array([m + d * np.cos(2 * ang), m - d * np.cos(2 * ang), np.sqrt(2.0) * d * np.sin(2 * ang)])


def phi_np(p1, p2, a):
    v = np.abs([p1, p2, p1 - p2])
    m = v.max()
    return m * (0.5 * ((v / m) ** a).sum()) ** (1.0 / a)


def inputs(sig0, a):
    """trial stresses, and which of them keep loading in the second increment"""
    sig, far = [], []
    angles = (0.0, 0.3, 0.7853981633974483, 1.9, 2.9)
    for k in range(24):
        psi = 2 * np.pi * (k + 0.37) / 24
        d1, d2 = np.cos(psi), np.sin(psi)
        for j, ang in enumerate(angles):
            over = OVERSHOOTS[(k + 3 * j) % len(OVERSHOOTS)]
            sc = over * sig0 / phi_np(d1, d2, a)
            sig.append(rotate(d1 * sc, d2 * sc, ang))
            far.append(over >= 1e3)
    # the special rows: near-vertex directions, equal principal values with and without a frame angle, pure shear, no shear, the
    # axes of the folded quadrant (T_x = 0 is pure shear, T_y = 0 equal principal values)
    for over in (2.0, 50.0):
        for d1, d2 in ((1, 0), (1, 1), (0, 1), (-1, 0), (-1, -1), (0, -1)):
            sc = over * sig0 / phi_np(float(d1), float(d2), a)
            sig.append(rotate(d1 * sc, d2 * sc, 0.3))
            far.append(False)
        sc = over * sig0
        sig += [np.array([sc, sc, 0.0]), np.array([-sc, -sc, 0.0]), rotate(sc * (1 + 2.0 ** -50), sc, 0.7),   # (equal to 1e-15, a frame angle)
                np.array([0.0, 0.0, np.sqrt(2.0) * sc]), np.array([sc, -sc, 0.0]), np.array([-sc, sc, 0.0]),
                np.array([1.5 * sc, 0.4 * sc, 0.0]), np.array([-0.2 * sc, 1.1 * sc, 0.0])]
        far += [False] * 8
    # elastic points
    for k in range(6):
        psi = 2 * np.pi * (k + 0.11) / 6
        d1, d2 = np.cos(psi), np.sin(psi)
        sc = (0.3, 0.999)[k % 2] * sig0 / phi_np(d1, d2, a)
        sig.append(rotate(d1 * sc, d2 * sc, 0.4 * k))
        far.append(False)
    return np.array(sig), np.array(far)


def to_strain(E, nu, sig):
    S = np.array([[1.0, -nu, 0.0], [-nu, 1.0, 0.0], [0.0, 0.0, 1.0 + nu]]) / E
    return np.atleast_2d(sig) @ S.T


def second_increment(E, nu, sig0, eps1, epsp1, keep_loading, rng):
    """unload a third of the batch towards its plastic strain (elastic), reload the rest in a new direction; the far points keep going"""
    eps2 = np.empty_like(eps1)
    for i in range(len(eps1)):
        el = eps1[i] - epsp1[i]
        if keep_loading[i]:
            eps2[i] = eps1[i] + 0.5 * el
        elif i % 3 == 0:
            eps2[i] = eps1[i] - rng.uniform(0.3, 0.7) * el
        else:
            v = rng.normal(size=3)
            eps2[i] = eps1[i] + to_strain(E, nu, v / np.linalg.norm(v) * sig0 * rng.uniform(0.5, 3.0))[0]
    return eps2


def run_case(args):
    tag, prm, seed = args
    mp.mp.dps = 50
    E, nu, sig0, a = prm
    rng = np.random.default_rng(seed)
    law = Law(E, nu, sig0, a)
    sig_tr, far = inputs(sig0, a)
    eps = to_strain(E, nu, sig_tr)
    n = len(eps)
    epn = np.zeros((n, 3))
    out = {}
    for inc in (1, 2):
        res = [law.point(eps[i], epn[i]) for i in range(n)]
        out[f"{tag}_eps{inc}"] = eps
        out[f"{tag}_stress{inc}"] = np.array([[float(r[0][k]) for k in range(3)] for r in res])
        out[f"{tag}_state{inc}"] = np.array([[float(r[1][k]) for k in range(3)] for r in res])
        out[f"{tag}_tangent{inc}"] = np.array([[float(r[2][i][j]) for i in range(3) for j in range(3)] for r in res])
        out[f"{tag}_plastic{inc}"] = np.array([bool(r[3]) for r in res])
        epn = out[f"{tag}_state{inc}"]
        if inc == 1:
            eps = second_increment(E, nu, sig0, eps, epn, far, rng)
    out[f"{tag}_prm"] = np.array([E, nu, sig0, a, 0.0])
    return out, dict(tag=tag, points=n, yielded=[int(out[f"{tag}_plastic{k}"].sum()) for k in (1, 2)])


def main():
    E, sig0 = 70e3, 30.0
    jobs = [(f"a{a}_nu20", (E, 0.2, sig0, float(a)), 100 + a) for a in (2, 6, 8, 10, 20, 100)]
    jobs += [(f"a10_nu{tag}", (E, nu, sig0, 10.0), 200 + k) for k, (tag, nu) in enumerate((("0", 0.0), ("45", 0.45), ("m50", -0.5)))]
    out, cases = {}, []
    with ProcessPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
        for o, c in pool.map(run_case, jobs):
            out.update(o)
            cases.append(c)
            print(c, flush=True)
    out["meta"] = np.array(json.dumps(dict(digits=mp.mp.dps, margin=MARGIN, cases=cases)))
    np.savez_compressed(os.path.join(HERE, "plane_stress_hosford.npz"), **out)


if __name__ == "__main__":
    main()
