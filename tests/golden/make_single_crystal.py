"""Writes tests/golden/single_crystal_kat.npz: known answers of the FCC single-crystal viscoplastic law (law id 14) at 250 material
points -- 2 parameter sets x 5 frame classes (none, axis turns by 45 / 60 / 90 degrees about z, random) x 5 history stages
(elastic, first yield, developed flow, after a load reversal, near back-strain saturation) x 5 strain directions -- with every
expected number from a 50-digit evaluation that shares nothing with the float64 restatement but the equations:

* MFront's 18-unknown form (six elastic-strain components and twelve slip increments), solved by Newton at 50 digits with a
  difference-quotient Jacobian (step 1e-25);
* tensors as 3x3 arrays, the stiffness as a fourth-order tensor C_ijkl, frames applied as R eps R^T and R^T sigma R: neither the
  6x6 image Q of a frame nor a Mandel Schmid vector is ever formed;
* the tangent by implicit differentiation of those 18 equations with respect to the global strain components.

The histories that lead to each point's initial state are run by the restatement (tests/single_crystal_ref.py) with increments
of norm 1e-4 and dt = 0.1; the fixture stores that state, the last strain, and what the 50-digit law makes of them, plus the
deviation of the restatement from the 50-digit values relative to the field scale (the GPU bound is max(1e-12, 8 x that)).

    python tests/golden/make_single_crystal.py"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import single_crystal_ref as sc  # noqa: E402

mp.mp.dps = 50
DT = 0.1
STEP = 1e-4
STAGES = {"elastic": (3, 0), "first_yield": (11, 0), "developed": (30, 0), "reversal": (30, 14), "saturation": (60, 0)}
FRAMES = ("none", "z45", "z60", "z90", "random")
SETS = {
    "mfront": sc.param_vector(),
    "variant": sc.param_vector(dict(E1=150000.0, E2=180000.0, nu12=0.25, G13=70000.0, n=6.0, K=30.0, tau0=50.0, Q=20.0, b=4.0,
                                    d=300.0, C=10000.0), interaction=(1.0, 1.4, 0.7, 9.0, 1.9, 2.3)),
}
PER_CELL = 5
IJ = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def frame_of(cls, rng):
    if cls == "none":
        return None
    if cls == "random":
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[2] *= -1
        return q
    return sc.rot_z(np.deg2rad(float(cls[1:])))


# ---- the 50-digit law --------------------------------------------------------------------------------------
def mp_tensor(v6):
    """Mandel 6-vector (float or mp) -> symmetric 3x3 of mp numbers"""
    r2 = mp.sqrt(2)
    t = [[mp.mpf(0)] * 3 for _ in range(3)]
    for I, (i, j) in enumerate(IJ):
        x = mp.mpf(v6[I]) if I < 3 else mp.mpf(v6[I]) / r2
        t[i][j] = t[j][i] = x
    return t


def mp_mandel(t):
    r2 = mp.sqrt(2)
    return [t[i][j] if I < 3 else r2 * t[i][j] for I, (i, j) in enumerate(IJ)]


def mp_stiffness(p):
    E1, E2, E3, nu12, nu23, nu13, G12, G23, G13 = (mp.mpf(float(x)) for x in p[:9])
    S = mp.matrix([[1 / E1, -nu12 / E1, -nu13 / E1], [-nu12 / E1, 1 / E2, -nu23 / E2], [-nu13 / E1, -nu23 / E2, 1 / E3]])
    A = S ** -1
    Cc = [[[[mp.mpf(0)] * 3 for _ in range(3)] for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for j in range(3):
            Cc[i][i][j][j] = A[i, j]
    for (i, j), G in (((0, 1), G12), ((0, 2), G13), ((1, 2), G23)):
        Cc[i][j][i][j] = Cc[i][j][j][i] = Cc[j][i][i][j] = Cc[j][i][j][i] = G
    return Cc


def ddot4(Cc, e):
    return [[mp.fsum(Cc[i][j][k][l] * e[k][l] for k in range(3) for l in range(3)) for j in range(3)] for i in range(3)]


def rotate(R, t, back=False):
    """R t R^T, or R^T t R"""
    if back:
        return [[mp.fsum(R[k][i] * t[k][l] * R[l][j] for k in range(3) for l in range(3)) for j in range(3)] for i in range(3)]
    return [[mp.fsum(R[i][k] * t[k][l] * R[j][l] for k in range(3) for l in range(3)) for j in range(3)] for i in range(3)]


class MpLaw:
    def __init__(self, p):
        self.C4 = mp_stiffness(p)
        self.n, self.K, self.tau0, self.Q, self.b, self.d, self.C = (mp.mpf(float(x)) for x in p[9:16])
        h = [mp.mpf(float(x)) for x in p[16:22]]
        # the geometry again, on its own: plane-major systems and the class of every pair [self, coplanar, Hirth, collinear, glissile, Lomer]
        planes, dirs = ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1)), ((0, 1, -1), (1, 0, -1), (1, -1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0))
        pairs = [(n, s) for n in planes for s in dirs if sum(a * b for a, b in zip(n, s)) == 0]
        nrm, sl = [n for n, _ in pairs], [s for _, s in pairs]
        cross = lambda u, v: (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])  # noqa: E731
        par = lambda u, v: cross(u, v) == (0, 0, 0)  # noqa: E731

        def klass(i, j):
            if i == j:
                return 0
            if nrm[i] == nrm[j]:
                return 1
            if par(sl[i], sl[j]):
                return 3
            if sum(a * b for a, b in zip(sl[i], sl[j])) == 0:
                return 2
            return 4 if par(sl[i], cross(nrm[i], nrm[j])) or par(sl[j], cross(nrm[i], nrm[j])) else 5
        self.h = [[h[klass(i, j)] for j in range(12)] for i in range(12)]
        s3, s2 = mp.sqrt(3), mp.sqrt(2)
        self.sch = []
        for ni, si in zip(nrm, sl):
            nv, sv = [mp.mpf(int(x)) / s3 for x in ni], [mp.mpf(int(x)) / s2 for x in si]
            self.sch.append([[(sv[i] * nv[j] + sv[j] * nv[i]) / 2 for j in range(3)] for i in range(3)])

    def residual(self, x, em, g0, p0, a0, dt):
        """x: 6 elastic-strain components (IJ order, tensor values) + 12 slip increments"""
        eel = [[mp.mpf(0)] * 3 for _ in range(3)]
        for I, (i, j) in enumerate(IJ):
            eel[i][j] = eel[j][i] = x[I]
        dg = x[6:]
        sig = ddot4(self.C4, eel)
        out = []
        for I, (i, j) in enumerate(IJ):
            out.append(eel[i][j] - em[i][j] + mp.fsum((g0[k] + dg[k]) * self.sch[k][i][j] for k in range(12)))
        ex = [mp.exp(-self.b * (p0[k] + abs(dg[k]))) for k in range(12)]
        for k in range(12):
            tau = mp.fsum(sig[i][j] * self.sch[k][i][j] for i in range(3) for j in range(3))
            r = self.tau0 + self.Q * mp.fsum(self.h[k][j] * (1 - ex[j]) for j in range(12))
            da = (dg[k] - self.d * a0[k] * abs(dg[k])) / (1 + self.d * abs(dg[k]))
            y = tau - self.C * (a0[k] + da)
            f = max(abs(y) - r, mp.mpf(0))
            s = 1 if y > 0 else -1
            out.append(dg[k] - dt * (f / self.K) ** self.n * s)
        return out, sig

    def jacobian(self, x, F0, args):
        hstep = mp.mpf(10) ** -25
        J = mp.matrix(18, 18)
        for c in range(18):
            xp = list(x)
            xp[c] += hstep
            Fp, _ = self.residual(xp, *args)
            for r in range(18):
                J[r, c] = (Fp[r] - F0[r]) / hstep
        return J

    def solve(self, eps6, R, g0, p0, a0, dt, dg_start):
        eg = mp_tensor(eps6)
        Rm = None if R is None else [[mp.mpf(float(R[i][j])) for j in range(3)] for i in range(3)]
        em = eg if Rm is None else rotate(Rm, eg)
        g0, p0, a0 = ([mp.mpf(v) for v in w] for w in (g0, p0, a0))   # floats, or the 50-digit state of a path
        dt = mp.mpf(dt)
        args = (em, g0, p0, a0, dt)
        dg = [mp.mpf(float(v)) for v in dg_start]
        x = [em[i][j] - mp.fsum((g0[k] + dg[k]) * self.sch[k][i][j] for k in range(12)) for (i, j) in IJ] + dg
        for it in range(12):
            F, sig = self.residual(x, *args)
            if max(abs(v) for v in F) < mp.mpf(10) ** -45:
                break
            J = self.jacobian(x, F, args)
            dx = mp.lu_solve(J, mp.matrix(F))
            x = [x[k] - dx[k] for k in range(18)]
        else:
            raise RuntimeError("the 50-digit Newton did not converge")
        F, sig = self.residual(x, *args)
        J = self.jacobian(x, F, args)
        # d x / d (global strain component K): F depends on the strain through em only
        cols = []
        for K, (k, l) in enumerate(IJ):
            dE = [[mp.mpf(0)] * 3 for _ in range(3)]
            dE[k][l] = dE[l][k] = mp.mpf(1)
            dem = dE if Rm is None else rotate(Rm, dE)
            rhs = mp.matrix([dem[i][j] for (i, j) in IJ] + [0] * 12)
            dx = mp.lu_solve(J, rhs)
            deel = [[mp.mpf(0)] * 3 for _ in range(3)]
            for I, (i, j) in enumerate(IJ):
                deel[i][j] = deel[j][i] = dx[I]
            dsm = ddot4(self.C4, deel)
            cols.append(dsm if Rm is None else rotate(Rm, dsm, back=True))
        r2 = mp.sqrt(2)
        ct = [[(cols[K][i][j] * (1 if I < 3 else r2)) / (1 if K < 3 else r2) for K in range(6)] for I, (i, j) in enumerate(IJ)]
        sg = sig if Rm is None else rotate(Rm, sig, back=True)
        dg = x[6:]
        eel = [[mp.mpf(0)] * 3 for _ in range(3)]
        for I, (i, j) in enumerate(IJ):
            eel[i][j] = eel[j][i] = x[I]
        new_a = [a0[k] + (dg[k] - self.d * a0[k] * abs(dg[k])) / (1 + self.d * abs(dg[k])) for k in range(12)]
        return {"stress": mp_mandel(sg), "tangent": ct, "eel": mp_mandel(eel), "g": [g0[k] + dg[k] for k in range(12)],
                "p": [p0[k] + abs(dg[k]) for k in range(12)], "a": new_a}


def material_point_path():
    """The material-point form of the reference's test_mfront_single_cristal at 50 digits: strain [exx, eyy, 0, exy, 0, 0] with
    sigma_yy = sigma_xy = 0, 50 increments of exx to 5e-3, dt = 0.1, the crystal turned about z by 0, pi/4, pi/3, pi/2.  The
    restatement walks the path first (outer Newton with its own tangent); at each increment the 50-digit law starts from that
    strain, carries its own 50-digit state, and corrects (eyy, exy) by Newton with its own tangent until the two stresses vanish
    to 1e-25.  Returns sigma_xx after the first and after the last increment, per angle."""
    prm = SETS["mfront"]
    law = MpLaw(prm)
    angles = (0.0, np.pi / 4, np.pi / 3, np.pi / 2)
    first, last = [], []
    for ang in angles:
        R = sc.rot_z(ang)
        st = sc.zero_state(1)
        eps = np.zeros((1, 6))
        g, p, a = ([mp.mpf(0)] * 12 for _ in range(3))
        for k in range(1, 51):
            eps[0, 0] = k * STEP
            for _ in range(30):
                out = sc.update(eps, st, prm, DT, R=R[None])
                r = out["stress"][:, [1, 3]]
                if np.abs(r).max() <= 1e-9:
                    break
                eps[:, [1, 3]] -= np.linalg.solve(out["tangent"][:, [1, 3]][:, :, [1, 3]], r[:, :, None])[:, :, 0]
            dg = out["g"][0] - st["g"][0]
            st = sc.next_state(out)
            e = [mp.mpf(float(v)) for v in eps[0]]
            for _ in range(6):
                ref = law.solve(e, R, g, p, a, DT, dg)
                ryy, rxy = ref["stress"][1], ref["stress"][3]
                if max(abs(ryy), abs(rxy)) < mp.mpf(10) ** -25:
                    break
                T = ref["tangent"]
                dx = mp.lu_solve(mp.matrix([[T[1][1], T[1][3]], [T[3][1], T[3][3]]]), mp.matrix([ryy, rxy]))
                e[1] -= dx[0]
                e[3] -= dx[1]
            else:
                raise RuntimeError("the 50-digit outer Newton did not converge")
            g, p, a = ref["g"], ref["p"], ref["a"]
            if k == 1:
                first.append(float(ref["stress"][0]))
        last.append(float(ref["stress"][0]))
        print("material point", ang, first[-1], last[-1], flush=True)
    return np.array(angles), np.array(first), np.array(last)


def tofloat(v):
    return np.array([[float(x) for x in row] for row in v]) if isinstance(v[0], list) else np.array([float(x) for x in v])


def main():
    rng = np.random.default_rng(20260114)
    rec = {k: [] for k in ("set", "frame", "stage", "has_frame", "R", "eps", "g0", "p0", "a0", "eel0", "stress", "tangent", "eel", "g", "p", "a",
                           "plastic", "iters")}
    dev = {"stress": 0.0, "tangent": 0.0, "state": 0.0}
    antisym = 0.0
    for si, (sname, prm) in enumerate(SETS.items()):
        law = MpLaw(prm)
        for fi, fcls in enumerate(FRAMES):
            for gi, (stage, (up, down)) in enumerate(STAGES.items()):
                for rep in range(PER_CELL):
                    R = frame_of(fcls, rng)
                    dirn = rng.normal(size=6) * np.array([1, 1, 1, 0.7, 0.7, 0.7])
                    dirn[rep % 3] += 1.5   # a strong normal component: slip is reached within the history
                    dirn /= np.linalg.norm(dirn)
                    path = [k * STEP * dirn for k in range(1, up + 1)] + [(up - k) * STEP * dirn for k in range(1, down + 1)]
                    st = sc.zero_state(1)
                    for e in path[:-1]:
                        out = sc.update(e[None], st, prm, DT, R=None if R is None else R[None])
                        assert out["status"][0] == 0
                        st = sc.next_state(out)
                    eps = path[-1]
                    out = sc.update(eps[None], st, prm, DT, R=None if R is None else R[None])
                    assert out["status"][0] == 0
                    dg = out["g"][0] - st["g"][0]
                    ref = law.solve(eps, R, st["g"][0], st["p"][0], st["a"][0], DT, dg)
                    S, T = tofloat(ref["stress"]), tofloat(ref["tangent"])
                    dev["stress"] = max(dev["stress"], np.abs(out["stress"][0] - S).max() / np.abs(S).max())
                    dev["tangent"] = max(dev["tangent"], np.abs(out["tangent"][0] - T).max() / np.abs(T).max())
                    for k in ("eel", "g", "p", "a"):
                        v = tofloat(ref[k])
                        scale = max(np.abs(v).max(), np.abs(tofloat(ref["eel"])).max())
                        dev["state"] = max(dev["state"], np.abs(out[k][0] - v).max() / scale)
                    antisym = max(antisym, np.abs(T - T.T).max() / np.abs(T).max())
                    for k, v in (("set", si), ("frame", fi), ("stage", gi), ("has_frame", R is not None), ("R", np.eye(3) if R is None else R),
                                 ("eps", eps), ("g0", st["g"][0]), ("p0", st["p"][0]), ("a0", st["a"][0]), ("eel0", st["eel"][0]),
                                 ("stress", S), ("tangent", T), ("eel", tofloat(ref["eel"])), ("g", tofloat(ref["g"])),
                                 ("p", tofloat(ref["p"])), ("a", tofloat(ref["a"])), ("plastic", bool(out["plastic"][0])),
                                 ("iters", int(out["iters"][0]))):
                        rec[k].append(v)
            print(sname, fcls, dev, antisym, flush=True)
    meta = {"restatement_deviation": dev, "max_antisymmetric_part": antisym, "sets": list(SETS), "frames": list(FRAMES),
            "stages": list(STAGES), "dt": DT, "digits": mp.mp.dps}
    arrays = {k: np.array(v) for k, v in rec.items()}
    arrays["params"] = np.array([SETS[k] for k in SETS])
    arrays["mp_angles"], arrays["mp_first_sxx"], arrays["mp_last_sxx"] = material_point_path()
    np.savez_compressed(os.path.join(HERE, "single_crystal_kat.npz"), meta=json.dumps(meta), **arrays)
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
