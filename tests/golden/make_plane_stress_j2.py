#!/usr/bin/env python3
"""Writes ``tests/golden/plane_stress_j2.npz``: plane-stress J2 plasticity with isotropic hardening (DXM_LAW_PS_J2_LINEAR = 30,
DXM_LAW_PS_J2_VOCE = 31) at 50 digits (mpmath), in a formulation of its own -- the NESTED one, not the kernel's in-plane form:

* the 3-D radial return of laws 1 / 2 on the 6-wide strain ``[xx, yy, zz, sqrt(2) xy, 0, 0]`` is written out here (deviator, trial
  von Mises stress, ``dp`` in closed form for linear hardening and by a bracketing ``findroot`` on ``seq - 3 mu dp - R(p_n + dp)`` for
  Voce), with the plastic strain embedded as ``epsp_zz = -(epsp_xx + epsp_yy)``;
* ``eps_zz`` is found by a bracketing ``findroot`` (Illinois) so that ``sig_zz = 0``;
* the tangent is the 6x6 consistent tangent ``c1 1x1 + c2 I + c3 n x n`` of that return, condensed: ``D_ij - D_iz D_zj / D_zz`` on the
  components ``[0, 1, 3]``.

About 250 points per law over two increments from the virgin state; the second increment unloads part of the batch.  Trial
overshoots ``seq_trial / R(p_n)`` from 1.0001 to 1e4 (and elastic points); every point is at least 1e-6 ``sig0`` off the surface in
both increments.  Parameters: ``H = 0, 5e3, E`` and Voce ``(350, 500, 1e3)``, ``E = 70e3, nu = 0.3``.  Fixed seed.

    python tests/golden/make_plane_stress_j2.py
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
LINEAR, VOCE = 30, 31
E, NU = 70e3, 0.3
CASES = (("linear_H0", LINEAR, [E, NU, 250.0, 0.0], 84), ("linear_H5e3", LINEAR, [E, NU, 250.0, 5e3], 84), ("linear_HE", LINEAR, [E, NU, 250.0, E], 84),
         ("voce", VOCE, [E, NU, 350.0, 500.0, 1e3], 250))
OFF = 1e-6     # of sig0: the least distance of a trial from the surface
ONE = [1, 1, 1, 0, 0, 0]


def hardening(law, prm):
    if law == LINEAR:
        sig0, H = mp.mpf(prm[2]), mp.mpf(prm[3])
        return (lambda p: sig0 + H * p), (lambda p: H)
    sig0, sigu, b = mp.mpf(prm[2]), mp.mpf(prm[3]), mp.mpf(prm[4])
    return (lambda p: sig0 + (sigu - sig0) * (1 - mp.exp(-b * p))), (lambda p: (sigu - sig0) * b * mp.exp(-b * p))


def radial_return(law, prm, eps6, epsp6, p_n):
    """the 3-D update: (sig (6), dp, n (6), (c1, c2, c3), f_trial)"""
    Em, num = mp.mpf(prm[0]), mp.mpf(prm[1])
    lam, mu = Em * num / (1 + num) / (1 - 2 * num), Em / 2 / (1 + num)
    R, dR = hardening(law, prm)
    e = [a - b for a, b in zip(eps6, epsp6)]
    tr = e[0] + e[1] + e[2]
    se = [2 * mu * (e[k] - tr / 3 * ONE[k]) for k in range(6)]
    seq = mp.sqrt(mp.mpf(3) / 2 * sum(s * s for s in se))
    f = seq - R(p_n)
    if f <= 0:
        sig = [lam * tr * ONE[k] + 2 * mu * e[k] for k in range(6)]
        return sig, mp.mpf(0), [mp.mpf(0)] * 6, (lam, 2 * mu, mp.mpf(0)), f
    if law == LINEAR:
        dp = f / (mp.mpf(prm[3]) + 3 * mu)
    else:
        r = lambda x: seq - 3 * mu * x - R(p_n + x)    # noqa: E731  r(0) = f > 0, r(f / (3 mu)) <= 0 for a hardening R
        hi = f / (3 * mu)
        while r(hi) > 0:                               # a softening R: the root lies beyond, the end moves out until r is negative
            hi *= 2
        assert r(mp.mpf(0)) > 0 >= r(hi)
        dp = mp.findroot(r, (mp.mpf(0), hi), solver="illinois", tol=mp.mpf(10) ** -47, maxsteps=400, verify=False)
        assert abs(r(dp)) <= mp.mpf(10) ** -44 * seq
    n = [mp.mpf(3) / 2 * s / seq for s in se]
    e = [e[k] - dp * n[k] for k in range(6)]
    tr = e[0] + e[1] + e[2]
    sig = [lam * tr * ONE[k] + 2 * mu * e[k] for k in range(6)]
    beta, gamma = dp / seq, 1 / (dR(p_n + dp) + 3 * mu)
    return sig, dp, n, (lam + 2 * mu * mu * beta, 2 * mu - 6 * mu * mu * beta, 4 * mu * mu * (beta - gamma)), f


def plane_stress_update(law, prm, eps3, epsp3, p_n):
    """eps_zz with sig_zz = 0; the in-plane outputs and the condensed tangent"""
    eps3 = [mp.mpf(float(v)) for v in eps3]
    epsp6 = [epsp3[0], epsp3[1], -(epsp3[0] + epsp3[1]), epsp3[2], mp.mpf(0), mp.mpf(0)]
    eps6 = lambda z: [eps3[0], eps3[1], z, eps3[2], mp.mpf(0), mp.mpf(0)]    # noqa: E731
    szz = lambda z: radial_return(law, prm, eps6(z), epsp6, p_n)[0][2]      # noqa: E731  increasing in z
    scale = sum(abs(v) for v in eps3) + sum(abs(v) for v in epsp3) + mp.mpf(10) ** -6
    lo, hi = -4 * scale, 4 * scale
    assert szz(lo) < 0 < szz(hi)
    z = mp.findroot(szz, (lo, hi), solver="illinois", tol=mp.mpf(10) ** -47, maxsteps=1000, verify=False)
    sig, dp, n, (c1, c2, c3), f = radial_return(law, prm, eps6(z), epsp6, p_n)
    assert abs(sig[2]) <= mp.mpf(10) ** -42 * mp.mpf(prm[0]) * scale and sig[4] == 0 and sig[5] == 0
    Dfull = [[c1 * ONE[i] * ONE[j] + (c2 if i == j else 0) + c3 * n[i] * n[j] for j in range(6)] for i in range(6)]
    idx = (0, 1, 3)
    D = [[Dfull[i][j] - Dfull[i][2] * Dfull[2][j] / Dfull[2][2] for j in idx] for i in idx]
    epsp = [epsp3[k] + dp * n[i] for k, i in enumerate(idx)]
    return dict(stress=[sig[i] for i in idx], tangent=[v for row in D for v in row], p=p_n + dp, epsp=epsp, plastic=f > 0, ezz=z)


def trial_overshoot(law, prm, eps3, epsp3, p_n):
    """seq of C_ps (eps - epsp) over R(p_n), in double precision: what decides how far a point is from the surface"""
    Ed, nud = prm[0], prm[1]
    C = (Ed / (1 - nud**2)) * np.array([[1.0, nud, 0.0], [nud, 1.0, 0.0], [0.0, 0.0, 1.0 - nud]])
    t = C @ (np.asarray(eps3, dtype=float) - np.array([float(v) for v in epsp3]))
    seq = np.sqrt(t[0] ** 2 + t[1] ** 2 - t[0] * t[1] + 1.5 * t[2] ** 2)
    R, _ = hardening(law, prm)
    return seq, float(R(p_n))


def main():
    rng = np.random.default_rng(20261020)
    out, meta = {}, {"cases": [], "dps": mp.mp.dps, "off_surface": OFF}
    for tag, law, prm, count in CASES:
        Ed, nud, sig0 = prm[0], prm[1], prm[2]
        S = np.array([[1.0, -nud, 0.0], [-nud, 1.0, 0.0], [0.0, 0.0, 1.0 + nud]]) / Ed
        eps1, eps2 = np.zeros((count, 3)), np.zeros((count, 3))
        res = [[], []]
        for k in range(count):
            zero3, zero = [mp.mpf(0)] * 3, mp.mpf(0)
            while True:
                v = rng.normal(size=3)
                v *= sig0 / np.sqrt(v[0] ** 2 + v[1] ** 2 - v[0] * v[1] + 1.5 * v[2] ** 2)
                # a fifth elastic, the rest at overshoots 1.0001 ... 1e4 (log-uniform, both ends present)
                if k % 5 == 0:
                    over = rng.uniform(0.05, 0.99)
                else:
                    over = {1: 1.0001, 2: 1e4}.get(k, float(np.exp(rng.uniform(np.log(1.0001), np.log(1e4)))))
                e1 = S @ (v * over)
                seq, R0 = trial_overshoot(law, prm, e1, zero3, zero)
                if abs(seq - R0) >= OFF * sig0:
                    break
            r1 = plane_stress_update(law, prm, e1, zero3, zero)
            while True:
                # a third unloads (elastic from the new state), the others go on: further along, or in a new direction
                kind = k % 3
                w = rng.normal(size=3)
                w *= sig0 / np.sqrt(w[0] ** 2 + w[1] ** 2 - w[0] * w[1] + 1.5 * w[2] ** 2)
                if kind == 0:
                    e2 = e1 - S @ (np.array([float(s) for s in r1["stress"]]) * rng.uniform(0.1, 0.9))
                elif kind == 1:
                    e2 = e1 * rng.uniform(1.05, 3.0)
                else:
                    e2 = e1 + S @ (w * float(np.exp(rng.uniform(np.log(0.1), np.log(1e3)))))
                seq, Rn = trial_overshoot(law, prm, e2, r1["epsp"], r1["p"])
                if abs(seq - Rn) >= OFF * sig0:
                    break
            r2 = plane_stress_update(law, prm, e2, r1["epsp"], r1["p"])
            eps1[k], eps2[k] = e1, e2
            res[0].append(r1)
            res[1].append(r2)
        out[f"{tag}_prm"] = np.array(prm)
        out[f"{tag}_eps1"], out[f"{tag}_eps2"] = eps1, eps2
        for inc, rs in zip((1, 2), res):
            out[f"{tag}_stress{inc}"] = np.array([[float(v) for v in r["stress"]] for r in rs])
            out[f"{tag}_tangent{inc}"] = np.array([[float(v) for v in r["tangent"]] for r in rs])
            out[f"{tag}_p{inc}"] = np.array([float(r["p"]) for r in rs])
            out[f"{tag}_epsp{inc}"] = np.array([[float(v) for v in r["epsp"]] for r in rs])
            out[f"{tag}_ezz{inc}"] = np.array([float(r["ezz"]) for r in rs])
            out[f"{tag}_plastic{inc}"] = np.array([bool(r["plastic"]) for r in rs])
        meta["cases"].append({"tag": tag, "law": law, "points": count,
                              "plastic": [int(out[f"{tag}_plastic1"].sum()), int(out[f"{tag}_plastic2"].sum())]})
        print(tag, meta["cases"][-1], flush=True)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "plane_stress_j2.npz"), **out)


if __name__ == "__main__":
    main()
