#!/usr/bin/env python3
"""Writes ``tests/golden/plane_stress_j2_sweep.npz``: plane-stress J2 plasticity with isotropic hardening (laws 30 and 31) at 50
digits over the seeded parameter draws, one-increment points and six-increment histories of ``tests/plane_stress_j2_cases.py``, in
the NESTED formulation of ``make_plane_stress_j2.py`` (3-D radial return, ``eps_zz`` from ``sig_zz = 0``, condensed tangent), which is
imported, not restated.  Its Voce root-finder moves the upper end of its bracket out until the residual is negative, so that it
holds for a softening ``R`` as well.

Per draw ``<law><k>``: ``_prm``, the inputs ``_eps, _epsp_n, _p_n`` and the results ``_stress, _tangent (D00, D01, D02, D11, D12,
D22), _p, _epsp, _plastic``; per history ``<law><k>_h<q>_...`` the strain and the results of increment q, the state carried at 50
digits.  Every point is at least 1e-6 ``sig0`` off the surface (asserted: the cases module draws such points again).

On the softening draws the generator also asserts, at every point: R >= 0.5 sig0 at the returned state; the residuals it solves
(``sig_zz`` over its bracket in ``eps_zz``, and for Voce ``seq - 3 mu dp - R(p_n + dp)`` over its bracket in ``dp``) change sign over
the bracket and are monotone on nine samples of it.

    python tests/golden/make_plane_stress_j2_sweep.py        (about a minute)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_plane_stress_j2 as base  # noqa: E402
import plane_stress_j2_cases as cs  # noqa: E402

SAMPLES = 9


def monotone(values, sign):
    return all(sign * (b - a) > 0 for a, b in zip(values[:-1], values[1:]))


def softening_asserts(law, prm, eps3, epsp3, p_n, res):
    """what the issue asks of a softening draw, at one point"""
    R, _ = base.hardening(law, prm)
    assert R(res["p"]) >= cs.R_FLOOR * mp.mpf(prm[2]), (prm, float(R(res["p"])))
    e3 = [mp.mpf(float(v)) for v in eps3]
    ep6 = [epsp3[0], epsp3[1], -(epsp3[0] + epsp3[1]), epsp3[2], mp.mpf(0), mp.mpf(0)]
    scale = sum(abs(v) for v in e3) + sum(abs(v) for v in epsp3) + mp.mpf(10) ** -6
    zs = [-4 * scale + 8 * scale * q / (SAMPLES - 1) for q in range(SAMPLES)]
    szz = [base.radial_return(law, prm, [e3[0], e3[1], z, e3[2], mp.mpf(0), mp.mpf(0)], ep6, p_n)[0][2] for z in zs]
    assert szz[0] < 0 < szz[-1] and monotone(szz, +1), [float(v) for v in szz]
    if law == base.VOCE and res["plastic"]:
        _, dp, _, _, f = base.radial_return(law, prm, [e3[0], e3[1], res["ezz"], e3[2], mp.mpf(0), mp.mpf(0)], ep6, p_n)
        mu = mp.mpf(prm[0]) / 2 / (1 + mp.mpf(prm[1]))
        seq = f + R(p_n)
        r = lambda x: seq - 3 * mu * x - R(p_n + x)      # noqa: E731
        hi = f / (3 * mu)
        while r(hi) > 0:
            hi *= 2
        rs = [r(hi * q / (SAMPLES - 1)) for q in range(SAMPLES)]
        assert rs[0] > 0 >= rs[-1] and monotone(rs, -1) and 0 < dp <= hi, [float(v) for v in rs]


def run(law, prm, k, eps, epsp_n, p_n):
    """one increment of every row at 50 digits; the state goes in and comes out as mpmath numbers"""
    out = []
    for i in range(len(eps)):
        seq, Rn = base.trial_overshoot(law, prm, eps[i], epsp_n[i], p_n[i])
        assert abs(seq - Rn) >= 0.999 * cs.OFF * prm[2], (cs.tag(law, k), i)
        r = base.plane_stress_update(law, prm, eps[i], list(epsp_n[i]), p_n[i])
        if cs.softening(law, k):
            softening_asserts(law, prm, eps[i], list(epsp_n[i]), p_n[i], r)
        out.append(r)
    return out


def store(out, key, rs):
    f = lambda v: np.array([[float(x) for x in r[v]] for r in rs])      # noqa: E731
    out[f"{key}_stress"], out[f"{key}_epsp"] = f("stress"), f("epsp")
    out[f"{key}_tangent"] = f("tangent")[:, [0, 1, 2, 4, 5, 8]]
    out[f"{key}_p"] = np.array([float(r["p"]) for r in rs])
    out[f"{key}_plastic"] = np.array([bool(r["plastic"]) for r in rs])


def main():
    out, meta = {}, {"dps": mp.mp.dps, "off_surface": cs.OFF, "draws": [], "histories": []}
    for law in cs.LAWS:
        for k in range(cs.N_DRAWS):
            prm, t = cs.draw(law, k), cs.tag(law, k)
            eps, ep, p, _ = cs.points(law, k)
            rs = run(law, prm, k, eps, [[mp.mpf(float(v)) for v in row] for row in ep], [mp.mpf(float(v)) for v in p])
            out[f"{t}_prm"], out[f"{t}_eps"], out[f"{t}_epsp_n"], out[f"{t}_p_n"] = np.array(prm), eps, ep, p
            store(out, t, rs)
            meta["draws"].append({"tag": t, "law": law, "draw": k, "points": len(eps), "plastic": int(out[f"{t}_plastic"].sum())})
            print(meta["draws"][-1], flush=True)
        for k in cs.HISTORY_DRAWS[law]:
            prm, t = cs.draw(law, k), cs.tag(law, k)
            n = cs.N_HISTORY
            ep, p = [[mp.mpf(0)] * 3 for _ in range(n)], [mp.mpf(0)] * n
            counts = []
            for q, eps in enumerate(cs.history(law, k)):
                rs = run(law, prm, k, eps, ep, p)
                ep, p = [r["epsp"] for r in rs], [r["p"] for r in rs]
                out[f"{t}_h{q}_eps"] = eps
                store(out, f"{t}_h{q}", rs)
                counts.append(int(out[f"{t}_h{q}_plastic"].sum()))
            meta["histories"].append({"tag": t, "law": law, "draw": k, "points": n, "plastic": counts})
            print(meta["histories"][-1], flush=True)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(cs.GOLDEN, **out)


if __name__ == "__main__":
    main()
