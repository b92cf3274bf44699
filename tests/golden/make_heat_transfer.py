"""Writes ``heat_transfer_kat.npz``: known answers for the two heat-transfer laws from a 50-digit mpmath evaluation of the equations of
``StationaryHeatTransfer.mfront`` and ``HeatTransferPhaseChange.mfront`` (lines 41-56).

* The inputs (parameters, g, T) are doubles and are taken exactly; the arithmetic is carried out with 50 digits, ``Ts = Tm - Tsmooth/2``
  and ``Tl = Tm + Tsmooth/2`` included.  Only the BRANCH is chosen as the kernel and the restatement choose it: by comparing T with the
  doubles ``Ts`` and ``Tl`` (one rounded operation each).  k and h are continuous at both ends of the transition, so a point that the
  double comparison puts on the other side of the exact boundary differs by rounding only: no point is excluded.
* Two parameter sets per law: the file defaults; for the phase-change law the demo's ``Tsmooth = 1.0`` (``phase_change.py:266``), for
  the stationary law a second pair (A, B) of the same magnitude.
* Phase change: T spread over the three branches and placed exactly at Ts, Tm and Tl and at ``nextafter`` on both sides of Ts and Tl.
* ``meta`` records, per case and output group (flux, each tangent block, enthalpy), the deviation of the numpy restatement
  (``tests/heat_transfer_ref.py``) from the 50-digit values, relative to the group's largest magnitude.

    python tests/golden/make_heat_transfer.py        (needs mpmath; 272 points)"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import heat_transfer_ref as ht  # noqa: E402

mp.mp.dps = 50


def exact_stationary(g, T, prm):
    A, B = (mp.mpf(float(v)) for v in prm)
    flux, ct = [], []
    for gi, Ti in zip(g, T):
        k = 1 / (A + B * mp.mpf(float(Ti)))
        gv = [mp.mpf(float(x)) for x in gi]
        flux.append([-k * x for x in gv])
        ct.append([-k, 0, 0, 0, -k, 0, 0, 0, -k] + [B * k * k * x for x in gv])
    return flux, ct, None


def exact_phase_change(g, T, prm):
    Tm, ks, cs, kl, cl, dh, Tsm = (mp.mpf(float(v)) for v in prm)
    Ts_d, Tl_d = ht.solidus_liquidus(prm)          # the doubles the branch is chosen with
    Ts, Tl = Tm - Tsm / 2, Tm + Tsm / 2            # exact
    flux, ct, hs = [], [], []
    for gi, Ti in zip(g, T):
        t = mp.mpf(float(Ti))
        if Ti < Ts_d:
            k, c, h, kp = ks, cs, cs * t, mp.mpf(0)
        elif Ti > Tl_d:
            k, c, h, kp = kl, cl, cl * (t - Tl) + dh + cs * Ts + (cs + cl) * Tsm / 2, mp.mpf(0)
        else:
            k = ks + (kl - ks) * (t - Ts) / Tsm
            c = (cs + cl) / 2 + dh / Tsm
            h = cs * Ts + c * (t - Ts)
            kp = -(kl - ks) / Tsm
        gv = [mp.mpf(float(x)) for x in gi]
        flux.append([-k * x for x in gv])
        ct.append([-k, 0, 0, 0, -k, 0, 0, 0, -k] + [kp * x for x in gv] + [c])
        hs.append([h])
    return flux, ct, hs


def to_double(rows):
    return np.array([[float(x) for x in r] for r in rows], dtype=np.float64)


def phase_temperatures(prm, rng, nrandom):
    Ts, Tl = ht.solidus_liquidus(prm)
    Tm = np.float64(prm[0])
    edge = [Ts, Tm, Tl, np.nextafter(Ts, -np.inf), np.nextafter(Ts, np.inf), np.nextafter(Tl, -np.inf), np.nextafter(Tl, np.inf)]
    spread = np.concatenate([rng.uniform(300.0, Ts - 1.0, nrandom), rng.uniform(Ts, Tl, nrandom), rng.uniform(Tl + 1.0, 1500.0, nrandom),
                             Ts - rng.uniform(0, 1e-9, 4), Tl + rng.uniform(0, 1e-9, 4)])
    return np.concatenate([np.array(edge, dtype=np.float64), spread])


def main():
    rng = np.random.default_rng(20261019)
    out, cases = {}, []
    sets = [(ht.STATIONARY, "st0", ht.STATIONARY_DEFAULTS), (ht.STATIONARY, "st1", (0.05, 1.0e-4)),
            (ht.PHASE_CHANGE, "pc0", ht.PHASE_CHANGE_DEFAULTS), (ht.PHASE_CHANGE, "pc1", ht.PHASE_CHANGE_DEFAULTS[:6] + (1.0,))]
    for law, tag, prm in sets:
        prm = np.array(prm, dtype=np.float64)
        if law == ht.STATIONARY:
            T = np.concatenate([rng.uniform(250.0, 1600.0, 38), [ht.T_DEFAULT, 0.0]])
        else:
            T = phase_temperatures(prm, rng, 27)
        g = rng.normal(size=(len(T), 3)) * rng.choice([1.0, 1e3, 1e-3], size=(len(T), 1))
        g[0] = 0.0
        flux, ct, hs = (exact_stationary if law == ht.STATIONARY else exact_phase_change)(g, T, prm)
        exp = {"flux": to_double(flux)}
        ctd = to_double(ct)
        for name, cols in ht.GROUPS[law].items():
            exp[name] = ctd[:, cols]
        if hs is not None:
            exp["enthalpy"] = to_double(hs)
        got = ht.group_values(law, ht.update(law, g, T, prm))
        dev = {name: ht.relative_deviation(got[name], exp[name]) for name in exp}
        out[f"{tag}_params"], out[f"{tag}_g"], out[f"{tag}_T"] = prm, g, T
        for name, v in exp.items():
            out[f"{tag}_{name}"] = v
        cases.append({"law": law, "tag": tag, "points": int(len(T)), "groups": list(exp), "restatement_deviation": dev})
        print(tag, len(T), dev)
    total = sum(c["points"] for c in cases)
    assert total <= 300, total
    meta = {"digits": 50, "points": total, "cases": cases,
            "note": "restatement_deviation: max |numpy restatement - 50-digit value| per output group / max |50-digit value| of the group"}
    np.savez_compressed(os.path.join(HERE, "heat_transfer_kat.npz"), meta=np.array(json.dumps(meta)), **out)


if __name__ == "__main__":
    main()
