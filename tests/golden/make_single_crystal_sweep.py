"""Writes tests/golden/single_crystal_sweep.npz: the harvested single-step cases of ``single_crystal_cases.harvest`` (every branch of the
local Newton of law id 14) and, for the histories of ``single_crystal_cases.history``, how far the float64 restatement
``single_crystal_ref.update`` is from the 50-digit 18-unknown law of ``make_single_crystal.py`` (imported, not copied).

* Harvested cases with status 0, the halved ones among them: the 50-digit Newton starts at the restatement's converged (eel, dg) and
  has to reach a residual below 1e-40 (``MpLaw.solve`` stops below 1e-45 or raises): the halved iteration landed on a root.  The
  50-digit stress, tangent and state are stored with the restatement's deviation from them, per case.
* Histories: at the first MP_SAMPLE points of a seed that never leave status 0 the whole history is walked at 50 digits, increment
  after increment, carrying the 50-digit state (the Newton starts at the restatement's slip increment).  Stored: the restatement's
  deviation at the last increment, at the increment after the reversal and the largest over all increments, and the 50-digit values
  at the first two of these.
* Bounds, per field group (stress, state, tangent), per seed and per harvest corner: max(the field's existing bound, 8 x the
  largest recorded deviation); the existing bounds are 1e-12, 1e-12 and 3.8e-11.  Deviations and bounds are both stored.  Nothing
  about the GPU enters the file.

    python tests/golden/make_single_crystal_sweep.py          (about two minutes on 16 cores; the harvest is most of it)"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_single_crystal as gen  # noqa: E402
import single_crystal_cases as cs  # noqa: E402
import single_crystal_ref as sc  # noqa: E402

GROUPS = ("stress", "tangent", "state")


def deviation(out, i, ref):
    """the restatement's point i against 50-digit values, relative to the field scale, as make_single_crystal.py measures it"""
    S, T = gen.tofloat(ref["stress"]), gen.tofloat(ref["tangent"])
    vals = {k: gen.tofloat(ref[k]) for k in cs.FIELDS}
    scale = max(np.abs(v).max() for v in vals.values())
    dev = {"stress": np.abs(out["stress"][i] - S).max() / np.abs(S).max(), "tangent": np.abs(out["tangent"][i] - T).max() / np.abs(T).max(),
           "state": max(np.abs(out[k][i] - vals[k]).max() for k in cs.FIELDS) / scale}
    return dev, S, T, np.concatenate([vals[k] for k in cs.FIELDS])


def solve_case(args):
    """one harvested case of status 0 at 50 digits"""
    prm, dt, eps, R, state = args
    out = sc.update(eps[None], {k: v[None] for k, v in state.items()}, prm, dt, R=R[None])
    assert out["status"][0] == 0
    ref = gen.MpLaw(prm).solve(eps, R, state["g"], state["p"], state["a"], dt, out["g"][0] - state["g"])
    return deviation(out, 0, ref)


def walk_point(args):
    """one point of one seed's history at 50 digits: the deviations of every increment and the values at two of them"""
    seed, i = args
    hist = cs.history(seed, cs.N_SWEEP)
    law = gen.MpLaw(hist["prm"])
    g, p, a = ([gen.mp.mpf(0)] * 12 for _ in range(3))
    g_prev = np.zeros(12)
    devs, keep = [], {}
    for inc in range(cs.N_INC):
        out = hist["ref"][inc]
        ref = law.solve(hist["eps"][inc][i], hist["R"][i], g, p, a, hist["dt"], out["g"][i] - g_prev)
        g, p, a, g_prev = ref["g"], ref["p"], ref["a"], out["g"][i]
        dev, S, T, V = deviation(out, i, ref)
        devs.append([dev[k] for k in GROUPS])
        if inc in (cs.REVERSAL + 1, cs.N_INC - 1):
            keep[inc] = (S, T, V)
    return seed, i, np.array(devs), keep


def bound(group, dev):
    return max(cs.EXISTING_BOUND[group], 8.0 * float(dev))


def sample_points(hist):
    return np.nonzero(hist["first_fail"] == 0)[0][:cs.MP_SAMPLE]


def main():
    hv = cs.harvest(verbose=True)
    n = len(hv["cls"])
    ok = np.nonzero(hv["status"] == 0)[0]
    points = [(seed, int(i)) for seed in cs.SEEDS for i in sample_points(cs.history(seed, cs.N_SWEEP))]   # computed before the fork
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        jobs = []
        for i in ok:
            _, prm, dt = cs.CORNERS[hv["corner"][i]]
            eps, R, st = cs.harvest_inputs(hv, i)
            jobs.append((prm, dt, eps, R, st))
        solved = pool.map(solve_case, jobs)
        walked = pool.map(walk_point, points)
    arrays = {f"hv_{k}": v for k, v in hv.items()}
    arrays["hv_stress"], arrays["hv_tangent"], arrays["hv_state"] = np.full((n, 6), np.nan), np.full((n, 6, 6), np.nan), np.full((n, 42), np.nan)
    arrays["hv_dev"] = np.full((n, 3), np.nan)
    for i, (dev, S, T, V) in zip(ok, solved):
        arrays["hv_stress"][i], arrays["hv_tangent"][i], arrays["hv_state"][i] = S, T, V
        arrays["hv_dev"][i] = [dev[k] for k in GROUPS]
    nc = len(cs.CORNERS)
    arrays["hv_corner_dev"] = np.array([[np.nanmax(arrays["hv_dev"][hv["corner"] == c, g], initial=0.0) for g in range(3)] for c in range(nc)])
    arrays["hv_corner_bound"] = np.array([[bound(GROUPS[g], arrays["hv_corner_dev"][c, g]) for g in range(3)] for c in range(nc)])
    ns, m = len(cs.SEEDS), cs.MP_SAMPLE
    arrays["hist_sample"] = np.zeros((ns, m), dtype=int)
    for k in ("hist_dev_last", "hist_dev_reversal", "hist_dev_all"):
        arrays[k] = np.zeros((ns, 3))
    for tag in ("last", "reversal"):
        arrays[f"hist_{tag}_stress"], arrays[f"hist_{tag}_tangent"], arrays[f"hist_{tag}_state"] = np.zeros((ns, m, 6)), np.zeros((ns, m, 6, 6)), np.zeros((ns, m, 42))
    slot = {seed: 0 for seed in cs.SEEDS}
    for seed, i, devs, keep in walked:
        j = slot[seed]
        slot[seed] += 1
        arrays["hist_sample"][seed, j] = i
        arrays["hist_dev_all"][seed] = np.maximum(arrays["hist_dev_all"][seed], devs.max(axis=0))
        arrays["hist_dev_last"][seed] = np.maximum(arrays["hist_dev_last"][seed], devs[-1])
        arrays["hist_dev_reversal"][seed] = np.maximum(arrays["hist_dev_reversal"][seed], devs[cs.REVERSAL + 1])
        for tag, inc in (("last", cs.N_INC - 1), ("reversal", cs.REVERSAL + 1)):
            arrays[f"hist_{tag}_stress"][seed, j], arrays[f"hist_{tag}_tangent"][seed, j], arrays[f"hist_{tag}_state"][seed, j] = keep[inc]
    assert all(v == m for v in slot.values())
    arrays["hist_bound"] = np.array([[bound(GROUPS[g], arrays["hist_dev_all"][s, g]) for g in range(3)] for s in range(ns)])
    meta = {"groups": list(GROUPS), "classes": list(cs.CLASSES), "corners": [c[0] for c in cs.CORNERS], "digits": gen.mp.mp.dps,
            "mp_sample": m, "n_points": cs.N_SWEEP, "increments": cs.N_INC, "step_norm": list(cs.STEP_NORM)}
    np.savez_compressed(os.path.join(HERE, "single_crystal_sweep.npz"), meta=json.dumps(meta), **arrays)
    print("harvest deviations per corner", arrays["hv_corner_dev"], "\nhistory deviations (all increments)", arrays["hist_dev_all"], flush=True)


if __name__ == "__main__":
    main()
