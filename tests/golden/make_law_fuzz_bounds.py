#!/usr/bin/env python3
"""Writes ``tests/golden/law_fuzz_bounds.npz``: for every seed of the parameter-space sweeps (``tests/law_fuzz.py``) the largest
deviation of each law's float64 restatement from its high-precision version on that seed's sample of ``law_fuzz.MP_SAMPLE`` points,
and the bounds ``tests/test_gpu_fuzz_laws.py`` applies: 8 x the largest deviation (a factor 2 for kernel and restatement each sitting
within that error of the truth, a factor 4 for the different formulation and fma / libm differences,
``make_hosford_degenerate.py``), never less than the bound the law's fixed-parameter GPU tests already apply:

* Hosford: ``bound_state`` and ``bound_tangent`` of ``hosford_degenerate.npz`` (1e-12);
* Ogden: ``BOUND`` of ``tests/test_gpu_ogden.py``, min(16 E0, 1e-11);
* Ramberg-Osgood: the 1e-12 (stress) and 1e-11 (tangent) of ``test_gpu_ramberg_osgood.check_against_ref``.

    python tests/golden/make_law_fuzz_bounds.py        (about a minute)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import law_fuzz as lf  # noqa: E402

OGDEN_E0 = 2e-13        # test_ogden_cpu.E0 (asserted equal by test_law_fuzz_cpu.py)
FLOORS = dict(hosford_state=1e-12, hosford_tangent=1e-12, ogden=min(16 * OGDEN_E0, 1e-11), ro_stress=1e-12, ro_tangent=1e-11)


def main():
    gold = np.load(os.path.join(HERE, "hosford_degenerate.npz"))
    assert float(gold["bound_state"]) == FLOORS["hosford_state"] and float(gold["bound_tangent"]) == FLOORS["hosford_tangent"]
    dev = {k: [] for k in FLOORS}
    for s in lf.HOSFORD_SEEDS:
        a, b = lf.hosford_deviation(s)
        dev["hosford_state"].append(a)
        dev["hosford_tangent"].append(b)
        print(f"hosford seed {s} {lf.draw_hosford(s)}: state {a:.2e} tangent {b:.2e}", flush=True)
    for s in lf.OGDEN_SEEDS:
        dev["ogden"].append(lf.ogden_deviation(s))
        print(f"ogden seed {s} {lf.draw_ogden(s)}: {dev['ogden'][-1]:.2e}", flush=True)
    for s in lf.RO_SEEDS:
        a, b = lf.ramberg_osgood_deviation(s)
        dev["ro_stress"].append(a)
        dev["ro_tangent"].append(b)
        print(f"ramberg-osgood seed {s} {lf.draw_ramberg_osgood(s)}: stress {a:.2e} tangent {b:.2e}", flush=True)
    out = {}
    for k, floor in FLOORS.items():
        out[f"dev_{k}"] = np.array(dev[k])
        out[f"floor_{k}"] = floor
        out[f"bound_{k}"] = max(8 * max(dev[k]), floor)
        print(f"{k:16s} largest deviation {max(dev[k]):.3e}  bound {out[f'bound_{k}']:.3e}")
    path = os.path.join(HERE, "law_fuzz_bounds.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
