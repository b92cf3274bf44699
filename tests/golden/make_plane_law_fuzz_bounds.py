#!/usr/bin/env python3
"""Writes ``tests/golden/plane_law_fuzz_bounds.npz``: for every seed of the parameter-space sweep of the plane-strain Hosford and Ogden
kernels (``tests/plane_law_fuzz.py``) the largest deviation of the law's float64 definition from its high-precision version on that
seed's sample of ``law_fuzz.MP_SAMPLE`` points, and the bounds ``tests/test_gpu_fuzz_plane_laws.py`` applies: 8 x the largest deviation
(a factor 2 for kernel and restatement each sitting within that error of the truth, a factor 4 for the different formulation and
fma / libm differences, ``make_hosford_degenerate.py``), never less than the bound the law's fixed-parameter GPU tests already apply:

* Hosford (law 40): ``bound_state`` and ``bound_tangent`` of ``hosford_plane.npz``;
* Ogden (law 38): ``BOUND`` of ``tests/test_gpu_ogden.py``, min(16 E0, 1e-11).

Measured on the CPU against mpmath, never against the kernels.

    python tests/golden/make_plane_law_fuzz_bounds.py        (about a minute)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import plane_law_fuzz as pf  # noqa: E402


def main():
    gold = np.load(os.path.join(HERE, "hosford_plane.npz"))
    floors = dict(hosford_state=float(gold["bound_state"]), hosford_tangent=float(gold["bound_tangent"]), ogden=min(16 * pf.OGDEN_E0, 1e-11))
    dev = {k: [] for k in floors}
    for s in pf.HOSFORD_SEEDS:
        a, b = pf.plane_hosford_deviation(s)
        dev["hosford_state"].append(a)
        dev["hosford_tangent"].append(b)
        print(f"plane hosford seed {s} {pf.draw_hosford(s)}: state {a:.2e} tangent {b:.2e}", flush=True)
    for s in pf.OGDEN_SEEDS:
        dev["ogden"].append(pf.plane_ogden_deviation(s))
        print(f"plane ogden seed {s} {pf.draw_ogden(s)}: {dev['ogden'][-1]:.2e}", flush=True)
    out = {}
    for k, floor in floors.items():
        out[f"dev_{k}"] = np.array(dev[k])
        out[f"floor_{k}"] = floor
        out[f"bound_{k}"] = max(8 * max(dev[k]), floor)
        print(f"{k:16s} largest deviation {max(dev[k]):.3e}  bound {out[f'bound_{k}']:.3e}")
    path = os.path.join(HERE, "plane_law_fuzz_bounds.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
