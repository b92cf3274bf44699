"""Writes ``tests/golden/log_strain_finite.npz``: logarithmic-strain J2 plasticity at finite stretches, over ten parameter sets and
on the rows where the kernel's branches meet (``log_strain_cases.fixture_points()``: 120 + 24 points), in mpmath at 100 digits by the
eigen-free formulation of ``make_log_strain.py`` (``one_point``: logm, work conjugacy, central differences).  Every point carries
its own parameters, label and old state.  Run once (16 s per point and core): ``python tests/golden/make_log_strain_finite.py``."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import log_strain_cases as lc  # noqa: E402
from make_log_strain import one_point  # noqa: E402


def main():
    F, Ep_n, p_n, params, dr, amp, labels = lc.fixture_points()
    n = len(F)
    assert n <= 144
    jobs = [(F[k], Ep_n[k], p_n[k], dict(zip(("E", "nu", "s0", "H0"), params[k]))) for k in range(n)]
    with multiprocessing.Pool(min(n, os.cpu_count() or 1)) as pool:
        res = pool.map(one_point, jobs, chunksize=1)
    out = {"F": F, "Ep_n": Ep_n, "p_n": p_n, "params": params, "draw": dr, "amp": amp, "labels": np.array(labels)}
    for q, key in enumerate(("P", "A", "eel", "p", "Ep", "plastic")):
        out[key] = np.array([x[q] for x in res])
    print("plastic:", int(out["plastic"].sum()), "of", n)
    np.savez_compressed(lc.GOLDEN, **out)
    print("wrote", lc.GOLDEN, os.path.getsize(lc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
