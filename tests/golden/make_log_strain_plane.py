"""Writes ``tests/golden/log_strain_plane.npz``: plane-strain logarithmic-strain J2 plasticity on
``log_strain_plane_ref.fixture_points()`` (three points of every draw and amplitude, then the special rows), in mpmath at 100 digits by
the eigen-free formulation of ``make_log_strain.py`` (``logm``, work conjugacy, central differences) on the embedded 3x3 F: no
eigenvector, no divided difference, no plane restatement.  Only the five columns and rows ``[00, 11, 22, 01, 10]`` of the tangent are
differentiated and kept; the symmetric tensors are kept as ``[xx, yy, zz, sqrt(2) xy]``.  Every point carries its own parameters, label
and old state.  Run once (about 9 s per point and core): ``python tests/golden/make_log_strain_plane.py``."""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import log_strain_plane_ref as lp  # noqa: E402
import make_log_strain as mk  # noqa: E402

RI, RJ = (0, 1, 2, 0, 1), (0, 1, 2, 1, 0)


def one_point(args):
    F5, ep4, p_n, prm = args
    with mp.workdps(mk.DPS):
        F = mp.matrix(3, 3)
        for t in range(5):
            F[RI[t], RJ[t]] = mp.mpf(float(F5[t]))
        Ep_n, p_n = mk.from_mandel(list(ep4) + [0.0, 0.0]), mp.mpf(float(p_n))
        E = mk.hencky(F)
        T, Ep, p, plastic = mk.radial_return(E, Ep_n, p_n, prm)
        P = mk.pk1(F, Ep_n, p_n, prm)
        h = mp.mpf(mk.H_OUTER)
        A = np.empty((5, 5))
        for col in range(5):
            dF = mp.matrix(3, 3)
            dF[RI[col], RJ[col]] = h
            dP = (mk.pk1(F + dF, Ep_n, p_n, prm) - mk.pk1(F - dF, Ep_n, p_n, prm)) / (2 * h)
            A[:, col] = [float(dP[RI[r], RJ[r]]) for r in range(5)]
        # what the restriction drops is zero to the working precision
        eel6, Ep6 = mk.mandel(E - Ep), mk.mandel(Ep)
        assert max(abs(x) for x in eel6[4:] + Ep6[4:]) < 1e-80 and max(abs(float(P[i, j])) for i, j in ((0, 2), (2, 0), (1, 2), (2, 1))) < 1e-60
        return ([float(P[RI[r], RJ[r]]) for r in range(5)], A, eel6[:4], float(p), Ep6[:4], bool(plastic))


def main():
    F, Ep_n, p_n, params, dr, amp, labels = lp.fixture_points()
    n = len(F)
    assert n <= 150
    jobs = [(F[k], Ep_n[k], p_n[k], dict(zip(("E", "nu", "s0", "H0"), params[k]))) for k in range(n)]
    with multiprocessing.Pool(min(n, os.cpu_count() or 1)) as pool:
        res = pool.map(one_point, jobs, chunksize=1)
    out = {"F": F, "Ep_n": Ep_n, "p_n": p_n, "params": params, "draw": dr, "amp": amp, "labels": np.array(labels)}
    for q, key in enumerate(("P", "A", "eel", "p", "Ep", "plastic")):
        out[key] = np.array([x[q] for x in res])
    print("plastic:", int(out["plastic"].sum()), "of", n)
    np.savez_compressed(lp.GOLDEN, **out)
    print("wrote", lp.GOLDEN, os.path.getsize(lp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
