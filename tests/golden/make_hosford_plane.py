#!/usr/bin/env python3
"""Writes ``tests/golden/hosford_plane.npz``: for every exponent of ``hosford_ref.EXPONENTS`` and every input class of
``hosford_plane_ref.CLASSES`` five points (250 in all) -- the 4-wide inputs, the 50-digit results of ``hosford_plane_ref.update_mp``
rounded to float64, the largest deviation of the float64 restatement ``hosford_plane_ref.update`` from them and the bounds the GPU
tests apply: 8 x that deviation, never less than 1e-12 (a factor 2 for kernel and restatement each sitting within that error of the
truth, a factor 4 for the different formulation and fma / libm differences), as ``make_hosford_degenerate.py`` does for law 10.

    python tests/golden/make_hosford_plane.py        (about a minute)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hosford_plane_ref as hp  # noqa: E402

PER = 5


def main():
    P = hp.PROPS
    rows = []
    for ia, a in enumerate(hp.EXPONENTS):
        for ic, cls in enumerate(hp.CLASSES):
            eps, ep, p = hp.make_inputs(cls, PER, a, 4000 + 10 * ia + ic)
            for k in range(PER):
                m = hp.update_mp(eps[k], ep[k], p[k], **P, a=a)
                rows.append((a, ic, eps[k], ep[k], p[k], m["sig"], m["eel"], m["p"], m["Ct"], m["plastic"]))
        print("a =", a, "done", flush=True)
    a = np.array([r[0] for r in rows])
    ref = dict(sig=np.array([r[5] for r in rows]), eel=np.array([r[6] for r in rows]), p=np.array([r[7] for r in rows]),
               Ct=np.array([r[8] for r in rows]))
    eps, ep, p = np.array([r[2] for r in rows]), np.array([r[3] for r in rows]), np.array([r[4] for r in rows])
    plastic = np.array([r[9] for r in rows])
    dev_s, dev_c = np.zeros(len(rows)), np.zeros(len(rows))
    for av in hp.EXPONENTS:
        k = a == av
        got = hp.update(eps[k], ep[k], p[k], **P, a=av)
        assert got["converged"].all() and (got["plastic"] == plastic[k]).all() and got["dropped"] == 0.0
        dev_s[k], dev_c[k] = hp.errors(got, {q: v[k] for q, v in ref.items()}, P["E"], P["R0"])
    out = os.path.join(HERE, "hosford_plane.npz")
    bs, bc = max(8 * dev_s.max(), 1e-12), max(8 * dev_c.max(), 1e-12)
    np.savez_compressed(out, a=a, cls=np.array([r[1] for r in rows]), eps=eps, ep_n=ep, p_n=p, plastic=plastic, **ref,
                        props=np.array([P["E"], P["nu"], P["R0"], P["H"]]), dev_state=dev_s, dev_tangent=dev_c,
                        bound_state=bs, bound_tangent=bc)
    for ic, cls in enumerate(hp.CLASSES):
        k = np.array([r[1] for r in rows]) == ic
        print(f"{cls:14s} stress/state {dev_s[k].max():.2e}  tangent {dev_c[k].max():.2e}")
    print(f"bounds: state {bs:.3e}  tangent {bc:.3e}  ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
