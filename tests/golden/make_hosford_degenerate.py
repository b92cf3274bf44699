#!/usr/bin/env python3
"""Writes ``tests/golden/hosford_degenerate.npz``: for every exponent of ``hosford_ref.EXPONENTS`` and every input class of
``hosford_ref.CLASSES`` six points (240 in all) -- inputs, the 50-digit results of ``hosford_ref.update_mp`` rounded to float64, the
largest deviation of the float64 restatement ``hosford_ref.update`` from them and the bounds the GPU tests apply:
8 x that deviation, never less than 1e-12 (a factor 2 for kernel and restatement each sitting within that error of the truth, a
factor 4 for the different formulation and fma / libm differences).

    python tests/golden/make_hosford_degenerate.py        (about a minute)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hosford_ref as hr  # noqa: E402

PER = 6


def errors(got, ref, E, R0):
    """(stress / state, tangent) deviations per row: relative to the row's largest stress (strains as E x strain), floored at R0;
    the tangent relative to the row's largest entry."""
    n = ref["sig"].shape[0]
    sc = np.maximum(np.abs(ref["sig"]).max(axis=1), R0)
    es = np.abs(got["sig"] - ref["sig"]).max(axis=1) / sc
    ee = E * np.abs(got["eel"] - ref["eel"]).max(axis=1) / sc
    ep = E * np.abs(got["p"] - ref["p"]) / sc
    ct = np.abs(got["Ct"] - ref["Ct"]).reshape(n, -1).max(axis=1) / np.abs(ref["Ct"]).reshape(n, -1).max(axis=1)
    return np.maximum(es, np.maximum(ee, ep)), ct


def main():
    P = hr.PROPS
    rows = []
    for ia, a in enumerate(hr.EXPONENTS):
        for ic, cls in enumerate(hr.CLASSES):
            eps, ep, p = hr.make_inputs(cls, PER, a, 1000 + 10 * ia + ic)
            for k in range(PER):
                m = hr.update_mp(eps[k], ep[k], p[k], **P, a=a)
                rows.append((a, ic, eps[k], ep[k], p[k], m["sig"], m["eel"], m["p"], m["Ct"], m["plastic"]))
        print("a =", a, "done", flush=True)
    a = np.array([r[0] for r in rows])
    ref = dict(sig=np.array([r[5] for r in rows]), eel=np.array([r[6] for r in rows]), p=np.array([r[7] for r in rows]),
               Ct=np.array([r[8] for r in rows]))
    eps, ep, p = np.array([r[2] for r in rows]), np.array([r[3] for r in rows]), np.array([r[4] for r in rows])
    dev_s, dev_c = np.zeros(len(rows)), np.zeros(len(rows))
    for av in hr.EXPONENTS:
        k = a == av
        got = hr.update(eps[k], ep[k], p[k], **P, a=av)
        assert got["converged"].all() and (got["plastic"] == np.array([r[9] for r in rows])[k]).all()
        dev_s[k], dev_c[k] = errors(got, {q: v[k] for q, v in ref.items()}, P["E"], P["R0"])
    out = os.path.join(HERE, "hosford_degenerate.npz")
    np.savez_compressed(out, a=a, cls=np.array([r[1] for r in rows]), eps=eps, ep_n=ep, p_n=p, plastic=np.array([r[9] for r in rows]), **ref,
                        props=np.array([P["E"], P["nu"], P["R0"], P["H"]]), dev_state=dev_s, dev_tangent=dev_c,
                        bound_state=max(8 * dev_s.max(), 1e-12), bound_tangent=max(8 * dev_c.max(), 1e-12))
    for ic, cls in enumerate(hr.CLASSES):
        k = np.array([r[1] for r in rows]) == ic
        print(f"{cls:14s} stress/state {dev_s[k].max():.2e}  tangent {dev_c[k].max():.2e}")
    print(f"bounds: state {max(8 * dev_s.max(), 1e-12):.3e}  tangent {max(8 * dev_c.max(), 1e-12):.3e}  ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
