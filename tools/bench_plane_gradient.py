#!/usr/bin/env python3
"""Times the plane gradient kernels (csrc/plane_gradient.hip) on one GPU: kinds 2 and 3 on a tri6 mesh with 3 Gauss points and on a
quad4 mesh with 4, at about 1e6 and 1e7 points, with ``simplex_gradient_kernel<0>`` (kind 0 of a ``SimplexMesh``) on the same tri6
mesh in the same process beside them.  Device events around ``--reps`` back-to-back launches after ``--warmup`` ones, the variants
alternating, repeated ``--rounds`` times: the median per launch, its spread, and the bytes written per second.

    python tools/bench_plane_gradient.py [--sizes 1000000 10000000] [--reps 20] [--rounds 5] [--json FILE]

What profiles/r24_plane_gradient.md records.  No CPU fall-back: without a GPU it fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WIDTH = {0: 6, 1: 9, 2: 4, 3: 3}


def tri_grid(n):
    """unit square of 2 n^2 triangles (undistorted: the kernel's work does not depend on the coordinates)"""
    xs = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    i, j = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    idx = lambda a, b: (i + a) * (n + 1) + (j + b)   # noqa: E731
    lower, upper = np.stack([idx(0, 0), idx(1, 0), idx(1, 1)], axis=1), np.stack([idx(0, 0), idx(1, 1), idx(0, 1)], axis=1)
    cells = np.stack([lower, upper], axis=1).reshape(-1, 3).astype(np.int32)
    return np.stack([X.ravel(), Y.ravel()], axis=1), cells


def quad_grid(n):
    xs = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    i, j = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    idx = lambda a, b: (i + a) * (n + 1) + (j + b)   # noqa: E731
    return np.stack([X.ravel(), Y.ravel()], axis=1), np.stack([idx(0, 0), idx(1, 0), idx(0, 1), idx(1, 1)], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from dolfinx_materials_amd.gradient import PlaneMesh, SimplexMesh

    assert torch.cuda.is_available(), "bench_plane_gradient.py needs a GPU"
    from helpers import to_device

    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for size in a.sizes:
        nt = max(int(round((size / 6.0) ** 0.5)), 1)          # 2 nt^2 triangles x 3 points
        nq = max(int(round((size / 4.0) ** 0.5)), 1)          # nq^2 quadrilaterals x 4 points
        tri, xt = SimplexMesh.lagrange(*tri_grid(nt), degree=2, quadrature_degree=2)
        quad, xq = PlaneMesh.lagrange(*quad_grid(nq), degree=1, quadrature_degree=2)
        rng = np.random.default_rng(0)
        ut, uq = to_device(1e-3 * rng.standard_normal(xt.size)), to_device(1e-3 * rng.standard_normal(xq.size))
        variants = [("tri6x3 simplex_gradient_kernel<0>", tri, ut, 0), ("tri6x3 plane_gradient_kernel<2>", tri, ut, 2),
                    ("tri6x3 plane_gradient_kernel<3>", tri, ut, 3), ("quad4x4 plane_gradient_kernel<2>", quad, uq, 2),
                    ("quad4x4 plane_gradient_kernel<3>", quad, uq, 3)]
        outs = {name: torch.empty((m.npoints, WIDTH[k]), dtype=torch.float64, device="cuda:0") for name, m, _, k in variants}
        times = {name: [] for name, *_ in variants}
        for name, m, u, k in variants:
            for _ in range(a.warmup):
                m.gradient_device(u.data_ptr(), k, outs[name].data_ptr(), stream)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, m, u, k in variants:               # alternating: a drift of the machine hits every variant alike
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.reps):
                    m.gradient_device(u.data_ptr(), k, outs[name].data_ptr(), stream)
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / a.reps)       # microseconds per launch
        base = float(np.median(times[variants[0][0]]))
        for name, m, _, k in variants:
            t = np.array(times[name])
            med = float(np.median(t))
            row = dict(kernel=name, points=int(m.npoints), bytes_written_per_point=8 * WIDTH[k], us=med, us_min=float(t.min()), us_max=float(t.max()),
                       written_GBps=8 * WIDTH[k] * m.npoints / med / 1e3,
                       ratio_to_simplex_kind0=(med / base * (variants[0][1].npoints / m.npoints)) if base else None)
            results.append(row)
            print(json.dumps(row))
        tri.close()
        quad.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(results, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
