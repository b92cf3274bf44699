#!/usr/bin/env python3
"""Times the axisymmetric gradient kernel (csrc/axisym_gradient.hip) on one GPU: kind 0 (the 4-wide strain with the hoop term), with
and without the radius output, beside ``plane_gradient_kernel`` kind 2 (the 4-wide plane strain) on the SAME cells in the same process
with the same warm-up, on a tri6 mesh with 3 Gauss points and a quad4 mesh with 4 at about 1e6 and 1e7 points; then the law-26
device displacement form (gradient kernel into the handle's scratch, update kernel after it) on both kinds of mesh.  Device events
around ``--reps`` back-to-back launches after ``--warmup`` ones, the variants alternating, repeated ``--rounds`` times: the median per
launch and its spread.

    python tools/bench_axisym_gradient.py [--sizes 1000000 10000000] [--reps 20] [--rounds 5] [--json FILE]

What profiles/r29_axisym_gradient.md records.  No CPU fall-back: without a GPU it fails."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_plane_gradient import quad_grid, tri_grid  # noqa: E402

ELASTIC_PE = 26          # DXM_LAW_PE_ELASTIC_ISO
PRM = (70e3, 0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from dolfinx_materials_amd import _lib
    from dolfinx_materials_amd.gradient import AxisymmetricMesh, PlaneMesh

    assert torch.cuda.is_available(), "bench_axisym_gradient.py needs a GPU"
    from helpers import to_device

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for size in a.sizes:
        nt = max(int(round((size / 6.0) ** 0.5)), 1)          # 2 nt^2 triangles x 3 points
        nq = max(int(round((size / 4.0) ** 0.5)), 1)          # nq^2 quadrilaterals x 4 points
        shift = np.array([1.0, 0.0])                           # r in [1, 2]
        meshes = {}
        for tag, (xv, cells), degree in (("tri6x3", tri_grid(nt), 2), ("quad4x4", quad_grid(nq), 1)):
            plane, xd = PlaneMesh.lagrange(xv + shift, cells, degree=degree, quadrature_degree=2)
            axi, _ = AxisymmetricMesh.lagrange(xv + shift, cells, degree=degree, quadrature_degree=2)
            u = to_device(1e-3 * np.random.default_rng(0).standard_normal(xd.size))
            meshes[tag] = (plane, axi, u)
        variants, handles = [], []
        for tag, (plane, axi, u) in meshes.items():
            n = axi.npoints
            grad = torch.empty((n, 4), dtype=torch.float64, device="cuda:0")
            rad = torch.empty((n,), dtype=torch.float64, device="cuda:0")
            variants.append((f"{tag} plane_gradient_kernel<2>", n, 32,
                             lambda plane=plane, u=u, grad=grad: plane.gradient_device(u.data_ptr(), 2, grad.data_ptr(), stream)))
            variants.append((f"{tag} axisym_gradient_kernel<0, false>", n, 32,
                             lambda axi=axi, u=u, grad=grad: axi.axisymmetric_gradient_device(u.data_ptr(), 0, grad.data_ptr(), 0, stream)))
            variants.append((f"{tag} axisym_gradient_kernel<0, true>", n, 40,
                             lambda axi=axi, u=u, grad=grad, rad=rad: axi.axisymmetric_gradient_device(u.data_ptr(), 0, grad.data_ptr(), rad.data_ptr(), stream)))
            for name, mesh in (("plane", plane), ("axisymmetric", axi)):
                h = lib.dxm_create(ELASTIC_PE, (C.c_double * 2)(*PRM), 2, n, 0)
                assert h, _lib.last_error()
                handles.append(h)
                flux = torch.empty((n, 4), dtype=torch.float64, device="cuda:0")
                ct = torch.empty((n, 16), dtype=torch.float64, device="cuda:0")

                def form(h=h, mesh=mesh, u=u, flux=flux, ct=ct):
                    _lib.check(lib.dxm_integrate_displacement_device(h, mesh._handle, u.data_ptr(), 0.0, flux.data_ptr(), ct.data_ptr(), stream))

                variants.append((f"{tag} law 26 device displacement form, {name} mesh", n, None, form))
        times = {name: [] for name, *_ in variants}
        for _, _, _, run in variants:
            for _ in range(a.warmup):
                run()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, _, _, run in variants:               # alternating: a drift of the machine hits every variant alike
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.reps):
                    run()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / a.reps)       # microseconds per launch
        for name, n, written, _ in variants:
            t = np.array(times[name])
            med = float(np.median(t))
            row = dict(kernel=name, points=int(n), bytes_written_per_point=written, us=med, us_min=float(t.min()), us_max=float(t.max()),
                       written_GBps=(written * n / med / 1e3) if written else None)
            results.append(row)
            print(json.dumps(row))
        for h in handles:
            lib.dxm_destroy(h)
        for plane, axi, _ in meshes.values():
            plane.close()
            axi.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(results, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
