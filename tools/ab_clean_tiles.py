#!/usr/bin/env python3
"""Option ``elide_clean_state`` on against off, in ONE process (fresh processes draw different placements: VERDICT.md).

    python tools/ab_clean_tiles.py [--points 10000000] [--rounds 30] [--settle 20] [--out FILE.json]
    python tools/ab_clean_tiles.py --pmc [--points N] [--out FILE.json]      # HBM bytes written per launch, on and off
    python tools/ab_clean_tiles.py --same-handle [...]                       # the A/B on one set of handles, option switched per launch

A/B: the three load-step contexts of bench.py (J2 with linear hardening, seed 1234, increments 2, 3, 4 each from the converged
state of the one before) are built twice, with the option on and off, over the same strain, flux and tangent arrays.  After
``--settle`` launches per handle the six handles are interleaved launch by launch for ``--rounds`` rounds, every launch between
two HIP events.  The same is then done with two sets of handles that BOTH have the option off: the largest difference between
their medians is the noise the on / off differences are read against.  Prints one JSON line.

--pmc: one ``rocprofv3 --pmc WRITE_SIZE`` pass (counters only, no tracing) over a child process (``--pmc-child``, the program after
``--``) that launches the increment-4 context a few times with the option on and then off; WRITE_SIZE (KiB) per launch of each
kernel, against 336 B/point (on: stress + tangent; no tile of the unloading increment yields) and 392 B/point (off: + state)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (history, to_dev, the material constants: the workload is bench.py's)

CLEAN_KERNEL, PLAIN_KERNEL = "small_strain_clean_kernel<1", "small_strain_kernel<1"


def contexts(torch, n, eps, flux, ct, stream, elide):
    """bench.py::run_workload's `mats`: one handle per timed increment k = 2, 3, 4 with s0 = the converged state after k - 1"""
    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    mats = []
    for k in (2, 3, 4):
        m = JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=bench.E, nu=bench.NU), jm.LinearHardening(bench.SIG0, bench.H)))
        m.set_data_manager(n)
        m.set_option("elide_clean_state", 1 if elide else 0)
        for i in range(k - 1):
            m.integrate_device(eps[i].data_ptr(), flux.data_ptr(), ct.data_ptr(), stream)
            rc, st = m.stats()
            assert rc == 0 and st["n_nan"] == 0
            m.data_manager.update()
        mats.append(m)
    return mats


def leg(torch, sets, eps, flux, ct, stream, settle, rounds):
    """sets: name -> three handles.  Returns name -> [per-increment list of launch times in ms]."""
    def launch(m, j):
        m.integrate_device(eps[j + 1].data_ptr(), flux.data_ptr(), ct.data_ptr(), stream)

    for mats in sets.values():
        for i in range(settle):
            launch(mats[i % 3], i % 3)
    torch.cuda.synchronize()
    ev = {name: [[] for _ in range(3)] for name in sets}
    for _ in range(rounds):
        for j in range(3):
            for name, mats in sets.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(mats[j], j)
                b.record()
                ev[name][j].append((a, b))
    torch.cuda.synchronize()
    return {name: [[a.elapsed_time(b) for a, b in per] for per in ev[name]] for name in sets}


def summary(times):
    med = [float(np.median(t)) for t in times]
    return {"median_ms": [round(x, 5) for x in med], "mean3_ms": round(float(np.mean(med)), 5),
            "min_ms": [round(float(np.min(t)), 5) for t in times], "max_ms": [round(float(np.max(t)), 5) for t in times]}


def ab(args):
    import torch

    n = args.points
    dev = torch.device("cuda", 0)
    eps = [bench.to_dev(h, dev) for h in bench.history(n, 1234, bench.SIG0)]
    flux = torch.empty((n, 6), dtype=torch.float64, device=dev)
    ct = torch.empty((n, 36), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    on = contexts(torch, n, eps, flux, ct, stream, True)
    off = contexts(torch, n, eps, flux, ct, stream, False)
    off2 = contexts(torch, n, eps, flux, ct, stream, False)
    t1 = leg(torch, {"on": on, "off": off}, eps, flux, ct, stream, args.settle, args.rounds)
    t2 = leg(torch, {"off_a": off, "off_b": off2}, eps, flux, ct, stream, args.settle, args.rounds)
    clean = []
    for m in on:
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        m._lib.dxm_clean_tiles(m._handle, ctypes.byref(a), ctypes.byref(b))
        clean.append([a.value, b.value])
    plastic = []
    for m in on:
        rc, st = m.stats()
        plastic.append(round(st["n_plastic"] / n, 4))
    s = {k: summary(v) for k, v in {**t1, **t2}.items()}
    noise_inc = max(abs(a - b) for a, b in zip(s["off_a"]["median_ms"], s["off_b"]["median_ms"]))
    noise_mean = abs(s["off_a"]["mean3_ms"] - s["off_b"]["mean3_ms"])
    noise = max(noise_inc, noise_mean)
    gain4 = s["off"]["median_ms"][2] - s["on"]["median_ms"][2]
    gain_mean = s["off"]["mean3_ms"] - s["on"]["mean3_ms"]
    rec = {"tool": "ab_clean_tiles", "points": n, "rounds": args.rounds, "settle": args.settle, "increments": [2, 3, 4], "legs": s,
           "plastic_fraction": plastic, "clean_tiles_of_tiles_on": clean,
           "noise_ms": round(noise, 5), "increment4_gain_ms": round(gain4, 5), "mean3_gain_ms": round(gain_mean, 5),
           "accepted": {"increment4_and_mean_gain_above_3x_noise": bool(gain4 > 3 * noise and gain_mean > 3 * noise),
                        "increments_2_3_not_slower_than_noise": bool(all(s["on"]["median_ms"][j] - s["off"]["median_ms"][j] <= noise for j in (0, 1)))}}
    for mats in (on, off, off2):
        for m in mats:
            m.close()
    return rec


def same_handle(args):
    """Both settings on the SAME three handles, so that both run on the same allocations: per round and increment one timed launch
    with the option off, one untimed launch after switching it on (the switch makes every stamp stale, this launch marks the tiles
    again), one timed launch with it on, and a second timed launch with it off -- the two off series are the noise leg."""
    import torch

    n = args.points
    dev = torch.device("cuda", 0)
    eps = [bench.to_dev(h, dev) for h in bench.history(n, 1234, bench.SIG0)]
    flux = torch.empty((n, 6), dtype=torch.float64, device=dev)
    ct = torch.empty((n, 36), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    mats = contexts(torch, n, eps, flux, ct, stream, True)

    def launch(j, timed=None):
        if timed is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        mats[j].integrate_device(eps[j + 1].data_ptr(), flux.data_ptr(), ct.data_ptr(), stream)
        if timed is not None:
            b.record()
            timed.append((a, b))

    for i in range(args.settle):
        launch(i % 3)
    torch.cuda.synchronize()
    ev = {name: [[] for _ in range(3)] for name in ("off_a", "on", "off_b")}
    for _ in range(args.rounds):
        for j in range(3):
            mats[j].set_option("elide_clean_state", 0)
            launch(j, ev["off_a"][j])
            mats[j].set_option("elide_clean_state", 1)
            launch(j)
            launch(j, ev["on"][j])
            mats[j].set_option("elide_clean_state", 0)
            launch(j, ev["off_b"][j])
    torch.cuda.synchronize()
    s = {name: summary([[a.elapsed_time(b) for a, b in per] for per in ev[name]]) for name in ev}
    noise = max(max(abs(a - b) for a, b in zip(s["off_a"]["median_ms"], s["off_b"]["median_ms"])), abs(s["off_a"]["mean3_ms"] - s["off_b"]["mean3_ms"]))
    off_med = [0.5 * (a + b) for a, b in zip(s["off_a"]["median_ms"], s["off_b"]["median_ms"])]
    gain = [o - x for o, x in zip(off_med, s["on"]["median_ms"])]
    rec = {"tool": "ab_clean_tiles --same-handle", "points": n, "rounds": args.rounds, "settle": args.settle, "increments": [2, 3, 4], "legs": s,
           "noise_ms": round(noise, 5), "gain_ms": [round(g, 5) for g in gain], "mean3_gain_ms": round(float(np.mean(gain)), 5)}
    for m in mats:
        m.close()
    return rec


def pmc_child(args):
    import torch

    n = args.points
    dev = torch.device("cuda", 0)
    eps = [bench.to_dev(h, dev) for h in bench.history(n, 1234, bench.SIG0)]
    flux = torch.empty((n, 6), dtype=torch.float64, device=dev)
    ct = torch.empty((n, 36), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for elide in (True, False):
        m = contexts(torch, n, eps, flux, ct, stream, elide)[2]     # (the other two are built and dropped: one code path with the A/B)
        for _ in range(args.launches):
            m.integrate_device(eps[3].data_ptr(), flux.data_ptr(), ct.data_ptr(), stream)
        torch.cuda.synchronize()
    return 0


def pmc(args):
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"tool": "ab_clean_tiles --pmc", "error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="dxm_clean_pmc_")
    try:
        cmd = [exe, "--pmc", "WRITE_SIZE", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--pmc-child",
               "--points", str(args.points), "--launches", str(args.launches)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        rows = []
        for f in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
            rows += [row for row in csv.DictReader(open(f)) if row.get("Counter_Name") == "WRITE_SIZE"]
        if r.returncode != 0 or not rows:
            return {"tool": "ab_clean_tiles --pmc", "error": f"rc {r.returncode}, {len(rows)} samples: {r.stderr[-400:]}"}
        n = args.points
        out = {"tool": "ab_clean_tiles --pmc", "points": n, "counter": "WRITE_SIZE (KiB)"}
        for key, name in (("on", CLEAN_KERNEL), ("off", PLAIN_KERNEL)):
            # the last `launches` dispatches of each kernel: the ones of the increment-4 context (those before it build the contexts)
            vals = [float(row["Counter_Value"]) * 1024.0 for row in rows if name in row["Kernel_Name"]][-args.launches:]
            out[key] = {"kernel": name, "launches": len(vals), "write_bytes_per_point": [round(v / n, 3) for v in vals]}
        on, off = out["on"]["write_bytes_per_point"], out["off"]["write_bytes_per_point"]
        if on and off:
            # (the first launch of the on handle after its set-up still stores: its tiles become clean in it)
            out["saved_bytes_per_point"] = round(float(np.median(off)) - float(np.median(on[1:] or on)), 3)
            out["off_relative_deviation_from_392"] = round(abs(float(np.median(off)) - 392.0) / 392.0, 5)
            out["saved_relative_deviation_from_56"] = round(abs(out["saved_bytes_per_point"] - 56.0) / 56.0, 5)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--launches", type=int, default=4, help="--pmc: launches of the increment-4 context per setting")
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--same-handle", action="store_true", help="both settings on the same handles (same allocations), switched launch by launch")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.pmc_child:
        return pmc_child(a)
    rec = pmc(a) if a.pmc else (same_handle(a) if a.same_handle else ab(a))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
