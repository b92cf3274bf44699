#!/usr/bin/env python3
"""Option ``pack_old_state`` on against off on the three load-step contexts of bench.py (J2 with linear hardening, seed 1234,
increments 2, 3, 4 each from the converged state of the one before), in ONE process.

    python tools/ab_packed_state.py --same-handle [--points 10000000] [--rounds 30] [--settle 20] [--out FILE.json]
    python tools/ab_packed_state.py --two-sets [...]                         # separate handles on / off / off, all copies allocated at once
    python tools/ab_packed_state.py --pmc [--points N] [--launches 3] [--out FILE.json]

--same-handle: both settings on the SAME three handles, so that both run on the same allocations.  Per round and increment: one
timed launch with the option off; the option is switched on (a fresh s0 epoch), two untimed launches (today's kernel, then the one
that builds the copy), one timed launch that reads the copy; the option is switched off (the copy is freed) and one more launch is
timed.  The two off series are the noise leg: noise = the largest difference between their medians (per increment, and of the
3-step mean), the definition of profiles/r15_clean_tile_state.md.

--pmc: two ``rocprofv3 --pmc`` passes, counters only (FETCH_SIZE, then WRITE_SIZE), over a child process (``--pmc-child``, the
program after ``--``) that launches each of the three contexts with the option on (plain, build, ``--launches`` use launches) and
then off (``--launches`` launches), and writes down what it launched and, from ``dxm_get_state`` of s0 with the kernel's own test
(a slot that is not bit-zero), the k of every tile.  For the use launches 2 x FETCH_SIZE per point is held against
48 + sum_t roundup128(56 k_t) / N + 8 / 64; the allowed relative error is that of the option-off launches against their own 104
B/point; WRITE_SIZE must be what it is with the option off."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402  (history, to_dev, the material constants: the workload is bench.py's)
from ab_clean_tiles import contexts, summary  # noqa: E402

USE_KERNEL, BUILD_KERNEL, OFF_KERNEL = "small_strain_packed_kernel<1, 0, 2>", "small_strain_packed_kernel<1, 0, 1>", "small_strain_clean_kernel<1"


def arrays(torch, n):
    dev = torch.device("cuda", 0)
    eps = [bench.to_dev(h, dev) for h in bench.history(n, 1234, bench.SIG0)]
    flux = torch.empty((n, 6), dtype=torch.float64, device=dev)
    ct = torch.empty((n, 36), dtype=torch.float64, device=dev)
    return eps, flux, ct, torch.cuda.current_stream().cuda_stream


def packed_state(m):
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    m._lib.dxm_packed_state(m._handle, ctypes.byref(a), ctypes.byref(b))
    return [a.value, b.value]


def same_handle(args):
    import torch

    n = args.points
    eps, flux, ct, stream = arrays(torch, n)
    mats = contexts(torch, n, eps, flux, ct, stream, True)

    def launch(j, timed=None):
        if timed is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        mats[j].integrate_device(eps[j + 1].data_ptr(), flux.data_ptr(), ct.data_ptr(), stream)
        if timed is not None:
            b.record()
            timed.append((a, b))

    for m in mats:
        m.set_option("pack_old_state", 0)
    for i in range(args.settle):
        launch(i % 3)
    torch.cuda.synchronize()
    ev = {name: [[] for _ in range(3)] for name in ("off_a", "use", "off_b")}
    kept = [None] * 3
    for r in range(args.rounds):
        for j in range(3):
            launch(j, ev["off_a"][j])
            mats[j].set_option("pack_old_state", 1)
            launch(j)                      # today's kernel
            launch(j)                      # build
            launch(j, ev["use"][j])
            if r == 0:
                kept[j] = packed_state(mats[j])
            mats[j].set_option("pack_old_state", 0)
            launch(j, ev["off_b"][j])
    torch.cuda.synchronize()
    s = {name: summary([[a.elapsed_time(b) for a, b in per] for per in ev[name]]) for name in ev}
    noise_inc = [abs(a - b) for a, b in zip(s["off_a"]["median_ms"], s["off_b"]["median_ms"])]
    noise = max(max(noise_inc), abs(s["off_a"]["mean3_ms"] - s["off_b"]["mean3_ms"]))
    off_med = [0.5 * (a + b) for a, b in zip(s["off_a"]["median_ms"], s["off_b"]["median_ms"])]
    gain = [o - x for o, x in zip(off_med, s["use"]["median_ms"])]
    rec = {"tool": "ab_packed_state --same-handle", "points": n, "rounds": args.rounds, "settle": args.settle, "increments": [2, 3, 4],
           "legs": s, "tiles_packed_points_kept": kept, "kept_fraction": [round(k[1] / n, 4) for k in kept],
           "noise_ms": round(noise, 5), "noise_per_increment_ms": [round(x, 5) for x in noise_inc], "gain_ms": [round(g, 5) for g in gain],
           "gain_percent": [round(100 * g / o, 2) for g, o in zip(gain, off_med)], "mean3_off_ms": round(float(np.mean(off_med)), 5),
           "mean3_use_ms": s["use"]["mean3_ms"], "mean3_gain_ms": round(float(np.mean(gain)), 5),
           "accepted": {"increment2_gain_at_least_3x_noise": bool(gain[0] >= 3 * noise),
                        "no_increment_slower_than_noise": bool(all(g >= -noise for g in gain))}}
    rec["accepted"]["default_1"] = bool(all(rec["accepted"].values()))
    for m in mats:
        m.close()
    return rec


def two_sets(args):
    """The cadence of bench.py: three sets of three handles (option on; off; off again) over the same strain, flux and tangent arrays,
    all copies allocated at once, interleaved launch by launch; the second off set is the noise leg (tools/ab_clean_tiles.py: ab)."""
    import torch
    from ab_clean_tiles import leg

    n = args.points
    eps, flux, ct, stream = arrays(torch, n)
    sets = {name: contexts(torch, n, eps, flux, ct, stream, True) for name in ("on", "off", "off2")}
    for name in ("off", "off2"):
        for m in sets[name]:
            m.set_option("pack_old_state", 0)
    t1 = leg(torch, {"on": sets["on"], "off": sets["off"]}, eps, flux, ct, stream, args.settle, args.rounds)
    t2 = leg(torch, {"off_a": sets["off"], "off_b": sets["off2"]}, eps, flux, ct, stream, args.settle, args.rounds)
    s = {k: summary(v) for k, v in {**t1, **t2}.items()}
    noise = max(max(abs(a - b) for a, b in zip(s["off_a"]["median_ms"], s["off_b"]["median_ms"])), abs(s["off_a"]["mean3_ms"] - s["off_b"]["mean3_ms"]))
    rec = {"tool": "ab_packed_state --two-sets", "points": n, "rounds": args.rounds, "settle": args.settle, "increments": [2, 3, 4], "legs": s,
           "tiles_packed_points_kept": [packed_state(m) for m in sets["on"]], "noise_ms": round(noise, 5),
           "gain_ms": [round(a - b, 5) for a, b in zip(s["off"]["median_ms"], s["on"]["median_ms"])],
           "mean3_gain_ms": round(s["off"]["mean3_ms"] - s["on"]["mean3_ms"], 5)}
    for mats in sets.values():
        for m in mats:
            m.close()
    return rec


def pmc_child(args):
    import torch

    n = args.points
    eps, flux, ct, stream = arrays(torch, n)
    mats = contexts(torch, n, eps, flux, ct, stream, True)
    torch.cuda.synchronize()
    plan, expected, kept = [], [], []
    for j, m in enumerate(mats):
        # the k of every tile, from s0 as the handle returns it, with the kernel's test: a slot that is not bit-zero
        h = m._handle
        p, ep = np.empty((n, 1)), np.empty((n, 6))
        assert m._lib.dxm_get_state(h, 0, 0, p.ctypes.data) >= 0 and m._lib.dxm_get_state(h, 0, 1, ep.ctypes.data) >= 0
        nz = (ep.view(np.uint64) != 0).any(axis=1) | (p.view(np.uint64)[:, 0] != 0)
        pad = np.zeros(((n + 63) // 64) * 64, dtype=bool)
        pad[:n] = nz
        k = pad.reshape(-1, 64).sum(axis=1)
        expected.append(48.0 + float((((56 * k + 127) // 128) * 128).sum()) / n + 8.0 / 64.0)

        def launch(tag):
            m.integrate_device(eps[j + 1].data_ptr(), flux.data_ptr(), ct.data_ptr(), stream)
            plan.append([j, tag])

        m.set_option("pack_old_state", 1)
        launch("plain")
        launch("build")
        for _ in range(args.launches):
            launch("use")
        torch.cuda.synchronize()
        kept.append(packed_state(m) + [int(nz.sum())])
        m.set_option("pack_old_state", 0)
        for _ in range(args.launches):
            launch("off")
        torch.cuda.synchronize()
    with open(args.sidecar, "w") as f:
        json.dump({"plan": plan, "expected_use_read_bytes_per_point": expected, "packed_state_and_host_count": kept}, f)
    return 0


def pmc(args):
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"tool": "ab_packed_state --pmc", "error": "rocprofv3 not found"}
    n, L = args.points, args.launches
    out = {"tool": "ab_packed_state --pmc", "points": n, "launches": L, "counters": "FETCH_SIZE x 2, WRITE_SIZE (KiB), one pass each"}
    per = {}
    side = None
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="dxm_packed_pmc_")
        try:
            sidecar = os.path.join(tmp, "plan.json")
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--pmc-child",
                   "--points", str(n), "--launches", str(L), "--sidecar", sidecar]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            rows = []
            for f in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                rows += [row for row in csv.DictReader(open(f)) if row.get("Counter_Name") == counter]
            if r.returncode != 0 or not rows or not os.path.exists(sidecar):
                return {**out, "error": f"{counter}: rc {r.returncode}, {len(rows)} samples: {r.stderr[-400:]}"}
            side = json.load(open(sidecar))
            rows.sort(key=lambda row: int(row.get("Dispatch_Id", 0)))
            j2 = [row for row in rows if "small_strain_" in row["Kernel_Name"] and "_kernel<1" in row["Kernel_Name"]]
            tail = j2[-len(side["plan"]):]       # (the launches before them build the contexts)
            want = {"plain": OFF_KERNEL, "build": BUILD_KERNEL, "use": USE_KERNEL, "off": OFF_KERNEL}
            for (j, tag), row in zip(side["plan"], tail):
                if want[tag] not in row["Kernel_Name"]:
                    return {**out, "error": f"{counter}: launch ({j}, {tag}) ran {row['Kernel_Name'][:80]}"}
                per.setdefault(counter, {}).setdefault(tag, [[], [], []])[j].append(float(row["Counter_Value"]) * 1024.0 / n)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    med = lambda v: float(np.median(v))   # noqa: E731
    read = {tag: [round(2.0 * med(v), 3) for v in per["FETCH_SIZE"][tag]] for tag in per["FETCH_SIZE"]}
    write = {tag: [round(med(v), 3) for v in per["WRITE_SIZE"][tag]] for tag in per["WRITE_SIZE"]}
    exp = side["expected_use_read_bytes_per_point"]
    tol = max(abs(x - 104.0) / 104.0 for x in read["off"])
    dev = [abs(a - b) / b for a, b in zip(read["use"], exp)]
    out.update({"increments": [2, 3, 4], "read_bytes_per_point": read, "write_bytes_per_point": write,
                "expected_use_read_bytes_per_point": [round(x, 3) for x in exp], "packed_state_and_host_count": side["packed_state_and_host_count"],
                "off_relative_deviation_from_104": round(tol, 5), "use_relative_deviation_from_expected": [round(x, 5) for x in dev],
                "write_use_minus_off": [round(a - b, 3) for a, b in zip(write["use"], write["off"])],
                "bytes_per_point_use": [round(a + b, 2) for a, b in zip(read["use"], write["use"])],
                "bytes_per_point_off": [round(a + b, 2) for a, b in zip(read["off"], write["off"])]})
    out["accepted"] = {"use_reads_what_the_masks_say": bool(all(x <= tol for x in dev)),
                       "writes_unchanged": bool(all(abs(a - b) <= tol * b for a, b in zip(write["use"], write["off"])))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--launches", type=int, default=3, help="--pmc: use launches, and option-off launches, per context")
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--same-handle", action="store_true")
    ap.add_argument("--two-sets", action="store_true", help="separate handles with the option on and off, interleaved (the cadence of bench.py)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sidecar", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.pmc_child:
        return pmc_child(a)
    if not (a.pmc or a.same_handle or a.two_sets):
        ap.error("one of --same-handle, --two-sets and --pmc")
    rec = pmc(a) if a.pmc else same_handle(a) if a.same_handle else two_sets(a)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
