#!/usr/bin/env python3
"""Per-law kernel throughput on one GPU (device-resident inputs/outputs, HIP events on the launch
stream).  Not the headline bench (that is bench.py); used to fill the per-law table of DESIGN.md.

    python tools/bench_laws.py [--points 10000000] [--reps 20] [--laws elastic j2_linear j2_voce fefp ramberg_osgood ogden hosford orthotropic single_crystal heat_stationary heat_phase_change log_strain fs_single_crystal ps_vonmises ps_rankine ps_l1rankine plane_strain ps_j2 ps_hosford heat_plane ogden_plane pe_hosford log_strain_plane]

ramberg_osgood: the reference's curve parameters (tests/mfront/test_nonlinear_elasticity.py: E = 1e5, nu = 0.3, sig0 = 500,
alpha = 0.4, n = 100) on a fixed, seeded strain set whose equivalent strain is uniform over 0 ... 1e-2 (linear part, knee and
plateau of the curve).  Its line also carries the time of the arithmetic-free probe with the same three streams
(stream_mix_elastic_shape_launch in tools/libstreammix.so, same arrays, same grid) and the ratios to it and to the elastic
kernel when that ran in the same process.

orthotropic: a strongly orthotropic set (E1 / E3 = 20) on the headline strains; three lines -- no frame, one uniform frame, one
random proper rotation per point (dxm_set_frame / dxm_set_frame_field) -- each with three timings, its ratio to the elastic kernel of
the same process (run `--laws elastic orthotropic`) next to the byte yardsticks 384 / 384 and 456 / 384, and the spread of the elastic
kernel's own repeats.

single_crystal: the file's constants (YoungModulus1 = 208000, the copper interaction matrix), dt = 0.1, on the 512 directions of the
`pool` of tests/test_gpu_single_crystal.py, repeated over the batch: a yielded point carries the state of 14 increments of norm 1e-4
and takes the 15th, an elastic one is virgin at 2e-4.  Nine lines: the three frame states of a handle (none, one uniform frame, one
frame per point; the history of a point belongs to its frame) x 0 %, 50 % (every other point: 32 per tile, 8 Newton rounds) and 100 %
yielded points (16 rounds per tile), each with three timings, the
restatement's iteration count, and its ratio to the J2-linear kernel of the same process (run `--laws j2_linear single_crystal`) next
to the byte yardstick 1008 (1080) / 496.

heat_stationary, heat_phase_change: the behaviour files' parameters (the phase-change law with the demo's Tsmooth = 1.0) on seeded
temperature gradients.  Two lines each: a uniform temperature (the phase-change law: inside the transition) and one temperature per
point (the phase-change law: spread over the three branches), each with three timings and, when the elastic kernel ran in the same
process (run `--laws elastic heat_stationary heat_phase_change`), its time next to the elastic kernel's scaled by the byte ratio
120 (128) / 384 or 136 (144) / 384.

ps_vonmises, ps_rankine, ps_l1rankine: the plane-stress return mappings with the cvxpy demo's parameters (E = 70e3, nu = 0.2, sig0 = 30,
fc = 30, ft = 10).  Two lines each: a wholly elastic batch and a wholly yielded one (trials at 1.01 ... 100 times the surface; the
quadratic law's Newton takes a point-dependent number of steps), each with three timings and, when the elastic kernel ran in the same
process (run `--laws elastic heat_stationary ps_vonmises ps_rankine ps_l1rankine`), its time next to the elastic kernel's scaled by
168 / 384.

plane_strain: the three laws of the plane-strain hypothesis (ids 26 / 27 / 28, 4-wide) each next to its 6-wide law (0 / 1 / 2) of the
same process on the same strains, embedded; one line per law and batch (bench_plane_strain).

ps_j2: plane-stress J2 plasticity with linear and Voce hardening (ids 30 / 31, 184 B/point) on elastic, mixed and fully yielded batches,
each next to two yardsticks of the same process on the same strains: law 23 (q = 3/2, consistent tangent, the same sig0; 168 B/point)
and law 27 / 28 (plane strain, the strain embedded as [xx, yy, 0, sqrt(2) xy]; 272 B/point), both scaled to 184 B (bench_plane_stress_j2).
ps_hosford: plane-stress Hosford plasticity (id 33, 168 B/point) at the cvxpy demo's parameters and a = 10, both tangent modes, on wholly
elastic, mixed and fully yielded batches, next to ps_vonmises (law 23, the same bytes) of the same process on the same strains
(bench_plane_stress_hosford).
heat_plane: the two-dimensional heat-transfer laws (ids 35, 36; 64 / 80 B/point) next to laws 16 / 17 of the same process on the padded
gradient, their nodal form on a Q1 quadrilateral grid at both settings of fused_gradient, and the host form next to the padded 3-wide
route (bench_heat_plane).
--blocks-per-cu: the new kernels at each of these grid sizes as well.

--param-fields K [K ...] (j2_linear, j2_voce): after the uniform kernel, the kernel that reads K bound parameter streams
(dxm_set_param_field; 1 = sig0, 2 = lambda and mu from an E field, 3 = both, 4 / 5 = H | sigu, b as well), in the same process and on
the same arrays.  The fields hold the uniform values, so every point does the same work as in the uniform run.  Each line carries
the yardstick (496 + 8 K) / 496 times the uniform time and the spread of the uniform kernel's repeated timings in this run.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_port(law, ns, budget=4.0):
    """Plain-C oracle (oracle/oracle_c.c) on the host cores: best of a small thread-count scan."""
    import time

    from oracle import oracle_c as oc
    from oracle import constitutive_np as onp
    from helpers import E, NU, SIG0_LIN, H_LIN, SIG0_V, SIGU_V, B_V, SIG0_F, SIGU_F, B_F, j2_history, fefp_path

    if law == "fefp":
        path = fefp_path(ns)
        st = onp.fefp_initial_state(ns)
        r0 = oc.fefp(path[9], st["cpinv"], st["p"], E, NU, SIG0_F, SIGU_F, B_F, nthreads=8)
        cp, p = r0["cpinv"].copy(), r0["p"].copy()
        fn = lambda nt: oc.fefp(path[18], cp, p, E, NU, SIG0_F, SIGU_F, B_F, nthreads=nt, out=r0)  # noqa: E731
    elif law == "elastic":
        eps = j2_history(ns)[2]
        fn = lambda nt: oc.elastic_iso(eps, E, NU, nthreads=nt)  # noqa: E731
    else:
        kind, s0, h1, h2 = (0, SIG0_LIN, H_LIN, 0.0) if law == "j2_linear" else (1, SIG0_V, SIGU_V, B_V)
        h = j2_history(ns, sig0=s0)
        r0 = oc.j2(h[1], np.zeros((ns, 6)), np.zeros(ns), E, NU, kind, s0, h1, h2, nthreads=8)
        ep, p = r0["epsp"].copy(), r0["p"].copy()
        fn = lambda nt: oc.j2(h[2], ep, p, E, NU, kind, s0, h1, h2, nthreads=nt, out=r0)  # noqa: E731
    ncpu = os.cpu_count() or 1
    best = (0.0, 1)
    for nt in sorted({t for t in (1, 8, 16, 32, 64) if t <= ncpu}):
        fn(nt)
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < budget / 5 or calls < 2:
            fn(nt)
            calls += 1
        rate = ns * calls / (time.perf_counter() - t0) / 1e6
        if rate > best[0]:
            best = (rate, nt)
    return {"Mpoints_per_s": round(best[0], 2), "threads": best[1], "sample": ns, "kind": "port (oracle/oracle_c.c)"}


# tests/mfront/test_nonlinear_elasticity.py:11-15
RO_E, RO_NU, RO_SIG0, RO_ALPHA, RO_N = 100e3, 0.3, 500.0, 0.4, 100.0


def ramberg_osgood_strains(n, seed=2024, emax=1e-2):
    """Equivalent strain uniform over [0, emax], random deviatoric directions, a volumetric part of up to the same size."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 6))
    d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
    d /= np.linalg.norm(d, axis=1, keepdims=True) * np.sqrt(2.0 / 3.0)
    ee = rng.uniform(0.0, emax, n)
    eps = d * ee[:, None]
    eps[:, :3] += (ee * rng.uniform(-1.0, 1.0, n))[:, None]
    return eps


def probe_ms(g, flux, ct, n, blocks, reps, warmup):
    """Median time of the arithmetic-free elastic-shape stream (48 B in, 48 + 288 B out per point) on the same arrays."""
    import ctypes

    import torch

    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "libstreammix.so"))
    fn = lib.stream_mix_elastic_shape_launch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        assert fn(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), n, blocks, st) == 0
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), n, blocks, st)
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def single_crystal_inputs(n, frame, fraction):
    """(strain (n, 6), frames or None, state dict by MFront name, yielded mask) of the single_crystal lines: see the module docstring"""
    import single_crystal_ref as sc
    from test_gpu_single_crystal import DT, POOL, PRM, make_pool

    pool = make_pool()
    d = pool["d"]
    R = {"noframe": None, "uniform": pool["R"][5], "field": pool["R"]}[frame]
    if frame == "field":
        st = pool["state"]
    else:   # the same directions, their history walked under the frame of this line
        st = sc.zero_state(POOL)
        for k in range(1, 15):
            st = sc.next_state(sc.update(k * 1e-4 * d, st, PRM, DT, R=R))
    idx = np.arange(n) % POOL
    y = {0.0: np.zeros(n, dtype=bool), 0.5: np.arange(n) % 2 == 0, 1.0: np.ones(n, dtype=bool)}[fraction]
    eps = np.where(y[:, None], 15e-4, 2e-4) * d[idx]
    names = {"ElasticStrain": "eel", "ViscoplasticSlip": "g", "EquivalentViscoplasticSlip": "p", "BackStrain": "a"}
    state = {k: np.ascontiguousarray(np.where(y[:, None], st[v][idx], 0.0)) for k, v in names.items()}
    frames = None if R is None else (R if frame == "uniform" else np.ascontiguousarray(R[idx]))
    # the restatement over one period of the inputs: what the kernel's status words are read against
    m = min(n, 2 * POOL)
    ref = sc.update(eps[:m], {v: state[k][:m] for k, v in names.items()}, PRM, DT, R=None if R is None else (R if frame == "uniform" else frames[:m]))
    return eps, frames, state, y, ref


def bench_single_crystal(a, j2_linear_ms):
    """nine lines: frame state x yielded fraction (module docstring)"""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    for frame in ("noframe", "uniform", "field"):
        for fraction in (0.0, 0.5, 1.0):
            eps, frames, state, y, ref = single_crystal_inputs(n, frame, fraction)
            m = JAXMaterial(jm.MericCailletaudSingleCrystalViscoPlasticity.from_mfront_properties({"YoungModulus1": 208000.0}))
            m.set_data_manager(n)
            m.dt = 0.1
            if frames is not None:
                m.set_frame(frames)
            m.set_initial_state_dict(state)
            g = to_device(eps)
            del eps, frames, state
            flux = torch.empty((n, 6), dtype=torch.float64, device=g.device)
            ct = torch.empty((n, 36), dtype=torch.float64, device=g.device)

            def timed():
                for _ in range(a.warmup):
                    m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)   # every launch reads the same s0: no advance
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
                for e0, e1 in ev:
                    e0.record()
                    m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
                    e1.record()
                torch.cuda.synchronize()
                return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

            t = [timed(), timed(), timed()]
            ms = float(np.median(t))
            rc, stats = m.stats()
            ab = m.algorithmic_bytes_per_point
            r = {"law": f"single_crystal+{frame}+yielded{int(100 * fraction)}", "points": n, "dt": 0.1, "kernel": m.kernel_name,
                 "kernel_ms_repeats": [round(x, 4) for x in t], "kernel_ms": round(ms, 4), "Mpoints_per_s": round(n / ms / 1e3, 1),
                 "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / ms / 1e6, 1), "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4),
                 "plastic_fraction": round(stats["n_plastic"] / n, 4), "plastic_fraction_asked": round(float(y.mean()), 4),
                 "max_local_iters": stats["max_local_iters"], "restatement_max_iters": int(ref["iters"].max(initial=0)),
                 "not_converged": stats["n_not_converged"], "nan": stats["n_nan"], "rc": rc}
            if j2_linear_ms:
                r["ratio_to_j2_linear"] = round(ms / j2_linear_ms, 3)
                r["byte_ratio_to_j2_linear"] = round(ab / 496, 3)
            print(json.dumps(r), flush=True)
            del m, g, flux, ct
            torch.cuda.empty_cache()


def bench_fs_single_crystal(a):
    """nine lines of the finite-strain single-crystal law (id 21): frame state x yielded fraction, on the points of its 50-digit
    fixture (first parameter set, dt = 0.1; tests/fs_single_crystal_cases.py) repeated over the batch -- a yielded point carries the
    state the fixture recorded for it, and a history belongs to its frame: the lines without a frame draw from the fixture's
    frameless class, the uniform lines from its generic class under that class's one frame, the field lines from all three
    classes.  Run `--laws single_crystal fs_single_crystal` to have law 14's lines of the same process beside them."""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    import fs_single_crystal_cases as cs
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    names = {"PlasticSlip": "g", "EquivalentViscoplasticSlip": "p", "BackStrain": "a", "PlasticPartOfTheDeformationGradient": "Fp"}
    props = dict(zip(("E", "nu", "G", "n", "K", "tau0", "Q", "b", "d", "C"), cs.PRM[:10]))
    i = np.arange(n)
    G = cs.GOLD
    for frame in ("noframe", "uniform", "field"):
        cls = {"noframe": (0,), "uniform": (2,), "field": (0, 1, 2)}[frame]
        sel = (G["pset"] == 0) & (G["dt"] == cs.DT) & np.isin(G["has_frame"], cls)
        pool = {yy: {"F": G["F"][sel & (G["yielded"] == yy)], "R": G["R"][sel & (G["yielded"] == yy)],
                     **{k: G[k + "0"][sel & (G["yielded"] == yy)] for k in cs.STATE}} for yy in (True, False)}
        ny, ne = len(pool[True]["F"]), len(pool[False]["F"])
        for fraction in (0.0, 0.5, 1.0):
            y = {0.0: np.zeros(n, dtype=bool), 0.5: i % 2 == 0, 1.0: np.ones(n, dtype=bool)}[fraction]
            pick = lambda k: np.ascontiguousarray(np.where(y.reshape((n,) + (1,) * (pool[True][k].ndim - 1)),   # noqa: E731
                                                           pool[True][k][i % ny], pool[False][k][i % ne]))
            F = pick("F")
            state = {q: pick(k) for q, k in names.items()}
            m = JAXMaterial(jm.FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity.from_mfront_properties(props))
            m.set_data_manager(n)
            m.dt = cs.DT
            m.set_newton(cs.MAXIT, 1e-14)
            if frame == "uniform":
                m.set_frame(pool[True]["R"][0])
            elif frame == "field":
                m.set_frame(pick("R"))
            m.set_initial_state_dict(state)
            g = to_device(F)
            del F, state
            flux = torch.empty((n, 9), dtype=torch.float64, device=g.device)
            ct = torch.empty((n, 81), dtype=torch.float64, device=g.device)

            def timed():
                for _ in range(a.warmup):
                    m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)   # every launch reads the same s0: no advance
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
                for e0, e1 in ev:
                    e0.record()
                    m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
                    e1.record()
                torch.cuda.synchronize()
                return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

            t = [timed(), timed(), timed()]
            ms = float(np.median(t))
            rc, stats = m.stats()
            ab = m.algorithmic_bytes_per_point
            r = {"law": f"fs_single_crystal+{frame}+yielded{int(100 * fraction)}", "points": n, "dt": cs.DT, "kernel": m.kernel_name,
                 "kernel_ms_repeats": [round(x, 4) for x in t], "kernel_ms": round(ms, 4), "Mpoints_per_s": round(n / ms / 1e3, 1),
                 "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / ms / 1e6, 1), "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4),
                 "plastic_fraction": round(stats["n_plastic"] / n, 4), "plastic_fraction_asked": round(float(y.mean()), 4),
                 "max_local_iters": stats["max_local_iters"], "not_converged": stats["n_not_converged"], "nan": stats["n_nan"], "rc": rc}
            print(json.dumps(r), flush=True)
            del m, g, flux, ct
            torch.cuda.empty_cache()


def bench_heat_transfer(a, law, elastic_ms, elastic_repeats):
    """two lines: uniform temperature, one temperature per point (module docstring)"""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2026)
    beh = jm.StationaryHeatTransfer() if law == "heat_stationary" else jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0})
    m = JAXMaterial(beh)
    m.set_data_manager(n)
    g = to_device(rng.normal(size=(n, 3)) * 100.0)
    flux = torch.empty((n, 3), dtype=torch.float64, device=g.device)
    ct = torch.empty((n, m.tangent_size), dtype=torch.float64, device=g.device)

    def timed():
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    for tag in ("uniformT", "fieldT"):
        if tag == "uniformT":
            m.update_external_state_variable("Temperature", 933.4 if law == "heat_phase_change" else 700.0)
        else:
            m.update_external_state_variable("Temperature", rng.uniform(600.0, 1300.0, n) if law == "heat_phase_change" else rng.uniform(300.0, 1500.0, n))
        t = [timed(), timed(), timed()]
        ms = float(np.median(t))
        rc, stats = m.stats()
        ab = m.algorithmic_bytes_per_point
        r = {"law": f"{law}+{tag}", "points": n, "kernel": m.kernel_name, "kernel_ms_repeats": [round(x, 4) for x in t], "kernel_ms": round(ms, 4),
             "Mpoints_per_s": round(n / ms / 1e3, 1), "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / ms / 1e6, 1),
             "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4), "nan": stats["n_nan"], "rc": rc}
        if elastic_ms:
            r["ratio_to_elastic"] = round(ms / elastic_ms, 3)
            r["byte_ratio_to_elastic"] = round(ab / 384, 4)
            r["elastic_scaled_ms"] = round(elastic_ms * ab / 384, 4)
            r["ratio_to_yardstick"] = round(ms / (elastic_ms * ab / 384), 3)
            r["elastic_ms_repeats"] = elastic_repeats
        print(json.dumps(r), flush=True)
    del m, g, flux, ct
    torch.cuda.empty_cache()


def bench_plane_stress(a, law, elastic_ms, elastic_repeats):
    """ps_vonmises, ps_rankine, ps_l1rankine (the demo's E = 70e3, nu = 0.2, sig0 = 30, fc = 30, ft = 10): two lines each, a wholly
    elastic batch (trials at 0.05 ... 0.95 of the surface) and a wholly yielded one (1.01 ... 100 times), from a zero plastic strain;
    168 B/point, next to the elastic kernel of the same process scaled by the byte ratio"""
    import torch

    import plane_stress_ref as ps
    from dolfinx_materials_amd.plane_stress import L1Rankine, PlaneStressvonMises, Rankine
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    m = {"ps_vonmises": lambda: PlaneStressvonMises(70e3, 0.2, 30.0), "ps_rankine": lambda: Rankine(70e3, 0.2, ft=10.0, fc=30.0),
         "ps_l1rankine": lambda: L1Rankine(70e3, 0.2, ft=10.0, fc=30.0)}[law]()
    m.set_data_manager(n)
    flux = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
    ct = torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
    for tag, lo, hi in (("elastic", 0.05, 0.95), ("yielded", 1.01, 100.0)):
        g = to_device(ps.random_trials(m.behavior.law, m.behavior.params(), n, seed=2027, lo=lo, hi=hi))

        def timed():
            for _ in range(a.warmup):
                m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
                e1.record()
            torch.cuda.synchronize()
            return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

        t = [timed(), timed(), timed()]
        ms = float(np.median(t))
        rc, stats = m.stats()
        ab = m.algorithmic_bytes_per_point
        r = {"law": f"{law}+{tag}", "points": n, "kernel": m.kernel_name, "kernel_ms_repeats": [round(x, 4) for x in t], "kernel_ms": round(ms, 4),
             "Mpoints_per_s": round(n / ms / 1e3, 1), "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / ms / 1e6, 1),
             "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4), "plastic_fraction": round(stats["n_plastic"] / n, 4),
             "max_local_iters": stats["max_local_iters"], "not_converged": stats["n_not_converged"], "nan": stats["n_nan"], "rc": rc}
        if elastic_ms:
            r["ratio_to_elastic"] = round(ms / elastic_ms, 3)
            r["elastic_scaled_ms"] = round(elastic_ms * ab / 384, 4)
            r["ratio_to_yardstick"] = round(ms / (elastic_ms * ab / 384), 3)
            r["elastic_ms_repeats"] = elastic_repeats
        print(json.dumps(r), flush=True)
        del g
    del m, flux, ct
    torch.cuda.empty_cache()


def bench_plane_strain(a):
    """--laws plane_strain: laws 26 / 27 / 28 next to laws 0 / 1 / 2 of the same process on the same strains, embedded.  One JSON line
    per law and batch: kernel ms of both (median of three medians), fraction of 8 TB/s at the counted bytes (192 / 272 against 384 /
    496), and the ratio of the 4-wide time to the 6-wide time scaled by the byte ratio.  The elastic law: one batch; the J2 laws: an
    elastic batch (|eps| up to 0.9 sig0 / E), a mixed one (up to 3 sig0 / E) and a fully yielded one (deviatoric, 2 ... 4 sig0 / E),
    each from the virgin state.  --blocks-per-cu: the 4-wide kernels at each of these grid sizes as well."""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.conventions import embed_plane_strain
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import B_V, E, H_LIN, NU, SIG0_LIN, SIG0_V, SIGU_V, to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    el = jm.LinearElasticIsotropic(E=E, nu=NU)

    def strains(kind, sig0, seed=2028):
        rng = np.random.default_rng(seed)
        d = rng.standard_normal((n, 4))
        if kind == "yielded":
            d[:, :3] -= d[:, :3].mean(axis=1, keepdims=True)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        lo, hi = {"elastic": (0.0, 0.9), "mixed": (0.0, 3.0), "yielded": (2.0, 4.0)}[kind]
        return d * rng.uniform(lo, hi, n)[:, None] * (sig0 / E)

    def timed(m, g, flux, ct):
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    laws = (("elastic", lambda h: jm.ElasticBehavior(el, hypothesis=h), SIG0_LIN, ("mixed",)),
            ("j2_linear", lambda h: jm.vonMisesIsotropicHardening(el, jm.LinearHardening(SIG0_LIN, H_LIN), hypothesis=h), SIG0_LIN, ("elastic", "mixed", "yielded")),
            ("j2_voce", lambda h: jm.vonMisesIsotropicHardening(el, jm.VoceHardening(SIG0_V, SIGU_V, B_V), hypothesis=h), SIG0_V, ("elastic", "mixed", "yielded")))
    for name, make, sig0, batches in laws:
        m4, m6 = JAXMaterial(make("plane_strain")), JAXMaterial(make("3d"))
        m4.set_data_manager(n)
        m6.set_data_manager(n)
        f4, c4 = torch.empty((n, 4), dtype=torch.float64, device="cuda:0"), torch.empty((n, 16), dtype=torch.float64, device="cuda:0")
        f6, c6 = torch.empty((n, 6), dtype=torch.float64, device="cuda:0"), torch.empty((n, 36), dtype=torch.float64, device="cuda:0")
        for tag in batches:
            e4 = strains(tag, sig0)
            g4, g6 = to_device(e4), to_device(embed_plane_strain(e4))
            del e4
            t4, t6 = [], []
            for _ in range(3):          # interleaved: both kernels see the same drift of the machine
                t6.append(timed(m6, g6, f6, c6))
                t4.append(timed(m4, g4, f4, c4))
            _, s4 = m4.stats()
            _, s6 = m6.stats()
            ms4, ms6 = float(np.median(t4)), float(np.median(t6))
            b4, b6 = m4.algorithmic_bytes_per_point, m6.algorithmic_bytes_per_point
            r = {"law": f"plane_strain:{name}+{tag}", "points": n, "kernel": m4.kernel_name, "kernel_ms_repeats": [round(x, 4) for x in t4],
                 "kernel_ms": round(ms4, 4), "algorithmic_bytes_per_point": b4, "frac_of_8TBs": round(b4 * n / ms4 / 1e6 / 8000, 4),
                 "six_wide_kernel": m6.kernel_name, "six_wide_ms_repeats": [round(x, 4) for x in t6], "six_wide_ms": round(ms6, 4),
                 "six_wide_bytes_per_point": b6, "six_wide_frac_of_8TBs": round(b6 * n / ms6 / 1e6 / 8000, 4),
                 "ratio_to_six_wide": round(ms4 / ms6, 3), "byte_ratio": round(b4 / b6, 3), "ratio_to_byte_scaled_six_wide": round(ms4 / (ms6 * b4 / b6), 3),
                 "plastic_fraction": round(s4["n_plastic"] / n, 4), "same_plastic_count": s4["n_plastic"] == s6["n_plastic"],
                 "max_local_iters": s4["max_local_iters"], "not_converged": s4["n_not_converged"], "nan": s4["n_nan"]}
            if a.blocks_per_cu:
                sweep = {}
                for b in a.blocks_per_cu:
                    m4.set_option("blocks_per_cu", b)
                    sweep[b] = round(timed(m4, g4, f4, c4), 4)
                m4.set_option("blocks_per_cu", 256 if name == "j2_voce" else 128)      # the shipped grid again (plane_strain.hpp)
                r["kernel_ms_by_blocks_per_cu"] = sweep
            print(json.dumps(r), flush=True)
            del g4, g6
        m4.close()
        m6.close()
        del m4, m6, f4, c4, f6, c6
        torch.cuda.empty_cache()


def bench_plane_stress_j2(a):
    """--laws ps_j2: laws 30 / 31 next to law 23 (q = 3/2, consistent tangent) and to law 27 / 28 of the same process on the same
    strains.  One JSON line per law and batch: kernel ms of the three (median of three medians, interleaved), the fraction of 8 TB/s at
    the counted bytes, and the ratio of the new kernel's time to each yardstick scaled by the byte ratio (184 / 168, 184 / 272).
    Batches from the virgin state, trials log-uniform in 0.05 ... 0.95 (elastic), 0.2 ... 8 (mixed) and 1.01 ... 100 (yielded) times the
    initial yield surface.  --blocks-per-cu: the new kernel at each of these grid sizes as well."""
    import torch

    import dolfinx_materials_amd.materials as jm
    import plane_stress_j2_ref as pj
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from dolfinx_materials_amd.plane_stress import PlaneStressvonMises, PlaneStressvonMisesHardening
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream

    def timed(m, g, flux, ct):
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    el = jm.LinearElasticIsotropic(E=pj.E, nu=pj.NU)
    for name, hard in (("linear", jm.LinearHardening(250.0, 5e3)), ("voce", jm.VoceHardening(350.0, 500.0, 1e3))):
        mj = PlaneStressvonMisesHardening(pj.E, pj.NU, hard)
        m23 = PlaneStressvonMises(pj.E, pj.NU, hard.sig0, shear_weight=1.5, tangent="consistent")
        m27 = JAXMaterial(jm.vonMisesIsotropicHardening(el, hard, hypothesis="plane_strain"))
        for m in (mj, m23, m27):
            m.set_data_manager(n)
        prm = mj.behavior.params()
        f3, c3 = torch.empty((n, 3), dtype=torch.float64, device="cuda:0"), torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
        f4, c4 = torch.empty((n, 4), dtype=torch.float64, device="cuda:0"), torch.empty((n, 16), dtype=torch.float64, device="cuda:0")
        for tag, lo, hi in (("elastic", 0.05, 0.95), ("mixed", 0.2, 8.0), ("yielded", 1.01, 100.0)):
            e3 = pj.random_trials(prm, n, seed=2029, lo=lo, hi=hi)
            e4 = np.zeros((n, 4))
            e4[:, :2], e4[:, 3] = e3[:, :2], e3[:, 2]
            g3, g4 = to_device(e3), to_device(e4)
            del e3, e4
            tj, t23, t27 = [], [], []
            for _ in range(3):          # interleaved: the three kernels see the same drift of the machine
                t23.append(timed(m23, g3, f3, c3))
                t27.append(timed(m27, g4, f4, c4))
                tj.append(timed(mj, g3, f3, c3))
            _, sj = mj.stats()
            _, s23 = m23.stats()
            ms, ms23, ms27 = float(np.median(tj)), float(np.median(t23)), float(np.median(t27))
            ab = mj.algorithmic_bytes_per_point
            r = {"law": f"ps_j2:{name}+{tag}", "points": n, "kernel": mj.kernel_name, "kernel_ms_repeats": [round(x, 4) for x in tj],
                 "kernel_ms": round(ms, 4), "algorithmic_bytes_per_point": ab, "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4),
                 "law23_ms_repeats": [round(x, 4) for x in t23], "law23_ms": round(ms23, 4), "law23_scaled_ms": round(ms23 * ab / 168, 4),
                 "ratio_to_scaled_law23": round(ms / (ms23 * ab / 168), 3),
                 "plane_strain_kernel": m27.kernel_name, "plane_strain_ms_repeats": [round(x, 4) for x in t27], "plane_strain_ms": round(ms27, 4),
                 "plane_strain_scaled_ms": round(ms27 * ab / 272, 4), "ratio_to_scaled_plane_strain": round(ms / (ms27 * ab / 272), 3),
                 "plastic_fraction": round(sj["n_plastic"] / n, 4), "law23_plastic_fraction": round(s23["n_plastic"] / n, 4),
                 "max_local_iters": sj["max_local_iters"], "law23_max_local_iters": s23["max_local_iters"],
                 "not_converged": sj["n_not_converged"], "nan": sj["n_nan"]}
            if a.blocks_per_cu:
                sweep = {}
                for b in a.blocks_per_cu:
                    mj.set_option("blocks_per_cu", b)
                    sweep[b] = round(timed(mj, g3, f3, c3), 4)
                mj.set_option("blocks_per_cu", 32)      # the shipped grid again (plane_stress_j2.hpp)
                r["kernel_ms_by_blocks_per_cu"] = sweep
            print(json.dumps(r), flush=True)
            del g3, g4
        for m in (mj, m23, m27):
            m.close()
        del mj, m23, m27, f3, c3, f4, c4
        torch.cuda.empty_cache()


def bench_plane_stress_hosford(a):
    """--laws ps_hosford: law 33 at the demo's E = 70e3, nu = 0.2, sig0 = 30 and a = 10 next to law 23 (the demo's PlaneStressvonMises,
    the same tangent mode) of the same process on the same strains; both move 168 B/point.  One JSON line per tangent mode and batch:
    kernel ms of both (median of three medians, interleaved), the fraction of 8 TB/s at the counted bytes, their ratio.  Batches from the
    virgin state, trials log-uniform in 0.05 ... 0.95 (elastic), 0.2 ... 8 (mixed) and 1.01 ... 100 (yielded) times the Hosford surface.
    --blocks-per-cu: the new kernel at each of these grid sizes as well."""
    import torch

    import plane_stress_hosford_ref as psh
    from dolfinx_materials_amd.plane_stress import PlaneStressHosford, PlaneStressvonMises
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    E, nu, sig0, expo = 70e3, 0.2, 30.0, 10.0

    def timed(m, g, flux, ct):
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    f3, c3 = torch.empty((n, 3), dtype=torch.float64, device="cuda:0"), torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
    for tangent in ("elastic", "consistent"):
        mh = PlaneStressHosford(E=E, nu=nu, sig0=sig0, a=expo, tangent=tangent)
        m23 = PlaneStressvonMises(E=E, nu=nu, sig0=sig0, tangent=tangent)
        for m in (mh, m23):
            m.set_data_manager(n)
        for tag, lo, hi in (("elastic", 0.05, 0.95), ("mixed", 0.2, 8.0), ("yielded", 1.01, 100.0)):
            rng = np.random.default_rng(2033)
            v = rng.normal(size=(n, 3))
            v *= (sig0 / psh.phi(v, expo) * np.exp(rng.uniform(np.log(lo), np.log(hi), n)))[:, None]
            g3 = to_device(v @ psh.compliance(E, nu).T)
            del v
            th, t23 = [], []
            for _ in range(3):          # interleaved: both kernels see the same drift of the machine
                t23.append(timed(m23, g3, f3, c3))
                th.append(timed(mh, g3, f3, c3))
            _, sh = mh.stats()
            _, s23 = m23.stats()
            ms, ms23 = float(np.median(th)), float(np.median(t23))
            ab = mh.algorithmic_bytes_per_point
            r = {"law": f"ps_hosford:a10+{tangent}+{tag}", "points": n, "kernel": mh.kernel_name, "kernel_ms_repeats": [round(x, 4) for x in th],
                 "kernel_ms": round(ms, 4), "algorithmic_bytes_per_point": ab, "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4),
                 "ps_vonmises_ms_repeats": [round(x, 4) for x in t23], "ps_vonmises_ms": round(ms23, 4), "ratio_to_ps_vonmises": round(ms / ms23, 3),
                 "plastic_fraction": round(sh["n_plastic"] / n, 4), "ps_vonmises_plastic_fraction": round(s23["n_plastic"] / n, 4),
                 "max_local_iters": sh["max_local_iters"], "ps_vonmises_max_local_iters": s23["max_local_iters"],
                 "not_converged": sh["n_not_converged"], "nan": sh["n_nan"]}
            if a.blocks_per_cu:
                sweep = {}
                for b in a.blocks_per_cu:
                    mh.set_option("blocks_per_cu", b)
                    sweep[b] = round(timed(mh, g3, f3, c3), 4)
                mh.set_option("blocks_per_cu", 32)      # the shipped grid again (plane_stress_hosford.hpp)
                r["kernel_ms_by_blocks_per_cu"] = sweep
            print(json.dumps(r), flush=True)
            del g3
        for m in (mh, m23):
            m.close()
        del mh, m23
    del f3, c3
    torch.cuda.empty_cache()


def bench_heat_plane(a):
    """--laws heat_plane: the 2-wide laws 35 / 36 beside the 3-wide laws 16 / 17 OF THIS PROCESS on the padded gradient (array form,
    uniform temperature and one temperature per point; ratio to the 3-wide time scaled by the bytes, 64/120 and 80/136, + 8 each with a
    temperature stream); the nodal form on a Q1 grid of 4-point quadrilaterals next to "gradient kernel + array form" (option
    fused_gradient 0); with --blocks-per-cu the array form at each grid size; and the host form (nodal temperature up) next to the
    padded 3-wide route through law 16 (gradient and temperature up), time per update and bytes up."""
    import time

    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.gradient import PlaneScalarMesh
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import to_device

    side = max(2, int(round((a.points / 4) ** 0.5)))
    xs = np.linspace(0.0, 1.0, side + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    i, j = (v.ravel() for v in np.meshgrid(np.arange(side), np.arange(side), indexing="ij"))
    idx = lambda di, dj: (i + di) * (side + 1) + (j + dj)   # noqa: E731
    cells = np.stack([idx(0, 0), idx(1, 0), idx(0, 1), idx(1, 1)], axis=1).astype(np.int32)
    mesh, xd = PlaneScalarMesh.lagrange(coords, cells, degree=1)
    n = mesh.npoints
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2026)
    g2 = rng.normal(size=(n, 2)) * 100.0
    g = {2: to_device(g2), 3: to_device(np.concatenate([g2, np.zeros((n, 1))], axis=1))}
    t_nodal = np.ascontiguousarray(933.15 + 3.0 * (xd[:, 0] - 0.5) + 0.02 * rng.standard_normal(len(xd)))
    t_dev = to_device(t_nodal)

    def timed(call):
        def once():
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                call()
                e1.record()
            torch.cuda.synchronize()
            return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
        t = [once(), once(), once()]
        return float(np.median(t)), [round(x, 4) for x in t]

    def line(tag, m, ms, reps, **more):
        rc, stats = m.stats()
        ab = m.algorithmic_bytes_per_point
        r = {"law": tag, "points": n, "kernel": m.kernel_name, "kernel_ms_repeats": reps, "kernel_ms": round(ms, 4), "Mpoints_per_s": round(n / ms / 1e3, 1),
             "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / ms / 1e6, 1), "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4), "nan": stats["n_nan"], "rc": rc}
        r.update(more)
        print(json.dumps(r), flush=True)

    for name, make in (("stationary", lambda hyp: jm.StationaryHeatTransfer(hypothesis=hyp)),
                       ("phase_change", lambda hyp: jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0}, hypothesis=hyp))):
        m3, m2 = JAXMaterial(make("3d")), JAXMaterial(make("plane_strain"))
        out = {}
        for m, w in ((m3, 3), (m2, 2)):
            m.set_data_manager(n)
            out[w] = (torch.empty((n, w), dtype=torch.float64, device=g[w].device), torch.empty((n, m.tangent_size), dtype=torch.float64, device=g[w].device))
        Tfield = rng.uniform(600.0, 1300.0, n) if name == "phase_change" else rng.uniform(300.0, 1500.0, n)
        for tag in ("uniformT", "fieldT"):
            wide = {}
            for m, w in ((m3, 3), (m2, 2)):
                m.update_external_state_variable("Temperature", (933.4 if name == "phase_change" else 700.0) if tag == "uniformT" else Tfield)
                ms, reps = timed(lambda m=m, w=w: m.integrate_device(g[w].data_ptr(), out[w][0].data_ptr(), out[w][1].data_ptr(), st))
                if w == 3:
                    wide = dict(ms=ms, ab=m.algorithmic_bytes_per_point, reps=reps)
                    line(f"heat_{name}+{tag}", m, ms, reps)
                else:
                    scaled = wide["ms"] * m.algorithmic_bytes_per_point / wide["ab"]
                    line(f"heat_plane_{name}+{tag}", m, ms, reps, wide_ms=round(wide["ms"], 4), wide_ms_repeats=wide["reps"],
                         byte_ratio_to_wide=round(m.algorithmic_bytes_per_point / wide["ab"], 4), wide_scaled_ms=round(scaled, 4),
                         ratio_to_yardstick=round(ms / scaled, 3))
        # the nodal form: one launch, and "gradient kernel + array form" through the handle's scratch
        for fused in (1, 0):
            m2.set_option("fused_gradient", fused)
            ms, reps = timed(lambda: m2.integrate_displacement_device(mesh, t_dev.data_ptr(), out[2][0].data_ptr(), out[2][1].data_ptr(), st))
            line(f"heat_plane_{name}+nodal+fused{fused}", m2, ms, reps, n_dofs=int(mesh.n_dofs))
        m2.set_option("fused_gradient", 1)
        if name == "stationary":
            # the host forms: the nodal temperature up (n_dofs x 8 B) against grad(T) padded and T up through law 16 (32 B/point)
            g3_host, T_host = np.ascontiguousarray(np.concatenate([g2, np.zeros((n, 1))], axis=1)), np.ascontiguousarray(Tfield)
            for tag, call, up in (("nodal", lambda: m2.integrate_displacement(mesh, t_nodal), 8 * int(mesh.n_dofs)),
                                  ("padded3", lambda: (m3.update_external_state_variable("Temperature", T_host), m3.integrate(g3_host)), 32 * n)):
                for _ in range(3):
                    call()
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                print(json.dumps({"law": f"heat_plane_stationary+host+{tag}", "points": n, "update_ms_repeats": [round(x, 3) for x in ts],
                                  "update_ms": round(float(np.median(ts)), 3), "bytes_up": up}), flush=True)
            del g3_host, T_host
        for bpc in a.blocks_per_cu or ():      # last, the handle keeps the grid: the array form with a temperature stream at each grid size
            m2.set_option("blocks_per_cu", bpc)
            ms, reps = timed(lambda: m2.integrate_device(g[2].data_ptr(), out[2][0].data_ptr(), out[2][1].data_ptr(), st))
            line(f"heat_plane_{name}+fieldT+bpc{bpc}", m2, ms, reps)
        m3.close()
        m2.close()
        del out
        torch.cuda.empty_cache()
    mesh.close()


def bench_ogden_plane(a):
    """--laws ogden_plane: law 38 (Ogden on the 5-wide plane-strain F) next to law 7 OF THIS PROCESS on the same gradients, embedded.
    One JSON line: kernel ms of both (median of three medians, interleaved), fraction of 8 TB/s at the counted bytes (312 against
    840), the ratio of the 5-wide time to the 9-wide time and to the 9-wide time scaled by the byte ratio, and the resources the
    library reports for both kernels.  F5 = [1, 1, 1, 0, 0] + 0.2 U(-1/2, 1/2).  --blocks-per-cu: law 38 at each of these grid
    sizes as well."""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.conventions import embed_plane_F
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream

    def timed(m, g, flux, ct):
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    m5, m9 = JAXMaterial(jm.OgdenHyperelasticity(hypothesis="plane_strain")), JAXMaterial(jm.OgdenHyperelasticity())
    m5.set_data_manager(n)
    m9.set_data_manager(n)
    f5, c5 = torch.empty((n, 5), dtype=torch.float64, device="cuda:0"), torch.empty((n, 25), dtype=torch.float64, device="cuda:0")
    f9, c9 = torch.empty((n, 9), dtype=torch.float64, device="cuda:0"), torch.empty((n, 81), dtype=torch.float64, device="cuda:0")
    F5 = np.array([1.0, 1.0, 1.0, 0.0, 0.0])[None] + 0.2 * (np.random.default_rng(2031).random((n, 5)) - 0.5)
    g5, g9 = to_device(F5), to_device(embed_plane_F(F5))
    del F5
    t5, t9 = [], []
    for _ in range(3):          # interleaved: both kernels see the same drift of the machine
        t9.append(timed(m9, g9, f9, c9))
        t5.append(timed(m5, g5, f5, c5))
    _, s5 = m5.stats()
    _, s9 = m9.stats()
    # the restriction, on the device: what law 38 writes against rows / columns 0..4 of law 7's block
    dP = float((f5 - f9[:, :5]).abs().max() / f9.abs().max())
    dA = float((c5.view(n, 5, 5) - c9.view(n, 9, 9)[:, :5, :5]).abs().max() / c9.abs().max())
    ms5, ms9 = float(np.median(t5)), float(np.median(t9))
    b5, b9 = m5.algorithmic_bytes_per_point, m9.algorithmic_bytes_per_point
    r = {"law": "ogden_plane", "points": n, "kernel": m5.kernel_name, "kernel_ms_repeats": [round(x, 4) for x in t5], "kernel_ms": round(ms5, 4),
         "algorithmic_bytes_per_point": b5, "frac_of_8TBs": round(b5 * n / ms5 / 1e6 / 8000, 4),
         "nine_wide_kernel": m9.kernel_name, "nine_wide_ms_repeats": [round(x, 4) for x in t9], "nine_wide_ms": round(ms9, 4),
         "nine_wide_bytes_per_point": b9, "nine_wide_frac_of_8TBs": round(b9 * n / ms9 / 1e6 / 8000, 4),
         "ratio_to_nine_wide": round(ms5 / ms9, 3), "byte_ratio": round(b5 / b9, 3), "ratio_to_byte_scaled_nine_wide": round(ms5 / (ms9 * b5 / b9), 3),
         "max_abs_difference_to_nine_wide_restricted": {"P_over_max_P": dP, "A_over_max_A": dA}, "nan": s5["n_nan"], "nine_wide_nan": s9["n_nan"],
         "warmup": a.warmup, "reps": a.reps}
    if a.blocks_per_cu:
        sweep = {}
        for b in a.blocks_per_cu:
            m5.set_option("blocks_per_cu", b)
            sweep[b] = round(timed(m5, g5, f5, c5), 4)
        m5.set_option("blocks_per_cu", 32)      # the shipped grid again (ogden_plane.hpp)
        r["kernel_ms_by_blocks_per_cu"] = sweep
    print(json.dumps(r), flush=True)
    m5.close()
    m9.close()


def bench_pe_hosford(a):
    """--laws pe_hosford: law 40 (Hosford on the 4-wide plane-strain strain) next to law 10 OF THIS PROCESS on the same strains,
    embedded, at the multi-material demo's parameters (E 70e3, nu 0.3, R0 200, H 10, a 10), from the natural state.  Three batch kinds:
    elastic (seq_trial / R0 in 0.1 ... 0.9), mixed (every point elastic or yielded with probability 1/2) and fully yielded (1.05 ... 3).
    One JSON line: per kind the kernel ms of both (median of three medians, interleaved), the fraction of 8 TB/s at the counted bytes
    (304 against 544), the ratio of the 4-wide time to the 6-wide time beside the byte ratio, the plastic counts of both and the
    largest difference of stress and tangent to law 10 restricted; the resources the build reports are in DESIGN.md.
    --blocks-per-cu: law 40 at each of these grid sizes as well, on the mixed batch."""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.conventions import embed_plane_strain
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import to_device
    import hosford_plane_ref as hp

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    E, nu, R0, H, ex = 70e3, 0.3, 200.0, 10.0, 10.0

    def timed(m, g, flux, ct):
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    def behaviour(hypothesis):
        return jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=E, nu=nu), jm.LinearHardening(R0, H), a=ex, hypothesis=hypothesis)

    m4, m6 = JAXMaterial(behaviour("plane_strain")), JAXMaterial(behaviour("3d"))
    m4.set_data_manager(n)
    m6.set_data_manager(n)
    f4, c4 = torch.empty((n, 4), dtype=torch.float64, device="cuda:0"), torch.empty((n, 16), dtype=torch.float64, device="cuda:0")
    f6, c6 = torch.empty((n, 6), dtype=torch.float64, device="cuda:0"), torch.empty((n, 36), dtype=torch.float64, device="cuda:0")
    el = hp.make_inputs("elastic", n, ex, 2041, E=E, nu=nu, R0=R0, H=H, trivial_state=True)[0]
    yl = hp.make_inputs("generic", n, ex, 2042, E=E, nu=nu, R0=R0, H=H, trivial_state=True)[0]
    pick = np.random.default_rng(2043).random(n) < 0.5
    b4, b6 = m4.algorithmic_bytes_per_point, m6.algorithmic_bytes_per_point
    r = {"law": "pe_hosford", "points": n, "kernel": m4.kernel_name, "six_wide_kernel": m6.kernel_name, "params": [E, nu, R0, H, ex],
         "algorithmic_bytes_per_point": b4, "six_wide_bytes_per_point": b6, "byte_ratio": round(b4 / b6, 3), "batches": {},
         "warmup": a.warmup, "reps": a.reps}
    g4_mixed = None
    for kind, eps in (("elastic", el), ("mixed", np.where(pick[:, None], yl, el)), ("yielded", yl)):
        g4, g6 = to_device(eps), to_device(embed_plane_strain(eps))
        t4, t6 = [], []
        for _ in range(3):          # interleaved: both kernels see the same drift of the machine
            t6.append(timed(m6, g6, f6, c6))
            t4.append(timed(m4, g4, f4, c4))
        _, s4 = m4.stats()
        _, s6 = m6.stats()
        # the restriction, on the device: what law 40 writes against components / rows / columns 0..3 of law 10's outputs
        dS = float((f4 - f6[:, :4]).abs().max() / f6.abs().max())
        dC = float((c4.view(n, 4, 4) - c6.view(n, 6, 6)[:, :4, :4]).abs().max() / c6.abs().max())
        ms4, ms6 = float(np.median(t4)), float(np.median(t6))
        r["batches"][kind] = {"kernel_ms_repeats": [round(x, 4) for x in t4], "kernel_ms": round(ms4, 4), "frac_of_8TBs": round(b4 * n / ms4 / 1e6 / 8000, 4),
                              "six_wide_ms_repeats": [round(x, 4) for x in t6], "six_wide_ms": round(ms6, 4),
                              "six_wide_frac_of_8TBs": round(b6 * n / ms6 / 1e6 / 8000, 4), "ratio_to_six_wide": round(ms4 / ms6, 3),
                              "ratio_to_byte_scaled_six_wide": round(ms4 / (ms6 * b4 / b6), 3),
                              "n_plastic": s4["n_plastic"], "six_wide_n_plastic": s6["n_plastic"],
                              "n_not_converged": s4["n_not_converged"], "six_wide_n_not_converged": s6["n_not_converged"],
                              "n_nan": s4["n_nan"], "max_local_iters": s4["max_local_iters"],
                              "max_abs_difference_to_six_wide_restricted": {"stress_over_max_stress": dS, "tangent_over_max_tangent": dC}}
        if kind == "mixed":
            g4_mixed = g4
        del g6
    if a.blocks_per_cu:
        sweep = {}
        for b in a.blocks_per_cu:
            m4.set_option("blocks_per_cu", b)
            sweep[b] = round(timed(m4, g4_mixed, f4, c4), 4)
        m4.set_option("blocks_per_cu", 64)      # the shipped grid again (hosford_plane.hpp)
        r["mixed_kernel_ms_by_blocks_per_cu"] = sweep
    print(json.dumps(r), flush=True)
    m4.close()
    m6.close()


def bench_log_strain_plane(a):
    """--laws log_strain_plane: law 42 (logarithmic-strain J2 on the 5-wide plane-strain F) next to law 19 OF THIS PROCESS on the same
    gradients, embedded, at the demo's material properties, from the natural state.  F5 = [1, 1, 1, 0, 0] + amp U(-1/2, 1/2); three
    batch kinds: elastic (amp 5e-4: below the yield strain of 1.2e-3), fully yielded (amp 2e-2) and mixed (every point one or the other
    with probability 1/2).  One JSON line: per kind the kernel ms of both (median of three medians, interleaved), the fraction of 8 TB/s
    at the counted bytes (392 against 952), the ratio of the 5-wide time to the 9-wide time beside the byte ratio, the plastic counts of
    both and the largest difference of PK1 and tangent to law 19 restricted; the resources the build reports are in DESIGN.md.
    --blocks-per-cu: law 42 at each of these grid sizes as well, on the mixed batch."""
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.conventions import embed_plane_F
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import to_device

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    s0, H0 = 250e6, 1e6

    def timed(m, g, flux, ct):
        for _ in range(a.warmup):
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            m.integrate_device(g.data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    m5, m9 = JAXMaterial(jm.LogarithmicStrainPlasticity(s0, H0, hypothesis="plane_strain")), JAXMaterial(jm.LogarithmicStrainPlasticity(s0, H0))
    m5.set_data_manager(n)
    m9.set_data_manager(n)
    f5, c5 = torch.empty((n, 5), dtype=torch.float64, device="cuda:0"), torch.empty((n, 25), dtype=torch.float64, device="cuda:0")
    f9, c9 = torch.empty((n, 9), dtype=torch.float64, device="cuda:0"), torch.empty((n, 81), dtype=torch.float64, device="cuda:0")
    eye = np.array([1.0, 1.0, 1.0, 0.0, 0.0])[None]
    u = np.random.default_rng(2051).random((n, 5)) - 0.5
    pick = np.random.default_rng(2052).random(n) < 0.5
    b5, b9 = m5.algorithmic_bytes_per_point, m9.algorithmic_bytes_per_point
    r = {"law": "log_strain_plane", "points": n, "kernel": m5.kernel_name, "nine_wide_kernel": m9.kernel_name, "params": [210e9, 0.3, s0, H0],
         "algorithmic_bytes_per_point": b5, "nine_wide_bytes_per_point": b9, "byte_ratio": round(b5 / b9, 3), "batches": {},
         "warmup": a.warmup, "reps": a.reps}
    g5_mixed = None
    for kind, amp in (("elastic", 5e-4), ("mixed", np.where(pick, 2e-2, 5e-4)[:, None]), ("yielded", 2e-2)):
        F5 = eye + amp * u
        g5, g9 = to_device(F5), to_device(embed_plane_F(F5))
        del F5
        t5, t9 = [], []
        for _ in range(3):          # interleaved: both kernels see the same drift of the machine
            t9.append(timed(m9, g9, f9, c9))
            t5.append(timed(m5, g5, f5, c5))
        _, s5 = m5.stats()
        _, s9 = m9.stats()
        # the restriction, on the device: what law 42 writes against components / rows / columns 0..4 of law 19's outputs
        dP = float((f5 - f9[:, :5]).abs().max() / f9.abs().max())
        dA = float((c5.view(n, 5, 5) - c9.view(n, 9, 9)[:, :5, :5]).abs().max() / c9.abs().max())
        ms5, ms9 = float(np.median(t5)), float(np.median(t9))
        r["batches"][kind] = {"kernel_ms_repeats": [round(x, 4) for x in t5], "kernel_ms": round(ms5, 4), "frac_of_8TBs": round(b5 * n / ms5 / 1e6 / 8000, 4),
                              "nine_wide_ms_repeats": [round(x, 4) for x in t9], "nine_wide_ms": round(ms9, 4),
                              "nine_wide_frac_of_8TBs": round(b9 * n / ms9 / 1e6 / 8000, 4), "ratio_to_nine_wide": round(ms5 / ms9, 3),
                              "ratio_to_byte_scaled_nine_wide": round(ms5 / (ms9 * b5 / b9), 3),
                              "n_plastic": s5["n_plastic"], "nine_wide_n_plastic": s9["n_plastic"], "n_nan": s5["n_nan"], "nine_wide_n_nan": s9["n_nan"],
                              "max_abs_difference_to_nine_wide_restricted": {"P_over_max_P": dP, "A_over_max_A": dA}}
        if kind == "mixed":
            g5_mixed = g5
        del g9
    if a.blocks_per_cu:
        sweep = {}
        for b in a.blocks_per_cu:
            m5.set_option("blocks_per_cu", b)
            sweep[b] = round(timed(m5, g5_mixed, f5, c5), 4)
        m5.set_option("blocks_per_cu", 256)      # the shipped grid again (log_strain_plane.hpp)
        r["mixed_kernel_ms_by_blocks_per_cu"] = sweep
    print(json.dumps(r), flush=True)
    m5.close()
    m9.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches before the timed ones (a fresh allocation needs 10-20 launches to reach its steady time)")
    ap.add_argument("--laws", nargs="+", default=["elastic", "j2_linear", "j2_voce", "fefp"])
    ap.add_argument("--cpu-sample", type=int, default=0, help="also time the plain-C oracle on this many points")
    ap.add_argument("--sym", action="store_true", help="symmetric-packed tangent (small-strain laws)")
    ap.add_argument("--blocks-per-cu", type=int, nargs="+", default=None,
                    help="ramberg_osgood, plane_strain, ps_j2, ps_hosford, heat_plane, ogden_plane, pe_hosford, log_strain_plane: time the kernel at each of these grid sizes (dxm option blocks_per_cu) as well")
    ap.add_argument("--param-fields", type=int, nargs="+", default=None, metavar="K",
                    help="j2_linear / j2_voce: also time the kernel with K bound per-point parameter streams (1 ... 4 | 5)")
    a = ap.parse_args()
    if a.cpu_sample and ("ramberg_osgood" in a.laws or "ogden" in a.laws or "hosford" in a.laws or "orthotropic" in a.laws or "single_crystal" in a.laws or
                         "heat_stationary" in a.laws or "heat_phase_change" in a.laws or "heat_plane" in a.laws or "log_strain" in a.laws or "fs_single_crystal" in a.laws or
                         any(law.startswith("ps_") for law in a.laws) or "plane_strain" in a.laws or "ogden_plane" in a.laws or "pe_hosford" in a.laws or
                         "log_strain_plane" in a.laws):   # (ps_j2 among them)
        ap.error("--cpu-sample: the plain-C oracle (oracle/oracle_c.c) has no Ramberg-Osgood, Ogden, Hosford, orthotropic, single-crystal, heat-transfer or logarithmic-strain law")
    import torch

    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.jaxmat import JAXMaterial
    from helpers import E, NU, SIG0_LIN, H_LIN, SIG0_V, SIGU_V, B_V, SIG0_F, SIGU_F, B_F, j2_history, fefp_path

    dev = torch.device("cuda:0")
    n = a.points
    el = jm.LinearElasticIsotropic(E=E, nu=NU)
    res = []
    elastic_ms = None
    fefp_ms = None
    j2_linear_ms = None
    elastic_repeats = None
    for law in a.laws:
        if law == "single_crystal":   # its own inputs, state and nine lines
            bench_single_crystal(a, j2_linear_ms)
            continue
        if law == "fs_single_crystal":   # its own inputs, state and nine lines
            bench_fs_single_crystal(a)
            continue
        if law in ("heat_stationary", "heat_phase_change"):   # their own inputs and two lines each
            bench_heat_transfer(a, law, elastic_ms, elastic_repeats)
            continue
        if law in ("ps_vonmises", "ps_rankine", "ps_l1rankine"):   # their own inputs and two lines each
            bench_plane_stress(a, law, elastic_ms, elastic_repeats)
            continue
        if law == "plane_strain":   # laws 26 / 27 / 28 beside laws 0 / 1 / 2 of this process: seven lines
            bench_plane_strain(a)
            continue
        if law == "ps_j2":   # laws 30 / 31 beside law 23 and laws 27 / 28 of this process: six lines
            bench_plane_stress_j2(a)
            continue
        if law == "ps_hosford":   # law 33 beside law 23 of this process: six lines
            bench_plane_stress_hosford(a)
            continue
        if law == "heat_plane":   # laws 35 / 36 beside laws 16 / 17 of this process, the nodal forms, the host form
            bench_heat_plane(a)
            continue
        if law == "ogden_plane":   # law 38 beside law 7 of this process on the embedded gradient: one line
            bench_ogden_plane(a)
            continue
        if law == "pe_hosford":   # law 40 beside law 10 of this process on the embedded strain, three batch kinds: one line
            bench_pe_hosford(a)
            continue
        if law == "log_strain_plane":   # law 42 beside law 19 of this process on the embedded gradient, three batch kinds: one line
            bench_log_strain_plane(a)
            continue
        if law == "ramberg_osgood":
            ro_eps = ramberg_osgood_strains(n)
            beh, hist = jm.RambergOsgoodNonLinearElasticity(jm.LinearElasticIsotropic(E=RO_E, nu=RO_NU), RO_SIG0, RO_ALPHA, RO_N), [ro_eps, ro_eps]
            del ro_eps
        elif law == "ogden":
            # the behaviour file's parameters; F = I + 0.2 U(-1/2, 1/2), the family of the law's parity tests
            rng = np.random.default_rng(2025)
            eye = np.array([1.0, 1, 1, 0, 0, 0, 0, 0, 0])
            beh, hist = jm.OgdenHyperelasticity(), [eye + 0.2 * (rng.random((n, 9)) - 0.5) for _ in range(2)]
        elif law == "log_strain":
            # the demo's material properties; F = I + 2e-3 U(-1/2, 1/2), the family of the law's parity tests (half of the points
            # yield in either increment; every tile costs the same: the update is a closed form)
            rng = np.random.default_rng(2026)
            eye = np.array([1.0, 1, 1, 0, 0, 0, 0, 0, 0])
            beh, hist = jm.LogarithmicStrainPlasticity(250e6, 1e6), [eye + 2e-3 * (rng.random((n, 9)) - 0.5) for _ in range(2)]
        elif law == "hosford":
            # the J2-linear parameters with the behaviour file's exponent a = 10, uniform (zero) state, the headline increments
            beh, hist = jm.HosfordIsotropicHardening(el, jm.LinearHardening(SIG0_LIN, H_LIN), a=10.0), j2_history(n)[1:3]
        elif law == "orthotropic":
            # E1 / E3 = 20 (the "strong" set of tests/orthotropic_ref.py) on the headline increments
            beh, hist = jm.OrthotropicElasticity(200e3, 40e3, 10e3, 0.25, 0.3, 0.2, 12e3, 4e3, 7e3), j2_history(n)[1:3]
        elif law == "elastic":
            beh, hist = jm.ElasticBehavior(el), j2_history(n)[1:3]
        elif law == "j2_linear":
            beh, hist = jm.vonMisesIsotropicHardening(el, jm.LinearHardening(SIG0_LIN, H_LIN)), j2_history(n)[1:3]
        elif law == "j2_voce":
            beh, hist = jm.vonMisesIsotropicHardening(el, jm.VoceHardening(SIG0_V, SIGU_V, B_V)), j2_history(n, sig0=SIG0_V)[1:3]
        else:
            path = fefp_path(n)
            beh, hist = jm.FeFpJ2Plasticity(el, jm.VoceHardening(SIG0_F, SIGU_F, B_F)), [path[9], path[18]]
        sym = a.sym and law not in ("fefp", "ogden", "log_strain")
        m = JAXMaterial(beh, tangent_layout="sym" if sym else "full")
        m.set_data_manager(n)
        ng, nf = m._info.n_grad, m._info.n_flux
        from helpers import to_device

        g = [to_device(h) for h in hist]
        del hist
        flux = torch.empty((n, nf), dtype=torch.float64, device=dev)
        ct = torch.empty((n, nf * ng), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        m.integrate_device(g[0].data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
        m.data_manager.update()  # s0 = state after the first increment

        def timed():
            for _ in range(a.warmup):
                m.integrate_device(g[1].data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                m.integrate_device(g[1].data_ptr(), flux.data_ptr(), ct.data_ptr(), st)
                e1.record()
            torch.cuda.synchronize()
            return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

        ms = timed()
        rc, stats = m.stats()
        sweep = {}
        if law == "ramberg_osgood" and a.blocks_per_cu:   # (after the shipped grid's timing and status)
            for b in a.blocks_per_cu:
                m.set_option("blocks_per_cu", b)
                sweep[b] = round(timed(), 4)
        ab = m.algorithmic_bytes_per_point - (15 * 8 if sym else 0)
        r = {
            "law": law + ("+sym21" if sym else ""), "points": n, "kernel_ms": round(ms, 4), "Mpoints_per_s": round(n / ms / 1e3, 1),
            "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / ms / 1e6, 1), "frac_of_8TBs": round(ab * n / ms / 1e6 / 8000, 4),
            "plastic_fraction": round(stats["n_plastic"] / n, 4), "max_local_iters": stats["max_local_iters"],
            "not_converged": stats["n_not_converged"], "rc": rc,
        }
        if law == "elastic" and not sym:   # two more timings: the spread the orthotropic lines are read against
            elastic_repeats = [round(ms, 4), round(timed(), 4), round(timed(), 4)]
            r["kernel_ms_repeats"] = elastic_repeats
            elastic_ms = float(np.median(elastic_repeats))
        if law in ("j2_linear", "hosford") and not sym:   # same-process comparison with the J2-linear kernel: two more timings each
            r["kernel"] = m.kernel_name
            r["kernel_ms_repeats"] = [round(ms, 4), round(timed(), 4), round(timed(), 4)]
            if law == "j2_linear":
                j2_linear_ms = float(np.median(r["kernel_ms_repeats"]))
            elif j2_linear_ms:
                r["ratio_to_j2_linear"] = round(float(np.median(r["kernel_ms_repeats"])) / j2_linear_ms, 3)
                r["byte_ratio_to_j2_linear"] = round(544 / 496, 3)
        if law in ("fefp", "ogden", "log_strain"):   # same-process comparison of the two finite-strain kernels: two more timings each, for the spread
            r["kernel"] = m.kernel_name
            r["kernel_ms_repeats"] = [round(ms, 4), round(timed(), 4), round(timed(), 4)]
            if law == "fefp":
                fefp_ms = float(np.median(r["kernel_ms_repeats"]))
            elif fefp_ms:
                r["ratio_to_fefp"] = round(float(np.median(r["kernel_ms_repeats"])) / fefp_ms, 3)
                r["byte_ratio_to_fefp"] = round(ab / 976, 3)
        if law == "ramberg_osgood":
            r["kernel"] = m.kernel_name
            if sweep:
                r["kernel_ms_by_blocks_per_cu"] = sweep
            if not sym and n % 64 == 0:
                pms = probe_ms(g[1], flux, ct, n, 32 * torch.cuda.get_device_properties(0).multi_processor_count, a.reps, a.warmup)
                r["probe_ms"] = round(pms, 4)
                r["ratio_to_probe"] = round(ms / pms, 3)
            if elastic_ms:
                r["ratio_to_elastic"] = round(ms / elastic_ms, 3)
        if a.cpu_sample:
            r["cpu_port"] = cpu_port(law, a.cpu_sample)
        if law == "orthotropic":
            r["law"] += "+noframe"
            r["kernel"] = m.kernel_name
        print(json.dumps(r), flush=True)
        res.append(r)
        if law == "orthotropic":
            from orthotropic_ref import axis_rotation, random_rotations

            first = [ms, timed(), timed()]
            for tag, frames in (("noframe", None), ("uniform", axis_rotation(2, np.pi / 3) @ axis_rotation(0, 0.4)),
                                ("field", random_rotations(np.random.default_rng(7), n))):
                if frames is not None:
                    m.set_frame(frames)
                t = first if frames is None else [timed(), timed(), timed()]
                del frames
                ab = m.algorithmic_bytes_per_point - (15 * 8 if sym else 0)
                f = {"law": f"orthotropic+{tag}" + ("+sym21" if sym else ""), "points": n, "kernel": m.kernel_name,
                     "kernel_ms_repeats": [round(x, 4) for x in t], "kernel_ms": round(float(np.median(t)), 4),
                     "algorithmic_bytes_per_point": ab, "GBs": round(ab * n / float(np.median(t)) / 1e6, 1)}
                if elastic_ms and not sym:
                    f["ratio_to_elastic"] = round(float(np.median(t)) / elastic_ms, 3)
                    f["byte_ratio_to_elastic"] = round(ab / 384, 3)
                    f["elastic_ms_repeats"] = elastic_repeats
                    f["elastic_spread_ms"] = round(max(elastic_repeats) - min(elastic_repeats), 4)
                    f["excess_over_yardstick_ms"] = round(float(np.median(t)) - elastic_ms * ab / 384, 4)
                print(json.dumps(f), flush=True)
        if a.param_fields and law in ("j2_linear", "j2_voce") and not sym:
            import ctypes

            prm = beh.params()
            order = [2, 0, 3, 4]                       # sig0 (1 stream), E (2: lambda and mu), H | sigu, b
            uniform = [ms, timed(), timed()]           # the uniform kernel again: the spread the field timings are read against
            h = m._require()
            for k in a.param_fields:
                idx = {1: [2], 2: [0], 3: [2, 0]}.get(k, order[: k - 1])
                idx = [i for i in idx if i < len(prm)]
                for i in idx:
                    v = np.full(n, prm[i])
                    m._chk(m._lib.dxm_set_param_field(h, i, v.ctypes.data))
                streams = (m._lib.dxm_algorithmic_bytes(h) - 496) // 8
                t = [timed(), timed()]
                for i in idx:
                    m._chk(m._lib.dxm_set_param_field(h, i, ctypes.c_void_p(None)))
                uniform.append(timed())
                base = float(np.median(uniform))
                yard = base * (496 + 8 * streams) / 496
                f = {"law": law + f"+fields{streams}", "points": n, "kernel": "small_strain_field_kernel", "streams": streams,
                     "kernel_ms": [round(x, 4) for x in t], "uniform_ms": [round(x, 4) for x in uniform],
                     "uniform_spread_ms": round(max(uniform) - min(uniform), 4), "yardstick_ms": round(yard, 4),
                     "excess_over_yardstick_ms": round(min(t) - yard, 4), "algorithmic_bytes_per_point": 496 + 8 * streams,
                     "GBs": round((496 + 8 * streams) * n / min(t) / 1e6, 1)}
                print(json.dumps(f), flush=True)
        del m, g, flux, ct
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
