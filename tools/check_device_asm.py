#!/usr/bin/env python3
"""Build-time checks of the device code of libdxmat's first six translation units (csrc/{dxmat,ramberg_osgood,param_fields,hyperelastic,
hosford,orthotropic}.hip), on the cross-compiler alone:

1. the resources of every kernel, read from -Rpass-analysis=kernel-resource-usage: no scratch and no spilled VGPR anywhere, and
   the kernels with per-point parameter fields within the bounds of the uniform J2 kernels (at most 128 VGPRs, the same static LDS,
   exactly 32 instantiations);
   With --all-units the same for the units added since (LATER_UNITS, PLANE_FORM_UNITS and PLANE_F_UNITS below), whose kernels need not keep to the
   bounds of the J2 kernels;
2. (--parent REV) the device assembly of every unit is byte for byte what the sources of git revision REV give (but for the
   compilation-unit id, which hashes the source file's path); the parent's resource figures are printed beside the tree's.

    python tools/check_device_asm.py [--parent HEAD~1] [--write-digests FILE.json]

Prints one line per kernel, one line per unit and a JSON summary; exit status 1 if a bound is broken or an assembly file differs.
The helpers are what tests/test_*_build.py and tests/test_tile_fragments.py assert with; unit_text() is the text of a unit that
their scans for required and forbidden words read: the unit's file with the tile_*.hpp texts it includes in place."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dolfinx_materials_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-S", "--cuda-device-only"]
UNITS = ("dxmat", "ramberg_osgood", "param_fields", "hyperelastic", "hosford", "orthotropic")
# the units added since (--all-units): compared with the parent's where the parent has them
LATER_UNITS = ("small_strain_clean", "single_crystal", "heat_transfer", "log_strain", "fs_single_crystal", "plane_stress",
               "plane_strain", "plane_stress_j2", "plane_stress_hosford", "plane_gradient", "small_strain_packed",
               "heat_plane")
# the plane-strain forms of laws 7 and 10 (--all-units walks them after LATER_UNITS, in the same way).  A list of its own:
# tests/test_ogden_plane_build.py pins LATER_UNITS to the units that existed before ogden_plane
PLANE_FORM_UNITS = ("ogden_plane", "hosford_plane")
# the plane-strain form of law 19, walked after them in the same way.  Again a list of its own: tests/test_hosford_plane_build.py
# pins PLANE_FORM_UNITS to the two units above
PLANE_F_UNITS = ("log_strain_plane",)
# the gradient kernels of an axisymmetric mesh.  Not walked by --all-units, whose unit lists tests pin; tests/test_axisym_gradient_build.py
# reads the unit's resources with device_asm() / resource_table() above
AXISYM_UNITS = ("axisym_gradient",)
MAX_VGPRS = 128
J2_STATIC_LDS = 30848     # small_strain.hpp: 4 waves x (64 x 6 + 64 x 9) doubles + the 4 x 4 status words


def unit_text(csrc, name):
    """csrc/NAME with every `#include "tile_*.hpp"` line replaced by that file's contents: the tile I/O steps are text of the kernel"""
    src = open(os.path.join(csrc, name)).read()
    return re.sub(r'^[ \t]*#include "(tile_\w+\.hpp)"[^\n]*$', lambda m: open(os.path.join(csrc, m.group(1))).read(), src, flags=re.M)


def device_asm(csrc, unit, out, remarks=False):
    cmd = [HIPCC] + FLAGS + (["-Rpass-analysis=kernel-resource-usage"] if remarks else []) + ["-o", out, unit + ".hip"]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}")
    return r.stderr


def resource_table(remarks):
    """kernel name -> dict of the figures of its remark block"""
    table = {}
    for blk in remarks.split("Function Name: ")[1:]:
        name = blk.split()[0]
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))   # noqa: E731
        table[name] = {"vgprs": num("VGPRs"), "agprs": num("AGPRs"), "sgprs": num("SGPRs"), "scratch": num("ScratchSize [bytes/lane]"),
                       "vgpr_spill": num("VGPRs Spill"), "sgpr_spill": num("SGPRs Spill"), "lds": num("LDS Size [bytes/block]"),
                       "occupancy": num("Occupancy [waves/SIMD]")}
    return table


def field_kernel_table(tmp):
    remarks = device_asm(CSRC, "param_fields", os.path.join(tmp, "param_fields.s"), remarks=True)
    return {k: v for k, v in resource_table(remarks).items() if "small_strain_field_kernel" in k}


def broken_bounds(table):
    bad = []
    for name, r in table.items():
        if r["scratch"] or r["vgpr_spill"] or r["vgprs"] + r["agprs"] > MAX_VGPRS or r["lds"] != J2_STATIC_LDS:
            bad.append(name)
    return bad


def template_args(name):
    m = re.search(r"small_strain_field_kernelILi(\d)ELi(\d)ELi(\d)E", name)
    return tuple(int(x) for x in m.groups())


def sha(path):
    """Of the assembly text without the compilation-unit id: the compiler derives the one symbol `__hip_cuid_<hash>` from the
    PATH of the source file, and the parent's sources are compiled from a temporary directory."""
    return hashlib.sha256(re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_", open(path, "rb").read())).hexdigest()


def build_units(csrc, tmp, tag, units=UNITS):
    """unit -> (sha256 of its device assembly, resource table), the six units compiled side by side"""
    def one(unit):
        out = os.path.join(tmp, f"{unit}_{tag}.s")
        remarks = device_asm(csrc, unit, out, remarks=True)
        return unit, (sha(out), resource_table(remarks))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        return dict(pool.map(one, units))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="git revision whose device assembly must be reproduced")
    ap.add_argument("--write-digests", default=None, help="with --parent: write the parent's digests to this JSON file")
    ap.add_argument("--all-units", action="store_true", help="also the units added after the first six: " + ", ".join(LATER_UNITS + PLANE_FORM_UNITS + PLANE_F_UNITS))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        new = build_units(CSRC, tmp, "tree")
        later_new, later_old = {}, {}
        if a.all_units:
            later_new = build_units(CSRC, tmp, "tree", LATER_UNITS + PLANE_FORM_UNITS + PLANE_F_UNITS)
        old = None
        if a.parent:
            src = os.path.join(tmp, "parent")
            os.makedirs(src)
            tar = subprocess.run(["git", "archive", a.parent, "dolfinx_materials_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", src], input=tar.stdout, check=True)
            old = build_units(os.path.join(src, "dolfinx_materials_amd", "csrc"), tmp, "parent")
            if a.all_units:
                there = tuple(u for u in LATER_UNITS + PLANE_FORM_UNITS + PLANE_F_UNITS if os.path.exists(os.path.join(src, "dolfinx_materials_amd", "csrc", u + ".hip")))
                later_old = build_units(os.path.join(src, "dolfinx_materials_amd", "csrc"), tmp, "parent", there)

    fmt = lambda r: (f"VGPRs {r['vgprs']:3d}  AGPRs {r['agprs']}  SGPRs {r['sgprs']:3d}  scratch {r['scratch']}  spilled VGPRs {r['vgpr_spill']}  "   # noqa: E731
                     f"spilled SGPRs {r['sgpr_spill']:2d}  LDS {r['lds']:5d}  waves/SIMD {r['occupancy']}")
    spills = []
    for unit in UNITS:
        table = new[unit][1]
        print(f"== {unit}: {len(table)} kernels")
        for name in sorted(table):
            r = table[name]
            was = old[unit][1].get(name) if old else None
            print(f"{name}\n    {fmt(r)}" + ("" if was is None else "   parent: same" if was == r else f"\n    parent: {fmt(was)}"))
            if r["scratch"] or r["vgpr_spill"]:
                spills.append(name)
    # the later units: resources, and the parent's assembly where the parent has the unit (a line format of their own: the lines of
    # the first six are counted by tests)
    later_same = True
    for unit in LATER_UNITS + PLANE_FORM_UNITS + PLANE_F_UNITS if a.all_units else ():
        table = later_new[unit][1]
        print(f"== {unit}: {len(table)} kernels")
        for name in sorted(table):
            print(f"{name}\n    {fmt(table[name])}")
            if table[name]["scratch"] or table[name]["vgpr_spill"]:
                spills.append(name)
        if unit in later_old:
            same = later_new[unit][0] == later_old[unit][0]
            later_same = later_same and same
            print(f"later unit {unit}_gfx950.s  tree {later_new[unit][0]}  parent {later_old[unit][0]}  {'identical' if same else 'DIFFERENT'}")
        elif a.parent:
            print(f"later unit {unit}_gfx950.s  tree {later_new[unit][0]}  parent: not there")
    fields = {k: v for k, v in new["param_fields"][1].items() if "small_strain_field_kernel" in k}
    out = {"field_kernels": len(fields), "broken_bounds": broken_bounds(fields), "scratch_or_spilled_vgprs": spills}
    if old:
        out["assembly"] = {}
        for unit in UNITS:
            now, was = new[unit][0], old[unit][0]
            out["assembly"][unit + "_gfx950.s"] = {"sha256": now, "parent_sha256": was, "identical": now == was}
            print(f"{unit}_gfx950.s  tree {now}  parent {was}  {'identical' if now == was else 'DIFFERENT'}")
        if a.write_digests:
            digests = {k: v["parent_sha256"] for k, v in out["assembly"].items()}
            digests.update({u + "_gfx950.s": v[0] for u, v in later_old.items()})
            json.dump(digests, open(a.write_digests, "w"), indent=1)
    print(json.dumps(out))
    ok = len(fields) == 32 and not out["broken_bounds"] and not spills and all(v["identical"] for v in out.get("assembly", {}).values()) and later_same
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
