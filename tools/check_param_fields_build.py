#!/usr/bin/env python3
"""Two build-time checks of the kernels with per-point parameter fields (csrc/param_fields.hip), on the cross-compiler alone:

1. every kernel of the new translation unit stays within the resources of the uniform J2 kernels: no scratch, no spilled
   VGPRs, at most 128 VGPRs (four waves per SIMD), the same static LDS -- read from -Rpass-analysis=kernel-resource-usage;
2. (--parent REV) the device assembly of the two existing translation units, dxmat.hip and ramberg_osgood.hip, is byte for byte
   what the sources of git revision REV give (but for the compilation-unit id, which hashes the source file's path).

    python tools/check_param_fields_build.py [--parent HEAD~1]

Prints one line per kernel and a JSON summary; exit status 1 if a bound is broken or an assembly file differs."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dolfinx_materials_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-S", "--cuda-device-only"]
MAX_VGPRS = 128
J2_STATIC_LDS = 30848     # small_strain.hpp: 4 waves x (64 x 6 + 64 x 9) doubles + the 4 x 4 status words


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="git revision whose dxmat.hip / ramberg_osgood.hip assembly must be reproduced")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        table = field_kernel_table(tmp)
        for name in sorted(table, key=template_args):
            law, tl, grad = template_args(name)
            r = table[name]
            print(f"LAW={law} TL={tl} GRAD={grad}  VGPRs {r['vgprs']:3d}  AGPRs {r['agprs']}  scratch {r['scratch']}  spilled VGPRs {r['vgpr_spill']}  "
                  f"LDS {r['lds']}  waves/SIMD by registers {r['occupancy']}")
        out["field_kernels"] = len(table)
        out["broken_bounds"] = broken_bounds(table)
        if a.parent:
            old = os.path.join(tmp, "parent")
            os.makedirs(old)
            tar = subprocess.run(["git", "archive", a.parent, "dolfinx_materials_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", old], input=tar.stdout, check=True)
            out["assembly"] = {}
            for unit in ("dxmat", "ramberg_osgood"):
                device_asm(CSRC, unit, os.path.join(tmp, unit + ".s"))
                device_asm(os.path.join(old, "dolfinx_materials_amd", "csrc"), unit, os.path.join(tmp, unit + "_parent.s"))
                now, was = sha(os.path.join(tmp, unit + ".s")), sha(os.path.join(tmp, unit + "_parent.s"))
                out["assembly"][unit + "_gfx950.s"] = {"sha256": now, "parent_sha256": was, "identical": now == was}
    print(json.dumps(out))
    ok = len(table) == 32 and not out["broken_bounds"] and all(v["identical"] for v in out.get("assembly", {}).values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
