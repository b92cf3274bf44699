#!/usr/bin/env python3
"""Build-time check for the Hosford translation unit (csrc/hosford.hip), on the cross-compiler alone: the resources of its kernels,
and (--parent REV) that the device assembly of the units that existed before it -- dxmat, ramberg_osgood, param_fields,
hyperelastic -- is byte for byte what the sources of git revision REV give (but for the compilation-unit id).

    python tools/check_hosford_build.py [--parent HEAD~1] [--write-digests tests/golden/hosford_parent_asm_sha256.json]

Prints a JSON summary; exit status 1 if a kernel spills or an assembly file differs."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import check_param_fields_build as chk

UNITS = ("dxmat", "ramberg_osgood", "param_fields", "hyperelastic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--write-digests", default=None, help="write the parent's digests to this JSON file")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "hosford", os.path.join(tmp, "hosford.s"), remarks=True)
        out["kernels"] = {k: v for k, v in chk.resource_table(remarks).items() if "hosford_kernel" in k}
        if a.parent:
            old = os.path.join(tmp, "parent")
            os.makedirs(old)
            tar = subprocess.run(["git", "archive", a.parent, "dolfinx_materials_amd/csrc", "include"], cwd=chk.ROOT, capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", old], input=tar.stdout, check=True)
            out["assembly"] = {}
            for unit in UNITS:
                chk.device_asm(chk.CSRC, unit, os.path.join(tmp, unit + ".s"))
                chk.device_asm(os.path.join(old, "dolfinx_materials_amd", "csrc"), unit, os.path.join(tmp, unit + "_parent.s"))
                now, was = chk.sha(os.path.join(tmp, unit + ".s")), chk.sha(os.path.join(tmp, unit + "_parent.s"))
                out["assembly"][unit + "_gfx950.s"] = {"sha256": now, "parent_sha256": was, "identical": now == was}
            if a.write_digests:
                json.dump({k: v["parent_sha256"] for k, v in out["assembly"].items()}, open(a.write_digests, "w"), indent=1)
    print(json.dumps(out, indent=1))
    bad = [k for k, r in out["kernels"].items() if r["scratch"] or r["vgpr_spill"]]
    return 0 if not bad and all(v["identical"] for v in out.get("assembly", {}).values()) else 1


if __name__ == "__main__":
    sys.exit(main())
