"""Build-time checks of the orthotropic kernels on the cross-compiler alone (``tools/check_param_fields_build.py`` reads the remarks):
every instantiation of ``orthotropic_kernel`` -- three frame states x two tangent layouts -- without scratch and without spilled
VGPRs, within the registers of its ``__launch_bounds__(256, 2)`` (two waves per SIMD: 256), and with the static LDS DESIGN.md states."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_param_fields_build as chk  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
LDS_BYTES = 4 * (64 * 21 + 64 * 6) * 8 + 4 * 4 * 8     # per wave the staged upper triangles and the strain / stress staging; the stats words


@needs_hipcc
def test_orthotropic_kernels_have_no_scratch_no_spills_and_the_documented_lds():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "orthotropic", os.path.join(tmp, "orthotropic.s"), remarks=True)
    table = {k: v for k, v in chk.resource_table(remarks).items() if "orthotropic_kernel" in k}
    assert len(table) == 6, sorted(table)          # none / uniform / field x full / sym
    assert sorted(re.search(r"ILi(\d)ELi(\d)E", k).groups() for k in table) == [(str(f), str(s)) for f in range(3) for s in range(2)]
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["vgprs"] + r["agprs"] <= 256, r
        assert r["lds"] == LDS_BYTES == 55424 and 2 * r["lds"] <= 160 * 1024, r
        assert r["occupancy"] >= 2, r              # the Hosford kernel's residency
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "55 424" in design or "55424" in design


def test_the_unit_is_built_into_the_library_and_keeps_to_the_opaque_register_idiom():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\borthotropic\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\borthotropic\.hpp\b", mk, flags=re.M)
    # the asm target is one pattern over SRCS: what it would run for this unit
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o orthotropic_gfx950.s orthotropic.hip" in dry
    for f in ("orthotropic.hip", "orthotropic.hpp"):
        src = open(os.path.join(chk.CSRC, f)).read()
        for stmt in re.findall(r"asm\s*(?:volatile)?\s*\(([^;]*)\);", src):
            assert stmt.strip().startswith('""'), (f, stmt)
    # dxmat.hip names no kernel of the new unit: its device assembly stays the parent's
    assert "orthotropic_kernel<" not in re.sub(r'"[^"]*"', "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
