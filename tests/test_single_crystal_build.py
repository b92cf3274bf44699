"""Build-time checks of the single-crystal kernels on the cross-compiler alone (``tools/check_param_fields_build.py`` reads the
remarks): the three frame instantiations of ``single_crystal_kernel`` without scratch and without spilled VGPRs, with the static LDS
DESIGN.md states, and resident twice per CU by LDS and by registers: workgroups of two waves, one wave per SIMD (the kernel needs
more than the 256 registers that two waves per SIMD would leave it)."""
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
WAVES = 2
# per wave the 64 x 36 staged tangent entries and the 4 x 14 hand-over words; per workgroup the table of the twelve systems (16 x 30),
# the stiffness (36) and the stats words
LDS_BYTES = WAVES * (64 * 36 + 4 * 14) * 8 + 16 * 30 * 8 + 36 * 8 + WAVES * 4 * 8


@needs_hipcc
def test_single_crystal_kernels_have_no_scratch_no_spills_and_the_documented_lds():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "single_crystal", os.path.join(tmp, "single_crystal.s"), remarks=True)
    table = {k: v for k, v in chk.resource_table(remarks).items() if "single_crystal_kernel" in k}
    assert sorted(re.search(r"ILi(\d)E", k).group(1) for k in table) == ["0", "1", "2"], sorted(table)     # none / uniform / field
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds"] == LDS_BYTES == 41952, r
        # two workgroups per CU: by LDS (160 KiB), and by registers -- 2 workgroups x 2 waves on 4 SIMDs is one wave per SIMD,
        # which has the whole 512-entry file
        assert 2 * r["lds"] <= 160 * 1024, r
        assert r["occupancy"] >= 1 and r["occupancy"] * 4 >= 2 * WAVES, r
        assert r["vgprs"] + r["agprs"] <= 512 // max(1, (2 * WAVES) // 4), r
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "41 952" in design or "41952" in design


def test_the_unit_is_built_into_the_library_and_keeps_to_the_opaque_register_idiom():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bsingle_crystal\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bsingle_crystal\.hpp\b", mk, flags=re.M)
    assert re.search(r"^HDRS := .*\bstage_full36_store\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o single_crystal_gfx950.s single_crystal.hip" in dry
    for f in ("single_crystal.hip", "single_crystal.hpp", "stage_full36_store.hpp"):
        src = open(os.path.join(chk.CSRC, f)).read()
        for stmt in re.findall(r"asm\s*(?:volatile)?\s*\(([^;]*)\);", src):
            assert stmt.strip().startswith('""'), (f, stmt)
        code = re.sub(r"//[^\n]*", "", src)   # comments may speak of it
        assert "s_barrier" not in code
    # dxmat.hip names no kernel of the new unit: its device assembly stays the parent's
    assert "single_crystal_kernel<" not in re.sub(r'"[^"]*"', "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
    # LawParams, an argument of every other kernel, is what it was
    common = open(os.path.join(chk.CSRC, "dxm_common.hpp")).read()
    assert re.search(r"struct LawParams \{[^}]*double c\[6\];[^}]*\};", common)
