"""Build-time checks of the finite-strain single-crystal kernels on the cross-compiler alone (``tools/check_param_fields_build.py``
reads the remarks): the three frame instantiations of ``fs_single_crystal_kernel`` without scratch and without spilled VGPRs, with the
static LDS DESIGN.md states, and resident twice per CU by LDS and by registers: workgroups of two waves, one wave per SIMD, as for
law 14 (the kernel needs more than the 256 registers that two waves per SIMD would leave it)."""
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
# per wave: the out-tile of a tangent round (16 x 81, padded to the 1408 doubles the copy-out reads), the F / PK1 staging (64 x 9),
# 19 parked doubles per point, 4 x 21 exchanged 3x3 tensors, 16 x 16 hand-over words; per workgroup the table of the twelve systems
# (16 x 21) and the stats words
LDS_BYTES = WAVES * (1408 + 64 * 9 + 64 * 19 + 4 * 21 * 9 + 16 * 16) * 8 + 16 * 21 * 8 + WAVES * 4 * 8


@needs_hipcc
def test_fs_single_crystal_kernels_have_no_scratch_no_spills_and_the_documented_lds():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "fs_single_crystal", os.path.join(tmp, "fs_single_crystal.s"), remarks=True)
    table = {k: v for k, v in chk.resource_table(remarks).items() if "fs_single_crystal_kernel" in k}
    assert sorted(re.search(r"ILi(\d)E", k).group(1) for k in table) == ["0", "1", "2"], sorted(table)     # none / uniform / field
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds"] == LDS_BYTES == 70144, r
        # two workgroups per CU: by LDS (160 KiB), and by registers -- 2 workgroups x 2 waves on 4 SIMDs is one wave per SIMD,
        # which has the whole 512-entry file
        assert 2 * r["lds"] <= 160 * 1024, r
        assert r["occupancy"] >= 1 and r["occupancy"] * 4 >= 2 * WAVES, r
        assert r["vgprs"] + r["agprs"] <= 512 // max(1, (2 * WAVES) // 4), r
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "70 144" in design or "70144" in design


def test_the_unit_is_built_into_the_library_and_keeps_to_the_opaque_register_idiom():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bfs_single_crystal\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bfs_single_crystal\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o fs_single_crystal_gfx950.s fs_single_crystal.hip" in dry
    assert "fs_single_crystal" in chk.LATER_UNITS
    for f in ("fs_single_crystal.hip", "fs_single_crystal.hpp"):
        src = open(os.path.join(chk.CSRC, f)).read()
        for stmt in re.findall(r"asm\s*(?:volatile)?\s*\(([^;]*)\);", src):
            assert stmt.strip().startswith('""'), (f, stmt)
        code = re.sub(r"//[^\n]*", "", src)   # comments may speak of it
        assert "s_barrier" not in code
    # the tile I/O is the shared text, not a copy of it
    src = open(os.path.join(chk.CSRC, "fs_single_crystal.hip")).read()
    for frag in ("tile_rows9_load.hpp", "tile_rows9_take.hpp", "tile_rows9_put.hpp", "tile_rows9_store.hpp", "tile_out81_copyout.hpp"):
        assert f'#include "{frag}"' in src, frag
    # LawParams, an argument of every other kernel, is what it was
    common = open(os.path.join(chk.CSRC, "dxm_common.hpp")).read()
    assert re.search(r"struct LawParams \{[^}]*double c\[6\];[^}]*\};", common)
