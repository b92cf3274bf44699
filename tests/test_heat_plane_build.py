"""Build-time checks of the two-dimensional heat-transfer unit on the cross-compiler alone: the four instantiations of
``heat_plane_kernel`` (two laws x gradient array / nodal temperature) and ``scalar_gradient_kernel``, nothing else in the unit, without
scratch and without spilled VGPRs, with the static LDS ``heat_plane.hpp`` states and at least the occupancy asserted for
``heat_transfer_kernel``; and the device assembly of every unit that existed before, byte for byte what it was
(``tests/golden/heat_plane_parent_asm_sha256.json`` holds the digests of the parent commit's sources, made with
``tools/check_device_asm.py --parent <rev> --all-units --write-digests``)."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_device_asm as chk  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
# per wave the 64 x 4 tangent records; per workgroup the stats words
LDS_BYTES = 4 * (64 * 4) * 8 + 4 * 4 * 8
EARLIER = tuple(u for u in chk.UNITS + chk.LATER_UNITS if u != "heat_plane")


@needs_hipcc
def test_kernels_have_no_scratch_no_spilled_vgpr_the_stated_lds_and_the_occupancy_of_the_three_wide_kernels():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "heat_plane.s")
        remarks = chk.device_asm(chk.CSRC, "heat_plane", out, remarks=True)
        asm = open(out).read()
    table = chk.resource_table(remarks)
    assert all("heat_plane_kernel" in k or "scalar_gradient_kernel" in k for k in table), sorted(table)      # nothing else in the unit
    law = {k: v for k, v in table.items() if "heat_plane_kernel" in k}
    assert sorted(re.search(r"ILi(\d)ELi(\d)E", k).groups() for k in law) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(law)
    (grad,) = [v for k, v in table.items() if "scalar_gradient_kernel" in k]
    hpp = open(os.path.join(chk.CSRC, "heat_plane.hpp")).read()
    assert "constexpr int HP_REC = 4;" in hpp and "constexpr int SCALAR_GRAD_LDS_BYTES = 0;" in hpp
    assert "HP_LDS_BYTES = WAVES_PER_BLOCK * HP_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;" in hpp
    for name, r in law.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds"] == LDS_BYTES == 8320, r
        # what test_heat_transfer_build.py asserts for heat_transfer_kernel: eight workgroups per CU by LDS, four waves per SIMD by registers
        assert 8 * r["lds"] <= 160 * 1024 and r["occupancy"] >= 4 and r["vgprs"] + r["agprs"] <= 128, r
    print("scalar_gradient_kernel", grad)
    assert grad["scratch"] == 0 and grad["vgpr_spill"] == 0 and grad["sgpr_spill"] == 0 and grad["lds"] == 0, grad
    assert grad["vgprs"] + grad["agprs"] <= 64 and grad["occupancy"] == 8, grad
    assert "scratch_" not in asm and ";;#ASMSTART" not in asm
    # the rows: one 16 B load and one 16 B store per lane in the array form, no gradient load at all in the nodal form's tile loop
    body = {k: asm[asm.index(k + ":"):asm.index(".Lfunc_end", asm.index(k + ":"))] for k in table}
    for k, text in body.items():
        assert len(re.findall(r"global_store_dwordx4", text)) >= 1, k
        assert not re.findall(r"global_atomic|flat_atomic|ds_.*_rtn", text), k


@needs_hipcc
def test_every_earlier_unit_compiles_to_the_parents_assembly():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "heat_plane_parent_asm_sha256.json")))
    assert sorted(want) == sorted(u + "_gfx950.s" for u in EARLIER)
    with tempfile.TemporaryDirectory() as tmp:
        def one(unit):
            out = os.path.join(tmp, unit + ".s")
            chk.device_asm(chk.CSRC, unit, out)
            return unit, chk.sha(out)
        with ThreadPoolExecutor(max_workers=4) as pool:
            got = dict(pool.map(one, EARLIER))
    for unit in EARLIER:
        assert got[unit] == want[unit + "_gfx950.s"], unit


def test_the_unit_is_built_into_the_library_and_named_by_the_tool():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bheat_plane\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bheat_plane\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o heat_plane_gfx950.s heat_plane.hip" in dry
    assert "heat_plane" in chk.LATER_UNITS and "heat_plane" not in chk.UNITS
    hpp = open(os.path.join(chk.CSRC, "heat_plane.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 4                    # every host entry point of the unit
    src = chk.unit_text(chk.CSRC, "heat_plane.hip")                                   # with the tile I/O text it includes
    code = re.sub(r"//[^\n]*", "", src)
    assert "constexpr int NQ" in code                                                  # tile_entries_store.hpp, unchanged
    assert not re.findall(r"\basm\b", code) and "atomic" not in code.replace("__ATOMIC", "") and "__syncthreads" not in code
    hip = re.sub(r"//[^\n]*", "", open(os.path.join(chk.CSRC, "heat_plane.hip")).read())
    assert hip.count("#pragma clang fp contract(off)") == 2                            # the point evaluation and the law
    assert hip.count("scalar_point(") == 3                                              # ONE text: defined once, run by both kernels
    assert "static_assert(HP_LDS_BYTES == sizeof(lds_all) + sizeof(red)" in hip
    # the 3-wide unit is what it was: four instantiations, three hidden entry points (test_heat_transfer_build.py)
    ht = open(os.path.join(chk.CSRC, "heat_transfer.hip")).read()
    assert "heat_plane" not in ht
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "heat_plane.hip" in design and "profiles/r25_heat_plane.md" in design
