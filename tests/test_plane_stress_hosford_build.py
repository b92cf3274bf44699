"""Build-time checks of the plane-stress Hosford unit on the cross-compiler alone, from the compiler's resource remarks: exactly the two
instantiations of ``plane_stress_hosford_kernel`` (tangent 0, 1) and nothing else in the unit, without scratch and without spilled
VGPRs, with the static LDS ``plane_stress_hosford.hpp`` states and the VGPR counts DESIGN.md records; one workgroup barrier per
kernel; the unit in the Makefile and named by the tool; the plane-stress unit it took its skeleton from untouched."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_device_asm as chk  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
# per wave the 64 x 3 strain / stress staging and the 64 x 6 tangent records; per workgroup the stats words
LDS_BYTES = 4 * 64 * (3 + 6) * 8 + 4 * 4 * 8
VGPRS = {"0": 202, "1": 247}      # tangent 0, 1: what DESIGN.md records


@needs_hipcc
def test_two_instantiations_no_scratch_no_spilled_vgpr_the_stated_lds_and_one_barrier_each():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "plane_stress_hosford.s")
        remarks = chk.device_asm(chk.CSRC, "plane_stress_hosford", out, remarks=True)
        asm = open(out).read()
    table = chk.resource_table(remarks)
    assert all("plane_stress_hosford_kernel" in k for k in table), sorted(table)              # nothing else in the unit
    assert sorted(re.search(r"plane_stress_hosford_kernelILi(\d)E", k).group(1) for k in table) == ["0", "1"], sorted(table)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### Plane-stress Hosford plasticity"):]
    section = section[:section.index("\n### ", 10)]
    for name, r in table.items():
        print(name, r)
        tangent = re.search(r"plane_stress_hosford_kernelILi(\d)E", name).group(1)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["vgprs"] + r["agprs"] == VGPRS[tangent] and r["occupancy"] == 2, r
        assert f"{VGPRS[tangent]}" in section
        assert r["lds"] == LDS_BYTES == 18560 and 8 * r["lds"] <= 160 * 1024, r
    assert "18 560" in section
    # the tile loop orders its LDS traffic within a wave: the one workgroup barrier of a kernel is store_block_stats', after the loop
    assert len(re.findall(r"^\s*s_barrier\b", asm, flags=re.M)) == len(table)
    assert "scratch_" not in asm


def test_the_unit_is_built_into_the_library_and_named_by_the_tool():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bplane_stress_hosford\.hip\b", mk, flags=re.M)
    assert re.search(r"^HDRS := .*\bplane_stress_hosford\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o plane_stress_hosford_gfx950.s plane_stress_hosford.hip" in dry
    assert "plane_stress_hosford" in chk.LATER_UNITS and "plane_stress_hosford" not in chk.UNITS
    hpp = open(os.path.join(chk.CSRC, "plane_stress_hosford.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 2                    # every host entry point of the unit
    assert "PSH_LDS_BYTES == 18560" in hpp and "static_assert" in hpp
    hip = chk.unit_text(chk.CSRC, "plane_stress_hosford.hip")                         # with the tile I/O texts it includes
    assert "reinterpret_cast<const double2_t*>(g0)" in hip and "constexpr int NQ" in hip
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.findall(r"\basm\b", code)            # no inline assembly
    assert "__syncthreads" not in code and "s_barrier" not in code and "atomic" not in code.replace("__ATOMIC", "")
    assert "__launch_bounds__(BLOCK)" in code and "#pragma clang fp contract(off)" in code and "wave_lds_sync();" in code
    assert "store_block_stats(stats," in code and "stream_store<0>" in code           # non-temporal stress and tangent stores
    assert len(re.findall(r"plane_stress_hosford_kernel<[01]>", code)) == 3           # the resources' kernel and the two launches
    # the plane-stress unit it took its skeleton from is not touched: a unit of its own, not a third SURFACE
    ps = open(os.path.join(chk.CSRC, "plane_stress.hip")).read()
    assert "PS_QUADRATIC || TANGENT == 0" in ps and "osford" not in ps
