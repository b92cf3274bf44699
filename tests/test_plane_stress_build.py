"""Build-time checks of the plane-stress unit on the cross-compiler alone, from the compiler's resource remarks: exactly the three
instantiations of ``plane_stress_kernel`` (quadratic with the elastic / the algorithmic tangent, polygon) and nothing else in the
unit, without scratch and without spilled VGPRs, within 128 VGPRs, with the static LDS ``plane_stress.hpp`` states (at most twice the
heat-transfer kernels'); the unit in the Makefile and named by the tool; the header free of kernels."""
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
LDS_BYTES = 4 * (64 * 3 + 64 * 6) * 8 + 4 * 4 * 8
HEAT_LDS_BYTES = 16512      # tests/test_heat_transfer_build.py


@needs_hipcc
def test_three_instantiations_no_scratch_no_spilled_vgpr_and_the_stated_lds():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "plane_stress", os.path.join(tmp, "plane_stress.s"), remarks=True)
    table = chk.resource_table(remarks)
    assert all("plane_stress_kernel" in k for k in table), sorted(table)              # nothing else in the unit
    assert sorted(re.search(r"ILi(\d)ELi(\d)E", k).groups() for k in table) == [("0", "0"), ("0", "1"), ("1", "0")], sorted(table)
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["vgprs"] + r["agprs"] <= 128 and r["occupancy"] >= 4, r
        assert r["lds"] == LDS_BYTES == 18560 and r["lds"] <= 2 * HEAT_LDS_BYTES and 8 * r["lds"] <= 160 * 1024, r


def test_the_unit_is_built_into_the_library_and_named_by_the_tool():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bplane_stress\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bplane_stress\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o plane_stress_gfx950.s plane_stress.hip" in dry
    assert "plane_stress" in chk.LATER_UNITS and "plane_stress" not in chk.UNITS
    hpp = open(os.path.join(chk.CSRC, "plane_stress.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 3                    # every host entry point of the unit
    hip = chk.unit_text(chk.CSRC, "plane_stress.hip")                                 # with the tile I/O texts it includes
    assert "reinterpret_cast<const double2_t*>(g0)" in hip and "constexpr int NQ" in hip
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.findall(r"\basm\b", code)                                           # plain C++: no inline assembly at all
    assert "__syncthreads" not in code and "atomic" not in code.replace("__ATOMIC", "")
    assert "__launch_bounds__(BLOCK)" in code and "#pragma clang fp contract(off)" in code
    # dxmat.hip names no kernel of the new unit: its device module does not see it
    assert "plane_stress_kernel<" not in re.sub(r'"[^"]*"', "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
    # LawParams, an argument of every other kernel, is what it was
    common = open(os.path.join(chk.CSRC, "dxm_common.hpp")).read()
    assert re.search(r"struct LawParams \{[^}]*double c\[6\];[^}]*\};", common)
