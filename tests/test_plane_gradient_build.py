"""Build-time checks of the plane gradient unit on the cross-compiler alone, from the compiler's resource remarks: exactly the four
instantiations of ``plane_gradient_kernel`` and nothing else in the unit, without scratch and without spilled VGPRs, with the static
LDS that ``plane_gradient.hpp`` states (none); the unit in the Makefile and named by the tool."""
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


@needs_hipcc
def test_four_instantiations_no_scratch_no_spilled_vgpr_and_the_stated_lds():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "plane_gradient.s")
        remarks = chk.device_asm(chk.CSRC, "plane_gradient", out, remarks=True)
        asm = open(out).read()
    table = chk.resource_table(remarks)
    assert all("plane_gradient_kernel" in k for k in table), sorted(table)              # nothing else in the unit
    assert sorted(re.search(r"plane_gradient_kernelILi(\d)E", k).group(1) for k in table) == ["0", "1", "2", "3"], sorted(table)
    hpp = open(os.path.join(chk.CSRC, "plane_gradient.hpp")).read()
    lds = int(re.search(r"constexpr int PLANE_GRAD_LDS_BYTES = (\d+);", hpp).group(1))
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["vgprs"] + r["agprs"] <= 64 and r["occupancy"] == 8, r          # a streaming kernel: nothing may cost it residency
        assert r["lds"] == lds == 0, r
    assert "scratch_" not in asm and not re.findall(r"^\s*s_barrier\b", asm, flags=re.M) and ";;#ASMSTART" not in asm
    # the output rows: 16 B stores for the 48 B and 32 B rows, 8 B stores for the 24 B rows (plane_gradient.hpp)
    body = {k: asm[asm.index(k + ":"):asm.index(".Lfunc_end", asm.index(k + ":"))] for k in table}
    for k, text in body.items():
        kind = int(re.search(r"ILi(\d)E", k).group(1))
        wide, narrow = len(re.findall(r"global_store_dwordx4", text)), len(re.findall(r"global_store_dwordx2", text))
        if kind == 0:
            assert wide == 3 and narrow == 0, (k, wide, narrow)
        elif kind == 2:
            assert wide == 2 and narrow == 0, (k, wide, narrow)
        elif kind == 3:
            assert 16 * wide + 8 * narrow == 24 and narrow >= 1, (k, wide, narrow)


def test_the_unit_is_built_into_the_library_and_named_by_the_tool():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bplane_gradient\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bplane_gradient\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o plane_gradient_gfx950.s plane_gradient.hip" in dry
    assert "plane_gradient" in chk.LATER_UNITS and "plane_gradient" not in chk.UNITS
    hpp = open(os.path.join(chk.CSRC, "plane_gradient.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 1                    # the one host entry point of the unit
    assert "UNMEASURED" in hpp and "OPEN" in hpp                                      # the output-row choice and its open item
    hip = open(os.path.join(chk.CSRC, "plane_gradient.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.findall(r"\basm\b", code) and "__syncthreads" not in code and "__shared__" not in code and "atomic" not in code
    assert "__launch_bounds__(PLANE_GRAD_BLOCK)" in code and "if (gid >= s.npts) return;" in code
    dx = open(os.path.join(chk.CSRC, "dxmat.hip")).read()
    assert "plane_gradient_kernel" not in dx and "plane_gradient_launch(" in dx
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "plane_gradient.hip" in design and "profiles/r24_plane_gradient.md" in design
