"""Build-time checks of the axisymmetric gradient unit on the cross-compiler alone, from the compiler's resource remarks: exactly the
eight instantiations of ``axisym_gradient_kernel`` (four kinds, with and without the radius output) and nothing else in the unit,
without scratch and without spilled VGPRs, with the static LDS that ``axisym_gradient.hpp`` states (none); the unit in the Makefile;
``dxmat.hip`` names none of its kernels.  Nothing else in the assembly is looked at."""
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
def test_eight_instantiations_no_scratch_no_spilled_vgpr_and_the_stated_lds():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "axisym_gradient", os.path.join(tmp, "axisym_gradient.s"), remarks=True)
    table = chk.resource_table(remarks)
    assert all("axisym_gradient_kernel" in k for k in table), sorted(table)              # nothing else in the unit
    args = sorted(re.search(r"axisym_gradient_kernelILi(\d)ELb([01])E", k).groups() for k in table)
    assert args == [(str(kind), rad) for kind in range(4) for rad in "01"], sorted(table)
    hpp = open(os.path.join(chk.CSRC, "axisym_gradient.hpp")).read()
    lds = int(re.search(r"constexpr int AXISYM_GRAD_LDS_BYTES = (\d+);", hpp).group(1))
    for name, r in sorted(table.items()):
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds"] == lds == 0, r


def test_the_unit_is_built_into_the_library_and_dxmat_names_none_of_its_kernels():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\baxisym_gradient\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\baxisym_gradient\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o axisym_gradient_gfx950.s axisym_gradient.hip" in dry
    assert "axisym_gradient" in chk.AXISYM_UNITS
    hpp = open(os.path.join(chk.CSRC, "axisym_gradient.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 1                    # the one host entry point of the unit
    hip = open(os.path.join(chk.CSRC, "axisym_gradient.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.findall(r"\basm\b", code) and "__syncthreads" not in code and "__shared__" not in code and "atomic" not in code
    assert "__launch_bounds__(AXISYM_GRAD_BLOCK)" in code and "if (gid >= s.npts) return;" in code
    dx = open(os.path.join(chk.CSRC, "dxmat.hip")).read()
    assert "axisym_gradient_kernel" not in dx and "axisym_gradient_launch(" in dx and '#include "axisym_gradient.hpp"' in dx
