"""Build-time checks of the plane-strain unit on the cross-compiler alone, from the compiler's resource remarks: exactly the three
instantiations of ``plane_strain_kernel`` and nothing else in the unit, without scratch and without spilled VGPRs, with the static
LDS that ``plane_strain.hpp`` and DESIGN.md state; the unit in the Makefile and named by the tool; the source free of inline
assembly (but for the shared opaque-register idiom it calls) and of workgroup barriers."""
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
# per wave the 64 x 4 strain / stress staging and the 64 x 7 tangent records (c1, c2, c3, n0..n3); per workgroup the stats words
LDS_BYTES = 4 * 64 * (4 + 7) * 8 + 4 * 4 * 8


@needs_hipcc
def test_three_instantiations_no_scratch_no_spilled_vgpr_and_the_stated_lds():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "plane_strain.s")
        remarks = chk.device_asm(chk.CSRC, "plane_strain", out, remarks=True)
        asm = open(out).read()
    table = chk.resource_table(remarks)
    assert all("plane_strain_kernel" in k for k in table), sorted(table)              # nothing else in the unit
    assert sorted(re.search(r"plane_strain_kernelILi(\d)E", k).group(1) for k in table) == ["0", "1", "2"], sorted(table)
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["vgprs"] + r["agprs"] <= 128 and r["occupancy"] >= 4, r
        assert r["lds"] == LDS_BYTES == 22656 and 7 * r["lds"] <= 160 * 1024, r
    # the tile loop orders its LDS traffic within a wave: the one workgroup barrier of a kernel is store_block_stats', after the loop
    assert len(re.findall(r"^\s*s_barrier\b", asm, flags=re.M)) == len(table)
    assert "scratch_" not in asm
    # the only inline assembly is the empty opaque-register idiom of DXM_MUL (the Voce law): every block is empty
    blocks = re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", asm, flags=re.S)
    assert blocks and all(b.strip() == "" for b in blocks), [b for b in blocks if b.strip()][:3]


def test_the_unit_is_built_into_the_library_and_named_by_the_tool():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bplane_strain\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bplane_strain\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o plane_strain_gfx950.s plane_strain.hip" in dry
    assert "plane_strain" in chk.LATER_UNITS and "plane_strain" not in chk.UNITS
    import check_param_fields_build as by_its_other_name

    assert "plane_strain" in by_its_other_name.LATER_UNITS
    hpp = open(os.path.join(chk.CSRC, "plane_strain.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 4                    # every host entry point of the unit
    assert "PE_LDS_BYTES == 22656" in hpp and "static_assert" in hpp
    hip = open(os.path.join(chk.CSRC, "plane_strain.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.findall(r"\basm\b", code)            # no inline assembly of its own: only dxm_common.hpp's opaque(), through DXM_MUL
    common = open(os.path.join(chk.CSRC, "dxm_common.hpp")).read()
    assert 'asm("" : "+v"(x));' in common and "hardening_R<LAW>" in code
    assert "__syncthreads" not in code and "s_barrier" not in code and "atomic" not in code.replace("__ATOMIC", "")
    assert "__launch_bounds__(BLOCK)" in code and "#pragma clang fp contract(off)" in code and "wave_lds_sync();" in code
    assert "store_block_stats(stats," in code and "stream_store<0>" in code           # non-temporal stress and tangent stores
    # dxmat.hip names no kernel of the new unit: its device module does not see it
    dx = open(os.path.join(chk.CSRC, "dxmat.hip")).read()
    assert "plane_strain_kernel<" not in re.sub(r'"[^"]*"', "", dx)
    assert re.search(r"struct LawParams \{[^}]*double c\[6\];[^}]*\};", common)      # an argument of every other kernel: what it was
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "22 656" in design or "22656" in design
