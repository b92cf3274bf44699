"""Build-time checks of the heat-transfer unit on the cross-compiler alone: the four instantiations of ``heat_transfer_kernel`` (two laws
x uniform temperature / temperature stream) without scratch and without spilled VGPRs, with the static LDS ``heat_transfer.hpp``
states; and the device assembly of every unit that existed before -- dxmat, small_strain_clean, ramberg_osgood, param_fields,
hyperelastic, hosford, orthotropic, single_crystal -- byte for byte what it was (``tests/golden/heat_transfer_parent_asm_sha256.json`` holds
the digests of the parent commit's sources, made with ``tools/check_device_asm.py --parent <rev> --all-units --write-digests``)."""
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
# per wave the 64 x 3 gradient / flux staging and the 64 x 5 tangent records; per workgroup the stats words
LDS_BYTES = 4 * (64 * 3 + 64 * 5) * 8 + 4 * 4 * 8
EARLIER = ("dxmat", "small_strain_clean", "ramberg_osgood", "param_fields", "hyperelastic", "hosford", "orthotropic", "single_crystal")


@needs_hipcc
def test_heat_transfer_kernels_have_no_scratch_no_spilled_vgpr_and_the_stated_lds():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "heat_transfer", os.path.join(tmp, "heat_transfer.s"), remarks=True)
    table = {k: v for k, v in chk.resource_table(remarks).items() if "heat_transfer_kernel" in k}
    assert sorted(re.search(r"ILi(\d)ELi(\d)E", k).groups() for k in table) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(table)
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds"] == LDS_BYTES == 16512, r
        # 256-thread workgroups: eight per CU by LDS (160 KiB), at least four waves per SIMD by registers
        assert 8 * r["lds"] <= 160 * 1024 and r["occupancy"] >= 4 and r["vgprs"] + r["agprs"] <= 128, r


@needs_hipcc
def test_every_earlier_unit_compiles_to_the_parents_assembly():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "heat_transfer_parent_asm_sha256.json")))
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
    assert re.search(r"^SRCS := .*\bheat_transfer\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bheat_transfer\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o heat_transfer_gfx950.s heat_transfer.hip" in dry
    assert "heat_transfer" in chk.LATER_UNITS and "heat_transfer" not in chk.UNITS
    hpp = open(os.path.join(chk.CSRC, "heat_transfer.hpp")).read()
    assert hpp.count('__attribute__((visibility("hidden")))') == 3      # every host entry point of the unit
    for f in ("heat_transfer.hip", "heat_transfer.hpp"):
        src = chk.unit_text(chk.CSRC, f)                                            # with the tile I/O texts it includes
        assert f.endswith(".hpp") or ("reinterpret_cast<const double2_t*>(g0)" in src and "constexpr int NQ" in src)
        assert not re.findall(r"\basm\b", re.sub(r"//[^\n]*", "", src)), f          # plain C++: no inline assembly at all
        code = re.sub(r"//[^\n]*", "", src)
        assert "__syncthreads" not in code and "atomic" not in code.replace("__ATOMIC", "")
    # dxmat.hip names no kernel of the new unit: its device assembly stays the parent's
    assert "heat_transfer_kernel<" not in re.sub(r'"[^"]*"', "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
    # LawParams, an argument of every other kernel, is what it was
    common = open(os.path.join(chk.CSRC, "dxm_common.hpp")).read()
    assert re.search(r"struct LawParams \{[^}]*double c\[6\];[^}]*\};", common)
