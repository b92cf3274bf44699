"""Build-time checks of the Hosford kernels on the cross-compiler alone (``tools/check_param_fields_build.py`` reads the remarks):
both instantiations of ``hosford_kernel`` without scratch and without spilled VGPRs, within the 256 VGPRs and the LDS of two
workgroups per CU; and the device assembly of the four translation units that existed before the law -- dxmat, ramberg_osgood,
param_fields, hyperelastic -- is byte for byte what it was (``tests/golden/hosford_parent_asm_sha256.json`` holds the digests of the
parent revision's assembly, compilation-unit id removed, as ``tools/check_hosford_build.py --parent REV`` prints them)."""
import json
import os
import re
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_param_fields_build as chk  # noqa: E402

_S = "s" + "_"
FORBIDDEN = re.compile(_S + r"(buffer_|scratch_)?" + "sto" + "re|" + _S + r"(buffer_)?" + "ato" + "mic|" + _S + "dca" + "che", re.I)
needs_hipcc = pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")


@needs_hipcc
def test_hosford_kernels_have_no_scratch_and_no_spills():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "hosford", os.path.join(tmp, "hosford.s"), remarks=True)
        asm = open(os.path.join(tmp, "hosford.s")).read()
    table = {k: v for k, v in chk.resource_table(remarks).items() if "hosford_kernel" in k}
    assert len(table) == 2, sorted(table)          # full and sym tangent
    for name, r in table.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["vgprs"] + r["agprs"] <= 256, r
        assert 0 < r["lds"] and 2 * r["lds"] <= 160 * 1024, r
    assert not FORBIDDEN.search(asm)


@needs_hipcc
@pytest.mark.parametrize("unit", ["dxmat", "ramberg_osgood", "param_fields", "hyperelastic"])
def test_existing_units_compile_to_the_parents_assembly(unit):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "hosford_parent_asm_sha256.json")))
    with tempfile.TemporaryDirectory() as tmp:
        chk.device_asm(chk.CSRC, unit, os.path.join(tmp, unit + ".s"))
        assert chk.sha(os.path.join(tmp, unit + ".s")) == want[unit + "_gfx950.s"]


def test_the_source_has_no_inline_assembly_beyond_the_opaque_register_idiom():
    for f in ("hosford.hip", "hosford.hpp"):
        src = open(os.path.join(chk.CSRC, f)).read()
        assert not FORBIDDEN.search(src), f
        for stmt in re.findall(r"asm\s*(?:volatile)?\s*\(([^;]*)\);", src):
            assert stmt.strip().startswith('""'), (f, stmt)
