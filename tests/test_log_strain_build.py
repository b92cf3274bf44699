"""The resource budget of the logarithmic-strain plasticity kernel, asserted from the compiler's remarks of a cross-compile of
``csrc/log_strain.hip`` (``-Rpass-analysis=kernel-resource-usage``, read with ``tools/check_param_fields_build.py``): one
instantiation, no scratch, no spilled VGPR, at most the 256 registers of two waves per SIMD that ``__launch_bounds__(BLOCK, 2)`` asks
for, and at most the static LDS of the FeFp kernel whose I/O skeleton it shares -- two workgroups per CU fit, as for Ogden."""
import os
import re
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_param_fields_build as chk  # noqa: E402

FEFP_STATIC_LDS = 4 * 2464 * 8     # fefp.hpp: F2_LDS_PER_WAVE doubles for each of the 4 waves


@pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
def test_log_strain_kernel_stays_within_the_ogden_budget():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "log_strain", os.path.join(tmp, "log_strain.s"), remarks=True)
    table = {k: v for k, v in chk.resource_table(remarks).items() if "log_strain_kernel" in k}
    assert len(table) == 1, sorted(table)          # one instantiation: full tangent, F from the (N, 9) array
    assert len(chk.resource_table(remarks)) == 1   # and nothing else in the unit
    (name, r), = table.items()
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 256, r
    assert 0 < r["lds"] <= FEFP_STATIC_LDS and 2 * r["lds"] <= 160 * 1024, r


def test_the_source_has_no_inline_assembly_beyond_the_opaque_register_idiom():
    for f in ("log_strain.hip", "log_strain.hpp"):
        src = open(os.path.join(chk.CSRC, f)).read()
        stmts = re.findall(r"\basm\b\s*(?:volatile)?\s*\(([^;]*)\);", src)
        assert len(stmts) == src.count("asm"), f       # every mention is a statement this test has looked at
        for stmt in stmts:
            assert stmt.strip().startswith('""'), (f, stmt)


def test_the_unit_is_built_into_the_library_and_is_stock_only():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS := (.*)$", mk, re.M).group(1).split()
    assert "log_strain.hip" in srcs and "log_strain.hpp" in hdrs
    host = open(os.path.join(chk.CSRC, "dxmat.hip")).read()
    assert "DXM_STOCK_ONLY(log_strain_kernel_fn)" in host and "DXM_STOCK_ONLY(launch_log_strain)" in host
    # the device module of dxmat.hip does not see the law: the header declares host functions only
    assert "__global__" not in open(os.path.join(chk.CSRC, "log_strain.hpp")).read()
