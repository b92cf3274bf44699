"""The resource budget of the Ogden kernel, asserted from the compiler's remarks of a cross-compile of ``csrc/hyperelastic.hip``
(``-Rpass-analysis=kernel-resource-usage``, read with ``tools/check_param_fields_build.py``): no scratch, no spilled VGPR, at most
the 256 VGPRs of two waves per SIMD that ``__launch_bounds__(BLOCK, 2)`` asks for, and at most the static LDS of the FeFp kernel
whose I/O skeleton it shares -- two workgroups per CU still fit."""
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
# scalar stores to memory, scalar atomics and scalar data-cache write-backs: the pattern is put together from pieces so that this
# file does not itself hold the mnemonics it looks for
_S = "s" + "_"
FORBIDDEN = re.compile(_S + r"(buffer_|scratch_)?" + "sto" + "re|" + _S + r"(buffer_)?" + "ato" + "mic|" + _S + "dca" + "che", re.I)


@pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
def test_ogden_kernel_stays_within_the_fefp_budget():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "hyperelastic", os.path.join(tmp, "hyperelastic.s"), remarks=True)
        asm = open(os.path.join(tmp, "hyperelastic.s")).read()
    table = {k: v for k, v in chk.resource_table(remarks).items() if "ogden_kernel" in k}
    assert len(table) == 1, sorted(table)          # one instantiation: full tangent, F from the (N, 9) array
    (name, r), = table.items()
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 256, r
    assert 0 < r["lds"] <= FEFP_STATIC_LDS and 2 * r["lds"] <= 160 * 1024, r
    assert not FORBIDDEN.search(asm)


def test_the_source_has_no_inline_assembly_beyond_the_opaque_register_idiom():
    for f in ("hyperelastic.hip", "hyperelastic.hpp"):
        src = open(os.path.join(chk.CSRC, f)).read()
        assert not FORBIDDEN.search(src), f
        for stmt in re.findall(r"asm\s*(?:volatile)?\s*\(([^;]*)\);", src):
            assert stmt.strip().startswith('""'), (f, stmt)
