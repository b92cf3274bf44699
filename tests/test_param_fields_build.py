"""The resource bounds of the kernels with per-point parameter fields, asserted from the compiler's remarks of a cross-compile of
``csrc/param_fields.hip`` (``tools/check_param_fields_build.py``): every instantiation -- two laws, four tangent layouts, four
gradient sources -- has no scratch, no spilled VGPR, at most 128 VGPRs (four waves per SIMD, what ``__launch_bounds__(BLOCK, 4)``
asks for) and the static LDS of the uniform J2 kernels."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_param_fields_build as chk  # noqa: E402


@pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
def test_every_field_kernel_keeps_the_resources_of_the_uniform_j2_kernels():
    with tempfile.TemporaryDirectory() as tmp:
        table = chk.field_kernel_table(tmp)
    assert sorted(chk.template_args(k) for k in table) == [(law, tl, g) for law in (1, 2) for tl in range(4) for g in range(4)]
    for name, r in table.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 128, (name, r)
        assert r["lds"] == chk.J2_STATIC_LDS, (name, r)
    assert chk.broken_bounds(table) == []
