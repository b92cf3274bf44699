"""Build-time checks of the clean-tile unit (``csrc/small_strain_clean.hip``) on the cross-compiler alone: its eight kernels (two
J2 laws x four tangent layouts) within the bounds of the plain J2 kernels -- at most 128 VGPRs, no scratch, no spilled VGPR, the same
30 848 B of static LDS -- and the six translation units that existed before it compile to the device assembly of the parent
revision (``tools/check_device_asm.py --parent`` computes both sides; the shared tile body only gained ``if constexpr (CLEAN)``
blocks)."""
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
def test_clean_kernels_meet_the_resource_bounds_of_the_plain_j2_kernels():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, "small_strain_clean", os.path.join(tmp, "small_strain_clean.s"), remarks=True)
    table = {k: v for k, v in chk.resource_table(remarks).items() if "small_strain_clean_kernel" in k}
    args = sorted(tuple(int(x) for x in re.search(r"small_strain_clean_kernelILi(\d)ELi(\d)ELi(\d)E", k).groups()) for k in table)
    assert args == [(law, tl, 0) for law in (1, 2) for tl in (0, 1, 2, 3)], args
    for name, r in table.items():
        print(name, r)
    assert chk.broken_bounds(table) == []     # <= 128 VGPRs (+ AGPRs), no scratch, no spilled VGPR, LDS == 30848
    assert chk.MAX_VGPRS == 128 and chk.J2_STATIC_LDS == 30848


def _parent_revision():
    """The revision the existing units are compared with: the last commit that does not contain the clean-tile unit."""
    def git(*a):
        return subprocess.run(["git", *a], cwd=ROOT, capture_output=True, text=True)
    if git("rev-parse", "--git-dir").returncode != 0:
        return None
    unit = "dolfinx_materials_amd/csrc/small_strain_clean.hip"
    if git("cat-file", "-e", "HEAD:" + unit).returncode != 0:
        return "HEAD"                      # not committed yet: the working tree against HEAD
    first = git("log", "--diff-filter=A", "--format=%H", "--", unit).stdout.split()
    if not first:
        return None
    parent = first[-1] + "~1"
    return parent if git("rev-parse", "--verify", "-q", parent).returncode == 0 else None


@needs_hipcc
def test_existing_units_compile_to_the_parents_assembly():
    rev = _parent_revision()
    if rev is None:
        pytest.skip("no git history to take the parent's sources from")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_device_asm.py"), "--parent", rev], capture_output=True, text=True,
                       timeout=1500)
    lines = [ln for ln in r.stdout.splitlines() if re.match(r"\w+_gfx950\.s  tree ", ln)]
    print("\n".join(lines))
    assert len(lines) == len(chk.UNITS) == 6, r.stdout[-2000:] + r.stderr[-2000:]
    assert all(ln.endswith(" identical") for ln in lines), lines
    assert r.returncode == 0, r.stdout[-2000:]
