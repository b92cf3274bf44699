"""Build-time checks of the packed-old-state kernels (``csrc/small_strain_packed.hip``: ``small_strain_packed_kernel<law, layout,
PACKED>``, PACKED = 1 build / 2 use) on the cross-compiler alone:

* all sixteen instantiations (two J2 laws x four tangent layouts x build / use), and nothing else in the unit, within the bounds of
  the plain J2 kernels -- at most 128 VGPRs, no scratch, no spilled VGPR, the same 30 848 B of static LDS;
* the unit of the clean kernels (``small_strain_clean.hip``, PACKED = 0), which includes the same tile body, compiles to the device
  assembly the sources of the parent revision give, byte for byte;
* the unit is built into the library and named by the tool."""
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
UNIT = "small_strain_packed"


@needs_hipcc
def test_packed_kernels_meet_the_resource_bounds_of_the_plain_j2_kernels():
    with tempfile.TemporaryDirectory() as tmp:
        remarks = chk.device_asm(chk.CSRC, UNIT, os.path.join(tmp, UNIT + ".s"), remarks=True)
    table = chk.resource_table(remarks)
    assert all("small_strain_packed_kernel" in k for k in table), sorted(table)
    args = sorted(tuple(int(x) for x in re.search(r"small_strain_packed_kernelILi(\d)ELi(\d)ELi(\d)E", k).groups()) for k in table)
    assert args == [(law, tl, packed) for law in (1, 2) for tl in (0, 1, 2, 3) for packed in (1, 2)], args
    for name, r in sorted(table.items()):
        print(name, r)
    assert chk.broken_bounds(table) == []     # <= 128 VGPRs (+ AGPRs), no scratch, no spilled VGPR, LDS == 30848
    assert chk.MAX_VGPRS == 128 and chk.J2_STATIC_LDS == 30848


def _parent_revision():
    """The last commit without the packed kernels: HEAD while the unit is not committed, else the parent of the commit that added it."""
    def git(*a):
        return subprocess.run(["git", *a], cwd=ROOT, capture_output=True, text=True)
    if git("rev-parse", "--git-dir").returncode != 0:
        return None
    path = "dolfinx_materials_amd/csrc/" + UNIT + ".hip"
    if git("cat-file", "-e", "HEAD:" + path).returncode != 0:
        return "HEAD"
    first = git("log", "--diff-filter=A", "--format=%H", "--", path).stdout.split()
    if not first:
        return None
    parent = first[-1] + "~1"
    return parent if git("rev-parse", "--verify", "-q", parent).returncode == 0 else None


@needs_hipcc
def test_clean_unit_compiles_to_the_parents_assembly():
    rev = _parent_revision()
    if rev is None:
        pytest.skip("no git history to take the parent's sources from")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "parent")
        os.makedirs(src)
        tar = subprocess.run(["git", "archive", rev, "dolfinx_materials_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", src], input=tar.stdout, check=True)
        chk.device_asm(os.path.join(src, "dolfinx_materials_amd", "csrc"), "small_strain_clean", os.path.join(tmp, "parent.s"))
        chk.device_asm(chk.CSRC, "small_strain_clean", os.path.join(tmp, "tree.s"))
        assert os.path.getsize(os.path.join(tmp, "tree.s")) > 100000      # eight whole kernels
        assert chk.sha(os.path.join(tmp, "tree.s")) == chk.sha(os.path.join(tmp, "parent.s"))


def test_the_unit_is_built_into_the_library_and_named_by_the_tool():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert UNIT + ".hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert UNIT in chk.LATER_UNITS and UNIT not in chk.UNITS
    # dxmat.hip names no kernel of the unit: its device assembly stays the parent's
    assert "small_strain_packed_kernel<" not in re.sub(r'"[^"]*"', "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
