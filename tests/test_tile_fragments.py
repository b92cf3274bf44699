"""The tile I/O steps the update kernels share as text (``csrc/tile_*.hpp``, included inside the kernel bodies) and
``csrc/principal_axes.hpp``: the build sees them, each one really is shared, they carry no inline assembly beyond the opaque
register idiom (the per-law ``test_*_build.py`` scan the law's own files, and these files now hold part of that text), and the
kernels built from them keep their registers: no scratch and no spilled VGPR in any of the six translation units."""
import glob
import os
import re
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_param_fields_build as chk  # noqa: E402

FRAGMENTS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(chk.CSRC, "tile_*.hpp")))
SHARED = FRAGMENTS + ["principal_axes.hpp"]


def test_the_fragments_are_found():
    assert len(FRAGMENTS) >= 10, FRAGMENTS     # rows of six (3), the staged triangles (1), rows of nine (4), the 81-entry out-tile (2)


@pytest.mark.parametrize("name", SHARED)
def test_the_makefile_names_it_as_a_header(name):
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^HDRS := .*(?<![\w/])" + re.escape(name) + r"\b", mk, flags=re.M), name


@pytest.mark.parametrize("name", SHARED)
def test_it_is_included_from_at_least_two_kernels_sources(name):
    users = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(chk.CSRC, "*.h*")))
             if re.search(r'^\s*#include "' + re.escape(name) + '"', open(f).read(), flags=re.M)]
    assert len(users) >= 2, (name, users)


@pytest.mark.parametrize("name", SHARED)
def test_its_inline_assembly_is_the_opaque_register_idiom_only(name):
    src = open(os.path.join(chk.CSRC, name)).read()
    for stmt in re.findall(r"asm\s*(?:volatile)?\s*\(([^;]*)\);", src):
        assert stmt.strip().startswith('""'), (name, stmt)


@pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
def test_no_kernel_of_the_six_units_has_scratch_or_a_spilled_vgpr():
    with tempfile.TemporaryDirectory() as tmp:
        units = chk.build_units(chk.CSRC, tmp, "tree")
    assert sorted(units) == sorted(chk.UNITS) and "orthotropic" in units
    for unit, (_, table) in units.items():
        assert table, unit
        for name, r in table.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (unit, name, r)
