"""The tile I/O steps the update kernels share as text (``csrc/tile_*.hpp``, included inside the kernel bodies) and
``csrc/principal_axes.hpp``: the build sees them, each one really is shared, they carry no inline assembly beyond the opaque
register idiom (the per-law ``test_*_build.py`` scan the law's own files, and these files now hold part of that text), and the
kernels built from them keep their registers: no scratch and no spilled VGPR in any of the six translation units, nor in the four
3-wide units that share the rows of three; and the text those four copied from each other is gone from them."""
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
    # rows of six (3), the staged triangles (1), rows of nine (4), the 81-entry out-tile (2), rows of three (2), the entries' write-out (1)
    assert len(FRAGMENTS) >= 13, FRAGMENTS


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


ROWS3_UNITS = ("plane_stress", "plane_stress_j2", "plane_stress_hosford", "heat_transfer")


@pytest.mark.skipif(shutil.which(chk.HIPCC) is None, reason="needs the HIP compiler")
def test_no_kernel_of_the_four_three_wide_units_has_scratch_or_a_spilled_vgpr():
    assert all(u in chk.LATER_UNITS for u in ROWS3_UNITS)
    with tempfile.TemporaryDirectory() as tmp:
        units = chk.build_units(chk.CSRC, tmp, "tree", units=ROWS3_UNITS)
    assert sorted(units) == sorted(ROWS3_UNITS)
    for unit, (_, table) in units.items():
        assert table, unit
        for name, r in table.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (unit, name, r)


def test_the_three_wide_units_no_longer_carry_the_shared_text():
    for unit in ROWS3_UNITS:
        src = open(os.path.join(chk.CSRC, unit + ".hip")).read()
        assert "reinterpret_cast<const double2_t*>(g0)" not in src and "constexpr int NQ" not in src, unit
        for name in ("tile_rows3_load.hpp", "tile_rows3_store.hpp", "tile_entries_store.hpp"):
            assert src.count('#include "' + name + '"') == 1, (unit, name)
    # the slot map of the symmetric 3 x 3 record exists once
    holders = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(chk.CSRC, "*")))
               if os.path.isfile(f) and "col == 3 ? 1 : col - 1" in open(f, errors="replace").read()]
    assert holders == ["dxm_common.hpp"], holders
