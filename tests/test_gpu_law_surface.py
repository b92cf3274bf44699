"""GPU: everything the C ABI shows of the per-law descriptors (``kLaws`` of ``csrc/dxmat.hip``) against
``tests/golden/law_surface.npz``, which ``tests/golden/make_law_surface.py`` recorded from the library as it was BEFORE the host
side was made table-driven.  The host side computes none of the numbers: with the same device code and launch arguments the
arrays are equal bit for bit, and any difference is a host-side slip (wrong slot, wrong constant, wrong layout, wrong text)."""
import json
import os

import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import law_surface as ls

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "law_surface.npz"))
GOLD_META = json.loads(str(GOLD["meta"]))
KNOWN = sorted(GOLD_META["laws"], key=int)


@pytest.fixture(scope="module")
def surveyed():
    inputs = {int(law): [GOLD[f"law{law}/input0"], GOLD[f"law{law}/input1"]] for law in KNOWN}
    meta, arrays = ls.survey(_lib.load(), inputs)
    return json.loads(json.dumps(meta)), arrays   # (keys as the fixture has them: strings)


def test_the_fixture_covers_every_known_law_and_a_fair_share_of_yielded_points():
    assert [int(k) for k in KNOWN] == sorted(ls.PARAMS) == [0, 1, 2, 3, 4, 5, 7, 10]
    for law in ("1", "2", "3", "4", "10"):
        for per_layout in GOLD_META["laws"][law]["stats"].values():
            assert per_layout[1]["n_plastic"] >= ls.N // 4, (law, per_layout)


def test_unassigned_ids_are_refused_with_the_recorded_message(surveyed):
    meta, _ = surveyed
    assert sorted(meta["unassigned"], key=int) == ["-1", "6", "8", "9", "11"]
    for law, got in meta["unassigned"].items():
        assert got["create_null"] and got["law_info"]["rc"] == -1
        assert got == GOLD_META["unassigned"][law], (law, got)


@pytest.mark.parametrize("law", KNOWN)
def test_descriptor_layouts_refusals_and_validation_equal_the_recording(surveyed, law):
    got, want = surveyed[0]["laws"][law], GOLD_META["laws"][law]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], (law, key, got[key], want[key])


def test_initial_state_and_two_increments_per_layout_equal_the_recording_bit_for_bit(surveyed):
    _, arrays = surveyed
    recorded = sorted(k for k in GOLD.files if k != "meta" and "/input" not in k)
    assert sorted(arrays) == recorded
    for key in recorded:
        got, want = arrays[key], GOLD[key]
        assert got.shape == want.shape and got.dtype == want.dtype == np.float64, key
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (key, float(np.nanmax(np.abs(got - want))))
    # what the recording itself must show: zeros after dxm_create, the identity in the two FeFp tensors
    for law in KNOWN:
        for f, dim in enumerate(GOLD_META["laws"][law]["field_dims"]):
            for which in (0, 1):
                a = GOLD[f"law{law}/initial/s{which}/state{f}"]
                unit = law in ("3", "4") and f in (1, 2)
                assert np.array_equal(a, np.tile([1.0, 1, 1, 0, 0, 0], (ls.N, 1)) if unit else np.zeros((ls.N, dim))), (law, f, which)
