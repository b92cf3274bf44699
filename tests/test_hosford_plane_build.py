"""Build-time checks of the plane-strain Hosford unit on the cross-compiler alone: ``hosford_plane_kernel`` and nothing else in the
unit, without scratch and without spilled VGPRs, with the static LDS ``hosford_plane.hpp`` states, at least the waves per SIMD of
``hosford_kernel`` of the same tree and fewer VGPRs, 16 B loads and stores, no atomics, no workgroup barrier inside the tile loop and one
after it; and the device assembly of every unit that existed before, byte for byte what it was
(``tests/golden/hosford_plane_parent_asm_sha256.json`` holds the digests of the parent commit's sources, made with
``tools/check_device_asm.py --parent <rev> --all-units --write-digests``)."""
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
# per wave the 64 x 4 strain / stress staging and 64 records of 10 upper-triangle entries; the 4 x 4 status words
LDS_BYTES = 4 * 64 * (4 + 10) * 8 + 4 * 4 * 8
EARLIER = ("dxmat", "ramberg_osgood", "param_fields", "hyperelastic", "hosford", "orthotropic", "small_strain_clean", "single_crystal",
           "heat_transfer", "log_strain", "fs_single_crystal", "plane_stress", "plane_strain", "plane_stress_j2", "plane_stress_hosford",
           "plane_gradient", "small_strain_packed", "heat_plane", "ogden_plane")


@needs_hipcc
def test_kernel_has_no_scratch_no_spilled_vgpr_the_stated_lds_and_is_lighter_than_the_six_wide_kernel():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "hosford_plane.s")
        remarks = chk.device_asm(chk.CSRC, "hosford_plane", out, remarks=True)
        asm = open(out).read()
        wide = chk.resource_table(chk.device_asm(chk.CSRC, "hosford", os.path.join(tmp, "hosford.s"), remarks=True))
    table = chk.resource_table(remarks)
    assert len(table) == 1 and all("hosford_plane_kernel" in k for k in table), sorted(table)      # nothing else in the unit
    (name, r), = table.items()
    w = [v for k, v in wide.items() if "hosford_kernel" in k]
    print("hosford_plane_kernel", r)
    print("hosford_kernel      ", w)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
    hpp = open(os.path.join(chk.CSRC, "hosford_plane.hpp")).read()
    assert "HFP_LDS_BYTES = WAVES_PER_BLOCK * HFP_LDS_PER_WAVE * 8 + 4 * WAVES_PER_BLOCK * 8;" in hpp and "HFP_LDS_BYTES == 28800" in hpp
    assert r["lds"] == LDS_BYTES == 28800, r
    assert all(r["occupancy"] >= v["occupancy"] and r["vgprs"] < v["vgprs"] and r["lds"] < v["lds"] for v in w), (r, w)
    assert r["occupancy"] * r["lds"] <= 160 * 1024      # w waves per SIMD x 4 SIMDs / 4 waves per workgroup = w workgroups per CU fit the LDS
    body = asm[asm.index(name + ":"):asm.index(".Lfunc_end", asm.index(name + ":"))]
    assert "scratch_" not in body
    assert len(re.findall(r"global_store_dwordx4", body)) >= 10 and len(re.findall(r"global_load_dwordx4", body)) >= 2      # 2 + 8 passes out, 2 in
    assert not re.findall(r"global_atomic|flat_atomic|buffer_atomic|ds_.*_rtn", body)
    # the only inline assembly is the empty opaque-register / compiler-barrier idiom: nothing stands between the markers
    assert not [t for t in re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", body, flags=re.S) if t.strip()]
    # one workgroup barrier, after the tile loop (the stats reduction): no backward branch follows it
    assert len(re.findall(r"\bs_barrier\b", body)) == 1
    tail = body[body.index("s_barrier"):]
    labels_before = set(re.findall(r"^(\.LBB\d+_\d+):", body[:body.index("s_barrier")], flags=re.M))
    assert not [t for t in re.findall(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", tail) if t in labels_before]
    # DESIGN.md reports the compiler's figures
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### Hosford plasticity under the plane-strain hypothesis"):]
    assert f"{r['vgprs']} VGPRs" in sec and "28 800 B" in sec and f"{r['occupancy']} waves per SIMD" in sec


@needs_hipcc
def test_every_earlier_unit_compiles_to_the_parents_assembly():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "hosford_plane_parent_asm_sha256.json")))
    assert sorted(want) == sorted(u + "_gfx950.s" for u in EARLIER)
    assert sorted(EARLIER) == sorted(u for u in chk.UNITS + chk.LATER_UNITS + chk.PLANE_FORM_UNITS if u != "hosford_plane")
    with tempfile.TemporaryDirectory() as tmp:
        def one(unit):
            out = os.path.join(tmp, unit + ".s")
            chk.device_asm(chk.CSRC, unit, out)
            return unit, chk.sha(out)
        with ThreadPoolExecutor(max_workers=4) as pool:
            got = dict(pool.map(one, EARLIER))
    for unit in EARLIER:
        assert got[unit] == want[unit + "_gfx950.s"], unit


def test_the_unit_is_built_into_the_library_and_dxmat_names_no_kernel_of_it():
    mk = open(os.path.join(chk.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bhosford_plane\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bhosford_plane\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o hosford_plane_gfx950.s hosford_plane.hip" in dry
    hpp = open(os.path.join(chk.CSRC, "hosford_plane.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 2                    # every host entry point of the unit
    hip = open(os.path.join(chk.CSRC, "hosford_plane.hip")).read()
    assert '#include "principal_axes.hpp"' in hip and "sinhc_series(" in hip and '#include "tile_' not in hip
    code = re.sub(r"//[^\n]*", "", hip)
    assert code.count("__global__") == 1 and "atomic" not in code.replace("__ATOMIC", "") and "__syncthreads" not in code
    assert all(re.fullmatch(r'asm volatile\(""\s*:\s*(?:"\+v"\(\w+\)|::\s*"memory")\)', a) for a in re.findall(r"asm[^;]*", code)), re.findall(r"asm[^;]*", code)
    assert "stream_store<0>" in code and "stream_store<1>" in code and "stream_load<2>" in code and "stream_load<3>" in code and "wave_lds_sync()" in code
    assert code.count("hfp_divided_difference(") == 2                                  # its definition and ONE use: th_01 alone
    assert "jacobi_rotate(" not in code                                                # one closed-form rotation, no sweeps
    # no file of the unit is named tile_*.hpp (tests/test_tile_fragments.py: those need two users)
    assert not [f for f in os.listdir(chk.CSRC) if f.startswith("tile_") and "hosford_plane" in open(os.path.join(chk.CSRC, f)).read()]
    # dxmat.hip reaches the unit through its two host entry points only
    dx = re.sub(r"//[^\n]*", "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
    assert not re.findall(r"\bhosford_plane_kernel\b(?!_fn)", dx.replace('"hosford_plane_kernel"', ""))
    assert "hosford_plane_kernel_fn" in dx and "hosford_plane_launch(" in dx
    # law 10's unit and the plane-strain unit are what they were and do not know the new one
    assert "hosford_plane" not in open(os.path.join(chk.CSRC, "hosford.hip")).read()
    assert "hosford_plane" not in open(os.path.join(chk.CSRC, "plane_strain.hip")).read()
    assert "hosford_plane" in chk.PLANE_FORM_UNITS and "hosford_plane" not in chk.UNITS + chk.LATER_UNITS
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "hosford_plane.hip" in design and "profiles/r27_hosford_plane.md" in design
