"""Build-time checks of the plane-strain logarithmic-strain unit on the cross-compiler alone: ``log_strain_plane_kernel`` and nothing
else in the unit, without scratch and without spilled VGPRs, with the static LDS ``log_strain_plane.hpp`` states, MORE waves per SIMD
and fewer VGPRs than ``log_strain_kernel`` of the same tree, 16 B loads and stores, no atomics, no workgroup barrier inside the tile
loop and one after it; and the device assembly of every unit that existed before, byte for byte what it was
(``tests/golden/log_strain_plane_parent_asm_sha256.json`` holds the digests of the parent commit's sources, made with
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
# per wave the out-tile of one round: 32 points x 25 entries
LDS_BYTES = 4 * (32 * 25) * 8
EARLIER = ("dxmat", "ramberg_osgood", "param_fields", "hyperelastic", "hosford", "orthotropic", "small_strain_clean", "single_crystal",
           "heat_transfer", "log_strain", "fs_single_crystal", "plane_stress", "plane_strain", "plane_stress_j2", "plane_stress_hosford",
           "plane_gradient", "small_strain_packed", "heat_plane", "ogden_plane", "hosford_plane")
FRAGMENTS = ("plane5_rows5_load.hpp", "plane5_rows5_take.hpp", "plane5_rows5_put.hpp", "plane5_rows5_store.hpp", "plane5_out25_copyout.hpp")


@needs_hipcc
def test_kernel_has_no_scratch_no_spilled_vgpr_the_stated_lds_and_more_waves_than_the_nine_wide_kernel():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "log_strain_plane.s")
        remarks = chk.device_asm(chk.CSRC, "log_strain_plane", out, remarks=True)
        asm = open(out).read()
        wide = chk.resource_table(chk.device_asm(chk.CSRC, "log_strain", os.path.join(tmp, "log_strain.s"), remarks=True))
    table = chk.resource_table(remarks)
    assert len(table) == 1 and all("log_strain_plane_kernel" in k for k in table), sorted(table)      # nothing else in the unit
    (name, r), = table.items()
    (w,) = [v for k, v in wide.items() if "log_strain_kernel" in k]
    print("log_strain_plane_kernel", r)
    print("log_strain_kernel      ", w)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, r
    hpp = open(os.path.join(chk.CSRC, "log_strain_plane.hpp")).read()
    assert "constexpr int LSP_PPR = 32;" in hpp and "LSP_LDS_BYTES = WAVES_PER_BLOCK * LSP_LDS_PER_WAVE * 8;" in hpp
    assert "static_assert(LSP_LDS_BYTES == 25600" in hpp
    assert r["lds"] == LDS_BYTES == 25600, r
    assert w["occupancy"] == 2 and r["occupancy"] > w["occupancy"] and r["vgprs"] < w["vgprs"] and r["lds"] < w["lds"], (r, w)
    assert r["occupancy"] * r["lds"] <= 160 * 1024      # w waves per SIMD x 4 SIMDs / 4 waves per workgroup = w workgroups per CU fit the LDS
    body = asm[asm.index(name + ":"):asm.index(".Lfunc_end", asm.index(name + ":"))]
    assert "scratch_" not in body
    assert len(re.findall(r"global_store_dwordx4", body)) >= 1 and len(re.findall(r"global_load_dwordx4", body)) >= 1
    assert not re.findall(r"global_atomic|flat_atomic|buffer_atomic|ds_.*_rtn", body)
    # the only inline assembly is the empty opaque-register idiom: nothing stands between the markers
    assert not [t for t in re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", body, flags=re.S) if t.strip()]
    # one workgroup barrier, after the tile loop (the stats reduction): no backward branch follows it
    assert len(re.findall(r"\bs_barrier\b", body)) == 1
    tail = body[body.index("s_barrier"):]
    labels_before = set(re.findall(r"^(\.LBB\d+_\d+):", body[:body.index("s_barrier")], flags=re.M))
    assert not [t for t in re.findall(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", tail) if t in labels_before]
    # the header and DESIGN.md report the compiler's figures
    assert f"{r['vgprs']} VGPRs" in hpp and f"{r['occupancy']} waves per SIMD" in hpp
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### Logarithmic-strain J2 plasticity under the plane-strain hypothesis"):]
    assert f"{r['vgprs']} VGPRs" in sec and "25 600 B" in sec and f"{r['occupancy']} waves per SIMD" in sec


@needs_hipcc
def test_every_earlier_unit_compiles_to_the_parents_assembly():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "log_strain_plane_parent_asm_sha256.json")))
    assert sorted(want) == sorted(u + "_gfx950.s" for u in EARLIER)
    assert sorted(EARLIER) == sorted(chk.UNITS + chk.LATER_UNITS + chk.PLANE_FORM_UNITS) and chk.PLANE_F_UNITS == ("log_strain_plane",)
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
    assert re.search(r"^SRCS := .*\blog_strain_plane\.hip\b", mk, flags=re.M) and re.search(r"^HDRS := .*\blog_strain_plane\.hpp\b", mk, flags=re.M)
    dry = subprocess.run(["make", "-n", "asm"], cwd=chk.CSRC, capture_output=True, text=True, check=True).stdout
    assert "-o log_strain_plane_gfx950.s log_strain_plane.hip" in dry
    hpp = open(os.path.join(chk.CSRC, "log_strain_plane.hpp")).read()
    assert "__global__" not in hpp and "__device__" not in hpp                        # host entry points and constants only
    assert hpp.count('__attribute__((visibility("hidden")))') == 2                    # every host entry point of the unit
    hip = open(os.path.join(chk.CSRC, "log_strain_plane.hip")).read()
    # the rows-of-five text has its second user; the take / put pair is included once each, the PK1 store once
    for f in FRAGMENTS:
        assert hip.count(f'#include "{f}"') == 1, f
        assert f'#include "{f}"' in open(os.path.join(chk.CSRC, "ogden_plane.hip")).read(), f
    assert '#include "principal_axes.hpp"' in hip and "sinhc_series(" in hip and '#include "tile_' not in hip and '#include "log_strain.hpp"' not in hip
    src = hip
    for f in FRAGMENTS:
        src = src.replace(f'#include "{f}"', open(os.path.join(chk.CSRC, f)).read())
    code = re.sub(r"//[^\n]*", "", src)
    assert code.count("__global__") == 1 and "atomic" not in code.replace("__ATOMIC", "") and "__syncthreads" not in code
    assert all(re.fullmatch(r'asm volatile\(""\s*:\s*"\+v"\(\w+\)\)', a) for a in re.findall(r"asm[^;]*", code)), re.findall(r"asm[^;]*", code)
    assert "stream_store<0>" in code and "stream_store<1>" in code and "stream_load<2>" in code and "stream_load<3>" in code and "wave_lds_sync()" in code
    assert code.count("jacobi_rotate(") == 1                                           # ONE rotation, no sweeps
    assert code.count("lsp_theta(") == 2 and code.count("lsp_gamma(") == 3            # their definitions; th01; g001 and g110
    assert "__launch_bounds__(BLOCK)\n" in code                                        # no occupancy argument
    # dxmat.hip reaches the unit through its two host entry points only
    dx = re.sub(r"//[^\n]*", "", open(os.path.join(chk.CSRC, "dxmat.hip")).read())
    assert not re.findall(r"\blog_strain_plane_kernel\b(?!_fn)", dx.replace('"log_strain_plane_kernel"', ""))
    assert "log_strain_plane_kernel_fn" in dx and "log_strain_plane_launch(" in dx
    # law 19's unit is what it was and does not know the new one; the tool lists the unit in a tuple of its own
    assert "log_strain_plane" not in open(os.path.join(chk.CSRC, "log_strain.hip")).read()
    assert "log_strain_plane" not in chk.UNITS + chk.LATER_UNITS + chk.PLANE_FORM_UNITS
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "log_strain_plane.hip" in design and "profiles/r28_log_strain_plane.md" in design
