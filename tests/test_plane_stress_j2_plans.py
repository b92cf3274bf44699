"""The transfer plans of laws 30 and 31 (``csrc/host_side.hpp::plan_transfer``: the 9 numbers of their 3 x 3 tangent cross as they are, in
the full and the rows forms, like those of laws 23 and 24; ``p`` and ``epsp`` take the routes of every law's visible state) in a
stand-alone harness of their own, built with AddressSanitizer and UBSan and run directly, and every plan of every other law
unchanged: one digest over all fields of their plans over the same 426 240 requests, recorded by building this same harness against
the header of the commit before the laws existed (``-DDXM_HOST_SIDE_HEADER='"<that header>"'``)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "plane_stress_j2_plan_harness.cpp")
HDR = os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "host_side.hpp")
OUT = os.path.join(ROOT, "tests", "_san")
PARENT_DIGEST = "c30226069c55dc0b 426240"


@pytest.fixture(scope="module")
def harness():
    cc = next((c for c in (CLANG, shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "plane_stress_j2_plans_asan_ubsan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cmd = [cc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plans_of_plane_stress_j2(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 broken statements" in r.stdout, r.stdout + r.stderr[-3000:]


def test_every_plan_of_every_other_law_is_what_it_was(harness):
    r = subprocess.run([harness, "digest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == PARENT_DIGEST, r.stdout + r.stderr[-3000:]
