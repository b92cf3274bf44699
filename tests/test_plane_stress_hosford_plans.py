"""The transfer plans of law 33 (``csrc/host_side.hpp::plan_transfer``: the 9 numbers of its 3 x 3 tangent cross as they are, in the full
and the rows forms, and every plan equals that of law 23 for the same request) in a stand-alone harness of their own, built with
AddressSanitizer and UBSan and run directly.  Every other law's plans are pinned by ``tests/test_plane_stress_j2_plans.py``."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "plane_stress_hosford_plan_harness.cpp")
HDR = os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "host_side.hpp")
OUT = os.path.join(ROOT, "tests", "_san")


@pytest.fixture(scope="module")
def harness():
    cc = next((c for c in (CLANG, shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "plane_stress_hosford_plans_asan_ubsan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cmd = [cc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plans_of_plane_stress_hosford(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 broken statements" in r.stdout, r.stdout + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) == 3840
