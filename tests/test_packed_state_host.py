"""The rule that decides when a J2 launch builds or reads the packed copy of s0 (``host_side.hpp``: ``choose_state_launch`` with its
``pack_*`` inputs, ``pack_candidate``, ``PackEpoch``): every combination of the flags with the launch counts 0-3 of an s0 epoch, and
every sequence of six events, in a stand-alone program (``tests/packed_state_harness.cpp``, its own ``main``) built with
AddressSanitizer + UBSan on the CPU and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "packed_state_harness.cpp")
HDR = os.path.join(ROOT, "dolfinx_materials_amd", "csrc", "host_side.hpp")
OUT = os.path.join(ROOT, "tests", "_san")


def _compiler():
    for c in (CLANG, shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    return None


def test_packed_copy_rule_over_all_flags_counts_and_event_sequences():
    cc = _compiler()
    if cc is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "packed_state_asan_ubsan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cmd = [cc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    report = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0 and "all ok: 65536 combinations, 6 build, 4 use; 15625 sequences" in r.stdout, report
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert marker not in r.stderr, report
