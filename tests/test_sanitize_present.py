"""CPU sanitizer run of the present stage's host face and host planning, in the manner of tests/test_sanitize_overlay.py:
present_host.cpp (with stage_plan.cpp, whose cut it uses) behind tests/sanitize/present_main.cpp, built with gcc's AddressSanitizer
and UndefinedBehaviorSanitizer and run once — a program of its own, with nothing preloaded into Python.  A texel index past a mip, a
mip past the chain or an out-of-range float-to-integer conversion aborts the run; the program also checks the chain's layout, the cut
of a call's rows into pieces, and that whatever a tile's taps sample lies in the footprint the device stage would stage for it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_present_host_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "present_san")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "present_main.cpp"), os.path.join(csrc, "present_host.cpp"), os.path.join(csrc, "stage_plan.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "SANITIZE_PRESENT_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
