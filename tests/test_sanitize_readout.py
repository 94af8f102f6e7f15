"""CPU sanitizer run of the readout stage's host face, in the manner of tests/test_sanitize_text.py: readout_host.cpp and
text_host.cpp behind tests/sanitize/readout_main.cpp, built with gcc's AddressSanitizer and UndefinedBehaviorSanitizer and run once —
a program of its own, with nothing preloaded into Python.  The program draws a list of values (the clamp, values far beyond it,
NaN and the infinities among them) at image sizes from 1 x 1 to 4096 x 1 and font sizes from a hundredth of a pixel to 1024, into
exactly sized pictures, and checks that every drawn pixel lies in a tile of the grid the device stage would launch: a read or
write outside a buffer, or an out-of-range float-to-integer conversion, aborts the run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_readout_host_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "readout_san")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "readout_main.cpp"), os.path.join(csrc, "readout_host.cpp"), os.path.join(csrc, "text_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "SANITIZE_READOUT_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
