"""CPU sanitizer run of the backdrop stage's multisampled host face, in the manner of tests/test_sanitize_backdrop.py: backdrop_host.cpp
behind tests/sanitize/backdrop_msaa_main.cpp, built with gcc's AddressSanitizer and UndefinedBehaviorSanitizer and run once, stand-alone.
It draws with samples = 4 a mesh whose boxes leave the image, on a 1 x 1 image and on a 4096-wide image of one row among others: a pixel
box past the image or an index past the four sample planes aborts the run."""
import os
import shutil
import subprocess

import pytest

from test_sanitize_backdrop import ENV, ROOT, SAN


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_backdrop_msaa_host_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "backdrop_msaa_san")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "backdrop_msaa_main.cpp"), os.path.join(csrc, "backdrop_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    print(r.stdout[-300:])
    assert r.returncode == 0 and "SANITIZE_BACKDROP_MSAA_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
