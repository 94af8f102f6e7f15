"""The kernel product's per-wave stage streams (blockdft_plan.cpp: band_stages8) under ASan / UBSan, CPU only: the planner and
tests/sanitize/dots_stream_main.cpp as one instrumented executable.  It checks, over the six test geometries and a 3-bin range,
that every 8-bin block sits in exactly one wave's stream in deal order, stage by stage, that the padded counts are multiples of
the ring depth, and that every entry a wave can touch lies inside a frame tile's columns and inside the coefficient array."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_stage_streams_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "dots_stream_san")
    srcs = [os.path.join(csrc, f) for f in ("vqt_host.cpp", "blockdft_plan.cpp")]
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "dots_stream_main.cpp"), *srcs, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "SANITIZE_DOTS_STREAM_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
