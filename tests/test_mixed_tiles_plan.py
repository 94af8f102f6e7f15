"""Mixed column tiles of the fused GEMM's tile lists (blockdft_plan.hpp: MixedPair) on the host, CPU only: the planner behind
tests/sanitize/mixed_tiles_main.cpp, built with g++ under ASan / UBSan as tests/test_sanitize_cpu.py builds host_main.cpp (its own
main, no preload) and run once.  The program checks coverage, the pairing conditions, the stored frame ranges, the flop recount and
the entry counts of an interior row tile with mixing on (its head comment has the list); with mixing off it prints a hash per tile
list, compared here with the hashes recorded from the planner as it was before mixed tiles (tests/golden/mixed_tiles_off_lists.txt):
with mixing off every list stays what it was, entry for entry."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_mixed_tile_lists_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "mixed_tiles_san")
    srcs = [os.path.join(csrc, f) for f in ("vqt_host.cpp", "blockdft_plan.cpp", "batch_plan.cpp")]
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "mixed_tiles_main.cpp"), *srcs, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "MIXED_TILES_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = [l for l in r.stdout.splitlines() if l.startswith("OFF ")]
    with open(os.path.join(ROOT, "tests", "golden", "mixed_tiles_off_lists.txt")) as fh:
        want = fh.read().splitlines()
    assert len(want) == 240 and got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]
