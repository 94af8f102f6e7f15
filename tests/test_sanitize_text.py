"""CPU sanitizer run of the text stage's host face, in the manner of tests/test_sanitize_overlay.py: text_host.cpp behind
tests/sanitize/text_main.cpp, built with gcc's AddressSanitizer and UndefinedBehaviorSanitizer and run once — a program of its own,
with nothing preloaded into Python.  The test writes a TrueType file of the fixture's nine glyphs (fontTools) and passes its path;
the program lays out and draws the twelve labels, checks that every covered pixel lies in a tile the device stage would launch,
and feeds the reader every truncation of the file and 2 000 single-byte corruptions: a read outside the buffer or an
out-of-range float-to-integer conversion aborts the run."""
import os
import shutil
import subprocess

import pytest

import text_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_text_host_under_asan_ubsan(tmp_path):
    pytest.importorskip("fontTools")
    font = tmp_path / "pitch_glyphs.ttf"
    TC.build_ttf(font)
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "text_san")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "text_main.cpp"), os.path.join(csrc, "text_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(font)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "SANITIZE_TEXT_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
