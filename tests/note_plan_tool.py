"""The note model's and the note trainer's host planners behind tests/sanitize/note_plan_main.cpp: built once per test module with
-fsanitize=address,undefined (the flags of test_sanitize_cpu.py) and asked one question per run.  build() also makes the other
stand-alone programs of tests/sanitize/ over plain g++ units of pitchvis_amd/csrc (main file and unit list as arguments).  fill() restates how the program
fills a matrix, chunk geometry the constants of note_model_plan.hpp."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def build(tmp_dir, main="note_plan_main.cpp", units=("note_model_plan.cpp", "note_trainer_plan.cpp")):
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = os.path.join(str(tmp_dir), main[:-len("_main.cpp")])
    cmd = ["g++", "-std=c++17", "-Wall", *SAN, "-I", csrc, os.path.join(ROOT, "tests", "sanitize", main),
           *[os.path.join(csrc, u) for u in units], "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def fill(i):
    """element i of a matrix the program makes: exact in f32, never zero"""
    return (np.asarray(i, np.int64) % 16777213 + 1).astype(np.float32)
