"""CPU sanitizer run of the synth stage's host face, in the manner of tests/test_sanitize_text.py: synth_host.cpp (the bank, the
control rate, the planner and the replay of synth_math.hpp) behind tests/sanitize/synth_main.cpp, built with gcc's AddressSanitizer
and UndefinedBehaviorSanitizer and run once — a program of its own, with nothing preloaded into Python.  The test writes the bank and
every case of tests/synth_cases.py to a file; the program renders every case (in one call and in three), expects the runaway loop to
be refused, then corrupts every index field of the bank in turn and sweeps every event byte 0 .. 255: each corruption is either
rejected or rendered, and a read outside wave_data or an out-of-range conversion aborts the run."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import synth_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def write_inputs(path):
    a = SC.bank_arrays()
    cases = list(SC.CASES.values()) + [SC.RUNAWAY, (SC.ONE_NOTE, 60, 64)]
    igs, ismp = a["instrument_regions"]
    pgs, pins = a["preset_regions"]
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", a["wave_data"].size, a["samples"].shape[0], ismp.size, a["instruments"].shape[0], pins.size, a["presets"].shape[0],
                            len(cases), len(SC.CASES)))
        for arr, dt in ((a["wave_data"], np.int16), (a["samples"], np.int32), (igs, np.int16), (ismp, np.uint32), (a["instruments"], np.uint32),
                        (pgs, np.int16), (pins, np.uint32), (a["presets"], np.int32)):
            f.write(np.ascontiguousarray(arr, dt).tobytes())
        for events, n_blocks, poly in cases:
            f.write(struct.pack("<3Q", events[0].size, n_blocks, poly))
            f.write(np.ascontiguousarray(events[0], np.float64).tobytes())
            for k in range(1, 5):
                f.write(np.ascontiguousarray(events[k], np.int32).tobytes())


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_synth_host_under_asan_ubsan(tmp_path):
    inputs = tmp_path / "synth_inputs.bin"
    write_inputs(inputs)
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "synth_san")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "synth_main.cpp"), os.path.join(csrc, "synth_host.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(inputs)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "SANITIZE_SYNTH_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
