"""CPU sanitizer run of the synth stage's effects on the host, in the manner of tests/test_sanitize_synth.py: synth_host.cpp (the
planner with its sends, the replay with the three extra sums, SynthEffects over synth_fx_math.hpp) behind
tests/sanitize/synth_fx_main.cpp, built with gcc's AddressSanitizer and UndefinedBehaviorSanitizer and run once — a program of its
own, with nothing preloaded into Python.  The test writes the bank and every case of tests/synth_fx_cases.py to a file; the program
renders every case with effects (in one call and in three) and drives the effects-only face with a unit impulse at five sample rates:
an index outside a reverb buffer, the chorus ring or the delay table, or an out-of-range conversion, aborts the run."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import synth_fx_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def write_inputs(path):
    a = FC.bank_arrays()
    cases = list(FC.CASES.values())
    igs, ismp = a["instrument_regions"]
    pgs, pins = a["preset_regions"]
    with open(path, "wb") as f:
        f.write(struct.pack("<7Q", a["wave_data"].size, a["samples"].shape[0], ismp.size, a["instruments"].shape[0], pins.size, a["presets"].shape[0],
                            len(cases)))
        for arr, dt in ((a["wave_data"], np.int16), (a["samples"], np.int32), (igs, np.int16), (ismp, np.uint32), (a["instruments"], np.uint32),
                        (pgs, np.int16), (pins, np.uint32), (a["presets"], np.int32)):
            f.write(np.ascontiguousarray(arr, dt).tobytes())
        for events, n_blocks, poly, sr in cases:
            f.write(struct.pack("<4Q", events[0].size, n_blocks, poly, sr))
            f.write(np.ascontiguousarray(events[0], np.float64).tobytes())
            for k in range(1, 5):
                f.write(np.ascontiguousarray(events[k], np.int32).tobytes())


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_synth_effects_host_under_asan_ubsan(tmp_path):
    inputs = tmp_path / "synth_fx_inputs.bin"
    write_inputs(inputs)
    csrc = os.path.join(ROOT, "pitchvis_amd", "csrc")
    exe = str(tmp_path / "synth_fx_san")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *SAN, "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "synth_fx_main.cpp"), os.path.join(csrc, "synth_host.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(inputs)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "SANITIZE_SYNTH_FX_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
