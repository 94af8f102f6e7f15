"""Resource guard for the two replay kernels of the synth stage (no GPU needed: hipcc cross-compiles and reports what a kernel uses),
with the remarks tests/test_kernel_resources.py reads.  The effects kernel (synth_fx_batch.hip) must leave room for two workgroups in
a CU's 160 KiB of LDS and spill nothing; the dry kernel (synth_batch.hip) keeps the resources DESIGN 6j records for it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _usage(unit, tmp_path):
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", unit)
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "x.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            assert name not in usage, name
            usage[name] = {}
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs|AGPRs): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_effects_kernel_fits_two_workgroups_a_cu_and_the_dry_kernel_keeps_its_resources(tmp_path):
    fx = _usage("synth_fx_batch.hip", tmp_path)
    assert len(fx) == 1 and "synth_replay_fx" in next(iter(fx)), list(fx)
    u = next(iter(fx.values()))
    print("synth_replay_fx:", u)
    assert u["ScratchSize"] == 0 and 0 < u["LDS"] <= 81920, u
    dry = _usage("synth_batch.hip", tmp_path)
    assert len(dry) == 1 and "synth_replay" in next(iter(dry)) and "synth_replay_fx" not in next(iter(dry)), list(dry)
    u = next(iter(dry.values()))
    print("synth_replay:", u)
    assert u["ScratchSize"] == 0 and 0 < u["LDS"] <= 37632, u
