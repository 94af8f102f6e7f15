"""The many-streams conditioning (pvq_agc_batch_*: downmix, silence gate, MonoAgc on the device) as far as it goes without a GPU:
the symbols, the argument checks of the C ABI (the reference's MonoAgc::new errors, dagc_fork/src/lib.rs:36-49), the host-only
handle, and what the compiler made of the two kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pitchvis_amd as P
from pitchvis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_agc_batch_create", "pvq_agc_batch_destroy", "pvq_agc_batch_condition_device", "pvq_agc_batch_get_gains")


def test_symbols_exported():
    L = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed


@pytest.mark.parametrize("device_id", [-1, 0])
@pytest.mark.parametrize("rms,d,needle", [
    (0.0, 0.1, "`desired_output_rms` must be a finite positive number"),
    (-1.0, 0.1, "`desired_output_rms` must be a finite positive number"),
    (float("inf"), 0.1, "`desired_output_rms` must be a finite positive number"),
    (float("nan"), 0.1, "`desired_output_rms` must be a finite positive number"),
    (0.07, -0.1, "`distortion_factor` must be a number within `0.0 ..= 1.0`"),
    (0.07, 1.5, "`distortion_factor` must be a number within `0.0 ..= 1.0`"),
    (0.07, float("nan"), "`distortion_factor` must be a number within `0.0 ..= 1.0`"),
])
def test_create_rejects_like_the_reference(device_id, rms, d, needle):
    """the parameter list of test_mono_agc_rejects_like_the_reference; rejected before any device is touched, so device 0 may be absent"""
    L = _lib.load()
    h = C.c_void_p()
    assert L.pvq_agc_batch_create(device_id, 8, rms, d, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG
    assert not h.value
    assert needle in L.pvq_last_error().decode()
    with pytest.raises(ValueError, match=re.escape(needle)):
        P.AgcBatch(8, rms, d, device=None if device_id < 0 else device_id)


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    h = C.c_void_p()
    assert L.pvq_agc_batch_create(-1, 0, 0.07, 0.001, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG   # no streams
    assert L.pvq_agc_batch_create(-1, 3, 0.07, 0.001, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_agc_batch_create(-1, 3, 0.07, 0.001, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        n = 3
        # the pointers stand for device memory; a host-only handle never dereferences them
        buf = np.zeros(4096, np.float32)
        ptrs = (C.c_void_p * n)(*[buf.ctypes.data] * n)
        nc = (C.c_size_t * n)(2, 1, 2)
        call = L.pvq_agc_batch_condition_device
        assert call(h, ptrs, None, nc, 64, ptrs, None, 0, None) == _lib.PVQ_ERR_NO_DEVICE
        assert "GPU" in L.pvq_last_error().decode()
        assert call(h, ptrs, ptrs, nc, 64, ptrs, None, 0, None) == _lib.PVQ_ERR_NO_DEVICE
        assert call(h, ptrs, None, nc, 0, ptrs, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG      # chunk == 0
        assert call(h, None, None, nc, 64, ptrs, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG     # null tables
        assert call(h, ptrs, None, None, 64, ptrs, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, ptrs, None, nc, 64, None, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(None, ptrs, None, nc, 64, ptrs, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG  # null handle
        holes = (C.c_void_p * n)(buf.ctypes.data, None, buf.ctypes.data)
        assert call(h, holes, None, nc, 64, ptrs, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG    # a stream with chunks and no left row
        assert call(h, ptrs, None, nc, 64, holes, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, ptrs, None, nc, 64, ptrs, buf.ctypes.data, 1, None) == _lib.PVQ_ERR_INVALID_ARG   # gain_stride < n_chunks[0]
        assert "gain_stride" in L.pvq_last_error().decode()
        assert call(h, ptrs, None, nc, 64, ptrs, buf.ctypes.data, 2, None) == _lib.PVQ_ERR_NO_DEVICE
        gains = np.zeros(n, np.float32)
        assert L.pvq_agc_batch_get_gains(h, gains.ctypes.data_as(C.POINTER(C.c_float))) == _lib.PVQ_OK
        assert np.array_equal(gains, np.ones(n, np.float32))                                    # lib.rs:50
        assert L.pvq_agc_batch_get_gains(h, None) == _lib.PVQ_ERR_INVALID_ARG
    finally:
        L.pvq_agc_batch_destroy(h)
    L.pvq_agc_batch_destroy(None)
    b = P.AgcBatch(2, 0.07, 0.001, device=None)
    with pytest.raises(P.PvqError) as e:
        b.condition_device([buf.ctypes.data] * 2, None, [1, 1], 64)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        b.condition_device([buf.ctypes.data], None, [1], 64)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """in the manner of test_kernel_resources.py: neither kernel may spill (the recurrence holds two tiles' pieces in registers by design)"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "condition_batch.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "x.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    gate = [u for k, u in usage.items() if "cond_gate" in k]
    rec = [u for k, u in usage.items() if "cond_recurrence" in k]
    assert len(gate) == 1 and len(rec) == 2, list(usage)   # the recurrence: chunk a multiple of 4, and any chunk
    for u in gate + rec:
        print(u)
        assert u["ScratchSize"] == 0, u
        assert u["LDS"] % 16 == 0, u
