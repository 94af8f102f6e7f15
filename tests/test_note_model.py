"""The note model (pvq_note_model_*) as far as it goes without a GPU: the symbols, the argument checks and the host-only handle,
the derived sizes, what the compiler made of the kernels, and the one-row host function pvq_note_model_infer against
tests/note_model_ref.py, the float64 restatement of pitchvis_train/train.py:67-99.

Bar (tests/test_note_model_gpu.py holds the device to the same one): logits within 1e-5 * max|logit| of the f64 model, the project's
magnitude bar; probabilities within a quarter of that (the sigmoid's slope is <= 1/4) + 2e-7 (expf and the division round).  The
host function returns probabilities only, so it is held to the probability bar."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import note_model_ref as R
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import note_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_note_model_create", "pvq_note_model_destroy", "pvq_note_model_sizes", "pvq_note_model_infer",
           "pvq_note_model_rows_device", "pvq_note_model_set_workspace_limit")
LOGIT_REL, PROB_ABS = 1e-5, 2e-7
fp = C.POINTER(C.c_float)


def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("pvq_note_model_params", "pvq_note_model_weights", "pvq_note_model_outputs"):
        assert re.search(r"\}\s*%s;" % name, hdr), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.NoteModel is NM.NoteModel and P.NoteModelParams is NM.NoteModelParams


def _c_weights(w, layers):
    """(CNoteModelWeights, keep-alive) over the arrays of a state_dict-named dict"""
    cw = _lib.CNoteModelWeights()
    n = max(layers, 1)
    lw, lb = (fp * n)(), (fp * n)()
    for i in range(layers):
        lw[i], lb[i] = w[f"layers.{i}.weight"].ctypes.data_as(fp), w[f"layers.{i}.bias"].ctypes.data_as(fp)
    cw.conv_weight, cw.conv_bias = w["conv1.weight"].ctypes.data_as(fp), w["conv1.bias"].ctypes.data_as(fp)
    cw.fc1_weight, cw.fc1_bias = w["fc1.weight"].ctypes.data_as(fp), w["fc1.bias"].ctypes.data_as(fp)
    cw.output_weight, cw.output_bias = w["output.weight"].ctypes.data_as(fp), w["output.bias"].ctypes.data_as(fp)
    cw.layer_weight, cw.layer_bias = lw, lb
    return cw, (lw, lb)


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    w = R.weights("D")   # 180 bins, T 3, mlp 48, no hidden layer
    cw, _keep = _c_weights(w, 0)
    h = C.c_void_p()
    create = L.pvq_note_model_create

    def par(n_bins=180, t=3, mlp=48, layers=0):
        return C.byref(_lib.CNoteModelParams(n_bins, t, mlp, layers))
    assert create(-1, par(), C.byref(cw), None) == _lib.PVQ_ERR_INVALID_ARG
    for dev in (-1, 0):   # everything is rejected before any device is touched
        assert create(dev, None, C.byref(cw), C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, par(), None, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        for bad in (par(n_bins=0), par(t=0), par(mlp=0), par(mlp=40), par(mlp=1000)):
            assert create(dev, bad, C.byref(cw), C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        for bad in (par(n_bins=2), par(n_bins=1025), par(t=9), par(n_bins=3, t=2), par(n_bins=7, t=1), par(mlp=4112), par(layers=9)):
            assert create(dev, bad, C.byref(cw), C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
            assert L.pvq_last_error().decode()
        for field in ("conv_weight", "conv_bias", "fc1_weight", "fc1_bias", "output_weight", "output_bias"):
            cw2, _k2 = _c_weights(w, 0)
            setattr(cw2, field, None)
            assert create(dev, par(), C.byref(cw2), C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value, field
        cw2, _k2 = _c_weights(w, 0)
        cw2.layer_weight = None   # a hidden layer is asked for and its table is missing
        assert create(dev, par(layers=1), C.byref(cw2), C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        lw = (fp * 1)()           # ... or its entry
        cw2.layer_weight, cw2.layer_bias = lw, lw
        assert create(dev, par(layers=1), C.byref(cw2), C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    assert create(-1, par(n_bins=8, t=1, mlp=16), C.byref(cw), C.byref(h)) != _lib.PVQ_ERR_UNSUPPORTED   # the smallest window
    if h.value:
        L.pvq_note_model_destroy(h)
    assert create(-1, par(), C.byref(cw), C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        buf = np.zeros(4096, np.float32)   # stands for device memory; a host-only handle never dereferences it
        p = buf.ctypes.data
        rows = L.pvq_note_model_rows_device

        def outs(**kw):
            o = _lib.CNoteModelOutputs()
            for k, v in kw.items():
                setattr(o, k, v)
            return C.byref(o)
        nf = (C.c_size_t * 2)(5, 4)
        assert rows(None, p, nf, 2, 5, outs(d_prob=p), None) == _lib.PVQ_ERR_INVALID_ARG                       # null handle
        assert rows(h, None, nf, 2, 5, outs(d_prob=p), None) == _lib.PVQ_ERR_INVALID_ARG                       # null input
        assert rows(h, p, nf, 2, 5, outs(d_mask=p + 2), None) == _lib.PVQ_ERR_INVALID_ARG                      # the mask is stored as dwords
        assert "aligned" in L.pvq_last_error().decode()
        assert rows(h, p, nf, 2, 4, outs(d_prob=p), None) == _lib.PVQ_ERR_INVALID_ARG                          # n_frames[0] > stride_frames
        assert rows(h, p, nf, 2, 1 << 31, outs(d_prob=p), None) == _lib.PVQ_ERR_INVALID_ARG
        assert rows(h, p, nf, 2, 5, outs(d_prob=p, d_logits=p, d_mask=p), None) == _lib.PVQ_ERR_NO_DEVICE
        assert "GPU" in L.pvq_last_error().decode()
        assert rows(h, p, None, 2, 5, outs(d_mask=p), None) == _lib.PVQ_ERR_NO_DEVICE
        assert rows(h, p, nf, 2, 5, None, None) == _lib.PVQ_ERR_NO_DEVICE                                      # (checked before "nothing to do")
        out = np.zeros(128, np.float32)
        assert L.pvq_note_model_infer(None, buf.ctypes.data_as(fp), out.ctypes.data_as(fp)) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_note_model_infer(h, None, out.ctypes.data_as(fp)) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_note_model_infer(h, buf.ctypes.data_as(fp), None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_note_model_set_workspace_limit(None, 1 << 20) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_note_model_set_workspace_limit(h, 1 << 20) == _lib.PVQ_OK
        assert L.pvq_note_model_sizes(None, (C.c_uint32 * 4)()) == _lib.PVQ_ERR_INVALID_ARG
    finally:
        L.pvq_note_model_destroy(h)
    L.pvq_note_model_destroy(None)
    # the Python face
    m = P.NoteModel(P.NoteModelParams(180, 3, 48, 0), w, device=None)
    assert m.output_shape("d_mask", 2, 7) == ((2, 7, 4), np.uint32) and m.output_shape("d_prob", 2, 7) == ((2, 7, 128), np.float32)
    with pytest.raises(P.PvqError) as e:
        m.rows_device(buf.ctypes.data, [5, 4], 5, outputs={"d_prob": buf.ctypes.data}, n_streams=2)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        m.rows_device(buf.ctypes.data, [5, 4], 5, outputs={"nonsense": buf.ctypes.data}, n_streams=2)
    with pytest.raises(ValueError):
        m.rows_device(buf.ctypes.data, [5], 5, outputs={"d_prob": buf.ctypes.data}, n_streams=2)            # one count per stream
    with pytest.raises(ValueError):
        m.rows_device(buf.ctypes.data, outputs={"d_prob": buf.ctypes.data})                                 # raw pointer without sizes
    with pytest.raises(ValueError):
        m.infer(np.zeros(100, np.float32))
    with pytest.raises(ValueError):
        P.NoteModel(P.NoteModelParams(180, 3, 48, 1), w, device=None)                                       # layers.0 missing
    with pytest.raises(ValueError):
        P.NoteModel(P.NoteModelParams(180, 3, 40, 0), w, device=None)
    with pytest.raises(P.PvqError):
        P.NoteModel(P.NoteModelParams(1025, 3, 48, 0), w, device=None)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_derived_sizes(name):
    n_bins, T, mlp, layers, (o_conv, o_pool, n_feat) = R.SHAPES[name]
    assert R.sizes(n_bins, T) == (T * n_bins, o_conv, o_pool, n_feat)
    assert P.NoteModelParams(n_bins, T, mlp, layers).sizes() == (T * n_bins, o_conv, o_pool, n_feat)
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=None)   # what the library derives
    assert (m.window_len, m.o_conv, m.o_pool, m.n_features) == (T * n_bins, o_conv, o_pool, n_feat)
    m2 = P.NoteModel.from_state_dict(R.weights(name), n_bins, T, device=None)
    assert (m2.params.mlp_size, m2.params.mlp_layers) == (mlp, layers)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_host_infer_matches_f64_model(name):
    n_bins, T, mlp, layers, _ = R.SHAPES[name]
    w = R.weights(name)
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), w, device=None)
    win = R.db_like((6, T * n_bins), seed=77)
    win[5] = 0.0   # silence: the biases alone
    want = R.logits64(w, win)
    got = np.stack([m.infer(x) for x in win])
    assert got.dtype == np.float32 and got.shape == (6, 128)
    assert np.array_equal(m.infer(win[0].reshape(T, n_bins)), got[0])   # [T][n_bins] is the same window
    bar = 0.25 * LOGIT_REL * float(np.abs(want).max()) + PROB_ABS
    err = float(np.abs(got - R.sigmoid64(want)).max())
    print(f"shape {name}: host infer vs f64: max |dp| = {err:.2e} (bar {bar:.2e}), max |logit| = {np.abs(want).max():.3f}")
    assert err <= bar
    assert np.abs(want).max() > 0.1 and (want > 0).any() and (want < 0).any()   # the stimulus decides both ways


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """in the manner of test_render.py::test_kernel_resources: no scratch, LDS <= 80 KiB per workgroup (two fit a CU's 160 KiB),
    VGPRs + AGPRs <= 256 (two waves per SIMD).  Resource figures only."""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "note_model.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "x.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    kern = {k: u for k, u in usage.items() if "nm_conv_fc1" in k or "nm_dense" in k}
    assert sum("nm_conv_fc1" in k for k in kern) == 1 and sum("nm_dense" in k for k in kern) == 2, list(usage)
    for k, u in sorted(kern.items()):
        print(f"{k}: {u}")
        assert u["ScratchSize"] == 0, (k, u)
        assert u["LDS"] <= 80 * 1024, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (k, u)
