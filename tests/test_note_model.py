"""The note model (pvq_note_model_*) as far as it goes without a GPU: the symbols, the argument checks and the host-only handle,
the derived sizes, what the compiler made of the kernels, and the one-row host function pvq_note_model_infer against
tests/note_model_ref.py, the float64 restatement of pitchvis_train/train.py:67-99.

Bar (tests/test_note_model_gpu.py holds the device to the same one): logits within 1e-5 * max|logit| of the f64 model, the project's
magnitude bar; probabilities within a quarter of that (the sigmoid's slope is <= 1/4) + 2e-7 (expf and the division round).  The
host function returns probabilities only, so it is held to the probability bar."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import note_model_ref as R
import note_plan_tool
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import note_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_note_model_create", "pvq_note_model_destroy", "pvq_note_model_sizes", "pvq_note_model_infer",
           "pvq_note_model_rows_device", "pvq_note_model_set_workspace_limit")
LOGIT_REL, PROB_ABS = 1e-5, 2e-7
fp = C.POINTER(C.c_float)
ALL_SHAPES = sorted(R.SHAPES) + sorted(R.EDGE_SHAPES)


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    return note_plan_tool.build(tmp_path_factory.mktemp("note_plan"))


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


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_derived_sizes(name):
    n_bins, T, mlp, layers, (o_conv, o_pool, n_feat) = R.shape(name)
    assert R.sizes(n_bins, T) == (T * n_bins, o_conv, o_pool, n_feat)
    assert P.NoteModelParams(n_bins, T, mlp, layers).sizes() == (T * n_bins, o_conv, o_pool, n_feat)
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=None)   # what the library derives
    assert (m.window_len, m.o_conv, m.o_pool, m.n_features) == (T * n_bins, o_conv, o_pool, n_feat)
    m2 = P.NoteModel.from_state_dict(R.weights(name), n_bins, T, device=None)
    assert (m2.params.mlp_size, m2.params.mlp_layers) == (mlp, layers)


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_host_infer_matches_f64_model(name):
    n_bins, T, mlp, layers, _ = R.shape(name)
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


def _packed_as_the_lanes_read_it(n, k, conv_order, o_pool):
    """The B operand as nm_conv_fc1 / nm_dense read it, restated from the kernels: column tile ct, stage st, chunk i of it (kc = 4 st +
    i), strip s, lane l: the float4 at ((ct * stages + st) * 4 + i) * 256 + s * 64 + l, whose element j is the operand of the chunk's j-th
    v_mfma_f32_16x16x4_f32.  The lane supplies column 64 ct + 16 s + (l & 15) and meets the A element of k index 4 (l >> 4) + j of the
    chunk: activation 16 kc + 4 (l >> 4) + j (nm_dense), or channel 4 (l >> 4) + j of pooled position kc, feature (4 (l >> 4) + j)
    o_pool + kc (nm_conv_fc1).  -> [n_ct][stages * 4][4][64][4] with zeros in padded chunks and columns >= n, and the chunk count"""
    n_ct, chunks = -(-n // 64), k // 16
    stages = -(-chunks // 4)
    want = np.zeros((n_ct, stages * 4, 4, 64, 4), np.float32)
    ct, kc, s, l, j = np.ogrid[0:n_ct, 0:chunks, 0:4, 0:64, 0:4]
    col = 64 * ct + 16 * s + (l & 15)
    kk = 4 * (l >> 4) + j
    src = kk * o_pool + kc if conv_order else 16 * kc + kk
    want[:, :chunks] = np.where(col < n, note_plan_tool.fill(np.minimum(col, n - 1).astype(np.int64) * k + src), np.float32(0.0))
    return want, chunks


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_pack_b_puts_every_element_where_its_lane_reads_it(name, plan_tool, tmp_path):
    """note_model_pack_b for the three kinds of matrix of a shape: fc1 (conv order), a hidden layer, the output layer.  Every real
    element at its lane's place, every padded chunk (edge shapes: 3 for O_pool = 1 and 45, 1 for 47 and 2047, 2 for 2; 3 for mlp 16, 1
    for mlp 112) and every column past n (mlp 16, 48, 80, 112: strips of the last column tile) zero."""
    n_bins, T, mlp, layers, (_, o_pool, n_feat) = R.shape(name)
    products = [("fc1", mlp, n_feat, 1, o_pool), ("output", 128, mlp, 0, 0)] + ([("layer", mlp, mlp, 0, 0)] if layers else [])
    for what, n, k, conv_order, op in products:
        path = str(tmp_path / (what + ".f32"))
        note_plan_tool.run(plan_tool, "pack", n, k, conv_order, op, path)
        want, chunks = _packed_as_the_lanes_read_it(n, k, conv_order, op)
        got = np.fromfile(path, np.float32)
        os.remove(path)
        assert got.size == want.size, (what, got.size, want.shape)
        got = got.reshape(want.shape)
        pad = got[:, chunks:]
        print(f"shape {name} {what}: W [{n}][{k}] -> {want.shape[0]} column tiles x {want.shape[1]} chunks ({want.shape[1] - chunks} padded), "
              f"{int((want == 0).sum())} zeros of {want.size}")
        assert not pad.any()                                   # the padded chunks of the last stage
        assert np.array_equal(got, want)
        assert int((got != 0).sum()) == n * k                  # every element of W exactly once (fill() is never zero)


def _tiles(plan_tool, T, stride, *rest):
    return [tuple(map(int, line.split())) for line in note_plan_tool.run(plan_tool, "tiles", T, stride, *rest).splitlines()]


@pytest.mark.parametrize("T", [1, 3, 5, 8])
def test_tiles_of_a_stream_with_three(T, plan_tool):
    """the edge call of tests/test_note_model_gpu.py: 257, 32, 33, 97 and 0 model rows -> 3 + 1 + 1 + 1 + 0 tiles"""
    n_frames, stride = [T + 256, T + 31, T + 32, T + 96, T - 1], T + 260
    got = _tiles(plan_tool, T, stride, *n_frames)
    want = [(0, T - 1, 128, 0), (0, T - 1 + 128, 128, 0), (0, T - 1 + 256, 1, 0), (1, T - 1, 32, 0), (2, T - 1, 33, 0), (3, T - 1, 97, 0)]
    assert got == want
    # the calls of shapes A - F: 1, 65, 129, 0 rows; a stream of exactly two tiles; no counts: every stream has stride frames
    assert _tiles(plan_tool, T, T + 130, T, T + 64, T + 128, T - 1) == [(0, T - 1, 1, 0), (1, T - 1, 65, 0), (2, T - 1, 128, 0), (2, T + 127, 1, 0)]
    assert _tiles(plan_tool, T, T + 255, T + 255, 0) == [(0, T - 1, 128, 0), (0, T + 127, 128, 0)]
    assert _tiles(plan_tool, T, T + 128, "x2") == [(0, T - 1, 128, 0), (0, T + 127, 1, 0), (1, T - 1, 128, 0), (1, T + 127, 1, 0)]
    for s, f0, n_valid, _ in got:       # what the kernels rely on: every row of a tile is a model row of its stream
        assert 1 <= n_valid <= 128 and f0 >= T - 1 and f0 + n_valid <= n_frames[s]


def test_admitted_sizes_are_the_header_s():
    """pvq_note_model_create and pvq_note_trainer_create (host-only handles) at every corner the edge shapes use, and one past each:
    n_bins 3 .. 1024, T 1 .. 8 with T n_bins >= 8, mlp 16 .. 4096 in multiples of 16, 0 .. 8 hidden layers (include/pvq.h)"""
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    assert re.search(r"n_bins 3 \.\. 1024; t_frames 1 \.\. 8 with t_frames \* n_bins >= 8; mlp_size a multiple of 16\s*\*?\s*in 16 \.\. 4096; mlp_layers 0 \.\. 8", hdr)
    for name in sorted(R.EDGE_SHAPES):      # the corners: 3 and 1024 bins, T 1 and 8, L = 9, mlp 16 and 4096, 0 and 8 layers
        n_bins, T, mlp, layers, _ = R.shape(name)
        m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=None)
        t = P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), None, 8, device=None)
        assert m.window_len == T * n_bins and t.n_params == sum(v.size for v in R.weights(name).values())
    w8 = {"conv1.weight": np.zeros((16, 1, 5), np.float32), "conv1.bias": np.zeros(16, np.float32), "fc1.weight": np.zeros((16, 16), np.float32),
          "fc1.bias": np.zeros(16, np.float32), "output.weight": np.zeros((128, 16), np.float32), "output.bias": np.zeros(128, np.float32)}
    assert P.NoteModel(P.NoteModelParams(8, 1, 16, 0), w8, device=None).o_pool == 1      # the smallest window: 8 values
    assert P.NoteModel(P.NoteModelParams(4, 2, 16, 0), w8, device=None).o_pool == 1
    big = np.zeros(1 << 20, np.float32)     # stands for every weight: a refused create reads none
    cw = _lib.CNoteModelWeights()
    lw = (fp * 9)(*[big.ctypes.data_as(fp)] * 9)
    for field in ("conv_weight", "conv_bias", "fc1_weight", "fc1_bias", "output_weight", "output_bias"):
        setattr(cw, field, big.ctypes.data_as(fp))
    cw.layer_weight, cw.layer_bias = lw, lw
    ch = P.NoteTrainerHyper()._c()
    past = {"2 bins": (2, 4, 16, 0), "1025 bins": (1025, 1, 16, 0), "T = 9": (3, 9, 16, 0), "T n_bins = 7": (7, 1, 16, 0), "mlp 0": (3, 3, 0, 0),
            "mlp 8": (3, 3, 8, 0), "mlp 4112": (3, 3, 4112, 0), "9 layers": (3, 3, 16, 9)}
    for what, par in past.items():
        for dev in (-1, 0):                 # refused before any device is touched
            h = C.c_void_p()
            st = L.pvq_note_model_create(dev, C.byref(_lib.CNoteModelParams(*par)), C.byref(cw), C.byref(h))
            msg = L.pvq_last_error().decode()
            h2 = C.c_void_p()
            st2 = L.pvq_note_trainer_create(dev, C.byref(_lib.CNoteModelParams(*par)), C.byref(cw), C.byref(ch), 8, C.byref(h2))
            print(f"{what}: model {st}, trainer {st2}: {msg}")
            assert st in (_lib.PVQ_ERR_UNSUPPORTED, _lib.PVQ_ERR_INVALID_ARG) and not h.value and msg, what
            assert st2 == st and not h2.value, what


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
