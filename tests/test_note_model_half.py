"""The note model's 16-bit precisions (pvq_note_model_create_precision, PVQ_NOTE_BF16 / PVQ_NOTE_F16) as far as they go without a
GPU: the rounding function, the handle and its refusals, the host face against tests/note_model_half_ref.py, the packed operand and
the workspace through a stand-alone program under ASan and UBSan, and what the compiler made of the kernels.

Bars of the host face (tests/test_note_model_half_gpu.py holds the device to the same ones), with L64 the unrounded float64 model
and Q64 the float64 model with the rule's rounding points:
  (a) max |logit - L64| <= 1.5 * max |Q64 - L64|: the path costs no more than the type itself costs;
  (b) rms(logit - Q64) <= 0.5 * rms(Q64 - L64): it rounds where the rule says, to nearest (truncation, or activations left in f32,
      lands near 1).
They are ratios and no fixed distances because a hidden activation whose f32 sum differs in its last bits can round to the
neighbouring 16-bit value: two correct implementations do not agree to accumulation accuracy.  The host face returns probabilities;
its logits are recovered in float64 (note_model_half_ref.logit_of), which costs under 2e-6 against a quantisation effect of 7e-5 and
more.  Every test prints the ratios before it asserts."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import note_model_half_ref as H
import note_model_ref as R
import note_plan_tool
import pitchvis_amd as P
from pitchvis_amd import _lib

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_note_model_create_precision", "pvq_note_model_precision", "pvq_note_round")
PREC = {"f32": 0, "bf16": 1, "f16": 2}
ALL_SHAPES = sorted(R.SHAPES) + sorted(R.EDGE_SHAPES)
fp = C.POINTER(C.c_float)


def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _same_bits(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)                       # NaN stays NaN (its payload is not part of the contract)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_note_round_is_torch_s_cast(precision):
    dt = H.DTYPES[precision]
    x = np.random.default_rng(5).integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    _same_bits(P.note_round(x, precision), torch.from_numpy(x).to(dt).float().numpy())
    assert np.array_equal(P.note_round(x, "f32").view(np.uint32), x.view(np.uint32))
    with pytest.raises(ValueError):
        P.note_round(x[:4], "fp8")


def test_note_round_edges():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    f16 = [  # (input, rounded)
        (1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9), (1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -10),   # ties to even, both ways
        (65504.0, 65504.0), (65519.99, 65504.0), (65520.0, inf), (-65520.0, -inf), (1e9, inf), (inf, inf),          # the overflow threshold
        (0.0, 0.0), (-0.0, -0.0),
        (2.0 ** -14, 2.0 ** -14), (2.0 ** -14 - 2.0 ** -25, 2.0 ** -14), (2.0 ** -24, 2.0 ** -24), (-2.0 ** -24, -2.0 ** -24),   # subnormals are kept
        (3 * 2.0 ** -25, 2.0 ** -23), (5 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -25, 0.0), (-2.0 ** -25, -0.0), (2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -24),
        (1e-40, 0.0),
    ]
    bf16 = [
        (1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6), (1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -7),
        (float(_f(0x7f7f0000)), float(_f(0x7f7f0000))), (float(_f(0x7f7f7fff)), float(_f(0x7f7f0000))), (float(_f(0x7f7f8000)), inf),
        (float(_f(0x7f7fffff)), inf), (float(_f(0xff7fffff)), -inf), (inf, inf),
        (0.0, 0.0), (-0.0, -0.0), (float(_f(0x00010000)), float(_f(0x00010000))), (float(_f(0x00008000)), 0.0), (float(_f(0x00018000)), float(_f(0x00020000))),
    ]
    for precision, table in (("f16", f16), ("bf16", bf16)):
        x = np.array([a for a, _ in table], np.float32)
        want = np.array([b for _, b in table], np.float32)
        got = P.note_round(x, precision)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (precision, x[got.view(np.uint32) != want.view(np.uint32)])
        _same_bits(got, torch.from_numpy(x).to(H.DTYPES[precision]).float().numpy())
        assert np.isnan(P.note_round(np.array([nan, -nan], np.float32), precision)).all()
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "pvq.h")).read())
    assert "rounds to a multiple of 2^-24 and is not flushed" in hdr      # what the header says of f16 subnormals is what is done
    # the C entry: in may be out; an unknown precision and a null pointer are refused
    L = _lib.load()
    buf = np.array([1 + 2.0 ** -8, 3.0], np.float32)
    assert L.pvq_note_round(1, buf.ctypes.data_as(fp), 2, buf.ctypes.data_as(fp)) == _lib.PVQ_OK and buf.tolist() == [1.0, 3.0]
    assert L.pvq_note_round(3, buf.ctypes.data_as(fp), 2, buf.ctypes.data_as(fp)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_note_round(1, None, 2, buf.ctypes.data_as(fp)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_note_round(1, None, 0, None) == _lib.PVQ_OK


def test_symbols_and_handles():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"typedef enum \{ PVQ_NOTE_F32 = 0, PVQ_NOTE_BF16 = 1, PVQ_NOTE_F16 = 2 \} pvq_note_precision;", hdr)
    assert L.pvq_abi_version() == 4   # additive
    n_bins, T, mlp, layers, _ = R.shape("D")
    w = R.weights("D")
    from pitchvis_amd.note_model import _c_weights
    par = _lib.CNoteModelParams(n_bins, T, mlp, layers)
    cw, _keep = _c_weights(P.NoteModelParams(n_bins, T, mlp, layers), w)
    h = C.c_void_p()
    create = L.pvq_note_model_create_precision
    for dev in (-1, 0):   # refused before any device is touched
        for bad in (3, -1, 77):
            assert create(dev, C.byref(par), C.byref(cw), bad, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "precision" in L.pvq_last_error().decode()
        assert create(dev, C.byref(par), C.byref(cw), 1, None) == _lib.PVQ_ERR_INVALID_ARG
        assert create(dev, None, C.byref(cw), 2, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        # an f16 weight of 7e4 is refused with its layer named; bf16 and f32 take it
        for key, layer in (("fc1.weight", "fc1.weight"), ("output.weight", "output.weight")):
            w2 = {k: v.copy() for k, v in w.items()}
            w2[key].reshape(-1)[-1] = -7e4
            cw2, _keep2 = _c_weights(P.NoteModelParams(n_bins, T, mlp, layers), w2)
            assert create(dev, C.byref(par), C.byref(cw2), 2, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert layer in L.pvq_last_error().decode() and "65504" in L.pvq_last_error().decode()
    w2 = {k: v.copy() for k, v in R.weights("C").items()}
    w2["layers.1.weight"][3, 5] = 7e4
    pc = P.NoteModelParams(*R.shape("C")[:4])
    with pytest.raises(ValueError, match=r"layers\.1\.weight"):
        P.NoteModel(pc, w2, device=None, precision="f16")
    w2["layers.1.weight"][3, 5] = 65504.0     # the largest finite f16 is a weight like any other
    assert P.NoteModel(pc, w2, device=None, precision="f16").precision == "f16"
    w2["layers.1.weight"][3, 5] = 7e4
    assert P.NoteModel(pc, w2, device=None, precision="bf16").precision == "bf16"
    with pytest.raises(ValueError):
        P.NoteModel(pc, w2, device=None, precision="half")
    # the query, and the f32 handle of the new entry: the bits of pvq_note_model_create's
    win = R.db_like((3, T * n_bins), seed=78)
    old = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), w, device=None)
    assert old.precision == "f32"
    for name, value in PREC.items():
        assert create(-1, C.byref(par), C.byref(cw), value, C.byref(h)) == _lib.PVQ_OK and h.value
        try:
            got = C.c_int(-1)
            assert L.pvq_note_model_precision(h, C.byref(got)) == _lib.PVQ_OK and got.value == value
            assert L.pvq_note_model_precision(None, C.byref(got)) == _lib.PVQ_ERR_INVALID_ARG
            assert L.pvq_note_model_precision(h, None) == _lib.PVQ_ERR_INVALID_ARG
            s4 = (C.c_uint32 * 4)()
            assert L.pvq_note_model_sizes(h, s4) == _lib.PVQ_OK and tuple(s4) == R.sizes(n_bins, T)
            out = np.zeros((3, 128), np.float32)
            for i in range(3):
                assert L.pvq_note_model_infer(h, win[i].ctypes.data_as(fp), out[i].ctypes.data_as(fp)) == _lib.PVQ_OK
            same = np.array_equal(out.view(np.uint32), np.stack([old.infer(x) for x in win]).view(np.uint32))
            assert same == (name == "f32")
            # a host-only handle of any precision: the argument checks, then PVQ_ERR_NO_DEVICE
            o = _lib.CNoteModelOutputs()
            o.d_prob = win.ctypes.data
            assert L.pvq_note_model_rows_device(h, None, None, 1, 3, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG
            assert L.pvq_note_model_rows_device(h, win.ctypes.data, None, 1, 3, C.byref(o), None) == _lib.PVQ_ERR_NO_DEVICE
            assert L.pvq_note_model_set_workspace_limit(h, 1 << 20) == _lib.PVQ_OK
        finally:
            L.pvq_note_model_destroy(h)
            h = C.c_void_p()
    m = P.NoteModel.from_state_dict(w, n_bins, T, device=None, precision="bf16")
    assert m.precision == "bf16" and (m.params.mlp_size, m.params.mlp_layers) == (mlp, layers)


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_host_infer_under_the_bars(name, precision):
    n_bins, T, mlp, layers, _ = R.shape(name)
    w = R.weights(name)
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), w, device=None, precision=precision)
    win = R.db_like((8, T * n_bins), seed=11)
    l64, q64 = R.logits64(w, win), H.logits_q64(w, win, precision)
    got = H.logit_of(np.stack([m.infer(x) for x in win]))
    a, b, quant = H.ratios(got, q64, l64)
    top = float(np.abs(l64).max())
    print(f"shape {name} {precision}: max |L64| {top:.3f}; max |Q64 - L64| = {quant:.2e} = {quant / top:.2e} of it; (a) {a:.3f} (bar {H.BAR_A}); (b) {b:.3f} (bar {H.BAR_B})")
    assert a <= H.BAR_A
    assert b <= H.BAR_B


# ---- the packed operand and the workspace, through the stand-alone program ----
@pytest.fixture(scope="module")
def half_tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    return note_plan_tool.build(tmp_path_factory.mktemp("note_half_plan"), main="note_half_plan_main.cpp", units=("note_model_plan.cpp",))


def _fill16(i):
    """element i of a matrix the program makes: (i % 255 + 1) * 2^((i / 255) % 16 - 8), exact in bf16 and f16, never zero"""
    i = np.asarray(i, np.int64)
    return np.ldexp((i % 255 + 1).astype(np.float32), ((i // 255) % 16 - 8).astype(np.int32)).astype(np.float32)


def _bits16(x, precision):
    x = np.ascontiguousarray(x, np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16) if precision == "bf16" else x.astype(np.float16).view(np.uint16)


def _packed16_as_the_lanes_read_it(n, k, conv_order, o_pool, precision):
    """The operand as nmh_dense reads it, restated from the kernel: column tile ct, chunk kc, strip s, lane l: the 16-byte word at
    ((ct * chunks_padded + kc) * 4 + s) * 64 + l, whose element j meets activation k' = 32 kc + 8 (l >> 4) + j.  The word is the
    instruction's A operand: matrix row l & 15 = 4 g' + r' of strip s, which the accumulator layout hands to lane group g' as
    register r': output column 64 ct + 16 g' + 4 s + r'.  In conv order k' = 16 p + c is feature c * o_pool + p.
    -> [n_ct][chunks_padded][4][64][8] with zeros at k' >= k, in padded chunks and at columns >= n; (chunks, chunks_padded)"""
    n_ct, chunks = -(-n // 64), -(-k // 32)
    padded = -(-chunks // 4) * 4
    want = np.zeros((n_ct, padded, 4, 64, 8), np.uint16)
    ct, kc, s, l, j = np.ogrid[0:n_ct, 0:chunks, 0:4, 0:64, 0:8]
    col = 64 * ct + 16 * ((l & 15) >> 2) + 4 * s + (l & 3)
    kk = 32 * kc + 8 * (l >> 4) + j
    src = (kk % 16) * o_pool + kk // 16 if conv_order else kk
    real = (col < n) & (kk < k)
    val = _fill16(np.minimum(col, n - 1).astype(np.int64) * k + np.minimum(src, k - 1))
    want[:, :chunks] = np.where(real, _bits16(val, precision).reshape(val.shape), np.uint16(0))
    return want, chunks, real


@pytest.mark.parametrize("name,precision", [(n, "bf16") for n in ALL_SHAPES] + [(n, "f16") for n in "CGHI"])
def test_pack_b16_puts_every_element_where_its_lane_reads_it(name, precision, half_tool, tmp_path):
    """note_model_pack_b16 for the three kinds of matrix of a shape: fc1 (conv order), a hidden layer, the output layer.  K with a half
    chunk: 16 (G's fc1; mlp 16 of G and J), 720 (H), 752 (I), 32752 (J's fc1: 2047 pooled positions), 80 (C), 48 (D), 112 (I)."""
    n_bins, T, mlp, layers, (_, o_pool, n_feat) = R.shape(name)
    products = [("fc1", mlp, n_feat, 1, o_pool), ("output", 128, mlp, 0, 0)] + ([("layer", mlp, mlp, 0, 0)] if layers else [])
    for what, n, k, conv_order, op in products:
        path = str(tmp_path / (what + ".u16"))
        note_plan_tool.run(half_tool, "pack16", n, k, conv_order, op, PREC[precision], path)
        want, chunks, real = _packed16_as_the_lanes_read_it(n, k, conv_order, op, precision)
        got = np.fromfile(path, np.uint16)
        os.remove(path)
        assert got.size == want.size, (what, got.size, want.shape)
        got = got.reshape(want.shape)
        print(f"shape {name} {precision} {what}: W [{n}][{k}] -> {want.shape[0]} column tiles x {want.shape[1]} chunks ({want.shape[1] - chunks} padded, "
              f"half chunk: {k % 32 == 16}), {int((want == 0).sum())} zeros of {want.size}")
        assert not got[:, chunks:].any()                       # the padded chunks of the last stage
        assert not got[:, :chunks][~np.broadcast_to(real, got[:, :chunks].shape)].any()   # the padded half chunk, the columns past n
        assert np.array_equal(got, want)
        assert int((got != 0).sum()) == n * k                  # every element of W exactly once (fill16 is never zero)


def _ws(tool, shape_name, limit, stride, *n_frames, precision=None):
    """the 16-bit layout ("ws"), or that of the precision named ("wsp")"""
    n_bins, T, mlp, layers, _ = R.shape(shape_name)
    cmd = ("ws",) if precision is None else ("wsp", PREC[precision])
    lines = note_plan_tool.run(tool, *cmd, n_bins, T, mlp, layers, limit, stride, *n_frames).splitlines()
    head = lines[0].split()
    return dict(zip(head[0::2], map(int, head[1::2]))), [tuple(map(int, x.split())) for x in lines[1:]]


def test_workspace_cut_of_three_tiles_in_one_stream(half_tool):
    """shape I (n_features 752 -> 768, mlp 112 -> 128), one stream of T + 256 frames: tiles of 128, 128 and 1 rows.  A tile is 128 rows x
    2 bytes x (768 + 2 * 128) = 256 KiB; the table of three entries takes 256 bytes."""
    T = R.shape("I")[1]
    tile = 128 * 2 * (768 + 2 * 128)
    for limit, cut in ((0, [(0, 1), (1, 1), (2, 1)]), (256 + tile, [(0, 1), (1, 1), (2, 1)]), (256 + 2 * tile - 1, [(0, 1), (1, 1), (2, 1)]),
                       (256 + 2 * tile, [(0, 2), (2, 1)]), (256 + 3 * tile, [(0, 3)]), (256 << 20, [(0, 3)])):
        w, chunks = _ws(half_tool, "I", limit, T + 260, T + 256)
        ct = cut[0][1]
        assert chunks == cut, (limit, chunks)
        assert (w["tiles"], w["tab"], w["tile"], w["chunk_tiles"], w["kf_pad"], w["mlp_pad"]) == (3, 256, tile, ct, 768, 128)
        assert (w["feat_at"], w["h0_at"], w["h1_at"], w["total"]) == (256, 256 + ct * 128 * 2 * 768, 256 + ct * 128 * 2 * (768 + 128), 256 + ct * tile)
    # whole rows: G (16 features, mlp 16 -> 32 each), A (5024 -> 5024, 1024), J (32752 -> 32768)
    for name, kf, mp in (("G", 32, 32), ("A", 5024, 1024), ("J", 32768, 32)):
        T = R.shape(name)[1]
        w, chunks = _ws(half_tool, name, 256 << 20, T + 260, T + 256, T + 31, T - 1)
        assert (w["tiles"], w["kf_pad"], w["mlp_pad"], w["tile"]) == (4, kf, mp, 256 * (kf + 2 * mp)) and chunks == [(0, 4)]
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "pvq.h")).read())
    assert "256 * (pad32(n_features) + 2 * pad32(mlp_size)) bytes" in hdr


def test_f32_workspace_cut_of_three_tiles_in_one_stream(half_tool):
    """the same call for an f32 handle: shape I (mlp 112), one stream of T + 256 frames, tiles of 128, 128 and 1 rows.  A tile is two
    hidden buffers of 128 rows x 112 floats = 114 688 bytes; the table takes 256 bytes; the 16-bit path's fields stay zero."""
    T = R.shape("I")[1]
    tile = 2 * 128 * 112 * 4
    assert tile == 114688
    for limit, cut in ((0, [(0, 1), (1, 1), (2, 1)]), (256 + tile, [(0, 1), (1, 1), (2, 1)]), (256 + 2 * tile - 1, [(0, 1), (1, 1), (2, 1)]),
                       (256 + 2 * tile, [(0, 2), (2, 1)]), (256 + 3 * tile, [(0, 3)]), (256 << 20, [(0, 3)])):
        w, chunks = _ws(half_tool, "I", limit, T + 260, T + 256, precision="f32")
        ct = cut[0][1]
        assert chunks == cut, (limit, chunks)
        assert (w["tiles"], w["tab"], w["tile"], w["chunk_tiles"]) == (3, 256, tile, ct)
        assert w["total"] == 256 + ct * tile
        assert (w["h0_at"], w["h1_at"]) == (256, 256 + ct * tile // 2)      # the two buffers, back to back behind the table
        assert (w["feat_at"], w["kf_pad"], w["mlp_pad"]) == (0, 0, 0)


def test_workspace_grid_cap(half_tool):
    """shape K (mlp 4096: 64 column tiles; 32 features -> pad32 32, two pooled positions: one block per row, 128 per tile), 40 000 000
    tiles under no limit: a chunk is what a launch's grid of 2^31 - 1 blocks takes.  Planning only."""
    n_bins, T, mlp, layers, _ = R.shape("K")
    cap = {name: int(note_plan_tool.run(half_tool, "cap", PREC[name], n_bins, T, mlp, layers, 40_000_000)) for name in PREC}
    print(cap)
    assert cap["f32"] == 0x7fffffff // 64 == 33_554_431
    assert cap["bf16"] == 0x7fffffff // 128 == 16_777_215
    assert cap["f16"] == cap["bf16"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """what DESIGN.md section 6b states of the 16-bit kernels: no scratch; nmh_dense 32 KiB of LDS and at least two waves per SIMD
    (VGPRs + AGPRs <= 256); nmh_features no LDS and eight waves per SIMD.  Both types, every instantiation."""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "note_model_half.hip")
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
    dense = {k: u for k, u in usage.items() if "nmh_dense" in k}
    feat = {k: u for k, u in usage.items() if "nmh_features" in k}
    assert len(dense) == 4 and len(feat) == 2, list(usage)
    for k, u in sorted(dense.items()):
        print(f"{k}: {u}")
        assert u["ScratchSize"] == 0 and u["LDS"] == 32 * 1024, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256 and u["Occupancy"] >= 2, (k, u)
    for k, u in sorted(feat.items()):
        print(f"{k}: {u}")
        assert u["ScratchSize"] == 0 and u["LDS"] == 0 and u["Occupancy"] == 8, (k, u)
