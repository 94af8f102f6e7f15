"""The note model's 16-bit precisions on the GPU (pvq_note_model_rows_device on a PVQ_NOTE_BF16 / PVQ_NOTE_F16 handle) against
tests/note_model_half_ref.py.  Shapes: the existing tables, which already sit on the tails of the 32-wide K chunk — G (K = 16 in fc1,
mlp 16: every product half a chunk), H (O_pool 45, eight hidden layers), I (mlp 112: three column strips, 3.5 chunks), C (mlp 80), K
(mlp 4096, O_pool 2), J (L = 8192), A and B (the trainer's and the viewer's models).  One call per shape and type of five streams
with 257, 32, 33, 97 and 0 model rows, as tests/test_note_model_gpu.py's edge call, with guard regions after every output.

Bars per case, with L64 the unrounded float64 model, Q64 the float64 model with the rule's rounding points (include/pvq.h) and
m = max |L64|:
  (a) max |device - L64| <= 1.5 * max |Q64 - L64|: the path costs no more than the type itself costs;
  (b) rms(device - Q64) <= 0.5 * rms(Q64 - L64): the device rounds where the rule says, to nearest (truncation, or activations left
      in f32, lands near 1);
  mask bit k == (device logit_k > 0) exactly; == (L64_k > 0) outside the band |L64| <= 2 * max |Q64 - L64|, and at most 10 % (bf16) or
  2 % (f16) of the decisions lie inside the band;
  probabilities within 0.25 * max |device - L64| + 2e-7 of the sigmoid of the device's own logits.
(a) and (b) are ratios because a hidden activation whose f32 sum differs in its last bits can round to the neighbouring 16-bit value:
two correct implementations do not agree to accumulation accuracy.  The factors leave room for the matrix instruction's own
summation order.  Every test prints its figures before it asserts; DESIGN.md section 6b records them."""
import functools

import numpy as np
import pytest

import note_model_half_ref as H
import note_model_ref as R
import pitchvis_amd as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = ["A", "B", "C", "G", "H", "I", "J", "K"]
PRECISIONS = ["bf16", "f16"]
BAND_SHARE = {"bf16": 0.10, "f16": 0.02}
PROB_ABS = 2e-7
GUARD = 1024   # elements after each output that no kernel may touch


def _layout(name):
    T = R.shape(name)[1]
    return [T + 256, T + 31, T + 32, T + 96, T - 1], T + 260


@functools.lru_cache(maxsize=None)
def _model(name, precision):
    n_bins, T, mlp, layers, _ = R.shape(name)
    return P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=0, precision=precision)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """the dB rows of a shape's call and the unrounded f64 model on them, shared by both types"""
    n_bins, T, _, _, _ = R.shape(name)
    n_frames, stride = _layout(name)
    db = R.db_like((len(n_frames), stride, n_bins), seed=500 + ord(name))
    want, valid = R.rows64(R.weights(name), db, n_frames, T)
    for a in (db, want, valid):
        a.setflags(write=False)
    return db, want, valid


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf


@functools.lru_cache(maxsize=None)
def _run(name, precision):
    db, l64, valid = _inputs(name)
    n_frames, stride = _layout(name)
    S = len(n_frames)
    prob, prob_all = _guarded((S, stride, 128), torch.float32, 7.0)
    logits, logits_all = _guarded((S, stride, 128), torch.float32, 7.0)
    mask, mask_all = _guarded((S, stride, 4), torch.int32, -1)
    _model(name, precision).rows_device(torch.from_numpy(db).cuda(), n_frames, stride, {"d_prob": prob, "d_logits": logits, "d_mask": mask})
    torch.cuda.synchronize()
    q64 = H.rows_q64(R.weights(name), db, n_frames, R.shape(name)[1], precision)
    q64.setflags(write=False)
    return dict(prob=prob.cpu().numpy(), logits=logits.cpu().numpy(), mask=mask.cpu().numpy().view(np.uint32), q64=q64,
                guards=(prob_all[-GUARD:].cpu().numpy(), logits_all[-GUARD:].cpu().numpy(), mask_all[-GUARD:].cpu().numpy()))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", SHAPES)
def test_rows_under_the_bars(name, precision):
    db, l64, valid = _inputs(name)
    r = _run(name, precision)
    assert valid.sum(axis=1).tolist() == [257, 32, 33, 97, 0]
    got, q64 = r["logits"].astype(np.float64)[valid], r["q64"][valid]
    a, b, quant = H.ratios(got, q64, l64[valid])
    top = float(np.abs(l64).max())
    dev = float(np.abs(got - l64[valid]).max())
    perr = float(np.abs(r["prob"].astype(np.float64) - R.sigmoid64(r["logits"].astype(np.float64)))[valid].max())
    bits = R.mask_bits(r["mask"])
    band = np.abs(l64) <= 2.0 * quant
    inside = int(band[valid].sum())
    n_dec = int(valid.sum()) * 128
    flips = int(((bits != (l64 > 0)) & ~band)[valid].sum())
    print(f"shape {name} {precision}: max |L64| {top:.3f}; max |Q64 - L64| {quant:.2e} = {quant / top:.2e} of it; (a) {a:.3f} (bar {H.BAR_A}); "
          f"(b) {b:.3f} (bar {H.BAR_B}); prob vs sigmoid(own logits) {perr:.2e} (bar {0.25 * dev + PROB_ABS:.2e}); "
          f"{inside} of {n_dec} decisions inside the band = {inside / n_dec:.2%} (cap {BAND_SHARE[precision]:.0%}), {flips} flips outside")
    assert a <= H.BAR_A
    assert b <= H.BAR_B
    assert perr <= 0.25 * dev + PROB_ABS
    assert np.array_equal(bits, r["logits"] > 0)          # the mask is the sign of the logits of the same call, exactly
    assert flips == 0 and inside <= BAND_SHARE[precision] * n_dec
    assert bits[valid].any() and not bits[valid].all()    # both decisions occur


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", SHAPES)
def test_rows_outside_a_stream_are_zero_and_nothing_else_is_written(name, precision):
    _, _, valid = _inputs(name)
    r = _run(name, precision)
    out = ~valid
    T = R.shape(name)[1]
    assert out[:, :T - 1].all() and out[-1].all() and out.sum() == out.shape[0] * out.shape[1] - 419
    assert not r["prob"][out].any() and not r["logits"][out].any() and not r["mask"][out].any()
    assert (r["prob"][valid] > 0).all()                   # (a model row is never all zero: sigmoid > 0)
    gp, gl, gm = r["guards"]
    assert (gp == 7.0).all() and (gl == 7.0).all() and (gm == -1).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["J", "K"])
def test_chunked_call_equals_the_whole_call(name, precision):
    """6 tiles (3 + 1 + 1 + 1 + 0): a workspace limit of one tile of the 16-bit layout makes 6 chunks, the third the one-row tile"""
    db, _, _ = _inputs(name)
    r = _run(name, precision)
    n_bins, T, mlp, layers, (_, _, n_feat) = R.shape(name)
    n_frames, stride = _layout(name)
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=0, precision=precision)
    pad32 = lambda k: -(-k // 32) * 32
    m.set_workspace_limit(256 * (pad32(n_feat) + 2 * pad32(mlp)) + 256)     # one 128-row tile and the table
    d_db = torch.from_numpy(db).cuda()
    o = m.rows_device(d_db, n_frames, stride)
    only = m.rows_device(d_db, n_frames, stride, outputs=("d_mask",))
    torch.cuda.synchronize()
    assert np.array_equal(o["d_logits"].cpu().numpy().view(np.uint32), r["logits"].view(np.uint32))
    assert np.array_equal(o["d_prob"].cpu().numpy().view(np.uint32), r["prob"].view(np.uint32))
    assert np.array_equal(o["d_mask"].cpu().numpy().view(np.uint32), r["mask"])
    assert list(only) == ["d_mask"] and np.array_equal(only["d_mask"].cpu().numpy().view(np.uint32), r["mask"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bits_do_not_depend_on_place(precision):
    """shape H: the same window as row T - 1 of one stream and as row T - 1 + 200 of another: the second tile, its third wave"""
    n_bins, T, _, _, _ = R.shape("H")
    m = _model("H", precision)
    stride = T + 210
    db = R.db_like((2, stride, n_bins), seed=902)
    db[1, 200:200 + T] = db[0, 0:T]          # row (1, 200 + T - 1) sees what row (0, T - 1) sees
    o = m.rows_device(torch.from_numpy(db).cuda(), [T + 3, stride], stride)
    torch.cuda.synchronize()
    lg, pr = o["d_logits"].cpu().numpy(), o["d_prob"].cpu().numpy()
    assert lg[0, T - 1].any()
    assert np.array_equal(lg[0, T - 1].view(np.uint32), lg[1, 200 + T - 1].view(np.uint32))
    assert np.array_equal(pr[0, T - 1].view(np.uint32), pr[1, 200 + T - 1].view(np.uint32))
    assert not np.array_equal(lg[0, T - 1], lg[1, 199 + T - 1])


def test_f32_handle_of_the_new_entry_equals_the_old_entry():
    """shape A: precision="f32" goes through pvq_note_model_create; the C entry with PVQ_NOTE_F32 is called here directly"""
    import ctypes as C
    from pitchvis_amd import _lib
    from pitchvis_amd.note_model import _c_weights
    n_bins, T, mlp, layers, _ = R.shape("A")
    db, _, _ = _inputs("A")
    n_frames, stride = _layout("A")
    old = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights("A"), device=0)
    new = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights("A"), device=0)
    L = _lib.load()
    L.pvq_note_model_destroy(new._h)
    new._h = C.c_void_p()
    cw, _keep = _c_weights(new.params, R.weights("A"))
    assert L.pvq_note_model_create_precision(0, C.byref(_lib.CNoteModelParams(n_bins, T, mlp, layers)), C.byref(cw), 0, C.byref(new._h)) == _lib.PVQ_OK
    d_db = torch.from_numpy(db).cuda()
    a, b = old.rows_device(d_db, n_frames, stride), new.rows_device(d_db, n_frames, stride)
    torch.cuda.synchronize()
    for k in ("d_logits", "d_prob", "d_mask"):
        assert np.array_equal(a[k].cpu().numpy().view(np.uint32), b[k].cpu().numpy().view(np.uint32)), k
    assert a["d_logits"].cpu().numpy().any()


def test_handles_of_three_precisions_share_no_state():
    """shape I, one stream of T + 130 frames (two tiles): an f32, a bf16 and an f16 handle called in turn, twice, give each the bits of
    its own first call, and those of a handle of its precision that no other call came between"""
    n_bins, T, mlp, layers, _ = R.shape("I")
    par, w = P.NoteModelParams(n_bins, T, mlp, layers), R.weights("I")
    stride = T + 130
    d_db = torch.from_numpy(R.db_like((1, stride, n_bins), seed=77)).cuda()
    keys = ("d_prob", "d_logits", "d_mask")

    def call(m):
        o = m.rows_device(d_db, [stride], stride)
        torch.cuda.synchronize()
        return [o[k].cpu().numpy().view(np.uint32) for k in keys]

    alone = {p: call(P.NoteModel(par, w, device=0, precision=p)) for p in ("f32", "bf16", "f16")}
    models = {p: P.NoteModel(par, w, device=0, precision=p) for p in alone}
    rounds = [{p: call(m) for p, m in models.items()} for _ in range(2)]
    for p in alone:
        assert alone[p][1].any()
        for k, first, second, single in zip(keys, rounds[0][p], rounds[1][p], alone[p]):
            assert np.array_equal(second, first), (p, k)
            assert np.array_equal(first, single), (p, k)
    assert not np.array_equal(alone["f32"][1], alone["bf16"][1]) and not np.array_equal(alone["bf16"][1], alone["f16"][1])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["G", "J"])
def test_host_infer_predicts_the_device_rows(name, precision):
    """rows (0, T - 1) and (0, T + 255), the one row of the third tile: the host face under (a), with the device's rows under (a) too"""
    db, l64, _ = _inputs(name)
    r = _run(name, precision)
    T = R.shape(name)[1]
    m = _model(name, precision)
    rows = [(0, T - 1), (0, T + 255)]
    host = H.logit_of(np.stack([m.infer(db[s, f - T + 1:f + 1]) for s, f in rows]))
    dev = np.stack([r["logits"][s, f] for s, f in rows]).astype(np.float64)
    l = np.stack([l64[s, f] for s, f in rows])
    q = np.stack([r["q64"][s, f] for s, f in rows])
    quant = float(np.abs(q - l).max())
    a_host, a_dev = float(np.abs(host - l).max()) / quant, float(np.abs(dev - l).max()) / quant
    print(f"shape {name} {precision}: host (a) {a_host:.3f}, device (a) {a_dev:.3f}, max |host - device| {np.abs(host - dev).max():.2e}, max |Q64 - L64| {quant:.2e}")
    assert a_host <= H.BAR_A and a_dev <= H.BAR_A
    assert float(np.abs(host - dev).max()) <= H.BAR_A * quant
