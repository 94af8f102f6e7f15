"""The note model on the GPU (pvq_note_model_rows_device) against tests/note_model_ref.py, the float64 restatement of
pitchvis_train/train.py:67-99.  Shapes A - F of note_model_ref.SHAPES, each with four streams of n_frames = (T, T + 64, T + 128,
T - 1) in a stride of T + 130 frames: 1, 65, 129 and 0 model rows, one past every plausible row-tile edge (the kernels' tile is 128
rows of one stream, a wave's share of it 32).

Bars:
  * logits within 1e-5 * max|logit| (over the call) of the f64 model: the project's magnitude bar.  torch's own CPU f32 forward sits
    at 4 - 7e-7 of the maximum on these inputs; a k-ordered f32 FMA chain of K = 7040 (what the matrix instruction computes) has room.
  * probabilities within 0.25 * that bar + 2e-7: the sigmoid's slope is <= 1/4, expf and the division round.
  * mask bit k == (logit64_k > 0), except where |logit64| < 1e-4 * max|logit|: those decisions are counted, left out, and may be at
    most 0.5 % of all (the f64 model alone puts under 0.05 % of them inside that band).  The mask equals d_logits > 0 of the same
    call exactly.
Every test prints the figures it observes before it asserts; DESIGN.md section 6b item 6 records them.

The edges of the admitted sizes: shapes G - K of note_model_ref.EDGE_SHAPES (3 and 1024 bins, T 1 and 8, mlp 16 and 4096, 0 and 8
hidden layers, O_pool = 1, 2 and 4 k + 1, 4 k + 3), each with five streams of n_frames = (T + 256, T + 31, T + 32, T + 96, T - 1) in a
stride of T + 260: 257, 32, 33, 97 and 0 model rows, so three tiles in one stream with the last holding one row, a tile that ends at a
wave's edge, one row past it, and one row into the fourth wave.  The bars are the ones above, unchanged.  The f64 model alone on these
inputs: the share of decisions inside the band is 6.2e-4 (G), 4.3e-4 (H), 3.5e-4 (I), 3.9e-4 (J), 6.5e-4 (K) against the cap of 5e-3;
46 - 49 % of the bits are positive; torch's f32 CPU forward is at most 4.5e-7 of max|logit| (I).  H's logits are small (max 0.24,
eight default-initialised layers); the bar is relative to that maximum."""
import functools

import numpy as np
import pytest

import note_model_ref as R
import pitchvis_amd as P
from helpers import get_geom
from synth import piano_roll

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGIT_REL, PROB_ABS, BAND_REL, BAND_SHARE = 1e-5, 2e-7, 1e-4, 0.005
GUARD = 1024   # elements after each output that no kernel may touch


def _frames(T):
    return [T, T + 64, T + 128, T - 1], T + 130


def _edge_frames(T):
    return [T + 256, T + 31, T + 32, T + 96, T - 1], T + 260


def _layout(name):
    """(n_frames, stride, model rows per stream) of a shape's shared call"""
    T = R.shape(name)[1]
    n_frames, stride = _edge_frames(T) if name in R.EDGE_SHAPES else _frames(T)
    return n_frames, stride, [max(n - (T - 1), 0) for n in n_frames]


@functools.lru_cache(maxsize=None)
def _model(name):
    n_bins, T, mlp, layers, _ = R.shape(name)
    return P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=0)


def _guarded(shape, dtype, fill):
    """(the output view, the whole buffer): GUARD elements of `fill` follow the view"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf


@functools.lru_cache(maxsize=None)
def _run(name):
    """one call per shape, shared by the tests below: inputs, the three outputs (host copies), their guard regions, the f64 model"""
    n_bins, T, _, _, _ = R.shape(name)
    n_frames, stride, _ = _layout(name)
    S = len(n_frames)
    db = R.db_like((S, stride, n_bins), seed=500 + ord(name))
    m = _model(name)
    prob, prob_all = _guarded((S, stride, 128), torch.float32, 7.0)
    logits, logits_all = _guarded((S, stride, 128), torch.float32, 7.0)
    mask, mask_all = _guarded((S, stride, 4), torch.int32, -1)
    m.rows_device(torch.from_numpy(db).cuda(), n_frames, stride, {"d_prob": prob, "d_logits": logits, "d_mask": mask})
    torch.cuda.synchronize()
    want, valid = R.rows64(R.weights(name), db, n_frames, T)
    for a in (want, valid, db):
        a.setflags(write=False)
    return dict(db=db, n_frames=n_frames, stride=stride, prob=prob.cpu().numpy(), logits=logits.cpu().numpy(),
                mask=mask.cpu().numpy().view(np.uint32), guards=(prob_all[-GUARD:].cpu().numpy(), logits_all[-GUARD:].cpu().numpy(),
                                                                 mask_all[-GUARD:].cpu().numpy()), want=want, valid=valid)


def _check_rows_match_f64_model(name, rows):
    r = _run(name)
    want, valid = r["want"], r["valid"]
    assert valid.sum(axis=1).tolist() == rows == _layout(name)[2]
    top = float(np.abs(want).max())
    bar = LOGIT_REL * top
    err = float(np.abs(r["logits"] - want)[valid].max())
    perr = float(np.abs(r["prob"] - R.sigmoid64(want))[valid].max())
    bits = R.mask_bits(r["mask"])
    decided = np.abs(want) >= BAND_REL * top
    inside = int((~decided)[valid].sum())
    n_dec = int(valid.sum()) * 128
    flips = int(((bits != (want > 0)) & decided)[valid].sum())
    print(f"shape {name}: max |logit| {top:.3f}; logits vs f64 {err:.2e} = {err / top:.2e} of the maximum (bar 1e-5); "
          f"prob {perr:.2e} (bar {0.25 * bar + PROB_ABS:.2e}); {inside} of {n_dec} decisions inside the band, {flips} flips outside")
    assert err <= bar
    assert perr <= 0.25 * bar + PROB_ABS
    assert inside <= BAND_SHARE * n_dec and flips == 0
    assert np.array_equal(bits, r["logits"] > 0)          # the mask is the sign of the logits of the same call, exactly
    assert bits[valid].any() and not bits[valid].all()    # both decisions occur


def _check_rows_outside(name, n_rows):
    """n_rows: the model rows of the call; the last stream has none"""
    r = _run(name)
    out = ~r["valid"]
    T = R.shape(name)[1]
    assert out[:, :T - 1].all() and out[-1].all() and out.sum() == out.shape[0] * r["stride"] - n_rows
    assert not r["prob"][out].any() and not r["logits"][out].any() and not r["mask"][out].any()
    assert (r["prob"][r["valid"]] > 0).all()              # (a model row is never all zero: sigmoid > 0)
    gp, gl, gm = r["guards"]
    assert (gp == 7.0).all() and (gl == 7.0).all() and (gm == -1).all()


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_rows_match_f64_model(name):
    _check_rows_match_f64_model(name, [1, 65, 129, 0])


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_rows_outside_a_stream_are_zero_and_nothing_else_is_written(name):
    assert _run(name)["valid"].shape[0] == 4
    _check_rows_outside(name, 195)


@pytest.mark.parametrize("name", sorted(R.EDGE_SHAPES))
def test_edge_rows_match_f64_model(name):
    """257 rows: tiles of 128, 128 and 1 (f0 = T - 1 + 256); 32, 33 and 97 rows: the wave-activity test 32 * wave < n_valid at its edges"""
    _check_rows_match_f64_model(name, [257, 32, 33, 97, 0])


@pytest.mark.parametrize("name", sorted(R.EDGE_SHAPES))
def test_edge_rows_outside_a_stream_are_zero_and_nothing_else_is_written(name):
    assert _run(name)["valid"].shape[0] == 5
    _check_rows_outside(name, 419)


def test_bits_do_not_depend_on_place():
    """shape A: the same window as row 0 of one stream and as row 70 of another (another tile row, wave and lane group)"""
    n_bins, T, _, _, _ = R.SHAPES["A"]
    m = _model("A")
    stride = T + 80
    db = R.db_like((2, stride, n_bins), seed=901)
    db[1, 70:70 + T] = db[0, 0:T]          # row (1, 70 + T - 1) sees what row (0, T - 1) sees
    o = m.rows_device(torch.from_numpy(db).cuda(), [T + 3, stride], stride)
    torch.cuda.synchronize()
    lg = o["d_logits"].cpu().numpy()
    assert lg[0, T - 1].any()
    assert np.array_equal(lg[0, T - 1].view(np.uint32), lg[1, 70 + T - 1].view(np.uint32))
    assert np.array_equal(o["d_prob"][0, T - 1].cpu().numpy().view(np.uint32), o["d_prob"][1, 70 + T - 1].cpu().numpy().view(np.uint32))
    assert not np.array_equal(lg[0, T - 1], lg[1, 69 + T - 1])


def test_bits_do_not_depend_on_place_second_tile():
    """shape H (T = 1, eight hidden layers): the same window as row T - 1 of one stream and as row T - 1 + 200 of another: the second
    tile, its third wave (row 72 of the tile)"""
    n_bins, T, _, _, _ = R.shape("H")
    m = _model("H")
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


def test_chunked_call_and_single_outputs_equal_the_whole_call():
    """shape A has 4 tiles here (1 + 1 + 2 + 0): a workspace limit of one tile makes 4 chunks"""
    r = _run("A")
    n_bins, T, mlp, layers, _ = R.SHAPES["A"]
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights("A"), device=0)
    m.set_workspace_limit(2 * 128 * mlp * 4 + 256)     # room for one 128-row tile and the table
    d_db = torch.from_numpy(r["db"]).cuda()
    o = m.rows_device(d_db, r["n_frames"], r["stride"])
    only = m.rows_device(d_db, r["n_frames"], r["stride"], outputs=("d_mask",))
    m.set_workspace_limit(256 << 20)
    whole_mask = m.rows_device(d_db, r["n_frames"], r["stride"], outputs=("d_mask",))
    torch.cuda.synchronize()
    assert list(only) == ["d_mask"]
    assert np.array_equal(o["d_logits"].cpu().numpy().view(np.uint32), r["logits"].view(np.uint32))
    assert np.array_equal(o["d_prob"].cpu().numpy().view(np.uint32), r["prob"].view(np.uint32))
    for got in (o["d_mask"], only["d_mask"], whole_mask["d_mask"]):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), r["mask"])


@pytest.mark.parametrize("name", ["J", "K"])
def test_chunked_edge_call_equals_the_whole_call(name):
    """the edge call has 6 tiles (3 + 1 + 1 + 1 + 0): a workspace limit of one tile makes 6 chunks, the third of them the one-row tile"""
    r = _run(name)
    n_bins, T, mlp, layers, _ = R.shape(name)
    assert sum(-(-n // 128) for n in _layout(name)[2]) == 6
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=0)
    m.set_workspace_limit(2 * 128 * mlp * 4 + 256)     # room for one 128-row tile and the table
    o = m.rows_device(torch.from_numpy(r["db"]).cuda(), r["n_frames"], r["stride"])
    torch.cuda.synchronize()
    assert np.array_equal(o["d_logits"].cpu().numpy().view(np.uint32), r["logits"].view(np.uint32))
    assert np.array_equal(o["d_prob"].cpu().numpy().view(np.uint32), r["prob"].view(np.uint32))
    assert np.array_equal(o["d_mask"].cpu().numpy().view(np.uint32), r["mask"])


# (rows of the shared call: A, C, F (0, T - 1) and (2, T + 100); G, J (0, T - 1) and the one row of the third tile)
@pytest.mark.parametrize("name", ["A", "C", "F", "G", "J"])
def test_device_row_matches_host_infer(name):
    r = _run(name)
    n_bins, T, _, _, _ = R.shape(name)
    m = _model(name)
    top = float(np.abs(r["want"]).max())
    for s, f in ((0, T - 1), (0, T + 255) if name in R.EDGE_SHAPES else (2, T + 100)):
        host = m.infer(r["db"][s, f - T + 1:f + 1])
        err = float(np.abs(host - r["prob"][s, f]).max())
        print(f"shape {name} row ({s}, {f}): device vs host infer: max |dp| = {err:.2e}")
        assert err <= 0.25 * LOGIT_REL * top + PROB_ABS    # the host face returns probabilities: the logit bar through the sigmoid


def test_transform_output_feeds_the_model_in_place():
    """48 kHz / 252 bins / hop 256, 2 streams x 40 frames: pvq_vqt_calculate_batch_db_streams writes the rows, the model reads the same
    buffer on the same stream with no host hop; compared with the f64 model on the downloaded dB rows.  Pins the layout hand-off."""
    pp, _ = get_geom("bench_48k_252")
    v = P.Vqt.new(pp, 0)
    hop, nf, T = 256, 40, 5
    pcms = []
    for s in range(2):
        x, _ = piano_roll(48000.0, 2.0, 40 + s)
        pcms.append(torch.from_numpy(np.ascontiguousarray(x[24000:24000 + hop * nf] * 2.0, np.float32)).cuda())   # notes are sounding
    m = _model("A")
    d_db = torch.empty((2, nf, v.n_bins), device="cuda")
    v.batch_streams_device(pcms, hop, [nf, nf], d_db, nf)
    o = m.rows_device(d_db, [nf, nf - 7], nf)
    torch.cuda.synchronize()
    db = d_db.cpu().numpy()
    assert np.isfinite(db).all() and db.max() > 1.0 and np.ptp(db) > 1.0
    want, valid = R.rows64(R.weights("A"), db, [nf, nf - 7], T)
    top = float(np.abs(want).max())
    lg = o["d_logits"].cpu().numpy()
    err = float(np.abs(lg - want)[valid].max())
    print(f"end to end: max |logit| {top:.3f}; logits vs f64 on the GPU's dB rows {err:.2e} = {err / top:.2e} of the maximum")
    assert valid.sum() == (nf - 4) + (nf - 11) and err <= LOGIT_REL * top
    assert not lg[~valid].any() and not o["d_mask"].cpu().numpy()[~valid].any()
    assert np.array_equal(R.mask_bits(o["d_mask"].cpu().numpy()), lg > 0)


def test_from_state_dict_of_a_saved_torchscript_module(tmp_path):
    """what train.py:205-208 saves: a traced module; its state_dict after torch.jit.load builds the same model"""
    n_bins, T, mlp, layers, _ = R.SHAPES["C"]
    w = R.weights("C")
    n_feat = R.sizes(n_bins, T)[3]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv1d(1, 16, 5, stride=2)
            self.fc1 = torch.nn.Linear(n_feat, mlp)
            self.layers = torch.nn.ModuleList([torch.nn.Linear(mlp, mlp) for _ in range(layers)])
            self.output = torch.nn.Linear(mlp, 128)

        def forward(self, x):
            h = torch.max_pool1d(torch.relu(self.conv1(x.unsqueeze(1))), 2).flatten(1)
            h = torch.relu(self.fc1(h))
            for layer in self.layers:
                h = torch.relu(layer(h))
            return torch.sigmoid(self.output(h))
    net = Net()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    path = str(tmp_path / "model.pt")
    torch.jit.trace(net, torch.zeros(1, T * n_bins)).save(path)
    m = P.NoteModel.from_state_dict(torch.jit.load(path).state_dict(), n_bins, T, device=0)
    assert (m.params.mlp_size, m.params.mlp_layers) == (mlp, layers)
    r = _run("C")
    o = m.rows_device(torch.from_numpy(r["db"]).cuda(), r["n_frames"], r["stride"])
    torch.cuda.synchronize()
    assert np.array_equal(o["d_logits"].cpu().numpy().view(np.uint32), r["logits"].view(np.uint32))
    assert np.array_equal(o["d_mask"].cpu().numpy().view(np.uint32), r["mask"])
    assert np.array_equal(m.infer(r["db"][1, 0:T]), _model("C").infer(r["db"][1, 0:T]))
