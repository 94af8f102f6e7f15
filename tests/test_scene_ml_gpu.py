"""The scene stage's `ml` branch on the GPU (SceneBatch.frames_device(ml_prob=...), pvq_ml_scene_batch_frames_device) against the
host face (SceneState.update(ml_prob=...)), with the helpers of tests/test_scene_gpu.py.

Bars: alpha and the EXACT fields (scene_model.EXACT: visible mask, params, bass_lit, bloom; z and scale too) bit-identical to the
host face; x, y and the colour channels within CHROMA_REL — the bars of test_scene_gpu.py, with alpha tightened to bits: the branch
is one compare and at most one f32 product, no libm.

The chain test feeds the note model's d_prob buffer, written through a NoteCarry in two calls, straight into the scene stage."""
import numpy as np
import pytest

import note_model_ref as R
import pitchvis_amd as P
import scene_cases as SC
import scene_ml_model as MM
import scene_model as M
import test_scene_gpu as G
from pitchvis_amd import scene as PS
from test_scene_ml import ABOVE, THRESH, alpha_bits_equal, planted_probs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

f32 = np.float32
NS, NF = 3, 40
PAD = 3                       # ml_stride_frames = n_frames + PAD, the padding rows hold NaN
GEOMS = [(61.74, 2, 24), (55.0, 8, 24), (55.0, 7, 36)]


def walk_ml(rng, streams, probs):
    """G.walk with a probability row per frame: probs [stream][frame][128]"""
    out = {k: [] for k in PS.SceneBatch.OUTPUTS}
    for frames, pr in zip(streams, probs):
        s = P.SceneState(rng)
        rows = {k: [] for k in out}
        for i, (pk, calm, acc, dev, scene) in enumerate(frames):
            s.update(pk, calm, acc, dev, scene, G.DT_NS, ml_prob=pr[i])
            for k, v in s.get().items():
                rows[k].append(v)
        for k in out:
            out[k].append(np.asarray(rows[k]))
    return {k: np.asarray(v) for k, v in out.items()}


def padded(probs, pad=PAD):
    """[ns][nf][128] -> device tensor [ns][nf + pad][128], NaN in the padding rows"""
    p = np.asarray(probs, f32)
    buf = np.full((p.shape[0], p.shape[1] + pad, 128), np.nan, f32)
    buf[:, :p.shape[1]] = p
    return torch.from_numpy(buf).cuda()


def hold_ml(tag, got, host):
    G.hold(tag, got, host)
    assert alpha_bits_equal(got, host), tag


def probs_for(ns, nf, seed):
    return np.stack([planted_probs(nf, seed + s) for s in range(ns)])


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[1]}x{g[2]}")
def base(request):
    geom = request.param
    _, octaves, bpo = geom
    n = octaves * bpo
    streams = [G.stream_frames(geom, 100 + 7 * s + n) for s in range(NS)]
    rng = P.VqtRange(*geom)
    probs = probs_for(NS, NF, 2000 + n)
    a = G.pack(streams, n)
    whole = G.download(P.SceneBatch(rng, NS).frames_device(G.to_device(a), frame_time=G.DT, ml_prob=padded(probs)))
    return rng, streams, a, probs, whole


def test_device_matches_host(base):
    rng, streams, a, probs, whole = base
    host = walk_ml(rng, streams, probs)
    hold_ml(f"{rng.octaves} x {rng.buckets_per_octave}", whole, host)
    # the branch really ran: against a walk without probabilities, alpha differs and nothing else does
    plain = G.walk(lambda: P.SceneState(rng), streams)
    assert not np.array_equal(whole["ball_rgba"][..., 3], plain["ball_rgba"][..., 3], equal_nan=True)
    assert np.array_equal(whole["ball_xyzs"][..., 2:], plain["ball_xyzs"][..., 2:], equal_nan=True)
    lit = (whole["ball_rgba"][..., 3] == 1.0) & (plain["ball_rgba"][..., 3] < 1.0)
    dim = whole["ball_rgba"][..., 3] < 0.1
    print(f"balls lifted to 1.0: {int(lit.sum())}, below 0.1: {int(dim.sum())}")
    assert lit.sum() >= 10 and dim.sum() >= 10


def test_two_calls_of_20_equal_one_of_40(base):
    rng, _, a, probs, whole = base
    b = P.SceneBatch(rng, NS)
    halves = [G.download(b.frames_device(G.to_device({k: np.ascontiguousarray(v[:, lo:lo + 20]) for k, v in a.items()}), frame_time=G.DT,
                                         ml_prob=padded(probs[:, lo:lo + 20])))
              for lo in (0, 20)]
    G.same_bits({k: np.concatenate([h[k] for h in halves], axis=1) for k in whole}, whole)


def test_a_raw_pointer_and_a_wider_stride_change_nothing(base):
    rng, _, a, probs, whole = base
    wide = padded(probs, pad=17)
    got = G.download(P.SceneBatch(rng, NS).frames_device(G.to_device(a), frame_time=G.DT, ml_prob=wide.data_ptr(), ml_stride_frames=NF + 17))
    G.same_bits(got, whole)


def test_none_equals_frames_device_by_bits(base):
    rng, _, a, _, _ = base
    d = G.to_device(a)
    plain = G.download(P.SceneBatch(rng, NS).frames_device(d, frame_time=G.DT))
    G.same_bits(G.download(P.SceneBatch(rng, NS).frames_device(d, frame_time=G.DT, ml_prob=None)), plain)
    # the C entry point with a NULL buffer: the stride is not looked at
    import ctypes as C
    from pitchvis_amd import _lib, _ptr
    b = P.SceneBatch(rng, NS)
    outs = {k: torch.empty(b.output_shape(k, NF)[0], dtype=torch.int32 if b.output_shape(k, NF)[1] == np.uint32 else torch.float32, device="cuda")
            for k in PS.SceneBatch.OUTPUTS}
    o = _lib.CSceneOutputs()
    for k, v in outs.items():
        setattr(o, k, _ptr(v))
    i = _lib.CSceneInputs(_ptr(d["center"]), _ptr(d["size"]), _ptr(d["peak_count"]), G.MAX_PEAKS, _ptr(d["calmness"]), _ptr(d["pitch_accuracy"]),
                          _ptr(d["pitch_deviation"]), _ptr(d["scene_calmness"]))
    L = _lib.load()
    assert L.pvq_ml_scene_batch_frames_device(b._h, NF, C.byref(i), None, 0, G.DT_NS, None, C.byref(o), None) == _lib.PVQ_OK
    G.same_bits(G.download(outs), plain)
    # a stride below n_frames is refused before anything runs
    some = torch.zeros((NS, NF, 128), device="cuda")
    assert L.pvq_ml_scene_batch_frames_device(b._h, NF, C.byref(i), _ptr(some), NF - 1, G.DT_NS, None, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        b.frames_device(d, frame_time=G.DT, ml_prob=some[:, :NF - 1].contiguous())


def test_record_pieces_index_the_right_row():
    """the three-piece call of test_scene_gpu.test_record_pieces with probabilities: pieces two and three start at f0 > 0"""
    limit, record, header = 256 << 20, 64, 32
    n, ns, nf, mp = 195, 4, 600, 4096
    pf = min(nf, max(1, limit // ((mp * record + header) * ns)))
    assert -(-nf // pf) >= 3 and nf % pf != 0
    streams = [[c[1:] for c in SC.plain_frames(n, nf, 700 + s, most=5)] for s in range(ns)]
    rng = P.VqtRange(55.0, 5, 39)
    probs = probs_for(ns, nf, 3000)
    want = walk_ml(rng, streams, probs)
    a = G.pack_at(streams, n, mp)
    got = G.download(P.SceneBatch(rng, ns).frames_device(G.to_device(a), frame_time=G.DT, ml_prob=padded(probs)))
    hold_ml(f"pieces of {pf} frames", got, want)
    del a
    keyed_after = sum(len(streams[s][f][0]) for s in range(ns) for f in range(pf, nf))
    assert keyed_after >= 100                                    # frames of the later pieces do key balls


def test_rows_past_the_peaks_grid_read_their_own_stream():
    """130 streams x 64 frames at 48 bins: rows 8192 .. of scene_peaks' grid-stride loop are streams 128 and 129; every stream has the
    same frames as stream s % 5 but probabilities of its own"""
    ns, nf, n = 130, 64, 48
    five = [[c[1:] for c in SC.plain_frames(n, nf, 1200 + s, most=8, every_empty=9)] for s in range(5)]
    rng = P.VqtRange(61.74, 2, 24)
    probs = probs_for(ns, nf, 4000)
    got = G.download(P.SceneBatch(rng, ns).frames_device(G.to_device(G.pack_at([five[s % 5] for s in range(ns)], n, 8)), frame_time=G.DT,
                                                          ml_prob=padded(probs)))
    check = [0, 1, 2, 3, 4, 63, 127, 128, 129]
    want = walk_ml(rng, [five[s % 5] for s in check], probs[check])
    hold_ml("8320 rows", {k: v[check] for k, v in got.items()}, want)
    assert not np.array_equal(got["ball_rgba"][128], got["ball_rgba"][3], equal_nan=True)      # same frames, other probabilities


# ---- the chain: dB -> note model through a carry -> scene ------------------------------------------------------------------------------
BIAS_OFFSET = 0.75   # subtracted from output.bias: chosen on the CPU with the host face (NoteModel.infer over these windows), where it
#                      leaves 40 % of the keyed balls' probabilities above 0.35 (98.8 % without it; 72 % at 0.5, 17 % at 1.0)


def test_chain_db_to_scene_through_a_carry():
    n_bins, T, mlp, layers, _ = R.shape("B")
    geom = (55.0, 7, 36)
    assert geom[1] * geom[2] == n_bins
    w = dict(R.weights("B"))
    w["output.bias"] = (w["output.bias"] - f32(BIAS_OFFSET)).astype(f32)
    db = R.db_like((NS, NF, n_bins), seed=4242)
    streams = [G.stream_frames(geom, 100 + 7 * s + n_bins) for s in range(NS)]
    rng = P.VqtRange(*geom)
    a = G.pack(streams, n_bins)
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), w, device=0)
    # one whole call of both stages
    d_db = torch.from_numpy(db).cuda()
    whole_prob = m.rows_device(d_db, outputs=("d_prob",))["d_prob"]
    whole = G.download(P.SceneBatch(rng, NS).frames_device(G.to_device(a), frame_time=G.DT, ml_prob=whole_prob))
    # two calls of 20 through a carry, d_prob handed over where it lies
    carry, scene, halves, probs = P.NoteCarry(m, NS), P.SceneBatch(rng, NS), [], []
    for lo in (0, 20):
        d_half = torch.from_numpy(np.ascontiguousarray(db[:, lo:lo + 20])).cuda()
        prob = m.rows_device(d_half, outputs=("d_prob",), carry=carry)["d_prob"]
        d_half.fill_(float("nan"))
        halves.append(G.download(scene.frames_device(G.to_device({k: np.ascontiguousarray(v[:, lo:lo + 20]) for k, v in a.items()}),
                                                     frame_time=G.DT, ml_prob=prob)))
        probs.append(prob.cpu().numpy())
    assert [carry.frames_seen(s) for s in range(NS)] == [NF] * NS
    prob_np = np.concatenate(probs, axis=1)
    assert np.array_equal(prob_np.view(np.uint32), whole_prob.cpu().numpy().view(np.uint32))
    assert not prob_np[:, :T - 1].any() and (prob_np[:, T - 1:] > 0).all()
    G.same_bits({k: np.concatenate([h[k] for h in halves], axis=1) for k in whole}, whole)
    # the host face fed the downloaded probabilities
    hold_ml("chain", whole, walk_ml(rng, streams, prob_np))
    # non-vacuity: the keyed balls of model rows fall on both sides of 0.35
    above = below = 0
    for s in range(NS):
        for f in range(T - 1, NF):
            for k in {M.as_usize(np.trunc(f32(c))) for c, _ in streams[s][f][0]}:
                mm = MM.midi_pitch(geom[2], k) if k < n_bins else None
                if mm is not None:
                    above, below = above + bool(prob_np[s, f, mm] > THRESH), below + (not prob_np[s, f, mm] > THRESH)
    print(f"keyed balls: {above} above 0.35, {below} at or below")
    assert above >= 0.1 * (above + below) and below >= 0.1 * (above + below)
