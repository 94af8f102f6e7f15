"""The pitch-ball scene on the device (pvq_scene_batch_*) against the host face (pvq_scene_state_*) and against tests/scene_model.py,
at the bars of tests/test_scene.py — and scale, z, the visible mask, the params, bass_lit and bloom bit-identical to the HOST face,
whose fade table the device uses."""
import numpy as np
import pytest

import pitchvis_amd as P
import scene_model as M
from pitchvis_amd import scene as PS
from test_render import CHROMA_REL

pytestmark = pytest.mark.gpu
f32 = np.float32
DT = 1.0 / 30.0
DT_NS = int(round(DT * 1e9))
MAX_PEAKS = 72
NS, NF = 3, 40
GEOMS = [(61.74, 2, 24), (55.0, 8, 24), (55.0, 5, 39), (55.0, 7, 36), (55.0, 7, 84), (32.70, 16, 64)]
_cache = {}


def stream_frames(geom, seed):
    """40 frames of one stream: oracle AnalysisState frames with the crafted frames of scene_model put in from frame 12 on"""
    key = (geom, seed)
    if key not in _cache:
        min_freq, octaves, bpo = geom
        frames = M.oracle_frames(min_freq, octaves, bpo, NF, seed)
        for i, c in enumerate(M.crafted_frames(octaves * bpo, bpo, seed)):
            frames[12 + 2 * i] = c[1:]
        _cache[key] = frames
    return _cache[key]


def pack(streams, n):
    """per-stream frame lists -> the arrays pvq_scene_inputs describes"""
    ns, nf = len(streams), len(streams[0])
    a = {"center": np.full((ns, nf, MAX_PEAKS), -7.0, f32), "size": np.full((ns, nf, MAX_PEAKS), -7.0, f32),
         "peak_count": np.zeros((ns, nf), np.int32), "calmness": np.zeros((ns, nf, n), f32), "pitch_accuracy": np.zeros((ns, nf, n), f32),
         "pitch_deviation": np.zeros((ns, nf, n), f32), "scene_calmness": np.zeros((ns, nf), f32)}
    for s, frames in enumerate(streams):
        for f, (pk, calm, acc, dev, scene) in enumerate(frames):
            assert len(pk) <= MAX_PEAKS
            a["peak_count"][s, f] = len(pk)
            for p, (c, z) in enumerate(pk):
                a["center"][s, f, p], a["size"][s, f, p] = c, z
            a["calmness"][s, f], a["pitch_accuracy"][s, f], a["pitch_deviation"][s, f], a["scene_calmness"][s, f] = calm, acc, dev, scene
    return a


def to_device(a):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in a.items()}


def download(outs):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if v.dtype == torch.int32 else v.cpu().numpy()) for k, v in outs.items()}


def walk(make, streams, dts=None):
    """a one-stream face over every stream's frames -> arrays shaped like the device's outputs"""
    out = {k: [] for k in PS.SceneBatch.OUTPUTS}
    for frames in streams:
        s = make()
        rows = {k: [] for k in out}
        for i, (pk, calm, acc, dev, scene) in enumerate(frames):
            s.update(pk, calm, acc, dev, scene, DT_NS if dts is None else dts[i])
            for k, v in s.get().items():
                rows[k].append(v)
        for k in out:
            out[k].append(np.asarray(rows[k]))
    return {k: np.asarray(v) for k, v in out.items()}


def hold(tag, got, host, model=None):
    for k in M.EXACT:
        assert np.array_equal(got[k], host[k], equal_nan=got[k].dtype.kind == "f"), (tag, k)
    worst = M.compare(got, host, CHROMA_REL)
    print(f"{tag}: device vs host: max |d| / max(1, |want|) = {worst:.2e}")
    if model is not None:
        print(f"{tag}: device vs model: max |d| / max(1, |want|) = {M.compare(got, model, CHROMA_REL):.2e}")


def same_bits(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32) if np.asarray(a[k]).dtype.itemsize == 4 else a[k],
                              np.asarray(b[k]).view(np.uint32) if np.asarray(b[k]).dtype.itemsize == 4 else b[k]), k


@pytest.mark.parametrize("geom", GEOMS)
def test_device_matches_host_and_model(geom):
    _, octaves, bpo = geom
    n = octaves * bpo
    streams = [stream_frames(geom, 100 + 7 * s + n) for s in range(NS)]
    rng = P.VqtRange(geom[0], octaves, bpo)
    b = P.SceneBatch(rng, NS)
    got = download(b.frames_device(to_device(pack(streams, n)), frame_time=DT))
    hold(f"{n} bins", got, walk(lambda: P.SceneState(rng), streams), walk(lambda: M.SceneModel(octaves, bpo), streams))
    st = b.state(NS - 1)
    for k in PS.SceneBatch.OUTPUTS:
        assert np.array_equal(np.asarray(st[k]), got[k][NS - 1, NF - 1], equal_nan=True), k


@pytest.fixture(scope="module")
def base():
    """7 x 36: the packed inputs of three streams and one call of 40 frames over them"""
    geom = (55.0, 7, 36)
    streams = [stream_frames(geom, 100 + 7 * s + 252) for s in range(NS)]
    a = pack(streams, 252)
    rng = P.VqtRange(*geom)
    b = P.SceneBatch(rng, NS)
    return rng, streams, a, download(b.frames_device(to_device(a), frame_time=DT)), [b.state(s) for s in range(NS)]


def test_state_carries_across_calls(base):
    rng, _, a, whole, states = base
    b = P.SceneBatch(rng, NS)
    halves = [download(b.frames_device(to_device({k: np.ascontiguousarray(v[:, lo:lo + 20]) for k, v in a.items()}), frame_time=DT))
              for lo in (0, 20)]
    same_bits({k: np.concatenate([h[k] for h in halves], axis=1) for k in whole}, whole)
    for s in range(NS):
        same_bits(b.state(s), states[s])


def test_one_frame_per_call(base):
    rng, _, a, whole, states = base
    b = P.SceneBatch(rng, NS)
    outs = [download(b.frames_device(to_device({k: np.ascontiguousarray(v[:, f:f + 1]) for k, v in a.items()}), frame_time=DT))
            for f in range(NF)]
    same_bits({k: np.concatenate([o[k] for o in outs], axis=1) for k in whole}, whole)
    same_bits(b.state(1), states[1])


def test_streams_are_independent(base):
    rng, streams, _, whole, _ = base
    many = [streams[s % NS] if s != 64 else streams[0] for s in range(65)]
    many[1:64] = [stream_frames((55.0, 7, 36), 900 + s % 5) for s in range(1, 64)]
    got = download(P.SceneBatch(rng, 65).frames_device(to_device(pack(many, 252)), frame_time=DT))
    one = download(P.SceneBatch(rng, 1).frames_device(to_device(pack([streams[0]], 252)), frame_time=DT))
    same_bits({k: got[k][64] for k in got}, {k: got[k][0] for k in got})
    same_bits({k: got[k][0] for k in got}, {k: one[k][0] for k in one})
    same_bits({k: one[k][0] for k in one}, {k: whole[k][0] for k in whole})


def test_per_frame_frame_times(base):
    rng, streams, a, _, _ = base
    times = [1.0 / 30.0 if f % 3 else 1.0 / 60.0 for f in range(NF)]
    got = download(P.SceneBatch(rng, NS).frames_device(to_device(a), frame_times=times))
    hold("frame_times", got, walk(lambda: P.SceneState(rng), streams, dts=[int(round(t * 1e9)) for t in times]))


def test_requested_output_subsets(base):
    import torch
    rng, _, a, whole, states = base
    d = to_device(a)
    for names in (("ball_visible", "bass_lit"), ("bloom",)):
        b = P.SceneBatch(rng, NS)
        # every output in one sentinel-filled buffer, back to back: a write outside a requested output shows in its neighbours
        sizes = {k: int(np.prod(b.output_shape(k, NF)[0])) for k in b.OUTPUTS}
        buf = torch.full((sum(sizes.values()) + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        at, views = 4, {}
        for k in b.OUTPUTS:
            views[k] = buf[at:at + sizes[k]]
            at += sizes[k]
        b.frames_device(d, outputs={k: views[k] for k in names}, frame_time=DT)
        torch.cuda.synchronize()
        for k in b.OUTPUTS:
            v = views[k].cpu().numpy().view(np.uint32)
            if k in names:
                assert np.array_equal(v.reshape(whole[k].shape), whole[k].view(np.uint32)), k
            else:
                assert np.all(v == 0x5A5A5A5A), k
        assert np.all(buf[:4].cpu().numpy() == 0x5A5A5A5A) and np.all(buf[at:].cpu().numpy() == 0x5A5A5A5A)
        same_bits(b.state(2), states[2])


@pytest.mark.parametrize("mode,geom", [(PS.PERFORMANCE, (55.0, 7, 36)), (PS.GALAXY, (55.0, 5, 39))])
def test_modes(mode, geom):
    _, octaves, bpo = geom
    n = octaves * bpo
    streams = [stream_frames(geom, 100 + 7 * s + n) for s in range(NS)]
    rng = P.VqtRange(*geom)
    got = download(P.SceneBatch(rng, NS, visuals_mode=mode, enable_bloom=False).frames_device(to_device(pack(streams, n)), frame_time=DT))
    hold(f"mode {mode}", got, walk(lambda: P.SceneState(rng, visuals_mode=mode, enable_bloom=False), streams))
    assert not got["bloom"].any() and (mode != PS.GALAXY or not got["bass_lit"].any())


def test_analysis_batch_outputs_as_fields():
    """input (b): the GPU AnalysisBatch's own outputs go in as fields=; downloaded, they feed the host face and the model"""
    import torch
    geom = (55.0, 7, 36)
    rng = P.VqtRange(*geom)
    n, mp = 252, 64
    db = np.stack([np.stack([f for f in _db_frames(n, 500 + s)]) for s in range(NS)]).astype(f32)
    ab = P.AnalysisBatch(rng, NS)
    dev = torch.device("cuda")
    fields = {"center": torch.zeros((NS, NF, mp), device=dev), "size": torch.zeros((NS, NF, mp), device=dev),
              "peak_count": torch.zeros((NS, NF), dtype=torch.int32, device=dev), "calmness": torch.zeros((NS, NF, n), device=dev),
              "pitch_accuracy": torch.zeros((NS, NF, n), device=dev), "pitch_deviation": torch.zeros((NS, NF, n), device=dev),
              "scene_calmness": torch.zeros((NS, NF), device=dev)}
    ab.preprocess_device(torch.from_numpy(db).cuda(), NF, DT, outputs=fields, max_peaks=mp)
    got = download(P.SceneBatch(rng, NS).frames_device(fields=fields, frame_time=DT))
    h = {k: v.cpu().numpy() for k, v in fields.items()}
    assert h["peak_count"].sum() > 0 and h["peak_count"].max() <= mp
    streams = [[([(float(h["center"][s, f, p]), float(h["size"][s, f, p])) for p in range(int(h["peak_count"][s, f]))], h["calmness"][s, f],
                 h["pitch_accuracy"][s, f], h["pitch_deviation"][s, f], h["scene_calmness"][s, f]) for f in range(NF)] for s in range(NS)]
    hold("AnalysisBatch fields", got, walk(lambda: P.SceneState(rng), streams), walk(lambda: M.SceneModel(7, 36), streams))


def _db_frames(n_bins, seed):
    rng = np.random.default_rng(seed)
    db = (rng.random((NF, n_bins), dtype=np.float32) * 6.0).astype(f32)
    for _ in range(6):
        b0, t0 = int(rng.integers(3, n_bins - 3)), int(rng.integers(0, NF - 10))
        lvl = float(rng.uniform(18.0, 50.0))
        for t in range(t0, min(NF, t0 + int(rng.integers(10, 40)))):
            db[t, b0] = lvl + 0.3 * np.sin(t / 7.0)
            db[t, b0 - 1] = max(db[t, b0 - 1], lvl - 9.0)
            db[t, b0 + 1] = max(db[t, b0 + 1], lvl - 11.0)
    return db
