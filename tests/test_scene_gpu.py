"""The pitch-ball scene on the device (pvq_scene_batch_*) against the host face (pvq_scene_state_*) and against tests/scene_model.py,
at the bars of tests/test_scene.py — and scale, z, the visible mask, the params, bass_lit and bloom bit-identical to the HOST face,
whose fade table the device uses."""
import numpy as np
import pytest

import pitchvis_amd as P
import scene_cases as SC
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


# ---- second round: the paths the tests above never take (cases: tests/scene_cases.py) -------------------------------------------------
def pack_at(streams, n, max_peaks, fill=(-7.0, -7.0)):
    """pack() at any max_peaks; entries beyond a row's count hold fill = (centre, size)"""
    ns, nf = len(streams), len(streams[0])
    a = {"center": np.full((ns, nf, max_peaks), fill[0], f32), "size": np.full((ns, nf, max_peaks), fill[1], f32),
         "peak_count": np.zeros((ns, nf), np.int32), "calmness": np.zeros((ns, nf, n), f32), "pitch_accuracy": np.zeros((ns, nf, n), f32),
         "pitch_deviation": np.zeros((ns, nf, n), f32), "scene_calmness": np.zeros((ns, nf), f32)}
    for s, frames in enumerate(streams):
        assert len(frames) == nf
        for f, (pk, calm, acc, dev, scene) in enumerate(frames):
            k = len(pk)
            assert k <= max_peaks
            a["peak_count"][s, f] = k
            if k:
                a["center"][s, f, :k], a["size"][s, f, :k] = [c for c, _ in pk], [z for _, z in pk]
            a["calmness"][s, f], a["pitch_accuracy"][s, f], a["pitch_deviation"][s, f], a["scene_calmness"][s, f] = calm, acc, dev, scene
    return a


def host_of(rng, **kw):
    return lambda: P.SceneState(rng, **kw)


def of_stream(d, s):
    return {k: v[s] for k, v in d.items()}


def edge_stream(geom, seed):
    """the 40-frame recipe of stream_frames at an edge geometry, then the long lists and the hide cases"""
    octaves, bpo = geom
    n = octaves * bpo
    db = None
    if n < 8:   # oracle_frames' own stimulus places three-bin partials, which need 7 bins
        db = (np.random.default_rng(seed).random((NF, n)) * 6.0).astype(f32)
        db[5:30, 1] = 30.0
    frames = M.oracle_frames(55.0, octaves, bpo, NF, seed, db_frames=db)
    for i, c in enumerate(M.crafted_frames(n, bpo, seed)):
        frames[12 + 2 * i] = c[1:]
    frames += [c[1:] for c in SC.long_lists(n, bpo, seed)]
    ends = []
    for hc in SC.hide_cases(octaves, bpo):
        frames += [c[1:] for c in hc[1]]
        ends.append((len(frames) - 1, hc))
    return frames, ends


@pytest.mark.parametrize("geom", SC.GEOMS_EDGE)
def test_edge_geometries(geom):
    octaves, bpo = geom
    n = octaves * bpo
    made = [edge_stream(geom, 300 + 7 * s + n) for s in range(NS)]
    streams, ends = [m[0] for m in made], made[0][1]
    assert max(len(f[0]) for f in streams[0]) == 200
    rng = P.VqtRange(55.0, octaves, bpo)
    b = P.SceneBatch(rng, NS)
    got = download(b.frames_device(to_device(pack_at(streams, n, 256)), frame_time=DT))
    hold(f"edge {octaves} x {bpo}", got, walk(host_of(rng), streams),
         walk(lambda: M.SceneModel(octaves, bpo), streams) if n <= 195 else None)
    for s in range(NS):                      # the known answers of the hide cases, on the device's own mask
        for f, hc in ends:
            SC.hide_holds({"ball_visible": got["ball_visible"][s, f]}, hc)
    st = b.state(NS - 1)
    for k in PS.SceneBatch.OUTPUTS:
        assert np.array_equal(np.asarray(st[k]), got[k][NS - 1, -1], equal_nan=True), k


@pytest.mark.parametrize("geom", [(1, 3), (5, 13), (5, 39), (31, 31)])   # 3, 65, 195, 961 bins: 1, 3, 7, 31 mask words — an odd last word
def test_mask_words_guarded(geom):
    import torch
    octaves, bpo = geom
    n = octaves * bpo
    assert ((n + 31) // 32) % 2 == 1
    streams = [[c[1:] for c in SC.plain_frames(n, NF, 400 + s + n, most=min(6, n))] for s in range(NS)]
    rng = P.VqtRange(55.0, octaves, bpo)
    d = to_device(pack_at(streams, n, 8))
    want = walk(host_of(rng), streams)
    assert np.unpackbits(want["ball_visible"].astype(np.uint32).view(np.uint8)).sum() > NS * NF   # the masks are not empty
    for names in (PS.SceneBatch.OUTPUTS, ("ball_visible",)):
        b = P.SceneBatch(rng, NS)
        sizes = {k: int(np.prod(b.output_shape(k, NF)[0])) for k in b.OUTPUTS}
        buf = torch.full((sum(sizes.values()) + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        at, views = 4, {}
        for k in b.OUTPUTS:
            views[k] = buf[at:at + sizes[k]]
            at += sizes[k]
        b.frames_device(d, outputs={k: views[k] for k in names}, frame_time=DT)
        torch.cuda.synchronize()
        got = {}
        for k in b.OUTPUTS:
            v = views[k].cpu().numpy()
            if k in names:
                shape, dt = b.output_shape(k, NF)
                got[k] = v.view(dt).reshape(shape)
            else:
                assert np.all(v.view(np.uint32) == 0x5A5A5A5A), k
        assert np.all(buf[:4].cpu().numpy() == 0x5A5A5A5A) and np.all(buf[at:].cpu().numpy() == 0x5A5A5A5A)
        if len(names) == 1:
            assert np.array_equal(got["ball_visible"], want["ball_visible"])
        else:
            hold(f"mask words, {n} bins", got, want)


LIST_GEOMS = {252: (7, 36), 64: (1, 64)}


def list_streams(n, max_peaks, seed):
    """three streams of plain frames with every long list that fits max_peaks put in, each at another frame per stream, and one
    list of exactly max_peaks entries at frame 20 + s"""
    octaves, bpo = LIST_GEOMS[n]
    streams = []
    for s in range(NS):
        frames = [c[1:] for c in SC.plain_frames(n, NF, seed + s)]
        longs = [c[1:] for c in SC.long_lists(n, bpo, seed + 10 * s) if len(c[1]) <= max_peaks]
        for i, fr in enumerate(longs):
            frames[3 + s + 2 * i] = fr
        frames[20 + s] = (SC.long_list(n, max_peaks, seed + 77 + s),) + frames[20 + s][1:]
        streams.append(frames)
    return streams


@pytest.mark.parametrize("n", [252, 64])
@pytest.mark.parametrize("max_peaks", [64, 65, 129, 487])
def test_long_lists_and_counts(n, max_peaks):
    rng = P.VqtRange(55.0, *LIST_GEOMS[n])
    streams = list_streams(n, max_peaks, 500 + n)
    assert max(len(f[0]) for f in streams[0]) == max_peaks
    want = walk(host_of(rng), streams)
    outs = []
    # beyond a row's count: an entry that would light ball 0 and become the maximum; NaN
    for fill in ((0.5, 1e6), (np.nan, np.nan)):
        a = pack_at(streams, n, max_peaks, fill)
        got = download(P.SceneBatch(rng, NS).frames_device(to_device(a), frame_time=DT))
        hold(f"{n} bins, max_peaks {max_peaks}, fill {fill}", got, want)
        outs.append(got)
    same_bits(outs[0], outs[1])
    # a count above max_peaks is taken as max_peaks (include/pvq.h)
    full = a["peak_count"] == max_peaks
    assert full.sum() >= NS
    for over in (max_peaks + 1, 0xFFFFFFFF):
        cnt = a["peak_count"].astype(np.int64)
        cnt[full] = over
        d = to_device({**a, "peak_count": cnt.astype(np.uint32).view(np.int32)})
        same_bits(download(P.SceneBatch(rng, NS).frames_device(d, frame_time=DT)), outs[1])


@pytest.mark.parametrize("n", [252, 64])
def test_max_peaks_does_not_change_the_bits(n):
    rng = P.VqtRange(55.0, *LIST_GEOMS[n])
    streams = list_streams(n, 72, 600 + n)
    assert sorted({len(f[0]) for f in streams[0] if len(f[0]) >= 64}) == [64, 65, 72]
    got = [download(P.SceneBatch(rng, NS).frames_device(to_device(pack_at(streams, n, mp, (0.5, 1e6))), frame_time=DT)) for mp in (72, 487)]
    hold(f"{n} bins, max_peaks 72", got[0], walk(host_of(rng), streams))
    same_bits(got[0], got[1])


def test_record_pieces():
    """a call whose records exceed the workspace: three pieces, the last one shorter"""
    # mirrors scene_batch.hip: WORKSPACE_LIMIT, sizeof(scene::PeakRecord) and sizeof(RowHeader)
    limit, record, header = 256 << 20, 64, 32
    n, ns, nf, mp = 195, 4, 600, 4096
    pf = min(nf, max(1, limit // ((mp * record + header) * ns)))
    pieces = -(-nf // pf)
    assert pieces >= 3 and nf % pf != 0, (pf, pieces)
    bounds = list(range(pf, nf, pf))
    streams = [[c[1:] for c in SC.plain_frames(n, nf, 700 + s, most=5)] for s in range(ns)]
    bright = lambda seed: SC.long_lists(n, 39, seed, counts=(200,))[0][1:]
    few = lambda seed: SC.plain_frames(n, 1, seed, most=4, every_empty=10 ** 9)[0][1:]
    for s in range(ns):
        for i, f0 in enumerate(bounds):
            streams[s][f0 - 1], streams[s][f0] = few(800 + 10 * s + i), few(900 + 10 * s + i)
        for i, f in enumerate((7, pf // 2, pf + 3, nf - 5)):
            streams[s][f + s] = bright(1000 + 10 * s + i)
    # stream 3: the last piece starts on a frame without peaks, whose workspace row held 200 bright records in the piece before
    streams[3][bounds[0]] = bright(1100)
    streams[3][bounds[1]] = ([],) + streams[3][bounds[1]][1:]
    rng = P.VqtRange(55.0, 5, 39)
    want = walk(host_of(rng), streams)
    for s in range(ns):
        for f0 in bounds:
            assert streams[s][f0 - 1][0] and (streams[s][f0][0] or (s, f0) == (3, bounds[1]))
            lit = want["ball_xyzs"][s, f0 - 1, :, 3] >= 0.019                  # above the cutoff before the boundary ...
            lit[[int(c) for c, _ in streams[s][f0][0]]] = False                # ... not lit anew by the frame after it ...
            assert (lit & (want["ball_xyzs"][s, f0, :, 3] >= 0.019)).any()     # ... and still above: the state crossed it
    a = pack_at(streams, n, mp)
    assert a["center"].nbytes < 41 << 20
    got = download(P.SceneBatch(rng, ns).frames_device(to_device(a), frame_time=DT))
    hold(f"{pieces} pieces of {pf} frames", got, want)
    del a
    one = download(P.SceneBatch(rng, ns).frames_device(to_device(pack_at(streams, n, 256)), frame_time=DT))
    same_bits(got, one)


def test_more_rows_than_the_peaks_grid():
    """scene_peaks' grid stops at 8192 workgroups: 130 streams x 64 frames are 8320 rows, rows 8192 .. are streams 128 and 129"""
    ns, nf, n, grid = 130, 64, 48, 256 * 32
    assert ns * nf > grid and grid // nf == 128 and grid % nf == 0
    five = [[c[1:] for c in SC.plain_frames(n, nf, 1200 + s, most=8, every_empty=9)] for s in range(5)]
    rng = P.VqtRange(61.74, 2, 24)
    got = download(P.SceneBatch(rng, ns).frames_device(to_device(pack_at([five[s % 5] for s in range(ns)], n, 8)), frame_time=DT))
    hold("8320 rows", {k: v[:5] for k, v in got.items()}, walk(host_of(rng), five))
    for s in (128, 129):
        same_bits(of_stream(got, s), of_stream(got, s % 5))
    for s in range(5, ns):
        same_bits(of_stream(got, s), of_stream(got, s % 5))


def test_fade_table_across_calls():
    """one handle: the fade table follows the frame time from call to call — scalar A, B, A; per-frame with 2 rows, then with 8
    (the table grows); scalar again"""
    n, nf = 252, 8
    rng = P.VqtRange(55.0, 7, 36)
    odd = [1.0 / 30.0, 0.0, 1.0 / 60.0, 1.0, 0.02, 5.000000007, 0.004, 1.0 / 24.0]
    plans = [("frame_time", 1.0 / 30.0), ("frame_time", 1.0 / 60.0), ("frame_time", 1.0 / 30.0),
             ("frame_times", [1.0 / 30.0 if f % 3 else 1.0 / 60.0 for f in range(nf)]), ("frame_times", odd), ("frame_time", 1.0 / 30.0)]
    assert len(set(plans[3][1])) == 2 and len(set(odd)) == 8
    streams = [[c[1:] for c in SC.plain_frames(n, nf * len(plans), 1300 + s, most=6, every_empty=5)] for s in range(NS)]
    a = pack_at(streams, n, 8)
    b = P.SceneBatch(rng, NS)
    outs, dts = [], []
    for i, (kind, t) in enumerate(plans):
        part = to_device({k: np.ascontiguousarray(v[:, nf * i:nf * (i + 1)]) for k, v in a.items()})
        outs.append(download(b.frames_device(part, **{kind: t})))
        dts += [int(round(x * 1e9)) for x in (t if kind == "frame_times" else [t] * nf)]
    assert {0, 1_000_000_000, 5_000_000_007} <= set(dts)
    got = {k: np.concatenate([o[k] for o in outs], axis=1) for k in outs[0]}
    hold("fade table across calls", got, walk(host_of(rng), streams, dts=dts))
    assert got["ball_xyzs"][..., -nf:, :, 3].max() >= 0.019          # the scene is lit again after the five-second frame


def test_workspace_regrows():
    """one handle, calls at max_peaks 8, 300 and 8: the workspace grows and is reused; the headers move with max_peaks"""
    n, nf = 252, 12
    rng = P.VqtRange(55.0, 7, 36)
    streams = [[c[1:] for c in SC.plain_frames(n, 3 * nf, 1400 + s, most=8)] for s in range(NS)]
    for s in range(NS):
        for i, fr in enumerate(SC.long_lists(n, 36, 1410 + s)):
            streams[s][nf + 1 + 2 * i - (i == 5)] = fr[1:]
    b = P.SceneBatch(rng, NS)
    outs = []
    for i, mp in enumerate((8, 300, 8)):
        part = [frames[nf * i:nf * (i + 1)] for frames in streams]
        outs.append(download(b.frames_device(to_device(pack_at(part, n, mp)), frame_time=DT)))
    hold("max_peaks 8, 300, 8", {k: np.concatenate([o[k] for o in outs], axis=1) for k in outs[0]}, walk(host_of(rng), streams))


def test_side_stream(base):
    import torch
    rng, _, a, whole, _ = base
    times = [1.0 / 30.0 if f % 3 else 1.0 / 60.0 for f in range(NF)]
    d = to_device(a)
    per_frame = download(P.SceneBatch(rng, NS).frames_device(d, frame_times=times))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for kw, want in (({"frame_time": DT}, whole), ({"frame_times": times}, per_frame)):
        outs = P.SceneBatch(rng, NS).frames_device(d, stream=side, **kw)
        side.synchronize()
        same_bits(download(outs), want)


def same_but_nan_bits(tag, got, want):
    """bit-identical, but a value that is NaN on both sides may differ in sign and payload: NaN in the same places, every other
    value by bits.  Returns whether any NaN differed."""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    differs = g != w
    both_nan = np.isnan(np.ascontiguousarray(got)) & np.isnan(np.ascontiguousarray(want))
    bad = np.argwhere(differs & ~both_nan)
    assert not len(bad), (tag, [(i.tolist(), float(np.asarray(got)[tuple(i)]), float(np.asarray(want)[tuple(i)])) for i in bad[:5]])
    return bool(differs.any())


def hold_odd(tag, got, host):
    """hold() for frames that hold NaN and infinities: the exact outputs through same_but_nan_bits, x, y and the colours through
    scene_cases.close_with_specials at CHROMA_REL"""
    loose = [k for k, gv, hv in (("ball_params", got["ball_params"], host["ball_params"]), ("bloom", got["bloom"], host["bloom"]),
                                 ("z / scale", got["ball_xyzs"][..., 2:], host["ball_xyzs"][..., 2:]))
             if same_but_nan_bits((tag, k), gv, hv)]
    for k in ("ball_visible", "bass_lit"):
        assert np.array_equal(got[k], host[k]), (tag, k)
    worst = SC.close_with_specials(got, host, CHROMA_REL)
    print(f"{tag}: device vs host: max |d| / max(1, |want|) = {worst:.2e}; NaN of another sign or payload in: {loose or 'none'}")


def test_edge_entries():
    """entries outside the usual domain, each stream starting at another case so that the cases sit in different rows"""
    n = 252
    rng = P.VqtRange(55.0, 7, 36)
    cases = SC.edge_entries(n)
    names = [c[0] for c in cases]
    assert {"zero_max_pos_first", "zero_max_neg_first", "nan_centre", "inf_centre", "huge_and_tiny"} <= set(names)
    streams = [[c[1:] for c in cases[2 * s:] + cases[:2 * s]] for s in range(NS)]
    got = download(P.SceneBatch(rng, NS).frames_device(to_device(pack_at(streams, n, 8, (np.nan, np.nan))), frame_time=DT))
    want = walk(host_of(rng), streams)
    f = names.index("zero_max_pos_first")
    key = int(cases[f][1][0][0])
    assert want["ball_xyzs"][0, f, key, 2] == -np.inf        # -1 / +0: the FIRST maximum is +0 (util.rs:48-57)
    hold_odd("edge entries", got, want)


def test_edge_fields():
    """NaN and infinities in the per-bin fields under lit keys; scene_calmness NaN, -1 and +inf: bloom by bits"""
    n = 252
    rng = P.VqtRange(55.0, 7, 36)
    cases = SC.edge_fields(n)
    streams = [[c[1:] for c in cases[2 * s:] + cases[:2 * s]] for s in range(NS)]
    got = download(P.SceneBatch(rng, NS).frames_device(to_device(pack_at(streams, n, 8, (np.nan, np.nan))), frame_time=DT))
    want = walk(host_of(rng), streams)
    assert np.isnan(want["ball_params"]).any() and np.isinf(want["ball_params"]).any()
    hold_odd("edge fields", got, want)
    assert np.array_equal(got["bloom"].view(np.uint32), want["bloom"].view(np.uint32))
