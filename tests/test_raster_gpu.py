"""The pitch balls as pixels on the device (pvq_raster_batch_*) against the host face (pvq_raster_frame / _touch) and against
tests/raster_model.py.  The bar is tests/test_raster.py's: no differing bit in any pixel channel or ball time.  Should one ever
appear it has to be shown to sit within the ~1e-9 ulp libm boundary DESIGN.md 6c describes (a double-precision sin, cos or atan2
whose last bits differ between two libms AND whose value lies that close to an f32 rounding boundary); it is not waived by a
tolerance.

Shapes are small and chosen for where the kernels can go wrong: images that are no multiple of the 16 x 16 tile or the 8 x 8 wave
block, lists across the 64-ball LDS chunk and the 256-thread ranking loop, 3 to 1024 bins."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import pitchvis_amd as P
import raster_cases as RC
import raster_model as M
from test_raster import bits, host_frame, model_frame, same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
MAX_PEAKS = 12


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def clocks(nf, start=0.4):
    return (start + 0.0333 * np.arange(nf)).astype(f32)


def walk_times(lists, elapsed, n, t0=None, max_peaks=MAX_PEAKS, face=None):
    """[ns][nf][n]: the times every frame is drawn with, by the host face (default) or the model"""
    out = []
    for s, frames in enumerate(lists):
        t = np.zeros(n, f32) if t0 is None else t0[s].copy()
        rows = []
        for f, centers in enumerate(frames):
            c = centers[:max_peaks]
            t = M.touch(t, c, elapsed[f], n) if face == "model" else P.raster_touch(t, c, elapsed[f])
            rows.append(t)
        out.append(rows)
    return np.asarray(out, f32)


def run(b, rows, lists, elapsed, max_peaks=MAX_PEAKS, counts=None, **kw):
    """one device call over [ns][nf] rows and peak lists -> (image or None, ball_time or None)"""
    balls = {k: to_device(v) for k, v in RC.stack(rows).items()}
    center, count = RC.pack_peaks(lists, max_peaks, counts)
    out = b.frames_device(balls, center=to_device(center), peak_count=to_device(count), elapsed=elapsed, **kw)
    return tuple(download(out[k]) if k in out else None for k in ("image", "ball_time"))


def expect(rows, times, W, H, frame=host_frame, **kw):
    return np.asarray([[frame(W, H, r, times[s][f], **kw) for f, r in enumerate(frames)] for s, frames in enumerate(rows)], f32)


def hold(tag, b, rows, lists, elapsed, W, H, model_kw=None, host_kw=None, **kw):
    n = b.n_bins
    img, bt = run(b, rows, lists, elapsed, ball_time=True, **kw)
    times = walk_times(lists, elapsed, n)
    same(bt, times, (tag, "times against the host face"))
    same(bt, walk_times(lists, elapsed, n, face="model"), (tag, "times against the model"))
    host = expect(rows, times, W, H, **(host_kw or {}))
    model = expect(rows, times, W, H, frame=model_frame, **(model_kw or {}))
    diff = bits(img) != bits(host)
    print(f"{tag}: {img.size} channels, {int(diff.sum())} differ from the host face, {int((bits(img) != bits(model)).sum())} from the model")
    same(img, host, (tag, "host face"))
    same(img, model, (tag, "model"))
    return img, bt


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (64, 64), (70, 50), (129, 33)])
def test_image_sizes(size):
    W, H = size
    n, ns, nf = 252, 2, 2
    rows = [[RC.row(n, 100 + 10 * s + f) for f in range(nf)] for s in range(ns)]
    rows[1][1] = RC.row(n, 5, drawable=40)
    rows[0][1] = RC.edge_row(n)
    hold(f"{W} x {H}", P.RasterBatch(P.VqtRange(55.0, 7, 36), ns, W, H), rows, RC.peak_lists(n, ns, nf, 7), clocks(nf), W, H)


@pytest.mark.parametrize("geom", [(1, 3), (3, 12), (7, 36), (16, 64)])
def test_geometries(geom):
    octaves, bpo = geom
    n, ns, nf, W, H = octaves * bpo, 2, 2, 40, 24
    rows = [[RC.row(n, 200 + 10 * s + f, drawable=min(n, 48)) for f in range(nf)] for s in range(ns)]
    hold(f"{n} bins", P.RasterBatch(P.VqtRange(55.0, octaves, bpo), ns, W, H), rows, RC.peak_lists(n, ns, nf, 8), clocks(nf), W, H)


@pytest.mark.parametrize("drawable", [(64, 65), (128, 129), (256, 257), (1023, 1024)])
def test_long_lists(drawable):
    """lists on both sides of the LDS chunk (64), of two chunks, of the ranking loop's stride (256) and the full 1024, at equal z"""
    n, W, H = 1024, 48, 40
    rows = [[RC.row(n, 300 + d, drawable=d, kind="small", z_levels=3, spread=5.0) for d in drawable]]
    for r in rows[0]:
        order = M.drawing_order(r["ball_xyzs"], r["ball_rgba"], r["ball_params"], r["ball_visible"], np.zeros(n, f32))
        assert len(order) in drawable and order != sorted(order)
    hold(f"{drawable} balls", P.RasterBatch(P.VqtRange(32.7, 16, 64), 1, W, H), rows, RC.peak_lists(n, 1, 2, 9), clocks(2), W, H)


def test_background_and_galaxy():
    n, ns, nf, W, H = 36, 1, 2, 33, 18
    rows = [[RC.edge_row(), RC.row(n, 21)]]
    lists = RC.peak_lists(n, ns, nf, 10)
    rng = P.VqtRange(55.0, 3, 12)
    bg = np.random.default_rng(4).uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    plain, _ = hold("clear", P.RasterBatch(rng, ns, W, H), rows, lists, clocks(nf), W, H)
    galaxy, _ = hold("galaxy", P.RasterBatch(rng, ns, W, H, visuals_mode=3), rows, lists, clocks(nf), W, H,
                     host_kw=dict(visuals_mode=3), model_kw=dict(mode=3))
    over, _ = hold("background", P.RasterBatch(rng, ns, W, H, visuals_mode=3), rows, lists, clocks(nf), W, H,
                   host_kw=dict(background=bg), model_kw=dict(background=bg), background=to_device(bg))
    wide, _ = hold("viewport 22", P.RasterBatch(rng, ns, W, H, viewport_height=22.0), rows, lists, clocks(nf), W, H,
                   host_kw=dict(viewport_height=22.0), model_kw=dict(viewport_height=22.0))
    assert not np.array_equal(plain, galaxy) and not np.array_equal(galaxy, over) and not np.array_equal(plain, wide)


def test_times():
    """the only state: carried across calls, one frame per call equals one call, streams independent, a frame without peaks leaves
    the times alone, a count above max_peaks is cut, trunc(center) >= n_bins is ignored"""
    n, ns, nf = 36, 3, 9
    rng = P.VqtRange(55.0, 3, 12)
    lists = RC.peak_lists(n, ns, nf, 11, most=5)
    lists[2][4] = [f32(c) + f32(0.5) for c in range(20, 36)]        # 16 entries: max_peaks 12 cuts the last four
    assert any(len(c) > MAX_PEAKS for c in lists[2]) and any(not c for c in lists[0])
    el = clocks(nf)
    want = walk_times(lists, el, n)
    same(want, walk_times(lists, el, n, face="model"), "host against model")
    assert want[2, 4, 31] == el[4] and want[2, 4, 32] != el[4]        # bins 32 .. 35 were past max_peaks
    for s in range(ns):
        for f in range(1, nf):
            if not lists[s][f]:
                same(want[s, f], want[s, f - 1], "no peaks")
    assert not np.array_equal(want[0], want[1])
    rows = [[RC.row(n, 1)] * nf] * ns
    b = P.RasterBatch(rng, ns, 8, 8)
    _, whole = run(b, rows, lists, el, image=False, ball_time=True)
    same(whole, want, "one call")
    for s in range(ns):
        same(b.times(s), want[s, -1], "state")
    # two calls, then one frame per call; the second call's counts claim more entries than max_peaks holds
    b2, b1 = P.RasterBatch(rng, ns, 8, 8), P.RasterBatch(rng, ns, 8, 8)
    cut = lambda lo, hi: ([frames[lo:hi] for frames in rows], [frames[lo:hi] for frames in lists], el[lo:hi])
    parts = []
    for lo, hi in ((0, 4), (4, 9)):
        r_, l_, e_ = cut(lo, hi)
        counts = [[len(c) + (50 if len(c) >= MAX_PEAKS else 0) for c in frames] for frames in l_]
        parts.append(run(b2, r_, l_, e_, counts=counts, image=False, ball_time=True)[1])
    same(np.concatenate(parts, 1), want, "two calls")
    singles = []
    for f in range(nf):
        r_, l_, e_ = cut(f, f + 1)
        singles.append(run(b1, r_, l_, e_, image=False, ball_time=True)[1])
    same(np.concatenate(singles, 1), want, "a frame per call")
    # the image follows the carried time: the same row drawn in a later call differs where the clock moved, and matches the host
    img, bt = run(b2, [[RC.row(n, 1)]] * ns, [[[]]] * ns, f32([99.0]), ball_time=True)
    same(bt[:, 0], want[:, -1], "a call without peaks")
    same(img, expect([[RC.row(n, 1)]] * ns, want[:, -1:], 8, 8), "image with carried times")


def test_output_subsets_and_guards():
    import torch
    n, ns, nf, W, H = 36, 2, 3, 19, 9
    rng = P.VqtRange(55.0, 3, 12)
    rows = [[RC.row(n, 400 + 10 * s + f, drawable=20) for f in range(nf)] for s in range(ns)]
    lists = RC.peak_lists(n, ns, nf, 12)
    el = clocks(nf)
    ref_img, ref_t = hold("all outputs", P.RasterBatch(rng, ns, W, H), rows, lists, el, W, H)
    sizes = {"image": ns * nf * H * W * 4, "ball_time": ns * nf * n}
    for asked in (("image",), ("ball_time",), ("image", "ball_time"), ()):
        bufs = {k: torch.full((sizes[k] + 8,), GUARD, dtype=torch.int32, device="cuda") for k in asked}   # 16 bytes of guard either side
        views = {k: v[4:-4].view(torch.float32) for k, v in bufs.items()}
        b = P.RasterBatch(rng, ns, W, H)
        balls = {k: to_device(v) for k, v in RC.stack(rows).items()}
        center, count = RC.pack_peaks(lists, MAX_PEAKS)
        out = b.frames_device(balls, center=to_device(center), peak_count=to_device(count), elapsed=el,
                              image=views.get("image"), ball_time=views.get("ball_time"))
        assert sorted(out) == sorted(asked)
        torch.cuda.synchronize()
        for k, v in bufs.items():
            host = v.cpu().numpy().view(np.uint32)
            assert np.all(host[:4] == GUARD) and np.all(host[-4:] == GUARD), (asked, k)
            same(host[4:-4].view(f32), (ref_img if k == "image" else ref_t).ravel(), (asked, k))
        same(b.times(1), ref_t[1, -1], (asked, "state"))


def test_side_stream():
    import torch
    n, ns, nf, W, H = 252, 2, 3, 40, 30
    rows = [[RC.row(n, 500 + 10 * s + f) for f in range(nf)] for s in range(ns)]
    lists = RC.peak_lists(n, ns, nf, 13)
    el = clocks(nf)
    rng = P.VqtRange(55.0, 7, 36)
    ref_img, ref_t = run(P.RasterBatch(rng, ns, W, H), rows, lists, el, ball_time=True)
    side = torch.cuda.Stream()
    b = P.RasterBatch(rng, ns, W, H)
    with torch.cuda.stream(side):
        balls = {k: to_device(v) for k, v in RC.stack(rows).items()}
        center, count = RC.pack_peaks(lists, MAX_PEAKS)
        first = b.frames_device({k: v[:, :1].contiguous() for k, v in balls.items()}, center=to_device(center[:, :1].copy()),
                                peak_count=to_device(count[:, :1].copy()), elapsed=el[:1], ball_time=True, stream=side)
        rest = b.frames_device({k: v[:, 1:].contiguous() for k, v in balls.items()}, center=to_device(center[:, 1:].copy()),
                               peak_count=to_device(count[:, 1:].copy()), elapsed=el[1:], ball_time=True, stream=side)
    side.synchronize()
    same(np.concatenate([download(first["image"]), download(rest["image"])], 1), ref_img, "image")
    same(np.concatenate([download(first["ball_time"]), download(rest["ball_time"])], 1), ref_t, "times")


def test_workspace_pieces(tmp_path):
    """the developer library's PVQ_RASTER_WS_KB cuts a call of 7 frames into pieces of 2, the last one shorter; same bits"""
    n, ns, nf, W, H = 252, 2, 7, 24, 20
    per_row = n * (64 + 4) + (8 + 1) * 4                       # mirrors raster_batch.hip: a Ball and a time per bin, marks, the count
    kb = (per_row * ns * 2 + per_row) // 1024 + 1
    assert (kb * 1024) // (per_row * ns) == 2 and nf % 2 == 1
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, "tests")
        import numpy as np
        import pitchvis_amd as P, raster_cases as RC
        from pitchvis_amd import _lib
        import test_raster_gpu as T
        assert _lib.LIB_PATH.endswith("libpvq_dev.so")
        rows, lists, el = T.pieces_case()
        img, bt = T.run(P.RasterBatch(P.VqtRange(55.0, 7, 36), len(rows), %d, %d), rows, lists, el, ball_time=True)
        np.savez(sys.argv[1], image=img, ball_time=bt)
        print("PIECES_OK")
    """ % (W, H))
    f = str(tmp_path / "pieces.npz")
    r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, PVQ_DEV_LIB="1", PVQ_RASTER_WS_KB=str(kb)), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "PIECES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    rows, lists, el = pieces_case()
    img, bt = hold("one piece", P.RasterBatch(P.VqtRange(55.0, 7, 36), ns, W, H), rows, lists, el, W, H)
    got = np.load(f)
    same(got["image"], img, "pieces: image")
    same(got["ball_time"], bt, "pieces: times")


def pieces_case():
    n, ns, nf = 252, 2, 7
    rows = [[RC.row(n, 600 + 10 * s + f, drawable=30 + 5 * f) for f in range(nf)] for s in range(ns)]
    return rows, RC.peak_lists(n, ns, nf, 14, empty_every=2), clocks(nf)


def test_from_a_scene_batch():
    """inputs taken straight from a SceneBatch call's outputs, the peak arrays shared by both stages"""
    import scene_cases as SC
    import torch
    geom, ns, nf, W, H, mp = (55.0, 7, 36), 2, 6, 48, 36, 16
    n = 252
    rng = P.VqtRange(*geom)
    streams = [[c[1:] for c in SC.plain_frames(n, nf, 900 + s, most=9)] for s in range(ns)]
    a = {"center": np.full((ns, nf, mp), -7.0, f32), "size": np.full((ns, nf, mp), -7.0, f32), "peak_count": np.zeros((ns, nf), np.int32),
         "calmness": np.zeros((ns, nf, n), f32), "pitch_accuracy": np.zeros((ns, nf, n), f32), "pitch_deviation": np.zeros((ns, nf, n), f32),
         "scene_calmness": np.zeros((ns, nf), f32)}
    for s, frames in enumerate(streams):
        for f, (pk, calm, acc, dev, scene) in enumerate(frames):
            a["peak_count"][s, f] = len(pk)
            for p, (c, z) in enumerate(pk):
                a["center"][s, f, p], a["size"][s, f, p] = c, z
            a["calmness"][s, f], a["pitch_accuracy"][s, f], a["pitch_deviation"][s, f], a["scene_calmness"][s, f] = calm, acc, dev, scene
    d = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    balls = P.SceneBatch(rng, ns).frames_device(d, frame_time=1.0 / 30.0)
    el = clocks(nf, start=2.0)
    out = P.RasterBatch(rng, ns, W, H, viewport_height=20.0).frames_device(balls, d, elapsed=el, ball_time=True)
    img, bt = download(out["image"]), download(out["ball_time"])
    g = {k: download(balls[k]) for k in ("ball_xyzs", "ball_rgba", "ball_params")}
    g["ball_visible"] = download(balls["ball_visible"]).view(np.uint32)
    rows = [[{k: g[k][s, f] for k in g} for f in range(nf)] for s in range(ns)]
    lists = [[[c for c, _ in pk] for pk, *_ in frames] for frames in streams]
    times = walk_times(lists, el, n, max_peaks=mp)
    same(bt, times, "times")
    assert len(np.unique(bt)) > 3
    same(img, expect(rows, times, W, H, viewport_height=20.0), "host face")
    same(img, expect(rows, times, W, H, frame=model_frame, viewport_height=20.0), "model")
    lit = (img != M.clear_color()).any(-1).mean()
    print(f"scene -> raster: {lit:.2%} of the pixels are covered")
    assert lit > 0.05


def _stride_pairs(total, cap, nf, m):
    """the rows a workgroup that starts on row r < total - cap takes next, as (pattern, frame) pairs: ((p, f), (p', f'))"""
    of = lambda r: ((r // nf) % m, r % nf)
    return sorted({(of(r), of(r + cap)) for r in range(total - cap)})


def test_row_stride_past_both_grid_caps():
    """raster_marks and raster_lists (8192 workgroups) and raster_tiles (gridDim.y 65 535) over 32 769 streams x 2 frames = 65 538
    rows of 3 bins on a 3 x 2 image, in one piece.  Stream s is pattern s % 61 of 61 distinct streams, which the host face and the
    model pin.  A list workgroup's next row, r + 8192, is pattern + 9's (another count of drawable balls: s_key and s_n as a row of
    three left them meet a row of none); a tile workgroup's, r + 65 535, is the other frame of pattern + 10 or + 11.  Rows
    65 535 .. 65 537 exist only if the tile kernel strides by the very cap the host clamps to."""
    import torch
    n, nf, W, H, m = 3, 2, 3, 2, RC.STRIDE_STREAMS
    ns = 65535 // nf + 2
    total = ns * nf
    assert total == 65538
    per_row = n * (64 + 4) + (1 + 1) * 4                        # mirrors raster_batch.hip, as test_workspace_pieces does
    assert per_row == 212 and per_row * total <= 256 << 20      # one piece: the strides are taken, not cut away
    rows, lists, el = RC.stride_rows(nf, W, H, 7000), RC.peak_lists(n, m, nf, 7001), clocks(nf)
    rng = P.VqtRange(55.0, 1, 3)
    img, bt = hold(f"{m} distinct streams", P.RasterBatch(rng, m, W, H), rows, lists, el, W, H)
    # no stride test passes by drawing nothing: a row is empty only where it has no drawable ball, a quarter of the rows at most
    clear = np.broadcast_to(np.asarray(M.clear_color(), f32), (H, W, 4))
    empty = [(p, f) for p in range(m) for f in range(nf) if not (bits(img[p, f]) != bits(clear)).any()]
    assert empty == [(p, f) for p in range(m) for f in range(nf) if RC.STRIDE_BALLS[p % 5] == 0] and 4 * len(empty) <= m * nf
    packed = RC.stack(rows)
    center, count = RC.pack_peaks(lists, MAX_PEAKS)
    for cap in (8192, 65535):
        assert cap % m != 0 and cap < total
        for (p, f), (q, g) in _stride_pairs(total, cap, nf, m):
            assert (bits(img[p, f]) != bits(img[q, g])).any(), (cap, p, f, q, g)
            assert all((packed[k][p, f] != packed[k][q, g]).any() for k in ("ball_xyzs", "ball_rgba", "ball_params")), (cap, p, f, q, g)
    # (three bins have eight bin masks and three clock values: the times of two rows can agree; those of most pairs do not, and a
    # frame without peaks follows one with peaks)
    marks = _stride_pairs(total, 8192, nf, m)
    assert 2 * sum(bool((bits(bt[p, f]) != bits(bt[q, g])).any()) for (p, f), (q, g) in marks) >= len(marks)
    assert any(lists[p][f] and not lists[q][g] for (p, f), (q, g) in marks)
    kinds = {(RC.STRIDE_BALLS[p % 5], RC.STRIDE_BALLS[q % 5]) for (p, _), (q, _) in _stride_pairs(total, 8192, nf, m)}
    assert {(3, 0), (0, 3), (0, 1), (2, 3)} <= kinds and any(f != g for (_, f), (_, g) in _stride_pairs(total, 65535, nf, m)), kinds
    idx = to_device(np.arange(ns, dtype=np.int64) % m)
    balls = {k: to_device(v)[idx].contiguous() for k, v in packed.items()}
    bufs = {"image": torch.full((total * H * W * 4 + 8,), GUARD, dtype=torch.int32, device="cuda"),
            "ball_time": torch.full((total * n + 8,), GUARD, dtype=torch.int32, device="cuda")}
    b = P.RasterBatch(rng, ns, W, H)
    b.frames_device(balls, center=to_device(center)[idx].contiguous(), peak_count=to_device(count)[idx].contiguous(), elapsed=el,
                    image=bufs["image"][4:-4].view(torch.float32), ball_time=bufs["ball_time"][4:-4].view(torch.float32))
    torch.cuda.synchronize()
    differing, unwritten = {}, {}
    for k, small in (("image", img), ("ball_time", bt)):
        assert not (bits(small) == GUARD).any(), k
        got = bufs[k][4:-4].view(ns, nf, -1)
        differing[k] = int((got != to_device(bits(small).view(np.int32).reshape(m, nf, -1))[idx]).sum())
        unwritten[k] = int((got.view(total, -1)[8192:] == GUARD).sum())                         # of rows 8192 .. and 65 535 ..
        assert bool((bufs[k][:4] == GUARD).all()) and bool((bufs[k][-4:] == GUARD).all()), k
    print(f"{total} rows over 8192 list workgroups and 65535 tile rows: differing 32-bit words against the {m}-stream call: {differing}; "
          f"words of rows 8192 .. still the fill value: {unwritten}")
    assert not any(differing.values()) and not any(unwritten.values()), (differing, unwritten)
    for s in (0, 1, ns - 2, ns - 1):
        same(b.times(s), bt[s % m, -1], ("state", s))
