"""The overlay stage on the device (pvq_overlay_batch_*) against the host face (pvq_overlay_state_*, pvq_overlay_frame).  The bar is
tests/test_overlay.py's: no differing bit in any pixel channel.

So that small images sample many texels the quad lies over the whole image: quad = (0, 0, vh W / H, vh) with vh = 3.  Shapes are
chosen for where the kernels can go wrong: images that are no multiple of the 16 x 16 tile or the 8 x 8 wave block, 3 to 1024 bins,
rings of 2 to 200 rows, calls shorter than, as long as and longer than a ring, one call against several.

So that a case cannot pass by drawing nothing, every case but 1 x 1 also asserts, from the model (tests/overlay_model.py, which
samples the literal texture and remembers which frame wrote each of its rows), over all the frames the case draws: at least half of
the image's pixels receive a texel with non-zero alpha in some frame (the zeroed row's share of the quad, a half of it at h = 2,
never does), at least min(h - 1, 4) ages and at least min(n_bins, H, 4) bins are sampled."""
import numpy as np
import pytest

import overlay_cases as OC
import overlay_model as M
import pitchvis_amd as P
from test_overlay import bits, same

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 0x5A5A5A5A
VH = 3.0


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def geometry(n):
    """(octaves, buckets_per_octave) of n bins"""
    return {3: (1, 3), 24: (2, 12), 252: (7, 36), 1024: (16, 64)}[n]


def batch(n, ns, W, H, h, full=True, **kw):
    if full:
        kw.update(viewport_height=VH, quad=OC.full_quad(W, H, VH))
    return P.OverlayBatch(P.VqtRange(55.0, *geometry(n)), ns, W, H, history_rows=h, **kw)


def draw(b, imgs, rows=None, chroma=None, **kw):
    """one device call -> the images [ns][nf][H][W][4]"""
    image = to_device(imgs)
    out = b.frames(imgs.shape[1], image, None if rows is None else to_device(rows), None if chroma is None else to_device(chroma), **kw)
    assert out is image
    return download(image)


def references(n, h, rows, chroma, imgs, full=True, before=None, **kw):
    """the host face and the model on every stream -> (host images, host states, per-frame model info)"""
    ns = imgs.shape[0]
    H, W = imgs.shape[2:4]
    q = OC.full_quad(W, H, VH) if full else None
    vh = VH if full else 0.0
    host, states, info = [], [], []
    for s in range(ns):
        pre = () if before is None else before[s]
        got, st = OC.host_chain(n, h, None if rows is None else rows[s], None if chroma is None else chroma[s], imgs[s], before=pre, quad_=q,
                                viewport_height=vh, **kw)
        want, _ = OC.model_chain(n, h, None if rows is None else rows[s], None if chroma is None else chroma[s], imgs[s], info=info, before=pre,
                                 quad_=q, viewport_height=vh, **kw)
        same(got, want, ("host against model", s))
        host.append(got)
        states.append(st)
    return np.asarray(host, f32), states, info


def drawn_enough(tag, info, host, imgs, n, h):
    """the conditions of the module's docstring"""
    H, W = imgs.shape[2:4]
    touched = (bits(host) != bits(imgs)).any(-1).any((0, 1))                   # [H][W]: drawn on in some frame of some stream
    ages = set().union(*(d["ages"] for d in info))
    bins = set().union(*(d["bins"] for d in info))
    print(f"{tag}: {int(touched.sum())} of {W * H} pixels drawn on, {len(ages)} ages, {len(bins)} bins, "
          f"{sum(d['drawn'] for d in info)} texels and {sum(d['boxed'] for d in info)} box pixels blended")
    if (W, H) == (1, 1):
        return ages
    assert 2 * touched.sum() >= W * H, (tag, int(touched.sum()))
    assert len(ages) >= min(h - 1, 4), (tag, sorted(ages))
    assert len(bins) >= min(n, H, 4), (tag, len(bins))
    return ages


def hold(tag, n, ns, nf, W, H, h, seed, with_rows=True, with_chroma=True, **kw):
    """one call of nf frames on a fresh handle against the host face"""
    rows = OC.rows(ns, nf, n, seed) if with_rows else None
    chroma = OC.chroma(ns, nf, seed + 1) if with_chroma else None
    imgs = OC.images(ns, nf, W, H, seed + 2)
    host, states, info = references(n, h, rows, chroma, imgs, **kw)
    got = draw(batch(n, ns, W, H, h, **kw), imgs, rows, chroma)
    print(f"{tag}: {got.size} channels, {int((bits(got) != bits(host)).sum())} differ from the host face")
    same(got, host, tag)
    if with_rows:
        drawn_enough(tag, info, host, imgs, n, h)
    return got, host, imgs


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (16, 16), (17, 33), (129, 33)])
def test_image_sizes(size):
    W, H = size
    hold(f"{W} x {H}", 24, 2, 7, W, H, 5, 100 + W)


@pytest.mark.parametrize("n", [3, 24, 252, 1024])
def test_geometries(n):
    hold(f"{n} bins", n, 1, 9, 40, 24, 6, 200 + n)


def test_every_bin_of_1024():
    W, H, n, h, nf = 4, 1030, 1024, 3, 5
    rows, imgs = OC.rows(1, nf, n, 250), OC.images(1, nf, W, H, 251)
    rows[..., 3] = np.maximum(rows[..., 3], 1)                                 # every texel draws: every bin can be seen sampled
    host, _, info = references(n, h, rows, None, imgs)
    same(draw(batch(n, 1, W, H, h), imgs, rows), host, "1024 bins")
    assert set().union(*(d["bins"] for d in info)) == set(range(n))
    drawn_enough("1024 bins", info, host, imgs, n, h)


@pytest.mark.parametrize("h", [2, 3, 5, 200])
def test_ring_heights(h):
    """calls of 1, h - 1, h, h + 1 and 2 h + 1 frames on one handle: shorter than, as long as and longer than the ring, each after
    the rings the calls before it left"""
    n, ns, W, H = 24, 2, 24, 8
    calls = [1, h - 1, h, h + 1, 2 * h + 1]
    total = sum(calls)
    rows, chroma = OC.rows(ns, total, n, 300 + h), OC.chroma(ns, total, 301)
    imgs = OC.images(ns, 1, W, H, 302).repeat(total, 1)                        # one picture under every frame
    host, states, info = references(n, h, rows, chroma, imgs)
    b = batch(n, ns, W, H, h)
    f0 = 0
    for k in calls:
        sl = slice(f0, f0 + k)
        got = draw(b, imgs[:, sl], rows[:, sl], chroma[:, sl])
        same(got, host[:, sl], (h, "call of", k, "after", f0))
        f0 += k
    for s in range(ns):
        tex, w = b.texture(s)
        want, ww = states[s].texture()
        assert np.array_equal(tex, want) and w == ww == total % h, (h, s)
    drawn_enough(f"h = {h}", info, host, imgs, n, h)


def test_ring_of_200_after_450_frames():
    n, W, H, h = 24, 260, 3, 200
    before = OC.rows(1, 447, n, 350)
    rows, imgs = OC.rows(1, 3, n, 351), OC.images(1, 3, W, H, 352)
    host, states, info = references(n, h, rows, None, imgs, before=before)
    b = batch(n, 1, W, H, h)
    sink = to_device(np.zeros((1, 447, H, W, 4), f32))
    b.frames(447, sink, to_device(before))                                     # 447 frames, then the 3 that are compared: 450
    same(draw(b, imgs, rows), host, "after 450 frames")
    ages = drawn_enough("h = 200, 450 frames", info, host, imgs, n, h)
    assert len(ages) >= 150 and max(ages) >= 190, (len(ages), max(ages))       # of 199; a seventh of the rows is all zero
    assert np.array_equal(b.texture(0)[0], states[0].texture()[0])


def test_reference_quad_and_view():
    n, ns, W, H, h, nf = 252, 1, 64, 36, 200, 3
    before = OC.rows(ns, 230, n, 400)
    rows, chroma, imgs = OC.rows(ns, nf, n, 401), OC.chroma(ns, nf, 402), OC.images(ns, nf, W, H, 403)
    host, _, info = references(n, h, rows, chroma, imgs, full=False, before=before)
    b = batch(n, ns, W, H, h, full=False)
    b.frames(230, to_device(np.zeros((ns, 230, H, W, 4), f32)), to_device(before))
    same(draw(b, imgs, rows, chroma), host, "the viewer's quad and view")
    assert info[-1]["drawn"] > 0.1 * W * H and len(info[-1]["ages"]) > 20 and len(info[-1]["bins"]) > 10


def test_carry_across_calls():
    """3 + 4 frames equal one call of 7; a call without rows in between changes nothing in the next call; texture() is the host's"""
    n, ns, W, H, h = 24, 2, 33, 17, 5
    rows, chroma, imgs = OC.rows(ns, 7, n, 500), OC.chroma(ns, 7, 501), OC.images(ns, 7, W, H, 502)
    host, states, info = references(n, h, rows, chroma, imgs)
    one = draw(batch(n, ns, W, H, h), imgs, rows, chroma)
    same(one, host, "one call of 7")
    b = batch(n, ns, W, H, h)
    first = draw(b, imgs[:, :3], rows[:, :3], chroma[:, :3])
    boxes_only = draw(b, imgs[:, :2], None, chroma[:, :2])                     # the rings do not advance
    second = draw(b, imgs[:, 3:], rows[:, 3:], chroma[:, 3:])
    same(np.concatenate([first, second], 1), one, "3 + 4 frames")
    box_host, _, _ = references(n, h, None, chroma[:, :2], imgs[:, :2])
    same(boxes_only, box_host, "boxes alone, between the calls")
    # some texel of the second call's first frame comes from a frame of the first call: an age above the frame's number in its call
    for s in range(ns):
        assert max(info[7 * s + 3]["ages"]) > 0 and max(info[7 * s + 4]["ages"]) > 1, s
        tex, w = b.texture(s)
        want, ww = states[s].texture()
        assert np.array_equal(tex, want) and w == ww == 7 % h
    drawn_enough("carry", info, host, imgs, n, h)
    fresh = batch(n, ns, W, H, h)
    tex, w = fresh.texture(1)
    assert not tex.any() and w == 0


@pytest.mark.parametrize("ns", [1, 2, 65])
def test_streams(ns):
    got, host, imgs = hold(f"{ns} streams", 24, ns, 6, 20, 12, 4, 600 + ns)
    if ns > 1:
        assert not np.array_equal(got[0], got[-1])                             # different rows per stream


@pytest.mark.parametrize("scale,W,H", [(1.0, 960, 56), (0.25, 240, 14)])
def test_boxes(scale, W, H):
    """boxes alone, quad alone, both, with the quad under the boxes"""
    n, ns, nf, h = 24, 2, 3, 5
    rows, chroma, imgs = OC.rows(ns, nf, n, 700), OC.chroma(ns, nf, 701), OC.images(ns, nf, W, H, 702)
    quad = OC.full_quad(W, H, VH)
    out = {}
    for tag, r, c in (("boxes", None, chroma), ("quad", rows, None), ("both", rows, chroma)):
        ref = []
        for s in range(ns):
            ref.append(OC.host_chain(n, h, None if r is None else r[s], None if c is None else c[s], imgs[s], quad_=quad, viewport_height=VH,
                                     ui_scale=scale)[0])
        b = P.OverlayBatch(P.VqtRange(55.0, 2, 12), ns, W, H, history_rows=h, viewport_height=VH, ui_scale=scale, quad=quad)
        out[tag] = draw(b, imgs, r, c)
        same(out[tag], np.asarray(ref, f32), (scale, tag))
    box_px = (bits(out["boxes"]) != bits(imgs)).any(-1)
    assert box_px.any((0, 1)).sum() >= 8 * 0.9 * (40 * scale) ** 2            # a row has a zero and a NaN among its twelve strengths
    assert not np.array_equal(out["both"], out["quad"]) and not np.array_equal(out["both"], out["boxes"])
    # the default palette against another
    pal = np.random.default_rng(703).uniform(0.0, 1.0, (12, 3)).astype(f32)
    b = P.OverlayBatch(P.VqtRange(55.0, 2, 12), ns, W, H, history_rows=h, ui_scale=scale, colors=pal)
    ref = [OC.host_chain(n, h, None, chroma[s], imgs[s], ui_scale=scale, colors=pal)[0] for s in range(ns)]
    same(draw(b, imgs, None, chroma), np.asarray(ref, f32), (scale, "palette"))


def test_guards_side_stream_and_untouched_pixels():
    """16 bytes of guard either side of the image, a side stream, and pixels outside both layers — NaN payloads included — keep
    their bits"""
    import torch
    n, ns, nf, W, H, h = 24, 2, 3, 150, 60, 5
    rows, chroma = OC.rows(ns, nf, n, 800), OC.chroma(ns, nf, 801)
    imgs = OC.images(ns, nf, W, H, 802)
    quad = np.asarray([-0.2, 0.4, 1.5, 1.0], f32)                              # a part of the picture: most pixels lie outside both layers
    kw = dict(viewport_height=VH, ui_scale=0.25, quad=quad)
    plain = np.asarray([OC.host_chain(n, h, rows[s], chroma[s], imgs[s], quad_=quad, viewport_height=VH, ui_scale=0.25)[0] for s in range(ns)], f32)
    outside = ~(bits(plain) != bits(imgs)).any(-1)
    assert 0.5 * outside.size < outside.sum() < outside.size
    flat = imgs.view(np.uint32)
    payload = 0x7FC00100 | (np.arange(int(outside.sum()), dtype=np.uint32) & 0xFFFF)
    flat[..., 1][outside] = payload                                            # a NaN of its own in every untouched pixel
    flat[..., 3][outside] = payload | 0x80000000
    host = np.asarray([OC.host_chain(n, h, rows[s], chroma[s], imgs[s], quad_=quad, viewport_height=VH, ui_scale=0.25)[0] for s in range(ns)], f32)
    assert np.array_equal(bits(host)[outside], bits(imgs)[outside])
    buf = torch.full((imgs.size + 8,), GUARD, dtype=torch.int32, device="cuda")
    buf[4:-4] = to_device(imgs.view(np.int32).ravel())
    b = P.OverlayBatch(P.VqtRange(55.0, 2, 12), ns, W, H, history_rows=h, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.frames(nf, buf[4:-4].view(torch.float32), to_device(rows), to_device(chroma), stream=side)
    side.synchronize()
    out = buf.cpu().numpy().view(np.uint32)
    assert np.all(out[:4] == GUARD) and np.all(out[-4:] == GUARD)
    got = out[4:-4].view(f32).reshape(imgs.shape)
    same(got, host, "side stream, guarded")
    assert np.array_equal(bits(got)[outside], bits(imgs)[outside]) and (bits(got) != bits(imgs)).any()


def test_chain():
    """AnalysisBatch fields -> RenderBatch.rows_device -> BackdropBatch.frames -> RasterBatch.frames_over -> OverlayBatch.frames on 2
    streams x 3 frames, both spectrogram modes: every row equals the host chain ending in overlay_frame"""
    import scene_cases as SC
    import torch
    geom, ns, nf, W, H, mp, vh, h = (55.0, 7, 36), 2, 3, 48, 36, 16, 20.0, 4
    n = 252
    rng = P.VqtRange(*geom)
    streams = [[c[1:] for c in SC.plain_frames(n, nf, 900 + s, most=9, every_empty=5)] for s in range(ns)]
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
    d["x_vqt_smoothed"] = torch.from_numpy(np.random.default_rng(8).uniform(0.0, 30.0, (ns, nf, n)).astype(f32)).cuda()
    rendered = P.RenderBatch(rng).rows_device(d, outputs=("spectrogram_vqt", "spectrogram_peaks", "chroma"))
    scene = P.SceneBatch(rng, ns).frames_device(d, frame_time=1.0 / 30.0)
    el = (2.0 + 0.0333 * np.arange(nf)).astype(f32)
    quad = np.asarray([-4.0, 2.0, 16.0, 12.0], f32)
    r = {k: download(v).reshape((ns, nf) + v.shape[1:]) for k, v in rendered.items()}
    for mode in ("spectrogram_vqt", "spectrogram_peaks"):
        back = P.BackdropBatch(rng, ns, W, H, viewport_height=vh).frames(nf, scene)
        P.RasterBatch(rng, ns, W, H, viewport_height=vh).frames_over(back, scene, d, elapsed=el)
        under = download(back).copy()
        ov = P.OverlayBatch(rng, ns, W, H, history_rows=h, viewport_height=vh, ui_scale=0.05, quad=quad)
        feed = rendered if mode == "spectrogram_vqt" else {"spectrogram_peaks": rendered["spectrogram_peaks"], "chroma": rendered["chroma"]}
        assert ov.frames(nf, back, feed) is back
        img = download(back)
        for s in range(ns):
            host, _ = OC.host_chain(n, h, r[mode][s], r["chroma"][s], under[s], quad_=quad, viewport_height=vh, ui_scale=0.05)
            same(img[s], host, ("chain", mode, s))
        assert not np.array_equal(img, under)
    assert r["spectrogram_peaks"][..., 3].any() and r["spectrogram_vqt"][..., 3].any()


def test_row_stride_past_the_draw_grid_cap():
    """overlay_draw (gridDim.y 65 535) over 32 769 streams x 2 frames = 65 538 rows of 3 bins, a ring of 3 rows, quad and boxes on a
    17 x 5 image (two tile columns; ui_scale 0.02 puts nine boxes on pixel centres).  Stream s is pattern s % 61 of 61 distinct
    streams, which the host face and the model pin.  Rows 0, 1, 2 have a second trip, to rows 65 535 .. 65 537: the other frame of
    pattern 10 or 11, so s, f, the ring slot and r - age all change inside the loop; those rows exist only if the kernel strides by
    the very cap the host clamps to."""
    import torch
    n, h, nf, W, H, scale, cap, m = 3, 3, 2, 17, 5, 0.02, 65535, OC.STRIDE_STREAMS
    ns = cap // nf + 2
    total = ns * nf
    assert total == 65538 and cap % m != 0 and cap % nf == 1
    rows, chroma, imgs = OC.stride_streams(nf, n, W, H, 5000)
    host, states, info = references(n, h, rows, chroma, imgs, ui_scale=scale)
    drawn_enough("61 distinct streams", info, host, imgs, n, h)
    assert sum(d["boxed"] for d in info) > m * nf                                   # chroma is present and shows
    # no stride test passes by drawing nothing: a row is empty only where it was crafted so, a quarter of the rows at most
    empty = [(p, f) for p in range(m) for f in range(nf) if not (bits(host[p, f]) != bits(imgs[p, f])).any()]
    assert empty == [(p, f) for p in range(m) for f in range(nf) if p % 11 in OC.STRIDE_EMPTY] and 4 * len(empty) <= m * nf
    of = lambda r: ((r // nf) % m, r % nf)
    for r in range(total - cap):                                                    # a workgroup's second row fits nothing of its first
        (p, f), (q, g) = of(r), of(r + cap)
        assert p != q and f != g and (p, f) not in empty and (q, g) not in empty
        assert (bits(host[p, f]) != bits(host[q, g])).any() and (rows[p, f] != rows[q, g]).any() and (bits(chroma[p, f]) != bits(chroma[q, g])).any()
    small = draw(batch(n, m, W, H, h, ui_scale=scale), imgs, rows, chroma)
    print(f"{m} distinct streams: {small.size} channels, {int((bits(small) != bits(host)).sum())} differ from the host face")
    same(small, host, "61 distinct streams")
    idx = to_device(np.arange(ns, dtype=np.int64) % m)
    buf = torch.full((total * H * W * 4 + 8,), GUARD, dtype=torch.int32, device="cuda")
    buf[4:-4] = to_device(bits(imgs).view(np.int32).reshape(m, -1))[idx].reshape(-1)
    b = batch(n, ns, W, H, h, ui_scale=scale)
    b.frames(nf, buf[4:-4].view(torch.float32), to_device(rows)[idx].contiguous(), to_device(chroma)[idx].contiguous())
    torch.cuda.synchronize()
    big = buf[4:-4].view(ns, -1)
    differing = int((big != to_device(bits(small).view(np.int32).reshape(m, -1))[idx]).sum())
    print(f"{total} rows over {cap} grid rows: {differing} 32-bit words differ from the {m}-stream call")
    assert differing == 0
    assert bool((buf[:4] == GUARD).all()) and bool((buf[-4:] == GUARD).all())
    last = buf[4:-4].view(total, -1)[cap:].cpu().numpy().view(np.uint32)            # rows 65 535 .. 65 537 were drawn on
    for k in range(total - cap):
        p, f = of(cap + k)
        assert (last[k] != bits(imgs[p, f]).ravel()).any(), k
    for s in (0, ns - 1):
        tex, w = b.texture(s)
        want, ww = states[s % m].texture()
        assert np.array_equal(tex, want) and w == ww == nf % h, s


def test_keep_stride_past_two_million_texels():
    """overlay_keep: 11 streams x the last 200 of 203 frames x 1024 bins = 2 252 800 texels over 8192 x 256 = 2 097 152 lanes, on a
    1 x 1 image; the second trip's texels are ring rows 48 .. 199 of the last stream.  Every stream's texture is the host state's,
    and a second call draws from that ring what the host draws"""
    n, h, ns, nf, more = 1024, 200, 11, 203, 3
    assert ns * min(nf, h) * n > 8192 * 256 > (ns - 1) * min(nf, h) * n
    rows, imgs = OC.rows(ns, nf + more, n, 5200), OC.images(ns, nf + more, 1, 1, 5201)
    rows[..., 3] = np.maximum(rows[..., 3], 1)
    b = batch(n, ns, 1, 1, h)
    first = draw(b, imgs[:, :nf], rows[:, :nf])
    ends = (0, ns - 1)
    host = {s: OC.host_chain(n, h, rows[s], None, imgs[s], quad_=OC.full_quad(1, 1, VH), viewport_height=VH) for s in ends}
    kept = {}
    for s in range(ns):
        st = P.OverlayState(n, h)
        for r in rows[s, :nf]:
            st.push(r)
        tex, w = b.texture(s)
        want, ww = st.texture()
        kept[s] = int((tex != want).sum())
        assert w == ww == nf % h and want.any(axis=(1, 2)).sum() == h - 1, s
    print(f"{ns * h * n} texels over {8192 * 256} lanes: differing texture bytes per stream: {kept}")
    assert not any(kept.values()), kept
    second = draw(b, imgs[:, nf:], rows[:, nf:])                                    # ages 3 .. 198 of these frames come from the ring
    for s in ends:
        got = np.concatenate([first[s], second[s]])
        print(f"stream {s}: {got.size} channels, {int((bits(got) != bits(host[s][0])).sum())} differ from the host face")
        same(got, host[s][0], ("images", s))
        assert np.array_equal(b.texture(s)[0], host[s][1].texture()[0]), s
