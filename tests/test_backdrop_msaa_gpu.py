"""The multisampled backdrop on the device (a backdrop batch handle made with samples = 4: backdrop_tiles_msaa) against the host face
(backdrop_frame(samples=4)).  The bar is the backdrop's own: no differing bit in any pixel channel.

Shapes are those of tests/test_backdrop_gpu.py where the kernel can go wrong: images off the 16 x 16 tile and the 8 x 8 wave block, the
ends of the bin range, lists on both sides of the 64-record ballot chunk and of the list pass, workspace pieces, rows past the grid
cap.  The inputs are that file's, so the one-sample pictures of the same rows are at hand to compare with."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import backdrop_cases as BC
import backdrop_msaa_model as MM
import pitchvis_amd as P
import raster_cases as RC
import test_backdrop_gpu as T
from pitchvis_amd import _lib
from test_backdrop import bits, same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = T.ROOT
GUARD = T.GUARD
ALL = T.ALL


def hold4(tag, geom, W, H, a, rows, vh, tr, mode=0, groups=ALL, background=None, samples=4, **kw):
    """one device call through a handle of `samples` against the host face of the same sample count on every row"""
    ns, nf = a["bass_lit"].shape
    b = P.BackdropBatch(P.VqtRange(55.0, *geom), ns, W, H, visuals_mode=mode, viewport_height=vh, samples=samples)
    assert b.samples == samples and b._L.pvq_msaa_batch_samples(b._h) == samples
    img = T.run(b, a, nf, tr, groups, background=None if background is None else T.to_device(background), **kw)
    host = T.expect(geom, rows, a, W, H, tr, groups, viewport_height=vh, visuals_mode=mode, background=background, samples=samples)
    print(f"{tag}: {img.size} channels, {int((bits(img) != bits(host)).sum())} differ from the host face with {samples} samples")
    same(img, host, tag)
    return img


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (16, 16), (17, 33)])
def test_image_sizes(size):
    W, H = size
    vh = 3.0
    a, rows, tr = T.case((2, 12), 2, 2, W, H, vh, 100 + W)
    img = hold4(f"{W} x {H}", (2, 12), W, H, a, rows, vh, tr)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > (1 if W * H == 1 else 4)
    if size != (17, 33):
        return
    # not vacuous: the picture differs from the one-sample device picture, and exactly where the model allows it to — every pixel
    # whose four samples and centre every triangle covers alike carries the one-sample bits
    one = hold4("17 x 33, one sample", (2, 12), W, H, a, rows, vh, tr, samples=1)
    n_alike = n_differ = 0
    for s in range(2):
        for f in range(2):
            panels = dict(rows[s][f], **tr)
            alike = np.ones((H, W), bool)
            MM.frame(2, 12, W, H, viewport_height=vh, bass_lit=int(a["bass_lit"][s, f]), bass_rgba=a["bass_rgba"][s, f], panels=panels, alike=alike)
            differ = (bits(img[s, f]) != bits(one[s, f])).any(-1)
            same(img[s, f][alike], one[s, f][alike], ("samples agree", s, f))
            assert differ.any() and not alike.all(), (s, f)
            n_alike += int(alike.sum())
            n_differ += int(differ.sum())
    print(f"17 x 33: {n_differ} of {4 * W * H} pixels differ from the one-sample device picture; {n_alike} pixels have all samples covered as "
          "the centre is and hold its bits")


@pytest.mark.parametrize("geom", [(1, 3), (16, 64)])
def test_geometries(geom):
    W, H, vh = 40, 24, 2.0 * geom[0] + 2.0
    a, rows, tr = T.case(geom, 1, 2, W, H, vh, 200 + geom[1], max_peaks=3, capacity=12)
    img = hold4(f"{geom[0] * geom[1]} bins", geom, W, H, a, rows, vh, tr)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > 8


LENGTHS = (0, 1, 63, 64, 65, 129, 257, 1500)


def test_list_lengths_and_order():
    """rows of 0 .. 1500 records in one call: both sides of the ballot chunk (64), of two chunks, of the list pass (256).  The late
    covering triangle of the crafted lines covers every sample of every pixel: drawn out of order it would show."""
    geom, W, H, vh = (16, 64), 24, 20, 4.0
    n, nf = 1024, len(LENGTHS)
    a, rows, _ = T.case(geom, 1, nf, W, H, vh, 300, max_peaks=1, capacity=4)
    a["line_pos"], a["line_rgba"] = T.crafted_lines(n, LENGTHS, W, H, vh, 301)
    ident = {"spectrum_transform": np.asarray([0.0, 0.0, 1.0, 1.0], f32)}
    for f in range(nf):
        rows[0][f]["line_pos"], rows[0][f]["line_rgba"] = a["line_pos"][0, f], a["line_rgba"][0, f]
    img = hold4("lengths", geom, W, H, a, rows, vh, ident, mode=3, groups=("line",))       # Galaxy: the rows' own lists alone
    for f, k in enumerate(LENGTHS):                                                      # no record: the clear colour alone
        assert np.all(img[0, f] == img[0, 0, 0, 0]) == (k == 0), k
    for f, k in enumerate(LENGTHS):
        if k >= 4:   # the same row with the covering triangle drawn first differs: order shows
            q = a["line_pos"][0, f].reshape(-1, 4, 3).copy()
            c = a["line_rgba"][0, f].reshape(-1, 4, 4).copy()
            big = (k - 2) // 2
            q[[0, big]], c[[0, big]] = q[[big, 0]], c[[big, 0]]
            other = P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3, samples=4,
                                     panels={"line_pos": q.reshape(-1, 3), "line_rgba": c.reshape(-1, 4)})
            assert not np.array_equal(other, img[0, f]), k
    hold4("lengths over the net", geom, W, H, a, rows, vh, ident, groups=("line", "bass"))


def test_modes_background_view_and_side_stream():
    import torch
    geom, W, H = (3, 12), 33, 18
    a, rows, tr = T.case(geom, 1, 2, W, H, 3.0, 500)
    bg = np.random.default_rng(4).uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    plain = hold4("full", geom, W, H, a, rows, 3.0, tr)
    galaxy = hold4("galaxy", geom, W, H, a, rows, 3.0, tr, mode=3)
    over = hold4("background", geom, W, H, a, rows, 3.0, tr, background=bg)
    wide = hold4("viewport 9", geom, W, H, a, rows, 9.0, tr)
    assert not np.array_equal(plain, galaxy) and not np.array_equal(plain, over) and not np.array_equal(plain, wide)
    # a side stream, into a guarded buffer: 16 bytes of guard either side
    buf = torch.full((plain.size + 8,), GUARD, dtype=torch.int32, device="cuda")
    b = P.BackdropBatch(P.VqtRange(55.0, *geom), 1, W, H, viewport_height=3.0, samples=4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        T.run(b, a, 2, tr, image=buf[4:-4].view(torch.float32), stream=side)
    side.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    assert np.all(host[:4] == GUARD) and np.all(host[-4:] == GUARD)
    same(host[4:-4].view(f32), plain.ravel(), "side stream, guarded")


def test_workspace_pieces(tmp_path):
    """the developer library's PVQ_BACKDROP_WS_KB cuts a call of 7 frames into pieces of 2, the last one shorter; same bits"""
    geom, W, H, vh, a, rows, tr = T.pieces_case()
    ns, nf = a["bass_lit"].shape
    cap = 2 * 23 + 12 * 4 + 2 * 15 + 2 * 23 + 2 * 143          # mirrors backdrop_batch.hip: every group at its maximum
    per_row = cap * 80 + 4
    kb = (per_row * ns * 2 + per_row) // 1024 + 1
    assert (kb * 1024) // (per_row * ns) == 2 and nf % 2 == 1
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, "tests")
        import numpy as np
        import pitchvis_amd as P
        from pitchvis_amd import _lib
        import test_backdrop_gpu as T
        assert _lib.LIB_PATH.endswith("libpvq_dev.so")
        geom, W, H, vh, a, rows, tr = T.pieces_case()
        b = P.BackdropBatch(P.VqtRange(55.0, *geom), a["bass_lit"].shape[0], W, H, viewport_height=vh, samples=4)
        np.save(sys.argv[1], T.run(b, a, a["bass_lit"].shape[1], tr))
        print("PIECES_OK")
    """)
    f = str(tmp_path / "pieces.npy")
    r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, PVQ_DEV_LIB="1", PVQ_BACKDROP_WS_KB=str(kb)), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "PIECES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    img = hold4("one piece", geom, W, H, a, rows, vh, tr)
    same(np.load(f), img, "pieces")


def test_row_stride_past_the_grid_cap():
    """backdrop_tiles_msaa (gridDim.y 65 535) over 2 streams x 32 799 frames = 65 598 rows of 3 bins on a 1 x 1 image in Galaxy mode (a
    row's own list alone), in one piece.  Row r is row r % 61 of 61 distinct ones, which the host face pins; a tile workgroup's next
    row, r + 65 535, is row + 21's of the 61.  Rows 65 535 .. 65 597 exist only if the kernel strides by the cap the host clamps to.
    The rows' triangles, a pixel or two wide, are halved about the pixel's centre, so that most of them cover some of its samples
    and not others."""
    import torch
    geom, W, H, vh, m = (1, 3), 1, 1, 2.0, BC.STRIDE_ROWS
    ns, nf = 2, 32799
    total = ns * nf
    assert total == 65535 + 63
    assert (2 * 2 + 12 * 1) * 80 + 4 <= (256 << 20) // total       # one piece: the stride is taken, not cut away
    a, rows = BC.stride_rows(W, H, vh, 9000)
    half = np.asarray([0.0, 0.0, 0.5, 0.5], f32)
    host = np.asarray([P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3, panels=dict(r, spectrum_transform=half), samples=4)
                       for r in rows], f32)
    one = np.asarray([P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3, panels=dict(r, spectrum_transform=half)) for r in rows], f32)
    clear = P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3, samples=4)
    drawn = [i for i in range(m) if (bits(host[i]) != bits(clear)).any()]
    stride_shows = [i for i in range(m) if (bits(host[i]) != bits(host[(i + 65535) % m])).any()]
    partial = int((bits(host) != bits(one)).any((1, 2, 3)).sum())
    print(f"{len(drawn)} of {m} rows draw on the one pixel, {partial} otherwise than with one sample, {len(stride_shows)} differ from the row a "
          "stride of 65535 further on")
    assert 2 * len(drawn) > m and 2 * partial > m and 2 * len(stride_shows) > m
    names = ("line_pos", "line_rgba", "disc_pos", "disc_rgba", "peak_count")
    small_in = {k: T.to_device(a[k]) for k in names}
    rng = P.VqtRange(55.0, *geom)
    small = P.BackdropBatch(rng, 1, W, H, visuals_mode=3, viewport_height=vh, samples=4).frames(m, spectrum_transform=half, **small_in)
    got = T.download(small)[0]
    print(f"{m} distinct rows: {got.size} channels, {int((bits(got) != bits(host)).sum())} differ from the host face")
    same(got, host, "61 distinct rows")
    idx = T.to_device(np.arange(total, dtype=np.int64) % m)
    buf = torch.full((total * H * W * 4 + 8,), GUARD, dtype=torch.int32, device="cuda")
    b = P.BackdropBatch(rng, ns, W, H, visuals_mode=3, viewport_height=vh, samples=4)
    b.frames(nf, **{k: v[idx].contiguous() for k, v in small_in.items()}, spectrum_transform=half, image=buf[4:-4].view(torch.float32))
    torch.cuda.synchronize()
    big = buf[4:-4].view(total, -1)
    differing = int((big != small.view(torch.int32).view(m, -1)[idx]).sum())
    unwritten = int((big[65535:] == GUARD).sum())
    print(f"{total} rows over 65535 tile rows: {differing} 32-bit words differ from the {m}-row call; {unwritten} words of rows 65535 .. are still "
          "the fill value")
    assert differing == 0 and unwritten == 0
    assert bool((buf[:4] == GUARD).all()) and bool((buf[-4:] == GUARD).all())


def test_one_sample_handle():
    """a handle made by pvq_msaa_batch_create with samples = 1 gives the bits of one made by the one-sample create"""
    geom, ns, nf, W, H, vh = (2, 12), 2, 3, 19, 9, 3.0
    a, rows, tr = T.case(geom, ns, nf, W, H, vh, 600)
    old = P.BackdropBatch(P.VqtRange(55.0, *geom), ns, W, H, viewport_height=vh)
    new = P.BackdropBatch(P.VqtRange(55.0, *geom), ns, W, H, viewport_height=vh)
    L = new._L
    L.pvq_backdrop_batch_destroy(new._h)
    new._h = C.c_void_p()
    assert L.pvq_msaa_batch_create(1, 0, geom[0], geom[1], 0, vh, ns, W, H, C.byref(new._h)) == _lib.PVQ_OK and new._h.value
    assert L.pvq_msaa_batch_samples(new._h) == 1 and L.pvq_msaa_batch_samples(old._h) == 1
    want, got = T.run(old, a, nf, tr), T.run(new, a, nf, tr)
    print(f"one-sample handle: {int((bits(got) != bits(want)).sum())} of {got.size} channels differ from the one-sample create's")
    same(got, want, "one-sample handle")
    same(got, T.expect(geom, rows, a, W, H, tr, viewport_height=vh), "and the host face")


def test_chain():
    """BackdropBatch(samples=4).frames -> RasterBatch.frames_over on 2 streams x 3 frames: every row equals the host chain
    backdrop_frame(samples=4) -> raster_frame(background=...): the later layers run on the resolved picture as they are"""
    geom, ns, nf, W, H, vh, mp = (2, 12), 2, 3, 24, 20, 3.0, 6
    n = geom[0] * geom[1]
    a, rows, tr = T.case(geom, ns, nf, W, H, vh, 800)
    ball_rows = [[RC.row(n, 40 + 7 * s + f, spread=0.4 * vh) for f in range(nf)] for s in range(ns)]
    for frames in ball_rows:
        for r in frames:
            r["ball_xyzs"][:, 3] *= f32(vh / 16.0)                    # balls sized for the narrowed view
    balls = {k: T.to_device(v) for k, v in RC.stack(ball_rows).items()}
    center, count = RC.pack_peaks(RC.peak_lists(n, ns, nf, 14), mp)
    el = (2.0 + 0.0333 * np.arange(nf)).astype(f32)
    rng = P.VqtRange(55.0, *geom)
    bd = P.BackdropBatch(rng, ns, W, H, viewport_height=vh, samples=4)
    ins = {k: T.to_device(a[k]) for g in ALL for k in T.GROUPS[g]}
    back = bd.frames(nf, max_peaks=a["disc_pos"].shape[2], graph_capacity=a["graph_pos"].shape[2] // 4 + 1, **ins, **tr)
    backdrop = T.download(back).copy()
    out = P.RasterBatch(rng, ns, W, H, viewport_height=vh).frames_over(back, balls, center=T.to_device(center), peak_count=T.to_device(count),
                                                                      elapsed=el, ball_time=True)
    assert out["image"] is back
    img, bt = T.download(out["image"]), T.download(out["ball_time"])
    host_back = T.expect(geom, rows, a, W, H, tr, viewport_height=vh, samples=4)
    same(backdrop, host_back, "backdrop, four samples")
    for s in range(ns):
        for f in range(nf):
            r = ball_rows[s][f]
            host = P.raster_frame(W, H, r["ball_xyzs"], r["ball_rgba"], r["ball_params"], r["ball_visible"], bt[s, f], viewport_height=vh,
                                  background=host_back[s, f])
            same(img[s, f], host, ("chain", s, f))
    print(f"chain: {img.size} channels equal the host chain; {int((bits(img) != bits(backdrop)).any(-1).sum())} pixels hold a ball")
    assert not np.array_equal(img, backdrop)
    assert not np.array_equal(backdrop, T.expect(geom, rows, a, W, H, tr, viewport_height=vh))
