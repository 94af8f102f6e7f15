"""The backdrop stage on the device (pvq_backdrop_batch_*, pvq_backdrop_balls_over_device) against the host face
(pvq_backdrop_frame, pvq_raster_frame).  The bar is tests/test_backdrop.py's: no differing bit in any pixel channel.

Shapes are small and chosen for where the kernels can go wrong: images that are no multiple of the 16 x 16 tile or the 8 x 8 wave
block, lists on both sides of the 64-record ballot chunk and of the 256-lane list-building pass, rows of different lengths in one
call, 3 to 1024 bins."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import backdrop_cases as BC
import pitchvis_amd as P
from test_backdrop import bits, same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
GROUPS = {"bass": ("bass_lit", "bass_rgba"), "line": ("line_pos", "line_rgba"), "disc": ("disc_pos", "disc_rgba", "peak_count"),
          "hist": ("hist_pos", "hist_rgba"), "graph": ("graph_pos", "graph_rgba")}
ALL = tuple(GROUPS)


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run(b, a, nf, tr, groups=ALL, **kw):
    """one device call over the packed arrays `a` -> image [ns][nf][H][W][4]"""
    ins = {k: to_device(a[k]) for g in groups for k in GROUPS[g]}
    return download(b.frames(nf, max_peaks=a["disc_pos"].shape[2], graph_capacity=a["graph_pos"].shape[2] // 4 + 1, **ins, **tr, **kw))


def expect(geom, rows, a, W, H, tr, groups=ALL, **kw):
    """the host face on every row"""
    out = []
    for s, frames in enumerate(rows):
        out.append([])
        for f, m in enumerate(frames):
            panels = {k: v for k, v in m.items() if k.split("_")[0] in groups}
            panels.update(tr)
            lit = int(a["bass_lit"][s, f]) if "bass" in groups else 0
            out[-1].append(P.backdrop_frame(geom[0], geom[1], W, H, bass_lit=lit, bass_rgba=a["bass_rgba"][s, f], panels=panels, **kw))
    return np.asarray(out, f32)


def hold(tag, geom, W, H, a, rows, vh, tr, mode=0, groups=ALL, background=None, **kw):
    ns, nf = a["bass_lit"].shape
    b = P.BackdropBatch(P.VqtRange(55.0, *geom), ns, W, H, visuals_mode=mode, viewport_height=vh)
    img = run(b, a, nf, tr, groups, background=None if background is None else to_device(background), **kw)
    host = expect(geom, rows, a, W, H, tr, groups, viewport_height=vh, visuals_mode=mode, background=background)
    print(f"{tag}: {img.size} channels, {int((bits(img) != bits(host)).sum())} differ from the host face")
    same(img, host, tag)
    return img


def case(geom, ns, nf, W, H, vh, seed, max_peaks=4, capacity=16, **kw):
    n = geom[0] * geom[1]
    a, rows = BC.device_rows(n, geom[1], ns, nf, seed, max_peaks, capacity, segments=min(72 * geom[0], 168) - 1, **kw)
    return a, rows, BC.transforms(rows[0][0], n, capacity, W, H, vh)


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (16, 16), (17, 33), (129, 33)])
def test_image_sizes(size):
    W, H = size
    vh = 3.0
    a, rows, tr = case((2, 12), 2, 2, W, H, vh, 100 + W)
    img = hold(f"{W} x {H}", (2, 12), W, H, a, rows, vh, tr)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > (1 if W * H == 1 else 4)


@pytest.mark.parametrize("geom", [(1, 3), (2, 12), (7, 36), (16, 64)])
def test_geometries(geom):
    W, H, vh = 40, 24, 2.0 * geom[0] + 2.0
    a, rows, tr = case(geom, 1, 2, W, H, vh, 200 + geom[1], max_peaks=3, capacity=12)
    img = hold(f"{geom[0] * geom[1]} bins", geom, W, H, a, rows, vh, tr)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > 8


LENGTHS = (0, 1, 63, 64, 65, 129, 255, 256, 257, 1500)


def crafted_lines(n, lengths, W, H, vh, seed):
    """line meshes [1][len(lengths)][4 (n - 1)][..] whose first `length` triangles lie on the image, translucent, and whose other
    triangles are degenerate (zeros; an odd length ends in a quad whose vertex 3 repeats vertex 0).  A triangle near the end of a
    row's list covers the whole image: drawn out of order it would show."""
    rng = np.random.default_rng(seed)
    hx, hy = 0.5 * vh * W / H, 0.5 * vh
    pos = np.zeros((1, len(lengths), n - 1, 4, 3), f32)
    col = np.zeros((1, len(lengths), n - 1, 4, 4), f32)
    for r, k in enumerate(lengths):
        quads = (k + 1) // 2
        c = rng.uniform([-0.8 * hx, -0.8 * hy], [0.8 * hx, 0.8 * hy], (quads, 1, 2))
        pos[0, r, :quads, :, :2] = c + rng.uniform(-0.35, 0.35, (quads, 4, 2)) * [hx, hy]
        col[0, r, :quads] = rng.uniform(0.0, 1.0, (quads, 1, 4))
        col[0, r, :quads, :, 3] = 0.5
        if k % 2:
            pos[0, r, quads - 1, 3] = pos[0, r, quads - 1, 0]
        if k >= 4:
            big = (k - 2) // 2                                   # its triangle (2, 1, 0), the covering one, is number k - 2 or k - 3
            pos[0, r, big, :, :2] = [[3 * hx, -3 * hy], [0.0, 5 * hy], [-3 * hx, -3 * hy], [0.0, 0.0]]
            col[0, r, big] = [0.2, 0.9, 0.4, 0.6]
    return pos.reshape(1, len(lengths), 4 * (n - 1), 3), col.reshape(1, len(lengths), 4 * (n - 1), 4)


def test_list_lengths_and_order():
    """rows of 0 .. 1500 records in one call: both sides of the ballot chunk (64), of two chunks, of the list pass (256)"""
    geom, W, H, vh = (16, 64), 24, 20, 4.0
    n, nf = 1024, len(LENGTHS)
    a, rows, _ = case(geom, 1, nf, W, H, vh, 300, max_peaks=1, capacity=4)
    a["line_pos"], a["line_rgba"] = crafted_lines(n, LENGTHS, W, H, vh, 301)
    ident = {"spectrum_transform": np.asarray([0.0, 0.0, 1.0, 1.0], f32)}
    for f in range(nf):
        rows[0][f]["line_pos"], rows[0][f]["line_rgba"] = a["line_pos"][0, f], a["line_rgba"][0, f]
    img = hold("lengths", geom, W, H, a, rows, vh, ident, mode=3, groups=("line",))       # Galaxy: the rows' own lists alone
    for f, k in enumerate(LENGTHS):                                                      # no record: the clear colour alone
        assert np.all(img[0, f] == img[0, 0, 0, 0]) == (k == 0), k
    for f, k in enumerate(LENGTHS):
        if k >= 4:   # the same row with the covering triangle drawn first differs: order shows
            m = dict(rows[0][f])
            q = a["line_pos"][0, f].reshape(-1, 4, 3).copy()
            c = a["line_rgba"][0, f].reshape(-1, 4, 4).copy()
            big = (k - 2) // 2
            q[[0, big]], c[[0, big]] = q[[big, 0]], c[[big, 0]]
            m["line_pos"], m["line_rgba"] = q.reshape(-1, 3), c.reshape(-1, 4)
            other = P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3, panels={"line_pos": m["line_pos"], "line_rgba": m["line_rgba"]})
            assert not np.array_equal(other, img[0, f]), k
    hold("lengths over the net", geom, W, H, a, rows, vh, ident, groups=("line", "bass"))


def test_disc_slots_and_counts():
    """slots beyond a row's count are zeros and draw nothing; a count above max_peaks is taken as max_peaks; rows differ"""
    geom, W, H, vh, mp = (2, 12), 33, 17, 3.0, 6
    a, rows, tr = case(geom, 2, 3, W, H, vh, 400, max_peaks=mp, peak_counts=[[0, 1, mp], [mp, 3, 2]])
    hold("slots", geom, W, H, a, rows, vh, tr)
    assert not a["disc_pos"][0, 1, 1:].any() and a["disc_pos"][0, 1, 0].any()
    a["peak_count"][1, 0] = mp + 1000
    hold("count above max_peaks", geom, W, H, a, rows, vh, tr)
    full = hold("discs alone", geom, W, H, a, rows, vh, tr, groups=("disc",))
    none = hold("nothing", geom, W, H, a, rows, vh, tr, groups=())
    assert not np.array_equal(full[1], none[1]) and np.array_equal(full[0, 0], none[0, 0])


def test_modes_background_and_view():
    geom, W, H = (3, 12), 33, 18
    a, rows, tr = case(geom, 1, 2, W, H, 3.0, 500)
    bg = np.random.default_rng(4).uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    plain = hold("full", geom, W, H, a, rows, 3.0, tr)
    galaxy = hold("galaxy", geom, W, H, a, rows, 3.0, tr, mode=3)
    over = hold("background", geom, W, H, a, rows, 3.0, tr, background=bg)
    wide = hold("viewport 9", geom, W, H, a, rows, 9.0, tr)
    bare = hold("no panels", geom, W, H, a, rows, 3.0, tr, groups=("bass",))
    assert not np.array_equal(plain, galaxy) and not np.array_equal(plain, over) and not np.array_equal(plain, wide)
    assert not np.array_equal(plain, bare)
    a["bass_lit"][:] = [[1, 10 ** 6]]                                 # above the segment count: all segments
    hold("bass counts", geom, W, H, a, rows, 3.0, tr)


def test_guards_and_side_stream():
    import torch
    geom, ns, nf, W, H, vh = (2, 12), 2, 3, 19, 9, 3.0
    a, rows, tr = case(geom, ns, nf, W, H, vh, 600)
    ref = hold("reference", geom, W, H, a, rows, vh, tr)
    buf = torch.full((ref.size + 8,), GUARD, dtype=torch.int32, device="cuda")   # 16 bytes of guard either side
    b = P.BackdropBatch(P.VqtRange(55.0, *geom), ns, W, H, viewport_height=vh)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(b, a, nf, tr, image=buf[4:-4].view(torch.float32), stream=side)
    side.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    assert np.all(host[:4] == GUARD) and np.all(host[-4:] == GUARD)
    same(host[4:-4].view(f32), ref.ravel(), "side stream, guarded")


def pieces_case():
    geom, ns, nf, W, H, vh = (2, 12), 2, 7, 24, 20, 3.0
    a, rows, tr = case(geom, ns, nf, W, H, vh, 700)
    return geom, W, H, vh, a, rows, tr


def test_workspace_pieces(tmp_path):
    """the developer library's PVQ_BACKDROP_WS_KB cuts a call of 7 frames into pieces of 2, the last one shorter; same bits"""
    geom, W, H, vh, a, rows, tr = pieces_case()
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
        b = P.BackdropBatch(P.VqtRange(55.0, *geom), a["bass_lit"].shape[0], W, H, viewport_height=vh)
        np.save(sys.argv[1], T.run(b, a, a["bass_lit"].shape[1], tr))
        print("PIECES_OK")
    """)
    f = str(tmp_path / "pieces.npy")
    r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, PVQ_DEV_LIB="1", PVQ_BACKDROP_WS_KB=str(kb)), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "PIECES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    img = hold("one piece", geom, W, H, a, rows, vh, tr)
    same(np.load(f), img, "pieces")


def test_chain():
    """SceneBatch -> PanelsBatch -> BackdropBatch -> RasterBatch.frames_over on 2 streams x 3 frames: every row equals the host chain
    backdrop_frame -> raster_frame(background=...), and the ball times those of a plain frames_device call on a second handle"""
    import scene_cases as SC
    import torch
    geom, ns, nf, W, H, mp, cap, vh = (55.0, 7, 36), 2, 3, 48, 36, 16, 12, 20.0
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
    scene = P.SceneBatch(rng, ns).frames_device(d, frame_time=1.0 / 30.0)
    pb = P.PanelsBatch(rng, ns, graph_capacity=cap)
    panels = pb.rows_device(d)
    graph = pb.graph_device(d["scene_calmness"], first_emitted=0)
    tr = {"spectrum_transform": np.asarray([-9.0, 1.0, 6.0, 2.0], f32), "histogram_transform": np.asarray([-9.0, -1.0, 6.0, -6.0], f32),
          "graph_transform": np.asarray([0.0, -8.0, 12.0, 3.0], f32)}                     # the panels spread over the +-13.3 x +-10 view
    el = (2.0 + 0.0333 * np.arange(nf)).astype(f32)
    back = P.BackdropBatch(rng, ns, W, H, viewport_height=vh).frames(nf, scene, panels, graph, peak_count=d["peak_count"], **tr)
    backdrop = download(back).copy()
    out = P.RasterBatch(rng, ns, W, H, viewport_height=vh).frames_over(back, scene, d, elapsed=el, ball_time=True)
    assert out["image"] is back
    img, bt = download(out["image"]), download(out["ball_time"])
    plain = P.RasterBatch(rng, ns, W, H, viewport_height=vh).frames_device(scene, d, elapsed=el, ball_time=True)
    same(bt, download(plain["ball_time"]), "ball times")
    g = {k: download(v) for k, v in {**scene, **panels, **graph}.items()}
    g = {k: v.reshape((ns, nf) + v.shape[(1 if v.shape[0] == ns * nf else 2):]) for k, v in g.items()}
    for s in range(ns):
        for f in range(nf):
            k = min(int(a["peak_count"][s, f]), mp)
            hp = {key: g[key][s, f] for key in ("line_pos", "line_rgba", "hist_pos", "hist_rgba", "graph_pos", "graph_rgba")}
            hp.update(disc_pos=g["disc_pos"][s, f, :k], disc_rgba=g["disc_rgba"][s, f, :k], **tr)
            hb = P.backdrop_frame(7, 36, W, H, viewport_height=vh, bass_lit=int(g["bass_lit"][s, f]), bass_rgba=g["bass_rgba"][s, f], panels=hp)
            same(backdrop[s, f], hb, ("backdrop", s, f))
            host = P.raster_frame(W, H, g["ball_xyzs"][s, f], g["ball_rgba"][s, f], g["ball_params"][s, f],
                                  g["ball_visible"][s, f].view(np.uint32), bt[s, f], viewport_height=vh, background=hb)
            same(img[s, f], host, ("chain", s, f))
    assert not np.array_equal(img, backdrop) and not np.array_equal(img, download(plain["image"]))
    assert g["bass_lit"].max() > 0 and len(np.unique(backdrop.reshape(-1, 4), axis=0)) > 20


def test_row_stride_past_both_grid_caps():
    """backdrop_lists (8192 workgroups) and backdrop_tiles (gridDim.y 65 535) over 2 streams x 32 799 frames = 65 598 rows of 3 bins on
    a 3 x 2 image in Galaxy mode (no net: a row's own list alone), in one piece.  Row r is row r % 61 of 61 distinct ones, which the
    host face pins.  A list workgroup's next row, r + 8192, is row + 18's of the 61 and a tile workgroup's, r + 65 535, row + 21's:
    another list length (none after four triangles and a disc), so s_base and the wave counts of one row meet the next.  Rows
    65 535 .. 65 597 exist only if the tile kernel strides by the very cap the host clamps to."""
    import torch
    geom, W, H, vh, m = (1, 3), 3, 2, 2.0, BC.STRIDE_ROWS
    ns, nf = 2, 32799
    total = ns * nf
    assert total == 65535 + 63
    cap = 2 * 2 + 12 * 1                                       # mirrors backdrop_batch.hip: two line quads and one disc slot
    per_row = cap * 80 + 4
    assert per_row * total <= 256 << 20                        # one piece: the strides are taken, not cut away
    a, rows = BC.stride_rows(W, H, vh, 9000)
    host = np.asarray([P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3, panels=r) for r in rows], f32)
    clear = P.backdrop_frame(*geom, W, H, viewport_height=vh, visuals_mode=3)
    # no stride test passes by drawing nothing: a row is empty only where it has no triangle, a quarter of the rows at most
    empty = [i for i in range(m) if not (bits(host[i]) != bits(clear)).any()]
    assert empty == [i for i in range(m) if BC.STRIDE_KINDS[i % 11] == (0, 0)] and 4 * len(empty) <= m
    for grid in (8192, 65535):
        assert grid % m != 0 and grid < total
        for i in range(m):
            j = (i + grid) % m
            assert (bits(host[i]) != bits(host[j])).any() and BC.STRIDE_KINDS[i % 11] != BC.STRIDE_KINDS[j % 11], (grid, i, j)
            assert (a["line_pos"][i] != a["line_pos"][j]).any() or (a["disc_pos"][i] != a["disc_pos"][j]).any(), (grid, i, j)
    follows = {(BC.STRIDE_KINDS[i % 11], BC.STRIDE_KINDS[(i + 8192) % m % 11]) for i in range(m)}
    assert ((4, 1), (0, 0)) in follows and any(x == (0, 0) and sum(y) for x, y in follows), follows
    names = ("line_pos", "line_rgba", "disc_pos", "disc_rgba", "peak_count")
    small_in = {k: to_device(a[k]) for k in names}
    rng = P.VqtRange(55.0, *geom)
    small = P.BackdropBatch(rng, 1, W, H, visuals_mode=3, viewport_height=vh).frames(m, **small_in)
    got = download(small)[0]
    print(f"{m} distinct rows: {got.size} channels, {int((bits(got) != bits(host)).sum())} differ from the host face")
    same(got, host, "61 distinct rows")
    assert not (bits(got) == GUARD).any()
    idx = to_device(np.arange(total, dtype=np.int64) % m)
    buf = torch.full((total * H * W * 4 + 8,), GUARD, dtype=torch.int32, device="cuda")
    b = P.BackdropBatch(rng, ns, W, H, visuals_mode=3, viewport_height=vh)
    b.frames(nf, **{k: v[idx].contiguous() for k, v in small_in.items()}, image=buf[4:-4].view(torch.float32))
    torch.cuda.synchronize()
    big = buf[4:-4].view(total, -1)
    differing = int((big != small.view(torch.int32).view(m, -1)[idx]).sum())
    unwritten = int((big[8192:] == GUARD).sum())                                    # of rows 8192 .. and 65 535 ..
    print(f"{total} rows over 8192 list workgroups and 65535 tile rows: {differing} 32-bit words differ from the {m}-row call; "
          f"{unwritten} words of rows 8192 .. are still the fill value")
    assert differing == 0 and unwritten == 0
    assert bool((buf[:4] == GUARD).all()) and bool((buf[-4:] == GUARD).all())
