"""Crafted ball rows and peak lists for the raster tests (tests/test_raster.py, tests/test_raster_gpu.py): deterministic, no library
call.  A row is a dict of the arrays pvq_scene_state_get gives for one frame: ball_xyzs [n][4], ball_rgba [n][4], ball_params [n][3],
ball_visible [ceil(n / 32)]."""
import numpy as np

f32 = np.float32
HALF_VIEW = 7.87     # half of the viewer's 38 * 0.41421357 world units


def pack_visible(bits):
    bits = np.asarray(bits, bool)
    pad = np.zeros((-len(bits)) % 32, bool)
    return np.packbits(np.concatenate([bits, pad]), bitorder="little").view(np.uint32).copy()


def row(n, seed, drawable=None, kind="mixed", z_levels=5, spread=HALF_VIEW):
    """n balls, `drawable` of them visible with a positive scale (default: about a third).  kind: "mixed" sizes from a tenth of
    a pixel to the whole view, "small" (a few pixels of a 64-row image: long lists stay cheap).  z comes from z_levels values, so
    equal z is the rule; both signs of zero are among them."""
    rng = np.random.default_rng(seed)
    xyzs, rgba, par = np.zeros((n, 4), f32), np.zeros((n, 4), f32), np.zeros((n, 3), f32)
    xyzs[:, 0] = rng.uniform(-spread * 1.2, spread * 1.2, n)      # some centres lie off the image
    xyzs[:, 1] = rng.uniform(-spread * 1.2, spread * 1.2, n)
    levels = np.concatenate([[0.0, -0.0], -rng.uniform(0.0, 12.0, max(z_levels - 2, 0))]).astype(f32)
    xyzs[:, 2] = levels[rng.integers(0, len(levels), n)]
    if kind == "small":
        xyzs[:, 3] = rng.uniform(0.01, 0.05, n)
    else:
        xyzs[:, 3] = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), n))   # side 0.02 (under a pixel) .. 40 (over the view)
    rgba[:, :3] = rng.uniform(0.0, 1.0, (n, 3))
    rgba[:, 3] = rng.uniform(0.3, 1.0, n)
    par[:, 0] = np.where(rng.random(n) < 0.3, rng.uniform(0.61, 1.0, n), rng.uniform(0.0, 0.6, n))   # calmness; >= 0.61: a flat disc
    par[:, 1] = rng.uniform(0.5, 1.05, n)                          # accuracy on both sides of 0.85
    par[:, 2] = rng.uniform(-0.6, 0.6, n)                          # deviation, |dev| > 0.5: a negative star brightness
    k = n // 3 if drawable is None else drawable
    vis = np.zeros(n, bool)
    vis[rng.permutation(n)[:k]] = True
    return {"ball_xyzs": xyzs, "ball_rgba": rgba, "ball_params": par, "ball_visible": pack_visible(vis)}


def edge_row(n=36):
    """every rule of the composition in one row of >= 24 balls: overlapping discs at equal z (bin order decides), z = -inf and the
    other non-finite values (skipped), +-0 as one z, balls off the image, across its edge, larger than it, smaller than a pixel,
    an invisible ball and scales <= 0 on top of everything (they must not show)"""
    assert n >= 24
    r = row(n, 77, drawable=0)
    x, c, p = r["ball_xyzs"], r["ball_rgba"], r["ball_params"]
    vis = np.zeros(n, bool)

    def put(b, pos, z, scale, rgba, calm=0.7, acc=0.5, dev=0.0, visible=True):
        x[b] = (pos[0], pos[1], z, scale)
        c[b] = rgba
        p[b] = (calm, acc, dev)
        vis[b] = visible
    put(0, (0.0, 0.0), -12.0, 3.0, (0.2, 0.3, 0.4, 1.0), calm=0.2, acc=1.0, dev=0.2)        # larger than the image, under all
    put(1, (-1.0, 0.5), -3.0, 0.3, (1.0, 0.0, 0.0, 0.5))                                     # two flat discs, equal z:
    put(5, (1.0, 0.5), -3.0, 0.3, (0.0, 1.0, 0.0, 0.5))                                      # bin 5 over bin 1
    put(2, (0.0, -1.0), 0.0, 0.25, (0.0, 0.0, 1.0, 0.6))                                     # +0 and -0 are one z:
    put(3, (0.5, -1.5), -0.0, 0.25, (1.0, 1.0, 0.0, 0.6))                                    # bin 3 over bin 2
    put(4, (0.0, 0.0), -np.inf, 0.4, (9.0, 9.0, 9.0, 1.0))                                   # z = -inf: not finite, skipped
    put(6, (HALF_VIEW, 0.0), -1.0, 0.2, (0.5, 0.1, 0.9, 0.9), calm=0.1, acc=0.95, dev=-0.3)  # across the right edge
    put(7, (0.0, HALF_VIEW + 1.5), -1.0, 0.2, (0.5, 0.9, 0.1, 0.9), calm=0.1)                # across the top edge
    put(8, (40.0, 3.0), -1.0, 0.3, (1.0, 1.0, 1.0, 1.0))                                     # off the image
    put(9, (0.3, 0.2), -0.5, 0.0005, (1.0, 1.0, 1.0, 1.0), calm=0.9)                         # side 0.01: under a pixel
    put(10, (0.0, 0.0), 5.0, 0.5, (7.0, 7.0, 7.0, 1.0), visible=False)                       # on top, but invisible
    put(11, (0.0, 0.0), 5.0, 0.0, (7.0, 7.0, 7.0, 1.0))                                      # scale 0
    put(12, (0.0, 0.0), 5.0, -0.5, (7.0, 7.0, 7.0, 1.0))                                     # scale < 0
    bad = [(0, np.nan), (1, np.inf), (2, np.nan), (3, np.inf)]                               # x, y, z, scale
    for i, (col, v) in enumerate(bad):
        put(13 + i, (0.0, 0.0), 5.0, 0.5, (7.0, 7.0, 7.0, 1.0))
        x[13 + i, col] = v
    for i in range(4):                                                                       # r, g, b, a
        put(17 + i, (0.0, 0.0), 5.0, 0.5, (7.0, 7.0, 7.0, 1.0))
        c[17 + i, i] = np.nan if i % 2 else -np.inf
    for i in range(3):                                                                       # calmness, accuracy, deviation
        put(21 + i, (0.0, 0.0), 5.0, 0.5, (7.0, 7.0, 7.0, 1.0))
        p[21 + i, i] = np.nan if i % 2 else np.inf
    r["ball_visible"] = pack_visible(vis)
    return r


def stack(rows_by_stream):
    """[streams][frames] rows -> arrays [ns][nf][...]"""
    return {k: np.ascontiguousarray(np.asarray([[r[k] for r in frames] for frames in rows_by_stream]))
            for k in ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible")}


def peak_lists(n, ns, nf, seed, most=6, empty_every=3):
    """[streams][frames] lists of centers: every empty_every-th frame has none; some centers are at or above n, negative or NaN"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(ns):
        frames = []
        for f in range(nf):
            if (f + s) % empty_every == empty_every - 1:
                frames.append([])
                continue
            c = list(rng.uniform(0.0, n, rng.integers(1, most + 1)).astype(f32))
            if f % 4 == 1:
                c += [f32(n), f32(n + 0.5), f32(-3.0), f32(np.nan), f32(n - 0.25), f32(0.99)]   # ignored: >= n; -3 and NaN key bin 0
            frames.append(c)
        out.append(frames)
    return out


def pack_peaks(lists, max_peaks, counts=None):
    """-> center [ns][nf][max_peaks] (entries past the count hold a bin that must not be touched), peak_count [ns][nf]"""
    ns, nf = len(lists), len(lists[0])
    center = np.full((ns, nf, max_peaks), 1.5, f32)
    count = np.zeros((ns, nf), np.uint32)
    for s in range(ns):
        for f in range(nf):
            c = lists[s][f][:max_peaks]
            center[s, f, :len(c)] = c
            count[s, f] = len(lists[s][f]) if counts is None else counts[s][f]
    return center, count


# ---- the row-stride test: 61 distinct streams of a few frames, 3 bins ------------------------------------------------------------
STRIDE_STREAMS = 61
STRIDE_BALLS = (3, 1, 3, 0, 2)          # drawable balls of stream pattern p, by p % 5: none after three where the patterns wrap


def stride_rows(nf, W, H, seed, vh=2.0 * HALF_VIEW, n=3):
    """[61][nf] rows of n balls whose drawable ones sit within a fifth of a pixel of a pixel centre of the W x H image and are 0.6
    to 2.5 pixels wide, so that on an image of a few pixels a drawable ball shows"""
    pitch = vh / H
    out = []
    for p in range(STRIDE_STREAMS):
        frames = []
        for f in range(nf):
            rng = np.random.default_rng(seed + 10 * p + f)
            r = row(n, seed + 10 * p + f, drawable=STRIDE_BALLS[p % 5])
            i, j = rng.integers(0, W, n), rng.integers(0, H, n)
            r["ball_xyzs"][:, 0] = (i + 0.5 - 0.5 * W) * pitch + rng.uniform(-0.2, 0.2, n) * pitch
            r["ball_xyzs"][:, 1] = (0.5 * H - (j + 0.5)) * pitch + rng.uniform(-0.2, 0.2, n) * pitch
            r["ball_xyzs"][:, 3] = rng.uniform(0.6, 2.5, n) * pitch / 20.0     # the rectangle's side is 20 scale
            frames.append(r)
        out.append(frames)
    return out
