"""Crafted inputs of the pitch-ball scene, shared by tests/test_scene.py (host face against tests/scene_model.py) and
tests/test_scene_gpu.py (device against host): peak lists longer than the device's chunk of 64 whose ORDER decides the scene, hide
ranges at the ends of the admitted buckets-per-octave with their known answers, entries outside the usual domain, frame times at
the edges of Duration::as_secs_f32, and plain random frames for the calls that only need many of them.

Frames have the tuple form of scene_model.crafted_frames: (name, peaks, calmness, pitch_accuracy, pitch_deviation, scene_calmness).
Everything is float32, from fixed seeds.  The builders check their own inputs with the model alone."""
from __future__ import annotations

import numpy as np

import scene_model as M

f32 = np.float32
DT = 33_333_333
LONG_COUNTS = (64, 65, 127, 128, 129, 200)     # either side of one and of two chunks of 64 peaks, and into the fourth
# (octaves, buckets_per_octave): 3 bins, the least the stage admits, both ways round; bpo below 12 (hide radius 0); 63 / 64 / 65
# bins, either side of one 64-chunk; 961, the first count of scene_frames<16>; 1023 and 1024, with the largest hide radius
GEOMS_EDGE = [(1, 3), (3, 1), (7, 9), (1, 64), (5, 13), (1, 65), (31, 31), (11, 93), (1, 1024), (2, 512)]
FRAME_TIMES_NS = (0, 1, 1_000_000_000, 5_000_000_007, 2 ** 40)   # as_secs_f32 splits seconds and nanoseconds: none, both, large


def fields(n, rng):
    return rng.random(n).astype(f32), rng.random(n).astype(f32), (rng.random(n).astype(f32) - f32(0.5)), f32(rng.random())


def plain_frames(n, n_frames, seed, most=6, every_empty=7):
    """n_frames ordinary frames: up to `most` peaks at random centres in [0, n) with sizes in 1 .. 40, random per-bin fields; every
    `every_empty`-th frame has no peaks"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n_frames):
        k = 0 if f % every_empty == every_empty - 1 else int(rng.integers(1, most + 1))
        c = (rng.random(k) * (n - 0.02)).astype(f32)
        z = (1.0 + 39.0 * rng.random(k)).astype(f32)
        out.append((f"plain_{f}", list(zip(c.tolist(), z.tolist()))) + fields(n, rng))
    return out


def balls(g):
    return np.concatenate([np.asarray(g["ball_xyzs"]).ravel(), np.asarray(g["ball_rgba"]).ravel()])


def long_list(n, count, seed):
    """`count` peaks whose keys repeat across the chunks of 64 both ways round.  Keys come from a pool of about count / 3 bins spread
    over [0, n), so most keys are entered several times and the LAST entry decides the ball.  Key A is entered in chunk 0 only
    (its last entry at index 40; the later chunks hold other keys); key B is entered at index 5 and again as the first entry of
    every later chunk (64, 128, 192).  Sizes are distinct."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.linspace(0, n - 1, min(n, max(3, count // 3))).round().astype(int))
    assert len(pool) >= 3
    a, b = int(pool[len(pool) // 2]), int(pool[-1])
    rest = np.array([k for k in pool if k != a])
    keys = rng.choice(pool, count)
    keys[64:] = rng.choice(rest, max(0, count - 64))
    keys[[3, 40]] = a
    keys[41:64][keys[41:64] == a] = rest[0]
    keys[5] = b
    keys[64::64] = b
    centres = (keys + 0.05 + 0.9 * rng.random(count)).astype(f32)
    assert np.array_equal(np.trunc(centres).astype(int), keys) and centres.max() < n
    sizes = rng.permutation(np.linspace(1.0, 40.0, count)).astype(f32)
    assert len(set(sizes.tolist())) == count
    assert a in keys[:64] and a not in keys[64:] and (count <= 64 or (keys[64] == b and keys[5] == b))
    return list(zip(centres.tolist(), sizes.tolist()))


_order_checked = set()


def order_decides(octaves, bpo, frame):
    """the model alone: the list and its reversal leave different balls (a list whose reversal looks the same cannot tell 'the last
    entry of a key wins' from 'the first wins')"""
    a, b = M.SceneModel(octaves, bpo), M.SceneModel(octaves, bpo)
    a.update(frame[1], *frame[2:], DT)
    b.update(frame[1][::-1], *frame[2:], DT)
    return not np.array_equal(balls(a.get()), balls(b.get()), equal_nan=True)


def long_lists(n, bpo, seed, counts=LONG_COUNTS):
    rng = np.random.default_rng(seed)
    out = [(f"long_{count}", long_list(n, count, seed + count)) + fields(n, rng) for count in counts]
    if (n, bpo, seed, counts) not in _order_checked:
        for fr in out:
            assert order_decides(n // bpo, bpo, fr), fr[0]
        _order_checked.add((n, bpo, seed, counts))
    return out


# ---- hide ranges: update.rs:307-330 with radius (bpo / 12) as f32 * 0.23 ---------------------------------------------------------------
# (octaves, bpo) -> (centre, the run of neighbouring balls lit first, the bins of the run the single peak hides)
HIDE_TABLE = {
    # radius 85 * 0.23 = 19.55
    (1, 1024): [(63.4, range(40, 90), range(44, 84)),        # round(43.85) ..= round(82.95), across the 63 / 64 chunk boundary
                (5.2, range(0, 30), range(0, 26)),           # round(-14.35) clamps at 0 ..= round(24.75)
                (1020.3, range(995, 1024), range(1001, 1024))],   # round(1000.75) ..= round(1039.85) clamps at 1023
    # radius 0: a peak hides exactly the bin round(centre), unless that is its own
    (7, 9): [(20.7, range(17, 25), [21]), (20.2, range(17, 25), [])],
    (1, 12): [(5.4, range(2, 10), [6]), (5.2, range(2, 10), [])],   # radius 0.23: round(5.17) ..= round(5.63); round(4.97) ..= round(5.43)
    (1, 11): [(5.4, range(2, 10), []), (5.7, range(2, 10), [6])],   # radius 0 again: 11 / 12 = 0
}


def hide_cases(octaves, bpo):
    """[(name, [frame that lights the run, single-peak frame], run, hidden, key)]: after the two frames the balls of `run` are
    visible except those of `hidden`; the peak's own ball `key` stays.  The named geometries carry the answers written out above;
    any other gets one case from the reference's expression in f32 (centre n / 2 + 0.7, away from every rounding boundary)."""
    n = octaves * bpo
    table = HIDE_TABLE.get((octaves, bpo))
    if table is None:
        radius = f32(f32(bpo // 12) * f32(0.23))
        c = f32(n // 2 + 0.7)
        lo = max(int(M.rround(f32(c - radius))), 0)
        hi = min(int(M.rround(f32(c + radius))), n - 1)
        run = range(max(lo - 3, 0), min(hi + 4, n))
        table = [(float(c), run, range(lo, hi + 1))]
    z = np.zeros(n, f32)
    out = []
    for c, run, hidden in table:
        key = int(c)
        hidden = sorted(set(hidden) - {key})
        assert key in run and set(hidden) <= set(run)
        light = ("hide_light", [(float(f32(b + 0.5)), 30.0) for b in run], z, z, z, f32(0.0))
        single = ("hide_single", [(float(f32(c)), 30.0)], z, z, z, f32(0.0))
        out.append((f"hide_{c}", [light, single], list(run), hidden, key))
    return out


def hide_holds(get, case):
    """the known answer of a hide case on a face's get() after the case's two frames"""
    _, _, run, hidden, key = case
    vis = set(np.nonzero(np.unpackbits(np.asarray(get["ball_visible"]).view(np.uint8), bitorder="little"))[0].tolist())
    assert set(run) & vis == set(run) - set(hidden) and key in vis, (case[0], sorted(set(run) & vis), hidden)


# ---- entries outside the usual domain ----------------------------------------------------------------------------------------------
def edge_entries(n, seed=7):
    """One odd list per frame, each between two ordinary frames (so what it leaves on its balls is seen to fade): sizes with both
    signs of zero as the maximum, NaN, infinite, negative and at both ends of f32; centres NaN, infinite, negative, at and beyond
    n, and whole numbers.  The sizes sit on distinct keys (from 4 bins on; at 3 bins one key repeats).  Names that hold 'nan_centre' mark the
    lists tests/scene_model.py refuses (its u8 conversion raises where Rust's `as u8` gives 0)."""
    nan, inf = float("nan"), float("inf")
    keys = [(1 + i) % n if n < 8 else 1 + i * ((n - 2) // 4) for i in range(4)]
    on = lambda sizes: [(float(f32(k + 0.3)), s) for k, s in zip(keys, sizes)]
    m = n // 2
    odd = [("zero_max_pos_first", on([-1.0, 0.0, -0.0, -3.0])),      # the first maximum is +0: z of entry 0 is -inf
           ("zero_max_neg_first", on([-2.0, -0.0, 0.0])),            # the first maximum is -0
           ("nan_size_first", on([nan, 5.0, 9.0, 2.0])),
           ("all_nan_sizes", on([nan, nan, nan])),                   # nothing exceeds f32::MIN: max_size is size[0]
           ("all_minus_inf", on([-inf, -inf, -inf])),
           ("one_plus_inf", on([4.0, inf, 7.0])),
           ("huge_and_tiny", on([3e38, 1e-40])),
           ("nan_centre", [(m + 0.3, 5.0), (nan, 9.0), (min(m + 1.6, n - 0.4), 3.0)]),
           ("nan_centre_first", [(nan, 6.0), (m + 0.3, 5.0)]),       # the bass spiral reads the first entry
           ("inf_centre", [(m + 0.3, 5.0), (inf, 9.0)]),
           ("negative_centres", [(m + 0.3, 5.0), (-0.5, 9.0), (-3.0, 4.0)]),   # both reach key 0, the later wins; x and y are NaN
           ("beyond_n", [(float(n), 8.0), (n - 0.5, 5.0), (1e12, 30.0)]),      # only n - 0.5 has a ball
           ("whole_centres", [(0.0, 3.0), (float(m), 8.0), (float(n - 1), 5.0)])]
    rng = np.random.default_rng(seed)
    plain = plain_frames(n, len(odd) + 1, seed + 1, most=4, every_empty=10 ** 9)
    out = [plain[0]]
    for i, (name, pk) in enumerate(odd):
        out.append((name, [(float(f32(c)), float(f32(s))) for c, s in pk]) + fields(n, rng))
        out.append(plain[i + 1])
    return out


def edge_fields(n, seed=11):
    """Ordinary lists over per-bin fields that hold NaN, +inf and -inf under lit keys, and scene_calmness NaN, -1, +inf, 0.5"""
    out = []
    for i, scene in enumerate((float("nan"), -1.0, float("inf"), 0.5)):
        name, pk, calm, acc, dev, _ = plain_frames(n, 1, seed + i, most=5, every_empty=10 ** 9)[0]
        pk = pk + [(float(f32(n // 2 + 0.4)), 12.0)]
        ks = [int(c) for c, _ in pk]
        for arr, vals in ((calm, (np.nan, np.inf, -np.inf)), (acc, (np.inf, np.nan, -np.inf)), (dev, (-np.inf, np.inf, np.nan))):
            arr[ks[i % len(ks)]] = vals[i % 3]
            arr[ks[-1]] = vals[(i + 1) % 3]
        out.append((f"fields_{i}", pk, calm, acc, dev, f32(scene)))
        out.append(plain_frames(n, 1, seed + 10 + i, most=3, every_empty=10 ** 9)[0])
    return out


def close_with_specials(got, want, rel):
    """x, y and the colour channels where the frames hold infinities (scene_model.compare takes the largest difference of an array,
    which a pair of equal infinities turns into NaN): NaN, +inf and -inf in the same places, every finite value within
    rel * max(1, |want|).  Returns the largest finite |difference| / max(1, |want|)."""
    worst = 0.0
    for k, cols in (("ball_xyzs", slice(0, 2)), ("ball_rgba", slice(None)), ("bass_rgba", slice(None))):
        g, w = np.asarray(got[k], np.float64)[..., cols], np.asarray(want[k], np.float64)[..., cols]
        for special in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(special(g), special(w)), (k, special.__name__)
        fin = np.isfinite(w)
        if fin.any():
            d = np.abs(g[fin] - w[fin]) / np.maximum(1.0, np.abs(w[fin]))
            worst = max(worst, float(d.max()))
    assert worst <= rel, worst
    return worst
