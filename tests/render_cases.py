"""Crafted inputs of the render stage, shared by tests/test_render.py (host face) and tests/test_render_gpu.py (device): peak lists
whose ORDER decides the picture, lists longer than the kernel's chunk of 64 peaks, centres and sizes at the edges of the domain,
dB rows with values the arithmetic treats specially — and the model's answer for each, computed once per distinct input.

Everything is float32, from fixed seeds, and inside the domain include/pvq.h admits: every centre lies in [0, n_bins), every size is
finite.  The builder checks its own inputs with tests/render_model.py alone (order_dependence, straddle_pair): a list whose reversal
paints the same picture could not tell a kernel that honours list order from one that does not."""
from __future__ import annotations

import numpy as np

import render_model as M

f32 = np.float32
LONG_COUNTS = (64, 65, 127, 128, 129)     # either side of one and of two chunks of 64 peaks
SHORT_COUNTS = (2, 5, 12)
MIN_ORDER_SHARE = 0.05                    # a reordered list must repaint at least this share of the bytes it lights


def spaced_list(n, count, seed, lo=0.3, hi=None, max_gap=3.0):
    """`count` peaks (None: as many as fit) in ascending centre within [lo, hi) (hi: n), neighbours 1.25 .. max_gap bins apart:
    footprints of radius 2 overlap their neighbours', and neighbours' x[lower], x[lower + 1] collide wherever the gap is below 2.
    Sizes are distinct, spread evenly over 1 .. 40 and dealt at random.  None if `count` peaks do not fit."""
    hi = float(n if hi is None else hi)
    rng = np.random.default_rng(seed)
    if count is None:
        u = rng.random(int(hi) + 1)
        c = lo + np.concatenate([[0.0], np.cumsum(1.25 + u * (max_gap - 1.25))])
    else:
        room = (hi - 0.05 - lo) / max(count - 1, 1)                  # mean gap that just fits
        if count > 1 and room < 1.26:
            return None
        u = rng.random(count - 1)
        top = min(max_gap, 2.0 * room - 1.25)                         # gaps uniform in [1.25, top]: their mean is at most `room`
        c = lo + np.concatenate([[0.0], np.cumsum(1.25 + u * (top - 1.25))])
        while c[-1] >= hi - 0.05:                                     # the draw came out above its mean: a lower top, same draw
            top = 1.25 + 0.97 * (top - 1.25)
            c = lo + np.concatenate([[0.0], np.cumsum(1.25 + u * (top - 1.25))])
    c = c.astype(f32)
    c = c[c < f32(hi - 0.01)]
    assert count is None or len(c) == count
    sizes = rng.permutation(np.linspace(1.0, 40.0, len(c))).astype(f32)
    assert len(set(sizes.tolist())) == len(c) and c.min() >= 0.0 and c.max() < n
    return list(zip(c.tolist(), sizes.tolist()))


def orders(peaks, seed):
    """the list in ascending centre, descending centre and a seeded shuffle"""
    asc = sorted(peaks)
    shuffled = [asc[i] for i in np.random.default_rng(seed).permutation(len(asc))]
    return {"ascending": asc, "descending": asc[::-1], "shuffled": shuffled}


def straddle_pair(n, seed):
    """Two lists that differ in the order of entries 63 and 64 alone — the last peak of the first chunk and the first of the second.
    These two are the only peaks that cover bin B, in the spectrogram (0.7 and 0.4 bins from it) and in the LED frame (x[lower + 1]
    of one, x[lower] of the other): whichever way round, the winner sits in another chunk than the loser.  Returns (P then Q,
    Q then P, B)."""
    B = n - 12
    fill = spaced_list(n, 63, seed, hi=B - 5)
    assert fill is not None and max(c for c, _ in fill) < B - 5
    p, q = (float(f32(B - 0.7)), 23.0), (float(f32(B + 0.4)), 31.0)
    tail = [(float(f32(B + 5.3)), 9.0), (float(f32(B + 8.1)), 17.5)]
    covering = [c for c, _ in fill + tail if abs(B - c) <= 2.0 or int(np.floor(c)) in (B - 1, B)]
    assert not covering
    return fill + [p, q] + tail, fill + [q, p] + tail, B


def centre_edges(n, seed):
    """centres 0.0, 0.3, an integer centre k.0 listed after its neighbour at k + 1.4 (fract == 0: x[k + 1] = 0 wipes what the
    neighbour left there), k' + 0.5, n - 3.0, n - 0.4 and n - 1.0 (both in the last bucket; its upper bin does not exist)"""
    k, k2 = n // 2, n // 3
    centres = [0.0, 0.3, k + 1.4, float(k), k2 + 0.5, n - 3.0, n - 0.4, n - 1.0]
    sizes = np.random.default_rng(seed).permutation(np.linspace(2.0, 38.0, len(centres)))
    assert all(0.0 <= f32(c) < n for c in centres)
    return [(float(f32(c)), float(f32(s))) for c, s in zip(centres, sizes)]


def size_sets(peaks):
    """the same centres with all sizes equal, all zero, and one zero among positive ones"""
    zero_one = [(c, 0.0 if i == len(peaks) // 2 else s) for i, (c, s) in enumerate(peaks)]
    return {"equal": [(c, 7.0) for c, _ in peaks], "all_zero": [(c, 0.0) for c, _ in peaks], "one_zero": zero_one}


def db_rows(n, seed):
    """name -> dB row: ordinary (0 .. 30 dB), all negative, one NaN, one +inf, one -inf, one bin whose 10^(v / 10) overflows f32"""
    rng = np.random.default_rng(seed)
    base = (rng.random(n, dtype=f32) * f32(30.0)).astype(f32)
    rows = {"ordinary": base, "negative": (-base - f32(0.5)).astype(f32)}
    for name, v in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf), ("overflow", 400.0)):   # 10^40 > f32::MAX
        r = base.copy()
        r[(2 * n) // 3] = v
        rows[name] = r
    return rows


def edge_rows(n, seed):
    """name -> (dB row, peak list): every dB row of db_rows under the centre-edge list, then an ordinary dB row under the
    centre-edge list reversed and under the size sets of the centre-edge list and of a short overlapping list"""
    xs = db_rows(n, seed)
    edges = centre_edges(n, seed)
    short = spaced_list(n, 12, seed + 12, max_gap=1.7) or spaced_list(n, 2, seed + 2, max_gap=1.7)
    rows = {"db_" + name: (x, edges) for name, x in xs.items()}
    rows["edges_reversed"] = (xs["ordinary"], edges[::-1])
    for tag, pk in (("edges", edges), ("short", short)):
        for name, lst in size_sets(pk).items():
            rows[f"{tag}_{name}"] = (xs["ordinary"], lst)
    return rows


# (min_freq, octaves, buckets_per_octave): every instantiation render_rows<NK>, NK = ceil(n / 64) = 1 .. 16, with both ends of NK = 1
# (3 bins: the least the stage admits), 2 and 16 (1024 bins: the most); buckets per octave below 12 (3, 8), not a multiple of 12
# and above 100 (101, 128, 141); min_freq C, B, A, E, G, D: chroma's bin-0 pitch classes 0, 11, 9, 4, 7, 2
CLASS_TABLE = [
    (32.70, 1, 3), (61.74, 8, 8),             # NK 1: 3, 64
    (55.0, 5, 13), (41.20, 1, 128),           # NK 2: 65, 128
    (49.0, 7, 25), (36.71, 2, 101),           # NK 3: 175; NK 4: 202
    (32.70, 5, 60), (61.74, 9, 41),           # NK 5: 300; NK 6: 369
    (55.0, 6, 72), (41.20, 7, 72),            # NK 7: 432; NK 8: 504
    (49.0, 9, 57), (36.71, 10, 64),           # NK 9: 513; NK 10: 640
    (65.41, 7, 96), (30.87, 5, 141),          # NK 11: 672; NK 12: 705
    (27.5, 11, 75), (82.41, 6, 144),          # NK 13: 825; NK 14: 864
    (98.0, 13, 73),                           # NK 15: 949
    (73.42, 31, 31), (32.70, 16, 64),         # NK 16: 961, 1024
]


def class_rows(n, seed):
    """(dB rows, peak lists) of a class case: an ordinary row, a peakless all-zero row, a centre-edge row and a crowded row —
    as many peaks as fit 1.25 .. 1.75 bins apart, shuffled: more than one chunk of 64 wherever the class has room (n >= 100)"""
    xs = db_rows(n, seed)
    ordinary = spaced_list(n, None, seed, max_gap=12.0)
    crowded = orders(spaced_list(n, None, seed + 1, max_gap=1.75), seed)["shuffled"]
    return [xs["ordinary"], np.zeros(n, f32), xs["negative"], xs["ordinary"]], [ordinary, [], centre_edges(n, seed), crowded]


def list_cases(n, seed):
    """name -> peak list: every long list that fits n bins, the fullest list, short lists, each in three orders; the straddle pair"""
    cases = {}
    for count in SHORT_COUNTS + LONG_COUNTS + (None,):
        # (a short list 1.25 .. 1.7 apart: from 0.3 the second centre falls in bucket 1, so even two peaks collide in the LED frame)
        pk = spaced_list(n, count, seed + (count or 999), max_gap=1.7 if count in SHORT_COUNTS else 3.0)
        if pk is None or (count is None and len(pk) in LONG_COUNTS + SHORT_COUNTS):
            continue
        for name, lst in orders(pk, seed + 1).items():
            cases[f"{'full' if count is None else count}_{name}"] = lst
    if spaced_list(n, 63, seed, hi=n - 17) is not None:
        a, b, _ = straddle_pair(n, seed)
        cases["straddle_pq"], cases["straddle_qp"] = a, b
    return cases


# ---- the model's answers, once per distinct input ---------------------------------------------------------------------------------
_of_peaks, _of_x = {}, {}


def model_of_peaks(n, bpo, peaks, colors=M.COLORS, gray=M.GRAY_LEVEL, easing=M.EASING_POW):
    """(spectrogram row in Peaks mode [n][4], LED frame [3 + 3 n]) of a peak list"""
    key = (n, bpo, tuple(peaks), np.asarray(colors, f32).tobytes(), gray, easing)
    if key not in _of_peaks:
        _of_peaks[key] = (M.spectrogram_row(M.PEAKS, n, bpo, None, peaks, colors=colors, gray_level=gray, easing_pow=easing),
                          np.frombuffer(M.led_frame(n, bpo, peaks, colors, gray, easing), np.uint8))
    return _of_peaks[key]


def model_of_x(min_freq, n, bpo, x):
    """(spectrogram row in VQT mode [n][4], chroma [12]) of a dB row"""
    key = (float(min_freq), n, bpo, np.asarray(x, f32).tobytes())
    if key not in _of_x:
        _of_x[key] = (M.spectrogram_row(M.VQT, n, bpo, x), M.chroma_row(min_freq, n, bpo, x))
    return _of_x[key]


def model_rows(min_freq, n, bpo, xs, peak_lists):
    """the four outputs of rows_device for rows (xs[i], peak_lists[i]), named as RenderBatch.OUTPUTS"""
    px = [model_of_x(min_freq, n, bpo, x) for x in xs]
    pp = [model_of_peaks(n, bpo, pk) for pk in peak_lists]
    return {"spectrogram_vqt": np.asarray([a for a, _ in px]), "chroma": np.asarray([b for _, b in px]),
            "spectrogram_peaks": np.asarray([a for a, _ in pp]), "led": np.asarray([b for _, b in pp])}


def order_dependence(n, bpo, peaks):
    """(spectrogram share, LED share): of the bytes that are non-zero in the picture of `peaks` or of its reversal, the share that
    differs between the two — the model alone"""
    shares = []
    for a, b in zip(model_of_peaks(n, bpo, peaks), model_of_peaks(n, bpo, peaks[::-1])):
        a, b = a.reshape(-1)[3 if a.ndim == 1 else 0:], b.reshape(-1)[3 if b.ndim == 1 else 0:]   # (the LED header is no picture)
        lit = (a != 0) | (b != 0)
        shares.append(float(((a != b) & lit).sum() / max(int(lit.sum()), 1)))
    return tuple(shares)


def pack(peak_lists, max_peaks):
    """(center, size [rows][max_peaks] f32, entries beyond a row's count NaN: never read; count [rows] i32)"""
    center = np.full((len(peak_lists), max_peaks), np.nan, f32)
    size = np.full((len(peak_lists), max_peaks), np.nan, f32)
    count = np.zeros(len(peak_lists), np.int32)
    for r, pk in enumerate(peak_lists):
        assert len(pk) <= max_peaks
        count[r] = len(pk)
        center[r, :len(pk)] = [p[0] for p in pk]
        size[r, :len(pk)] = [p[1] for p in pk]
    return center, size, count


def chroma_agrees(got, want, rel):
    """NaN and inf at identical positions; finite entries within `rel` relative.  Returns the largest relative difference seen."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert g.shape == w.shape
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    assert np.array_equal(np.isposinf(g), np.isposinf(w)) and np.array_equal(np.isneginf(g), np.isneginf(w)), (g, w)
    fin = np.isfinite(w)
    d, s = np.abs(g[fin] - w[fin]), np.abs(w[fin])
    assert np.all(d <= rel * s), float(np.max(d - rel * s))
    return float(np.max(d[s > 0] / s[s > 0])) if np.any(s > 0) else 0.0
