"""Inputs of the panels stage, shared by tests/test_panels.py (host face against tests/panels_model.py) and tests/test_panels_gpu.py
(device against the host face): rows of an oracle AnalysisState plus crafted rows, for one geometry and one list width.

Everything is float32 from fixed seeds.  A case holds x [rows][n], calmness [rows][n], the peak lists, and the packed arrays the
device reads (entries beyond a row's count are NaN: they must never show)."""
from __future__ import annotations

import numpy as np

import render_cases as RC
import render_model as RM

f32 = np.float32
# 180 / 252 / 588 / 840 bins, 192 | 195 either side of a 64-chunk edge (tests/test_render_gpu.py), then 3 and 1024 bins
GEOMETRIES = [(55.0, 5, 36), (55.0, 7, 36), (55.0, 7, 84), (27.5, 10, 84), (55.0, 8, 24), (55.0, 5, 39), (32.70, 1, 3), (32.70, 16, 64)]


def random_list(n, count, rng):
    """`count` peaks anywhere in [0, n), sizes 0.5 .. 40, in no order (a disc does not care what lies beside it)"""
    c = (rng.random(count, dtype=f32) * f32(n - 0.01)).astype(f32)
    z = (f32(0.5) + rng.random(count, dtype=f32) * f32(39.5)).astype(f32)
    return list(zip(c.tolist(), z.tolist()))


_oracle = {}


def make(min_freq, octaves, bpo, n_rows, seed, max_peaks=None):
    """dict(n, bpo, x, calmness, peaks, center, size, count, max_peaks).  The last five rows are crafted: an all-zero spectrum
    without peaks, a full list, the wrap pair (0.3 and n - 0.4: round reaches n, the table index wraps), centres that saturate
    (negative, NaN), and a calmness row that sits on the class edges."""
    n = octaves * bpo
    rng = np.random.default_rng(seed)
    base = n_rows - 5
    if n >= 8:
        key = (min_freq, octaves, bpo, base, seed)
        if key not in _oracle:                                           # once per geometry, whatever the list width
            _oracle[key] = RM.oracle_rows(min_freq, octaves, bpo, base, seed)
        x, peaks = np.array(_oracle[key][0], f32), [list(p) for p in _oracle[key][1]]
    else:
        x = (rng.random((base, n), dtype=f32) * f32(30.0)).astype(f32)
        peaks = [random_list(n, int(rng.integers(0, 3)), rng) for _ in range(base)]
    if max_peaks is None:
        max_peaks = max(12, max(len(p) for p in peaks))
    peaks = [list(p[:max_peaks]) for p in peaks]
    extra_x = (rng.random((5, n), dtype=f32) * f32(30.0)).astype(f32)
    extra_x[0] = 0.0
    extra_x[3, n // 2] = -3.0                                            # a negative level: alpha above 1 - sqrt(0.5)
    wrap = [(0.3, 5.0), (float(f32(n - 0.4)), 7.0)][:max_peaks]
    odd = [(-0.3, 2.0), (float("nan"), 3.0), (float(f32(n - 0.5)), 0.0)][:max_peaks]
    peaks += [[], random_list(n, max_peaks, rng), wrap, odd, random_list(n, min(max_peaks, 2), rng)]
    x = np.concatenate([x, extra_x])
    calm = rng.random((n_rows, n), dtype=f32)
    edge = np.array([0.71, 0.71, 0.7, 0.7, 0.31, 0.31, 0.3, 0.3, 0.0, 1.0, np.nan, 0.5], f32)
    calm[-1, :] = np.resize(edge, n)
    calm[-2, :] = 0.0
    center, size, count = RC.pack(peaks, max_peaks)
    assert x.shape == (n_rows, n) and count.min() == 0 and count.max() == max_peaks
    return dict(n=n, bpo=bpo, x=x, calmness=calm, peaks=peaks, center=center, size=size, count=count, max_peaks=max_peaks)


def host_rows(P, case):
    """the six outputs of PanelsBatch.rows_device from the host face, disc slots beyond a row's count zero"""
    n, bpo, k = case["n"], case["bpo"], case["max_peaks"]
    rows = len(case["peaks"])
    out = {"line_pos": np.zeros((rows, 4 * (n - 1), 3), f32), "line_rgba": np.zeros((rows, 4 * (n - 1), 4), f32),
           "disc_pos": np.zeros((rows, k, 13, 3), f32), "disc_rgba": np.zeros((rows, k, 13, 4), f32),
           "hist_pos": np.zeros((rows, 4 * (n - 1), 3), f32), "hist_rgba": np.zeros((rows, 4 * (n - 1), 4), f32)}
    for r, pk in enumerate(case["peaks"]):
        s = P.spectrum_mesh(n, bpo, case["x"][r], pk)
        h = P.calmness_histogram_mesh(n, case["calmness"][r])
        out["line_pos"][r], out["line_rgba"][r] = s["line_pos"], s["line_rgba"]
        out["disc_pos"][r, :len(pk)], out["disc_rgba"][r, :len(pk)] = s["disc_pos"], s["disc_rgba"]
        out["hist_pos"][r], out["hist_rgba"][r] = h["pos"], h["rgba"]
    return out


# ---- crafted spectra for util::arg_max, long disc lists, and the rows of the row-stride test ------------------------------------
EDGE_GEOMETRIES = [(55.0, 5, 13), (55.0, 5, 39)]   # 65 bins (the second 64-chunk holds one bin) and 195


def _negatives(n, rng):
    """every entry negative, -0.5 .. -30.5"""
    return (-(rng.random(n, dtype=f32) * f32(30.0)) - f32(0.5)).astype(f32)


def _ordinary(n, rng):
    """0 .. 30 with a negative entry in every fifth bin from bin 2, none of them the maximum"""
    x = (rng.random(n, dtype=f32) * f32(30.0)).astype(f32)
    x[2::5] = -x[2::5] - f32(0.25)
    return x


def edge_spectra(n, seed):
    """{name: (x [n], bin of util::arg_max or None: nothing exceeds f32::MIN and max_size is x[0])}.  Every row holds negative
    entries (but the all-NaN one), so the value and the sign of max_size show in the alphas: x / +0 = -inf, x / -0 = +inf.

    The zero rows hold only zeros and negatives, and come in pairs: `name` and `name_swapped`, the two zeros' signs exchanged.  Where
    the bin count allows it the two zeros sit in one lane of the device's scan (bins 3 and 67) or in two lanes, the lower bin in the
    higher lane's later chunk (bins 5 and 70); at 65 bins the only second-chunk bin is 64, lane 0's."""
    rng = np.random.default_rng(seed)
    out = {}
    pairs = [("zeros_first_and_last", 0, n - 1)]
    if n > 70:
        pairs += [("zeros_one_lane", 3, 67), ("zeros_two_lanes", 5, 70)]
    else:
        pairs += [("zeros_one_lane", 0, 64), ("zeros_two_lanes", 5, 64)]
    for name, lo, hi in pairs:
        base = _negatives(n, rng)
        for tag, first, second in ((name, -0.0, 0.0), (name + "_swapped", 0.0, -0.0)):
            x = base.copy()
            x[lo], x[hi] = first, second
            out[tag] = (x, lo)
    lane = 7
    for name, where in (("nan_at_0", [0]), ("nan_in_a_lane", list(range(lane, n, 64))), ("nan_scattered", [1, 31, 63, 64, n - 2])):
        x = _ordinary(n, rng)
        top = n // 2 + 3
        assert top not in where and top % 5 != 2
        x[top] = 41.5
        x[where] = np.nan
        out[name] = (x, top)
    out["all_nan"] = (np.full(n, np.nan, f32), None)
    out["all_minus_inf"] = (np.full(n, -np.inf, f32), None)
    out["all_minus_flt_max"] = (np.full(n, np.finfo(f32).min, f32), None)
    x = _ordinary(n, rng)
    x[n // 3] = np.inf
    out["plus_inf"] = (x, n // 3)
    for name, at in (("max_at_63", 63), ("max_at_64", 64), ("max_at_last", n - 1)):
        x = _ordinary(n, rng)
        x[at] = 37.25
        out[name] = (x, at)
    return out


def list_case(min_freq, octaves, bpo, max_peaks, counts, seed):
    """a case as `make` gives it whose row r has counts[r] peaks"""
    n = octaves * bpo
    rng = np.random.default_rng(seed)
    x = _ordinary(n, rng)[None].repeat(len(counts), 0) + rng.random((len(counts), 1), dtype=f32)
    peaks = [random_list(n, c, rng) for c in counts]
    center, size, count = RC.pack(peaks, max_peaks)
    return dict(n=n, bpo=bpo, x=x.astype(f32), calmness=rng.random((len(counts), n), dtype=f32), peaks=peaks, center=center, size=size, count=count,
                max_peaks=max_peaks)


DISC_COUNTS = {64: [63, 64, 0, 64, 63, 2], 65: [65, 63, 64, 0, 65, 3, 64], 129: [129, 63, 128, 64, 0, 65, 129, 3, 128]}

STRIDE_ROWS, STRIDE_BINS, STRIDE_PEAKS = 61, 65, 65
STRIDE_KINDS = ("full", "empty", "crossing", "short")


def stride_case(seed=4100):
    """61 distinct rows of 65 bins and 65 peak slots for the row-stride test.  Row i's list is full (65), empty, one that crosses the
    64-chunk (64 or 65) or short (1 .. 4), by i % 4; its spectrum is ordinary, or by i % 7 one with NaN (1), only zeros and
    negatives (3) or all -inf (5); the calmness rows are random, every ninth with a NaN.  Also returns the kinds."""
    n, m = STRIDE_BINS, STRIDE_ROWS
    rng = np.random.default_rng(seed)
    edge = edge_spectra(n, seed + 1)
    special = {1: "nan_scattered", 3: "zeros_two_lanes", 5: "all_minus_inf"}
    xs, peaks, kinds = [], [], []
    for i in range(m):
        kind = STRIDE_KINDS[i % 4]
        count = {"full": STRIDE_PEAKS, "empty": 0, "crossing": 64 + (i // 4) % 2, "short": 1 + (i // 4) % 4}[kind]
        peaks.append(random_list(n, count, rng))
        x = _ordinary(n, rng)
        if i % 7 in special:
            x = edge[special[i % 7]][0].copy()
            x[10 + i % 40] -= f32(1.0 + i)                                  # (a negative entry made lower: no two rows are the same)
        xs.append(x)
        kinds.append((kind, "nan" if i % 7 == 1 else "ordinary" if i % 7 not in special else "other"))
    calm = rng.random((m, n), dtype=f32)
    calm[::9, 5] = np.nan
    center, size, count = RC.pack(peaks, STRIDE_PEAKS)
    case = dict(n=n, bpo=13, x=np.asarray(xs, f32), calmness=calm, peaks=peaks, center=center, size=size, count=count, max_peaks=STRIDE_PEAKS)
    return case, kinds


def model_rows(M, case):
    """host_rows from tests/panels_model.py"""
    n, bpo, k = case["n"], case["bpo"], case["max_peaks"]
    out = {name: np.zeros_like(v) for name, v in host_rows_shapes(case).items()}
    for r, pk in enumerate(case["peaks"]):
        s = M.spectrum_mesh(n, bpo, case["x"][r], pk)
        h = M.calmness_histogram_mesh(n, case["calmness"][r])
        out["line_pos"][r], out["line_rgba"][r] = s["line_pos"], s["line_rgba"]
        out["disc_pos"][r, :len(pk)], out["disc_rgba"][r, :len(pk)] = s["disc_pos"], s["disc_rgba"]
        out["hist_pos"][r], out["hist_rgba"][r] = h["pos"], h["rgba"]
    return out


def host_rows_shapes(case):
    n, k, rows = case["n"], case["max_peaks"], len(case["peaks"])
    return {"line_pos": np.zeros((rows, 4 * (n - 1), 3), f32), "line_rgba": np.zeros((rows, 4 * (n - 1), 4), f32),
            "disc_pos": np.zeros((rows, k, 13, 3), f32), "disc_rgba": np.zeros((rows, k, 13, 4), f32),
            "hist_pos": np.zeros((rows, 4 * (n - 1), 3), f32), "hist_rgba": np.zeros((rows, 4 * (n - 1), 4), f32)}


def stride_follows(m, cap, differ):
    """for the guard of a row-stride test: every i in [0, m) with the row that a workgroup takes after it, (i + cap) % m; asserts
    that the cap is no multiple of m and that `differ(i, j)` holds for every such pair.  Returns the pairs."""
    assert cap % m != 0
    pairs = [(i, (i + cap) % m) for i in range(m)]
    for i, j in pairs:
        assert i != j and differ(i, j), (i, j)
    return pairs
