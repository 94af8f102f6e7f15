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
