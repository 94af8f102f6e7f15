"""REFERENCE MODEL (test infrastructure only) of the viewer's three debug panels: a literal NumPy-f32 restatement of
pitchvis_viewer/src/display_system/update.rs:474-638 (update_spectrum with CircleGeometry::new :435-471), :640-742
(update_scene_calmness_graph with SceneCalmnessHistory, mod.rs:114-133) and :744-869 (update_calmness_histogram), with
calmness_to_color (:27-35), as sequential loops, line for line; written independently of pitchvis_amd/csrc.  The colour mapping is
oracle/consumers.py's, unchanged.

Assumed third-party semantics: f32::hypot is the double-precision function rounded once to f32; powf(t, 0.5) is the correctly
rounded f32 square root; cos / sin of a disc angle are the double functions rounded once; Color::srgb(..).to_srgba() gives its
arguments back with alpha 1.0; Vec3::new stores its arguments."""
from __future__ import annotations

import math

import numpy as np

from render_model import COLORS, GRAY_LEVEL, _rem, calculate_color

f32 = np.float32
TAU = f32(6.2831855)                       # std::f32::consts::TAU
F32_MIN = f32(np.finfo(np.float32).min)


def _round(v):
    """f32::round: half away from zero; NaN and infinities pass"""
    v = float(v)
    if not math.isfinite(v):
        return v
    return math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)


def _usize(v):
    """`as usize` of an f64-held f32: saturating at both ends, NaN -> 0"""
    if v != v or v <= 0:
        return 0
    return 2 ** 64 - 1 if v >= 2.0 ** 64 else int(v)


def arg_max(sl):
    """util.rs:48-57: fold from (0, f32::MIN) with `>`"""
    cur = (0, F32_MIN)
    for i, x in enumerate(sl):
        if x > cur[1]:
            cur = (i, x)
    return cur[0]


def calmness_to_color(calmness):
    """update.rs:27-35, as [r, g, b, a] of to_srgba()"""
    if calmness > f32(0.7):
        return [f32(0.5), f32(0.8), f32(1.0), f32(1.0)]
    if calmness > f32(0.3):
        return [f32(1.0), f32(1.0), f32(0.5), f32(1.0)]
    return [f32(1.0), f32(0.5), f32(0.5), f32(1.0)]


def line_quad(p, q, thickness):
    """update.rs:531-541 = :691-700 = :815-827: [v0, v1, v2, v3], each (x, y, z); also the length l"""
    with np.errstate(all="ignore"):
        dx = f32(p[0] - q[0])
        dy = f32(p[1] - q[1])
        l = f32(np.sqrt(np.float64(dx) * dx + np.float64(dy) * dy))
        u = f32(f32(f32(dx * f32(thickness)) * f32(0.5)) / l)
        v = f32(f32(f32(dy * f32(thickness)) * f32(0.5)) / l)
        return [(f32(p[0] + v), f32(p[1] - u), f32(0.0)), (f32(p[0] - v), f32(p[1] + u), f32(0.0)),
                (f32(q[0] - v), f32(q[1] + u), f32(0.0)), (f32(q[0] + v), f32(q[1] - u), f32(0.0))], l


_colors = {}


def _spectrum_color(bpo, i, colors, gray_level):
    """update.rs:560-569 / :588-597 (remembered per argument tuple: the model is called row after row)"""
    key = (bpo, i, np.asarray(colors, f32).tobytes(), float(gray_level))
    if key not in _colors:
        _colors[key] = _spectrum_color_uncached(bpo, i, colors, gray_level)
    return _colors[key]


def _spectrum_color_uncached(bpo, i, colors, gray_level):
    return calculate_color(bpo, _rem(f32(f32(f32(i) + f32(0.5)) + f32(bpo - 3 * (bpo // 12))), f32(bpo)), colors, gray_level, 10.0)


def spectrum_mesh(n_buckets, bpo, x_vqt_smoothed, peaks_continuous=(), colors=COLORS, gray_level=GRAY_LEVEL):
    """update.rs:506-615: dict of line_pos [4 (n - 1)][3], line_rgba [4 (n - 1)][4], disc_pos [k][13][3], disc_rgba [k][13][4]"""
    x = np.asarray(x_vqt_smoothed, f32)
    assert x.size == n_buckets
    max_size = x[arg_max(x)]                                                    # update.rs:512-513
    with np.errstate(all="ignore"):
        points = [(f32(f32(i) * f32(0.011)), f32(amp / f32(10.0)), f32(0.0)) for i, amp in enumerate(x)]   # update.rs:520
        pos, rgba = [], []
        for p, q in zip(points[:-1], points[1:]):                               # tuple_windows
            pos += line_quad(p, q, 0.02)[0]
        for i in range(n_buckets - 1):                                          # update.rs:558-577
            r, g, b = _spectrum_color(bpo, i, colors, gray_level)
            coefficient = f32(f32(1.0) - np.sqrt(f32(f32(0.5) - f32(f32(x[i] / max_size) / f32(2.0)))))
            rgba += [[f32(r), f32(g), f32(b), coefficient]] * 4
        disc_pos, disc_rgba = [], []
        for center, size in peaks_continuous:                                   # update.rs:582-615
            center, size = f32(center), f32(size)
            peak_x = f32(center * f32(0.011))
            peak_y = f32(size / f32(10.0))
            bin_ = _usize(_round(center))
            r, g, b = _spectrum_color(bpo, bin_ % bpo, colors, gray_level)      # (exact in f32: the bucket depends on bin % bpo alone)
            verts = [(peak_x, peak_y, f32(0.0))]                                # update.rs:442
            for i in range(12):                                                 # update.rs:446-455
                angle = f32(f32(f32(i) / f32(12.0)) * TAU)
                verts.append((f32(peak_x + f32(f32(0.08) * f32(math.cos(float(angle))))),
                              f32(peak_y + f32(f32(0.08) * f32(math.sin(float(angle))))), f32(0.0)))
            disc_pos.append(verts)
            disc_rgba.append([[f32(r), f32(g), f32(b), f32(0.9)]] * 13)
    k = len(disc_pos)
    return {"line_pos": np.asarray(pos, f32).reshape(4 * (n_buckets - 1), 3), "line_rgba": np.asarray(rgba, f32).reshape(4 * (n_buckets - 1), 4),
            "disc_pos": np.asarray(disc_pos, f32).reshape(k, 13, 3), "disc_rgba": np.asarray(disc_rgba, f32).reshape(k, 13, 4)}


def calmness_histogram_mesh(n_buckets, calmness):
    """update.rs:787-845: dict of pos, rgba; the skipped count as "skipped" (always 0: see pitchvis_amd/csrc/panels_math.hpp)"""
    c = np.asarray(calmness, f32)
    assert c.size == n_buckets
    pos, rgba, skipped = [], [], 0
    with np.errstate(all="ignore"):
        for i in range(n_buckets - 1):
            c0, c1 = c[i], c[i + 1]
            p = (f32(f32(i) * f32(0.011)), f32(c0 * f32(0.5)), f32(0.0))
            q = (f32(f32(i + 1) * f32(0.011)), f32(c1 * f32(0.5)), f32(0.0))
            color = calmness_to_color(f32(f32(c0 + c1) / f32(2.0)))
            quad, l = line_quad(p, q, 0.01)
            if l < f32(0.0001):                                                 # update.rs:818-820
                skipped += 1
                continue
            pos += quad
            rgba += [color] * 4
    return {"pos": np.asarray(pos, f32).reshape(-1, 3), "rgba": np.asarray(rgba, f32).reshape(-1, 4), "skipped": skipped}


class CalmnessGraph:
    """SceneCalmnessHistory (mod.rs:114-133) and update_scene_calmness_graph (update.rs:652-718)"""

    def __init__(self, capacity=300):
        self.capacity = capacity
        self.values = [f32(0.0)] * capacity
        self.write_index = 0

    def push(self, value):                                                      # update.rs:656-658
        self.values[self.write_index] = f32(value)
        self.write_index = (self.write_index + 1) % self.capacity

    def mesh(self):
        cap = self.capacity
        with np.errstate(all="ignore"):
            points = []
            for i in range(cap):                                                # update.rs:662-667
                buffer_idx = (self.write_index + i) % cap
                points.append((f32(f32(f32(i) / f32(cap)) - f32(0.5)), self.values[buffer_idx], f32(0.0)))
            pos, rgba = [], []
            for i in range(len(points) - 1):                                    # update.rs:675-718
                color = calmness_to_color(self.values[(self.write_index + i) % cap])
                pos += line_quad(points[i], points[i + 1], 0.01)[0]
                rgba += [color] * 4
        return {"pos": np.asarray(pos, f32).reshape(4 * (cap - 1), 3), "rgba": np.asarray(rgba, f32).reshape(4 * (cap - 1), 4),
                "history": np.asarray([p[1] for p in points], f32)}


def panel_topology(n_quads, n_circles=0):
    """(indices, uvs) of n_quads quads (update.rs:543-554) followed by n_circles discs (update.rs:442, :454, :458-463)"""
    idx, uvs = [], []
    for _ in range(n_quads):
        prior_len = len(uvs)
        idx += [2 + prior_len, 1 + prior_len, prior_len, 2 + prior_len, prior_len, 3 + prior_len]
        uvs += [[0.0, 1.0], [0.0, 0.0], [1.0, 0.0], [1.0, 1.0]]
    for _ in range(n_circles):
        base = len(uvs)
        uvs.append([0.5, 0.5])
        for i in range(12):
            angle = f32(f32(f32(i) / f32(12.0)) * TAU)
            uvs.append([f32(f32(0.5) + f32(f32(0.5) * f32(math.cos(float(angle))))), f32(f32(0.5) + f32(f32(0.5) * f32(math.sin(float(angle)))))])
            idx += [base, base + 1 + i, base + 1 + ((i + 1) % 12)]
    return np.asarray(idx, np.uint32), np.asarray(uvs, f32).reshape(-1, 2)


def same_bits(got, want):
    """the number of 32-bit words that differ between two float32 arrays of one shape (a NaN matches a NaN of any payload)"""
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert g.shape == w.shape, (g.shape, w.shape)
    differ = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    return int(differ.sum())
