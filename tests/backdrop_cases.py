"""Inputs of the backdrop stage, shared by tests/test_backdrop.py (host face against tests/backdrop_model.py) and
tests/test_backdrop_gpu.py (device against the host face).  Everything is float32 from fixed seeds.

A panel mesh here is what the panels stage's host face makes of a random row.  Its transform is chosen so that the case tests
something: the centroid of one quad (or one disc's centre) is put on a pixel centre, and the scale makes a bin's step 1.5 pixels wide,
so the 0.01 - 0.02 thick lines are a few pixels thick and most of the mesh lies on the image.  The view is narrowed for the same
reason: at the viewer's +-7.87 the 0.05-wide net is below a pixel on every image a test can afford."""
from __future__ import annotations

import numpy as np

import pitchvis_amd as P

f32 = np.float32
OCTAVES, BPO = 2, 12
SIZES = [(1, 1), (7, 5), (33, 17), (128, 96)]


def view(W, H):
    """a viewport height at which net and bass are certain to show: on odd heights a pixel centre lies at (-0.6, 0), the first
    spiral point (the first bass segment reaches 0.005 beyond it, 0.025 to either side); 128 x 96 has a pixel pitch of 0.03125, under
    0.05 / sqrt(2)"""
    if (W, H) == (128, 96):
        return 3.0
    k = max(1, min((W - 1) // 2, 7))
    return float(f32(H * 0.6 / k))


def pixel_centre(W, H, vh, i, j):
    s = f32(vh) / f32(H)
    return float((f32(i) + f32(0.5) - f32(0.5) * f32(W)) * s), float((f32(0.5) * f32(H) - (f32(j) + f32(0.5))) * s)


def onto(points, W, H, vh, i, j, sx, sy):
    """(tx, ty, sx, sy) that puts the mean of `points` [k][>= 2] on the centre of pixel (i, j)"""
    cx, cy = pixel_centre(W, H, vh, i, j)
    m = np.asarray(points, np.float64)[:, :2].mean(0)
    return np.asarray([cx - sx * m[0], cy - sy * m[1], sx, sy], f32)


def random_meshes(n, bpo, seed, n_peaks=3, capacity=16, pushes=11):
    """the four meshes of a random row, named as pvq_backdrop_panels names them"""
    rng = np.random.default_rng(seed)
    x = (rng.random(n, dtype=f32) * f32(30.0)).astype(f32)
    peaks = [(float(c), float(z)) for c, z in zip(rng.random(n_peaks) * (n - 1), 2.0 + rng.random(n_peaks) * 25.0)]
    if peaks:   # the first disc sits on the middle of the line's middle quad, which `transforms` puts on a pixel centre
        k = (n - 1) // 2
        peaks[0] = (k + 0.5, float((x[k] + x[k + 1]) / 2))
    s = P.spectrum_mesh(n, bpo, x, peaks)
    h = P.calmness_histogram_mesh(n, rng.random(n, dtype=f32))
    g = P.CalmnessGraph(capacity)
    for v in rng.random(pushes):
        g.push(float(v))
    gm = g.mesh()
    return {"line_pos": s["line_pos"], "line_rgba": s["line_rgba"], "disc_pos": s["disc_pos"], "disc_rgba": s["disc_rgba"],
            "hist_pos": h["pos"], "hist_rgba": h["rgba"], "graph_pos": gm["pos"], "graph_rgba": gm["rgba"]}


def transforms(meshes, n, capacity, W, H, vh, top="spectrum"):
    """spectrum, histogram (mirrored: sy < 0) and graph transforms as the module's note describes.  On 1 x 1 all three would land
    on the one pixel, where the opaque histogram and graph hide what lies under them: there only `top` ("spectrum": line and discs,
    "graph" or "hist") stays on the pixel and the other two go beside it, and the cases take turns."""
    pitch = vh / H
    q = lambda a, b: (min(W - 1, a * W // 4), min(H - 1, b * H // 4))
    step = 1.5 * pitch
    k = (n - 1) // 2
    out = {"spectrum_transform": onto(meshes["line_pos"][4 * k:4 * k + 4], W, H, vh, *q(1, 1), step / 0.011, 0.3 * vh / 3.0),
           "histogram_transform": onto(meshes["hist_pos"][4 * k:4 * k + 4], W, H, vh, *q(3, 3), step / 0.011, -0.3 * vh / 0.5)}
    c = (capacity - 1) // 2
    out["graph_transform"] = onto(meshes["graph_pos"][4 * c:4 * c + 4], W, H, vh, *q(1, 3), step * capacity, 0.3 * vh)
    if (W, H) == (1, 1):
        for k, (name, axis) in enumerate((("spectrum", 1), ("histogram", 0), ("graph", 1))):
            if name[:4] != top[:4]:
                out[name + "_transform"][axis] += f32((40.0 + 10.0 * k) * vh)
    return out


def host_case(W, H, seed=1, n_peaks=3, capacity=16, top="spectrum"):
    """(vh, panels dict for pitchvis_amd.backdrop_frame) on the module's geometry"""
    n = OCTAVES * BPO
    vh = view(W, H)
    m = random_meshes(n, BPO, seed, n_peaks, capacity)
    m.update(transforms(m, n, capacity, W, H, vh, top))
    return vh, m


BASS_RGBA = np.asarray([0.9, 0.35, 0.2, 0.8], f32)


def frame_cases():
    """(W, H, mode, bass_lit, with panels, with background) — every size with both modes, the four bass counts, panels and
    background on and off"""
    segments = min(72 * OCTAVES, 168) - 1
    out = []
    for W, H in SIZES:
        for mode in (0, 3):
            for k, lit in enumerate((0, 1, segments, segments + 50)):
                out.append((W, H, mode, lit, bool(k & 1), bool(k & 2)))
        out += [(W, H, 0, 0, True, True), (W, H, 0, segments, True, False)]
    return out


# ---- device rows: [ns][nf] meshes from the host face, packed as the scene and panels stages lay them out -----------------------
def device_rows(n, bpo, ns, nf, seed, max_peaks, capacity, peak_counts=None, lit=None, segments=143):
    """dict of arrays [ns][nf][...] (disc slots beyond a row's count are zeros, as the panels stage leaves them), and per row the
    host panels dict without transforms"""
    rng = np.random.default_rng(seed)
    a = {"line_pos": np.zeros((ns, nf, 4 * (n - 1), 3), f32), "line_rgba": np.zeros((ns, nf, 4 * (n - 1), 4), f32),
         "hist_pos": np.zeros((ns, nf, 4 * (n - 1), 3), f32), "hist_rgba": np.zeros((ns, nf, 4 * (n - 1), 4), f32),
         "disc_pos": np.zeros((ns, nf, max_peaks, 13, 3), f32), "disc_rgba": np.zeros((ns, nf, max_peaks, 13, 4), f32),
         "graph_pos": np.zeros((ns, nf, 4 * (capacity - 1), 3), f32), "graph_rgba": np.zeros((ns, nf, 4 * (capacity - 1), 4), f32),
         "peak_count": np.zeros((ns, nf), np.int32), "bass_lit": np.zeros((ns, nf), np.int32), "bass_rgba": np.zeros((ns, nf, 4), f32)}
    rows = []
    for s in range(ns):
        rows.append([])
        for f in range(nf):
            k = int(rng.integers(0, max_peaks + 1)) if peak_counts is None else peak_counts[s][f]
            m = random_meshes(n, bpo, int(rng.integers(1 << 30)), k, capacity, pushes=capacity // 2 + f)
            for key, v in m.items():
                if key.startswith("disc"):
                    a[key][s, f, :k] = v
                else:
                    a[key][s, f] = v
            a["peak_count"][s, f] = k
            a["bass_lit"][s, f] = int(rng.integers(0, segments + 30)) if lit is None else lit[s][f]
            a["bass_rgba"][s, f] = rng.random(4, dtype=f32)
            rows[-1].append(m)
    return a, rows


# ---- the row-stride test: 61 distinct rows of 3 bins (two line quads) and one disc slot -------------------------------------------
STRIDE_ROWS = 61
# (line triangles, discs) of row i, by i % 11: 11 shares no factor with the steps a workgroup takes through the 61 rows
STRIDE_KINDS = ((4, 0), (1, 0), (4, 1), (0, 0), (2, 0), (4, 0), (0, 0), (1, 1), (2, 1), (0, 1), (4, 1))


def stride_rows(W, H, vh, seed):
    """(arrays [61][...] of line_pos, line_rgba, disc_pos, disc_rgba, peak_count; per row the host panels dict): translucent
    triangles a pixel or two wide around pixel centres; a row's unused line triangles are degenerate (zeros; an odd count ends in a
    quad whose vertex 3 repeats vertex 0), its unused disc slot is zeros"""
    m, n = STRIDE_ROWS, 3
    rng = np.random.default_rng(seed)
    pitch = vh / H
    a = {"line_pos": np.zeros((m, n - 1, 4, 3), f32), "line_rgba": np.zeros((m, n - 1, 4, 4), f32), "disc_pos": np.zeros((m, 1, 13, 3), f32),
         "disc_rgba": np.zeros((m, 1, 13, 4), f32), "peak_count": np.zeros(m, np.int32)}
    rows = []
    for r in range(m):
        tris, discs = STRIDE_KINDS[r % 11]
        quads = (tris + 1) // 2
        for q in range(quads):
            c = pixel_centre(W, H, vh, int(rng.integers(0, W)), int(rng.integers(0, H)))
            a["line_pos"][r, q, :, :2] = np.asarray(c) + np.asarray([[0.9, -0.8], [0.1, 1.1], [-1.0, -0.7], [0.2, -1.2]]) * pitch * rng.uniform(0.8, 1.6)
            a["line_rgba"][r, q] = np.append(rng.uniform(0.1, 1.0, 3), 0.5)
        if tris % 2:
            a["line_pos"][r, quads - 1, 3] = a["line_pos"][r, quads - 1, 0]
        if discs:
            c = pixel_centre(W, H, vh, int(rng.integers(0, W)), int(rng.integers(0, H)))
            ang = 2.0 * np.pi * np.arange(12) / 12.0
            a["disc_pos"][r, 0, 0, :2] = c
            a["disc_pos"][r, 0, 1:, :2] = np.asarray(c) + pitch * rng.uniform(0.7, 1.4) * np.stack([np.cos(ang), np.sin(ang)], 1)
            a["disc_rgba"][r, 0] = np.append(rng.uniform(0.1, 1.0, 3), 0.9)
        a["peak_count"][r] = discs
        rows.append({"line_pos": a["line_pos"][r].reshape(-1, 3), "line_rgba": a["line_rgba"][r].reshape(-1, 4),
                     "disc_pos": a["disc_pos"][r, :discs], "disc_rgba": a["disc_rgba"][r, :discs]})
    a["line_pos"], a["line_rgba"] = a["line_pos"].reshape(m, 4 * (n - 1), 3), a["line_rgba"].reshape(m, 4 * (n - 1), 4)
    return a, rows
