"""NumPy model of the backdrop stage (include/pvq.h, "the backdrop"): float32, operation for operation, with no pixel boxes and no
culling — it tries every triangle on every pixel.  The static geometry is restated from pitchvis_viewer/src/display_system/
setup.rs:127-222 with mod.rs:277-306 and util.rs:3-20; libm calls are Python's double-precision functions rounded once to f32."""
import math

import numpy as np

import panels_model as PM
import raster_model as RM
import scene_model as SM

f32 = np.float32
NET_SPIRAL, NET_RAYS, BASS = 0, 1, 2
GALAXY = 3
POINTS_PER_OCTAVE, BASS_POINTS = 72, 168
LAYERS = ("net", "line", "disc", "graph", "hist", "bass")
CHUNK = 128   # triangles whose coverage is worked out at a time


def counts(octaves):
    return {NET_SPIRAL: 72 * octaves - 1, NET_RAYS: 12, BASS: min(72 * octaves, 168) - 1}


def geometry(octaves, what):
    """[n][4][2]"""
    out = []
    if what == NET_RAYS:
        radius = f32(f32(octaves) * f32(2.2))
        for i in range(12):
            angle = f32(f32(f32(f32(i) / f32(12.0)) * f32(2.0)) * f32(math.pi))
            px, py = f32(math.cos(float(angle))), f32(math.sin(float(angle)))
            quad, _ = PM.line_quad((f32(0.0), f32(0.0)), (f32(radius * px), f32(radius * py)), 0.05)
            out.append([[v[0], v[1]] for v in quad])
        return np.asarray(out, f32)
    pts = [SM.bin_to_spiral(POINTS_PER_OCTAVE, i) for i in range(POINTS_PER_OCTAVE * octaves)]
    for i in range(counts(octaves)[what]):
        p, q = pts[i], pts[i + 1]
        if what == NET_SPIRAL:
            quad, _ = PM.line_quad(p, q, 0.05)
            out.append([[v[0], v[1]] for v in quad])
            continue
        dx, dy = f32(p[0] - q[0]), f32(p[1] - q[1])
        h = f32(np.sqrt(np.float64(dx) * dx + np.float64(dy) * dy))
        mx, my = f32(f32(p[0] + q[0]) * f32(0.5)), f32(f32(p[1] + q[1]) * f32(0.5))
        ux, uy = f32(dx / h), f32(dy / h)
        hw, hl = f32(f32(0.05) * f32(0.5)), f32(f32(h + f32(0.01)) * f32(0.5))
        ax, ay = f32(hw * uy), f32(hw * f32(-ux))
        bx, by = f32(hl * ux), f32(hl * uy)
        out.append([[f32(f32(mx + ax) + bx), f32(f32(my + ay) + by)], [f32(f32(mx - ax) + bx), f32(f32(my - ay) + by)],
                    [f32(f32(mx - ax) - bx), f32(f32(my - ay) - by)], [f32(f32(mx + ax) - bx), f32(f32(my + ay) - by)]])
    return np.asarray(out, f32)


def panel_transforms(n_bins, W, H, viewport_height=0.0):
    vh = RM.VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    max_y = f32(vh / f32(2.0))
    max_x = f32(max_y * f32(f32(W) / f32(H)))
    tx = f32(f32(max_x - f32(f32(n_bins) * f32(0.011))) - f32(0.2))
    ty = f32(max_y - f32(4.2))
    return np.asarray([[tx, ty, 1.0, 1.0], [tx, ty, 1.0, -1.0], [-5.0, -6.5, 3.0, 1.0]], f32)


def quad_triangles(quads):
    """[n][4][2] -> [2 n][3][2]: (2, 1, 0), (2, 0, 3)"""
    q = np.asarray(quads, f32).reshape(-1, 4, 2)
    return np.stack([q[:, [2, 1, 0]], q[:, [2, 0, 3]]], 1).reshape(-1, 3, 2)


def disc_triangles(discs):
    """[n][13][2] -> [12 n][3][2]: (0, 1 + i, 1 + (i + 1) % 12)"""
    d = np.asarray(discs, f32).reshape(-1, 13, 2)
    return np.stack([d[:, [0, 1 + i, 1 + (i + 1) % 12]] for i in range(12)], 1).reshape(-1, 3, 2)


def pixel_centres(W, H, vh):
    s = vh / f32(H)
    wx = (np.arange(W, dtype=f32) + f32(0.5) - f32(0.5) * f32(W)) * s
    wy = (f32(0.5) * f32(H) - (np.arange(H, dtype=f32) + f32(0.5))) * s
    return np.broadcast_arrays(wx[None, None, :], wy[None, :, None])


def _edges(tri):
    """tri [T][3][2] -> lo [T][3][2], d [T][3][2], sign [T][3] (the value of e at the third vertex)"""
    a, b, c = tri, np.roll(tri, -1, 1), np.roll(tri, -2, 1)
    a_lo = (a[..., 0] < b[..., 0]) | ((a[..., 0] == b[..., 0]) & (a[..., 1] <= b[..., 1]))
    lo, hi = np.where(a_lo[..., None], a, b), np.where(a_lo[..., None], b, a)
    d = hi - lo
    sign = d[..., 0] * (c[..., 1] - lo[..., 1]) - d[..., 1] * (c[..., 0] - lo[..., 0])
    return lo, d, sign


def coverage(tri, W, H, vh):
    """[T][H][W] bool: the rule, every triangle on every pixel"""
    tri = np.asarray(tri, f32).reshape(-1, 3, 2)
    out = np.zeros((len(tri), H, W), bool)
    wx, wy = pixel_centres(W, H, vh)
    with np.errstate(all="ignore"):
        for t0 in range(0, len(tri), CHUNK):
            lo, d, sign = _edges(tri[t0:t0 + CHUNK])
            ok = np.isfinite(tri[t0:t0 + CHUNK]).all((1, 2)) & np.isfinite(sign).all(1) & (sign != 0).all(1)
            inside = np.broadcast_to(ok[:, None, None], (len(ok), H, W)).copy()
            for k in range(3):
                e = d[:, k, 0, None, None] * (wy - lo[:, k, 1, None, None]) - d[:, k, 1, None, None] * (wx - lo[:, k, 0, None, None])
                pos = (sign[:, k] > 0)[:, None, None]
                inside &= np.where(pos, e >= 0, e < 0)
            out[t0:t0 + CHUNK] = inside
    return out


def place(pos, transform):
    p = np.asarray(pos, f32)[..., :2]
    if transform is None:
        return p
    t = np.asarray(transform, f32)
    return np.stack([p[..., 0] * t[2] + t[0], p[..., 1] * t[3] + t[1]], -1).astype(f32)


def draw(img, tri, rgba, vh, hits=None):
    """blend the triangles tri [T][3][2] of colours rgba [T][4] over img in index order, in place; hits: a list that receives the
    number of (pixel, triangle) pairs blended"""
    H, W = img.shape[:2]
    tri, rgba = np.asarray(tri, f32).reshape(-1, 3, 2), np.asarray(rgba, f32).reshape(-1, 4)
    cov = coverage(tri, W, H, vh)
    n = 0
    with np.errstate(all="ignore"):
        for t in np.nonzero(cov.any((1, 2)) & np.isfinite(rgba).all(1))[0]:
            hit, src = cov[t], rgba[t]
            dst = img[hit]
            k = f32(1.0) - src[3]
            out = np.empty_like(dst)
            for c in range(3):
                out[:, c] = src[c] * src[3] + dst[:, c] * k
            out[:, 3] = src[3] + dst[:, 3] * k
            img[hit] = out
            n += int(hit.sum())
    if hits is not None:
        hits.append(n)
    return img


def draw_mesh(image, pos, rgba, viewport_height=0.0, transform=None):
    vh = RM.VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    return draw(np.array(image, f32), place(np.asarray(pos, f32).reshape(-1, 3, 2), transform), rgba, vh)


def frame(octaves, bpo, W, H, viewport_height=0.0, mode=0, bass_lit=0, bass_rgba=None, panels=None, background=None, skip=()):
    """[H][W][4]: the layers in order; panels: the dict pitchvis_amd.backdrop_frame takes; skip: layers of LAYERS left out"""
    vh = RM.VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    img = np.array(background, f32) if background is not None else np.broadcast_to(RM.clear_color(mode), (H, W, 4)).copy()
    panels = panels or {}
    if mode != GALAXY and "net" not in skip:
        gray = np.asarray([RM.srgb_to_linear(0.3)] * 3 + [1.0], f32)
        for what in (NET_SPIRAL, NET_RAYS):
            tri = quad_triangles(geometry(octaves, what))
            draw(img, tri, np.broadcast_to(gray, (len(tri), 4)), vh)
    for name, key, discs in (("line", "spectrum_transform", False), ("disc", "spectrum_transform", True), ("graph", "graph_transform", False),
                             ("hist", "histogram_transform", False)):
        pos = panels.get(name + "_pos")
        if pos is None or name in skip:
            continue
        col = np.asarray(panels[name + "_rgba"], f32).reshape(-1, 4)
        p = place(np.asarray(pos, f32).reshape(-1, 3), panels.get(key))
        if discs:
            if len(p) == 0:
                continue
            tri, rgba = disc_triangles(p), np.repeat(col[0::13], 12, 0)
        else:
            tri, rgba = quad_triangles(p), np.repeat(col[0::4], 2, 0)
        draw(img, tri, rgba, vh)
    if mode != GALAXY and bass_lit and "bass" not in skip:
        lit = min(int(bass_lit), counts(octaves)[BASS])
        c = np.asarray([RM.srgb_to_linear(v) for v in np.asarray(bass_rgba, f32)[:3]] + [f32(bass_rgba[3])], f32)
        tri = quad_triangles(geometry(octaves, BASS)[:lit])
        draw(img, tri, np.broadcast_to(c, (len(tri), 4)), vh)
    return img
