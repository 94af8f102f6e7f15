"""NumPy model of the multisampled backdrop (include/pvq.h, "the backdrop multisampled"), written from the statement of the rule and
from nothing else: float32, operation for operation.  Coverage is tests/backdrop_model.py's edge routine evaluated at the sample
positions; there are no pixel boxes and no culling — every triangle is tried on every sample of every pixel.  The picture is kept
as [samples][H][W][4] until the end and then resolved."""
import numpy as np

import backdrop_model as M
import raster_model as RM

f32 = np.float32
POSITIONS = {1: ((0.5, 0.5),), 4: ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))}


def sample_world(W, H, vh, fx, fy):
    """world positions of the point (fx, fy) of every pixel, broadcast to [1][H][W]"""
    s = f32(vh) / f32(H)
    wx = ((np.arange(W, dtype=f32) + f32(fx)) - f32(0.5) * f32(W)) * s
    wy = (f32(0.5) * f32(H) - (np.arange(H, dtype=f32) + f32(fy))) * s
    return np.broadcast_arrays(wx[None, None, :], wy[None, :, None])


def coverage_at(tri, wx, wy):
    """[T][H][W] bool: the one-sample rule at the positions (wx, wy)"""
    tri = np.asarray(tri, f32).reshape(-1, 3, 2)
    out = np.zeros((len(tri),) + wx.shape[1:], bool)
    with np.errstate(all="ignore"):
        for t0 in range(0, len(tri), M.CHUNK):
            lo, d, sign = M._edges(tri[t0:t0 + M.CHUNK])
            ok = np.isfinite(tri[t0:t0 + M.CHUNK]).all((1, 2)) & np.isfinite(sign).all(1) & (sign != 0).all(1)
            inside = np.broadcast_to(ok[:, None, None], (len(ok),) + wx.shape[1:]).copy()
            for k in range(3):
                e = d[:, k, 0, None, None] * (wy - lo[:, k, 1, None, None]) - d[:, k, 1, None, None] * (wx - lo[:, k, 0, None, None])
                inside &= np.where((sign[:, k] > 0)[:, None, None], e >= 0, e < 0)
            out[t0:t0 + M.CHUNK] = inside
    return out


def resolve(planes):
    """[4][...] -> [...]: ((s0 + s1) + (s2 + s3)) * 0.25 in f32; one plane: itself"""
    if len(planes) == 1:
        return planes[0].copy()
    with np.errstate(all="ignore"):
        return ((planes[0] + planes[1]) + (planes[2] + planes[3])) * f32(0.25)


def draw(planes, tri, rgba, vh, alike=None):
    """blend the triangles over every sample plane of planes [S][H][W][4] in index order, in place.  alike [H][W] bool, if given, is
    cleared wherever a drawn triangle covers the samples and the pixel centre differently."""
    S, H, W = planes.shape[:3]
    tri, rgba = np.asarray(tri, f32).reshape(-1, 3, 2), np.asarray(rgba, f32).reshape(-1, 4)
    drawn = np.isfinite(rgba).all(1)
    centre = coverage_at(tri, *sample_world(W, H, vh, 0.5, 0.5)) if alike is not None else None
    for k, (fx, fy) in enumerate(POSITIONS[S]):
        cov = coverage_at(tri, *sample_world(W, H, vh, fx, fy))
        if alike is not None:
            alike &= ~((cov != centre) & drawn[:, None, None]).any(0)
        with np.errstate(all="ignore"):
            for t in np.nonzero(cov.any((1, 2)) & drawn)[0]:
                hit, src = cov[t], rgba[t]
                dst = planes[k][hit]
                kk = f32(1.0) - src[3]
                out = np.empty_like(dst)
                for c in range(3):
                    out[:, c] = src[c] * src[3] + dst[:, c] * kk
                out[:, 3] = src[3] + dst[:, 3] * kk
                planes[k][hit] = out
    return planes


def draw_mesh(image, pos, rgba, viewport_height=0.0, transform=None, samples=4):
    """the one-mesh face: every sample starts from its pixel of `image`; resolved"""
    vh = RM.VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    img = np.array(image, f32)
    planes = np.repeat(img[None], samples, 0)
    return resolve(draw(planes, M.place(np.asarray(pos, f32).reshape(-1, 3, 2), transform), rgba, vh))


def frame(octaves, bpo, W, H, viewport_height=0.0, mode=0, bass_lit=0, bass_rgba=None, panels=None, background=None, samples=4, alike=None):
    """[H][W][4]: layers 0 - 6 in order per sample, resolved.  alike: see draw"""
    vh = RM.VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    img = np.array(background, f32) if background is not None else np.broadcast_to(RM.clear_color(mode), (H, W, 4)).copy()
    planes = np.repeat(img[None], samples, 0)
    panels = panels or {}
    if mode != M.GALAXY:
        gray = np.asarray([RM.srgb_to_linear(0.3)] * 3 + [1.0], f32)
        for what in (M.NET_SPIRAL, M.NET_RAYS):
            tri = M.quad_triangles(M.geometry(octaves, what))
            draw(planes, tri, np.broadcast_to(gray, (len(tri), 4)), vh, alike)
    for name, key, discs in (("line", "spectrum_transform", False), ("disc", "spectrum_transform", True), ("graph", "graph_transform", False),
                             ("hist", "histogram_transform", False)):
        pos = panels.get(name + "_pos")
        if pos is None:
            continue
        col = np.asarray(panels[name + "_rgba"], f32).reshape(-1, 4)
        p = M.place(np.asarray(pos, f32).reshape(-1, 3), panels.get(key))
        if discs:
            if len(p) == 0:
                continue
            tri, rgba = M.disc_triangles(p), np.repeat(col[0::13], 12, 0)
        else:
            tri, rgba = M.quad_triangles(p), np.repeat(col[0::4], 2, 0)
        draw(planes, tri, rgba, vh, alike)
    if mode != M.GALAXY and bass_lit:
        lit = min(int(bass_lit), M.counts(octaves)[M.BASS])
        c = np.asarray([RM.srgb_to_linear(v) for v in np.asarray(bass_rgba, f32)[:3]] + [f32(bass_rgba[3])], f32)
        tri = M.quad_triangles(M.geometry(octaves, M.BASS)[:lit])
        draw(planes, tri, np.broadcast_to(c, (len(tri), 4)), vh, alike)
    return resolve(planes)
