"""NumPy model of the overlay stage (include/pvq.h, "the overlay"): float32, operation for operation.  It keeps the spectrogram
texture literally as pitchvis_viewer/src/display_system/update.rs:1066-1087 does — the vertical flip, the clear of the next line,
the write index — and samples it per pixel through the scroll material's fract, so the (age, bin) derivation of the device stage is
checked against the texture itself.  Beside the texture it remembers which frame wrote each texture row: that is what the tests'
conditions (ages and bins sampled) are computed from, not what the picture is drawn from."""
import numpy as np

import raster_model as RM

f32 = np.float32
HISTORY_ROWS = 200
# pitchvis_colors/src/lib.rs:19-36
COLORS = np.asarray([[0.85, 0.36, 0.36], [0.01, 0.52, 0.71], [0.97, 0.76, 0.05], [0.45, 0.34, 0.63], [0.47, 0.77, 0.22], [0.78, 0.32, 0.52],
                     [0.00, 0.64, 0.56], [0.95, 0.54, 0.23], [0.30, 0.37, 0.64], [1.00, 0.96, 0.03], [0.57, 0.30, 0.55], [0.12, 0.71, 0.34]], f32)
ALPHA = (np.arange(256).astype(f32) / f32(255.0)).astype(f32)
LINEAR = np.asarray([RM.srgb_to_linear(a) for a in ALPHA], f32)


def quad(n_bins, history_rows=HISTORY_ROWS):
    """Rectangle(12 * (h / n), 12) at (-7, 6), turned a quarter: (cx, cy, ex, ey)"""
    return np.asarray([-7.0, 6.0, 12.0, f32(12.0) * f32(f32(history_rows) / f32(n_bins))], f32)


class Texture:
    def __init__(self, n_bins, history_rows=HISTORY_ROWS):
        self.n, self.h, self.write_index, self.frames = n_bins, history_rows, 0, 0
        self.tex = np.zeros((history_rows, n_bins, 4), np.uint8)
        self.wrote = np.full(history_rows, -1)          # the frame whose row a texture row holds, -1: zeros

    def push(self, row):
        h, w = self.h, self.write_index
        self.tex[h - 1 - w] = row
        self.wrote[h - 1 - w] = self.frames
        nxt = (w + 1) % h
        self.tex[h - 1 - nxt] = 0
        self.wrote[h - 1 - nxt] = -1
        self.write_index = nxt
        self.frames += 1

    @property
    def scroll(self):
        return f32(f32(self.write_index) / f32(self.h))


def pixel_world(W, H, vh):
    s = f32(f32(vh) / f32(H))
    wx = ((np.arange(W).astype(f32) + f32(0.5)) - f32(0.5) * f32(W)) * s
    wy = (f32(0.5) * f32(H) - (np.arange(H).astype(f32) + f32(0.5))) * s
    return wx.astype(f32), wy.astype(f32)


def blend(src_rgb, src_a, dst):
    """AlphaMode2d::Blend of [..][3], [..] over [..][4]"""
    k = (f32(1.0) - src_a).astype(f32)
    out = np.empty_like(dst)
    for c in range(3):
        out[..., c] = (src_rgb[..., c] * src_a).astype(f32) + (dst[..., c] * k).astype(f32)
    out[..., 3] = src_a + (dst[..., 3] * k).astype(f32)
    return out


def sample(tex, q, W, H, vh):
    """(covered [H][W], ty [W], tx [H]) of the scroll material over the quad q"""
    wx, wy = pixel_world(W, H, vh)
    with np.errstate(all="ignore"):
        u = ((wy - q[1]) / q[3]).astype(f32) + f32(0.5)
        v = f32(0.5) - ((wx - q[0]) / q[2]).astype(f32)
        covered = ((u >= 0) & (u < 1))[:, None] & ((v >= 0) & (v < 1))[None, :]
        t = v + (f32(1.0) - tex.scroll)
        v2 = (t - np.floor(t)).astype(f32)
        ty = np.minimum(np.nan_to_num(np.floor(v2 * f32(tex.h))), tex.h - 1).astype(np.int64)
        tx = np.minimum(np.nan_to_num(np.floor(u * f32(tex.n))), tex.n - 1).astype(np.int64)
    return covered, np.clip(ty, 0, tex.h - 1), np.clip(tx, 0, tex.n - 1)


def box_masks(W, H, ui_scale):
    """[12][H][W]: the pixels whose centre lies in box pc's rounded rectangle"""
    s = f32(ui_scale)
    px, py = np.arange(W).astype(f32) + f32(0.5), np.arange(H).astype(f32) + f32(0.5)
    y0, y1 = f32(H) - f32(50.0) * s, f32(H) - f32(10.0) * s
    r = f32(4.0) * s
    in_y = (py >= y0) & (py < y1)
    ly, hy = y0 + r, y1 - r
    dy = np.where(py < ly, py - ly, np.where(py > hy, py - hy, f32(0.0))).astype(f32)
    out = np.zeros((12, H, W), bool)
    for pc in range(12):
        x0 = f32(f32(400.0) + f32(45.0) * f32(pc)) * s
        x1 = x0 + f32(40.0) * s
        in_x = (px >= x0) & (px < x1)
        lx, hx = x0 + r, x1 - r
        dx = np.where(px < lx, px - lx, np.where(px > hx, px - hx, f32(0.0))).astype(f32)
        corner = (dy != 0)[:, None] & (dx != 0)[None, :]
        d2 = ((dx * dx).astype(f32)[None, :] + (dy * dy).astype(f32)[:, None]).astype(f32)
        out[pc] = in_y[:, None] & in_x[None, :] & ~(corner & ~(d2 <= r * r))
    return out


def frame(image, tex=None, chroma=None, *, viewport_height=0.0, ui_scale=1.0, quad_=None, colors=COLORS, info=None):
    """both layers over image [H][W][4] (a new array); tex: a Texture whose last push is the frame drawn.  info (a dict) receives
    `drawn` (pixels a texel with alpha was blended on), `ages` and `bins` (the sets sampled there) and `boxed` (pixels a box drew)"""
    img = np.array(image, f32)
    H, W = img.shape[:2]
    vh = RM.VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    if info is not None:
        info.update(drawn=0, ages=set(), bins=set(), boxed=0)
    if tex is not None:
        q = quad(tex.n, tex.h) if quad_ is None else np.asarray(quad_, f32)
        covered, ty, tx = sample(tex, q, W, H, vh)
        texel = tex.tex[ty[None, :], tx[:, None]]                       # [H][W][4]
        hit = covered & (texel[..., 3] != 0)
        with np.errstate(all="ignore"):
            over = blend(LINEAR[texel[..., :3]], ALPHA[texel[..., 3]], img)
        img[hit] = over[hit]
        if info is not None:
            info["drawn"] = int(hit.sum())
            rows = np.broadcast_to(ty[None, :], hit.shape)[hit]
            info["ages"] = set((tex.frames - 1 - tex.wrote[rows]).tolist())
            info["bins"] = set(np.broadcast_to(tx[:, None], hit.shape)[hit].tolist())
    if chroma is not None:
        c = np.asarray(chroma, f32)
        lin = np.asarray([[RM.srgb_to_linear(x) for x in rgb] for rgb in np.asarray(colors, f32)], f32)
        for pc, mask in enumerate(box_masks(W, H, 1.0 if ui_scale == 0 else ui_scale)):
            if not (np.isfinite(c[pc]) and c[pc] > 0) or not mask.any():
                continue
            with np.errstate(all="ignore"):
                over = blend(np.broadcast_to(lin[pc], img.shape[:2] + (3,)), np.broadcast_to(c[pc], img.shape[:2]), img)
            img[mask] = over[mask]
            if info is not None:
                info["boxed"] += int(mask.sum())
    return img
