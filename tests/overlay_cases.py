"""Inputs for the overlay tests, and the two references built from them: random RGBA rows with some alpha-0 texels and some rows
all zero, chroma with zeros, ones and a NaN, backgrounds with NaN payloads; `model_chain` (tests/overlay_model.py) and `host_chain`
(pvq_overlay_state_*, pvq_overlay_frame) push a stream's rows one by one and draw every frame."""
import numpy as np

import overlay_model as M
import pitchvis_amd as P

f32 = np.float32


def rows(n_streams, n_frames, n_bins, seed):
    """uint8 [n_streams][n_frames][n_bins][4]: a fifth of the texels with alpha 0, every seventh row all zero (never the last)"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 256, (n_streams, n_frames, n_bins, 4), dtype=np.uint8)
    r[..., 3] = np.maximum(r[..., 3], 1)
    r[..., 3][rng.random((n_streams, n_frames, n_bins)) < 0.2] = 0
    for s in range(n_streams):
        r[s, (3 + s) % 7:max(n_frames - 1, 0):7] = 0
    return r


def chroma(n_streams, n_frames, seed):
    """float32 [n_streams][n_frames][12] in (0, 1] with zeros, ones and a NaN in every row"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.05, 1.0, (n_streams, n_frames, 12)).astype(f32)
    for s in range(n_streams):
        for f in range(n_frames):
            z, o, nan = rng.choice(12, 3, replace=False)
            c[s, f, z], c[s, f, o], c[s, f, nan] = 0.0, 1.0, np.nan
    return c


def images(n_streams, n_frames, W, H, seed, nans=False):
    """float32 [n_streams][n_frames][H][W][4] in (0, 2); nans: a NaN with a payload of its own in one channel of every 13th pixel"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, (n_streams, n_frames, H, W, 4)).astype(f32)
    if nans:
        flat = img.reshape(-1).view(np.uint32)
        flat[5::13 * 4] = 0x7FC00100 | (np.arange(flat[5::13 * 4].size, dtype=np.uint32) & 0xFFFF)
    return img


def full_quad(W, H, vh=3.0):
    """the quad laid over the whole image, so that small images sample many texels"""
    return np.asarray([0.0, 0.0, vh * W / H, vh], f32)


def model_chain(n_bins, h, rows_s, chroma_s, images_s, info=None, before=(), **kw):
    """one stream through the model: `before` rows are pushed first (earlier calls), then every row of rows_s is pushed and drawn
    over its image.  rows_s None: no quad.  info: a list that receives one dict a frame."""
    tex = M.Texture(n_bins, h)
    for r in before:
        tex.push(r)
    out = []
    for f, img in enumerate(images_s):
        if rows_s is not None:
            tex.push(rows_s[f])
        d = {} if info is not None else None
        out.append(M.frame(img, tex if rows_s is not None else None, None if chroma_s is None else chroma_s[f], info=d, **kw))
        if info is not None:
            info.append(d)
    return np.asarray(out, f32), tex


def host_chain(n_bins, h, rows_s, chroma_s, images_s, before=(), quad_=None, **kw):
    """the same through the host face"""
    st = P.OverlayState(n_bins, h)
    for r in before:
        st.push(r)
    out = []
    for f, img in enumerate(images_s):
        if rows_s is not None:
            st.push(rows_s[f])
        out.append(P.overlay_frame(img, st if rows_s is not None else None, None if chroma_s is None else chroma_s[f], quad=quad_, **kw))
    return np.asarray(out, f32), st


# ---- the row-stride test: 61 distinct streams of a few frames --------------------------------------------------------------------
STRIDE_STREAMS = 61
STRIDE_EMPTY = (3, 6)       # stream pattern p draws nothing where p % 11 is one of these: rows all zero, no box lit


def stride_streams(n_frames, n_bins, W, H, seed):
    """(rows, chroma, images) of 61 distinct streams; the crafted empty ones hold zero rows and zero strengths"""
    m = STRIDE_STREAMS
    r, c, img = rows(m, n_frames, n_bins, seed), chroma(m, n_frames, seed + 1), images(m, n_frames, W, H, seed + 2)
    r[:, :, :, 3] = np.maximum(r[:, :, :, 3], 1)               # few bins, few pixels: every texel of an ordinary row draws
    for p in range(m):
        if p % 11 in STRIDE_EMPTY:
            r[p], c[p] = 0, 0.0
    return r, c, img
