"""The present stage's rule (include/pvq.h, "the present stage") restated literally in NumPy float32: one function per formula, every
operation a float32 operation in the order the rule writes it, vectorised over the texels of a level.  powf and expf are NumPy's."""
import math

import numpy as np

f32 = np.float32
DEFAULTS = dict(low_frequency_boost=1.0, low_frequency_boost_curvature=1.0, high_pass_frequency=0.52, threshold=0.17, threshold_softness=0.82,
                composite_mode=1, max_mip_dimension=512, tonemapping=1)
TAPS = [(-2, 2), (0, 2), (2, 2), (-2, 0), (0, 0), (2, 0), (-2, -2), (0, -2), (2, -2), (-1, 1), (1, 1), (-1, -1), (1, -1)]   # a .. m
A, B, C, D, E, F, G, H, I, J, K, L, M = range(13)


def settings_of(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    if not s["max_mip_dimension"]:
        s["max_mip_dimension"] = 512
    return s


def mips(W, H, d=512):
    d = d or 512
    n = max(int(math.floor(math.log2(d))), 2) - 1
    ratio = f32(d) / f32(H)
    w0 = max(1, int(math.floor(float(f32(W) * ratio) + 0.5)))
    h0 = max(1, int(math.floor(float(f32(H) * ratio) + 0.5)))
    return [(max(1, w0 >> k), max(1, h0 >> k)) for k in range(n)]


def blend_factors(s, intensity, n):
    out = []
    with np.errstate(all="ignore"):
        for k in range(n):
            r = f32(k) / f32(n - 1) if n > 1 else f32(0)
            lf = (f32(1) - np.power(f32(1) - r, f32(1) / (f32(1) - f32(s["low_frequency_boost_curvature"])))) * f32(s["low_frequency_boost"])
            hpf = f32(s["high_pass_frequency"])
            hp = f32(1) - np.fmin(np.fmax((r - hpf) / hpf, f32(0)), f32(1))
            if s["composite_mode"] == 0:
                lf = lf * (f32(1) - f32(intensity))
            out.append(f32((f32(intensity) + lf) * hp))
    return np.asarray(out, f32)


def clamp(x, lo, hi):
    return np.fmin(np.fmax(x, f32(lo)), f32(hi))


def lerp(a, b, t):
    return a + (b - a) * t


def luma(v):
    return f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1] + f32(0.0722) * v[..., 2]


def uv_grid(wt, ht):
    u = (np.arange(wt, dtype=f32) + f32(0.5)) / f32(wt)
    v = (np.arange(ht, dtype=f32) + f32(0.5)) / f32(ht)
    return np.broadcast_to(u[None, :], (ht, wt)), np.broadcast_to(v[:, None], (ht, wt))


def sample(tex, u, v):
    """tex [h][w][3] at uv, bilinear, clamp-to-edge"""
    h, w = tex.shape[:2]
    px, py = u * f32(w) - f32(0.5), v * f32(h) - f32(0.5)
    x0f, y0f = np.floor(px), np.floor(py)
    fx, fy = (px - x0f)[..., None], (py - y0f)[..., None]
    x0, x1 = np.clip(x0f.astype(np.int64), 0, w - 1), np.clip((x0f + f32(1)).astype(np.int64), 0, w - 1)
    y0, y1 = np.clip(y0f.astype(np.int64), 0, h - 1), np.clip((y0f + f32(1)).astype(np.int64), 0, h - 1)
    top = lerp(tex[y0, x0], tex[y0, x1], fx)
    bottom = lerp(tex[y1, x0], tex[y1, x1], fx)
    return lerp(top, bottom, fy)


def taps13(src, wt, ht):
    hs, ws = src.shape[:2]
    u, v = uv_grid(wt, ht)
    return [sample(src, u + f32(ox) / f32(ws), v + f32(oy) / f32(hs)) for ox, oy in TAPS]


def down_plain(src, wt, ht):
    t = taps13(src, wt, ht)
    return (t[A] + t[C] + t[G] + t[I]) * f32(0.03125) + (t[B] + t[D] + t[F] + t[H]) * f32(0.0625) + (t[E] + t[J] + t[K] + t[L] + t[M]) * f32(0.125)


def down_first(src, wt, ht, threshold, softness):
    t = taps13(src, wt, ht)
    groups = [(t[A] + t[B] + t[D] + t[E]) * f32(0.03125), (t[B] + t[C] + t[E] + t[F]) * f32(0.03125), (t[D] + t[E] + t[G] + t[H]) * f32(0.03125),
              (t[E] + t[F] + t[H] + t[I]) * f32(0.03125), (t[J] + t[K] + t[L] + t[M]) * f32(0.125)]
    total = None
    for g in groups:
        weight = f32(1) / (f32(1) + luma(np.power(np.fmax(g, f32(0)), f32(1) / f32(2.2))) / f32(4))
        g = g * weight[..., None]
        total = g if total is None else total + g
    c = np.fmin(np.fmax(total, f32(1e-4)), f32(3.40282347e37))
    if threshold == 0:
        return c
    threshold, softness = f32(threshold), f32(softness)
    knee = threshold * softness
    br = np.fmax(np.fmax(c[..., 0], c[..., 1]), c[..., 2])
    s = clamp(br - (threshold - knee), 0, f32(2) * knee)
    s = s * s * (f32(0.25) / (knee + f32(1e-5)))
    contribution = np.fmax(br - threshold, s) / np.fmax(br, f32(1e-5))
    return c * contribution[..., None]


def tent(src, u, v, x, y):
    a, b, c = sample(src, u - x, v + y), sample(src, u, v + y), sample(src, u + x, v + y)
    d, e, f = sample(src, u - x, v), sample(src, u, v), sample(src, u + x, v)
    g, h, i = sample(src, u - x, v - y), sample(src, u, v - y), sample(src, u + x, v - y)
    return e * f32(0.25) + (b + d + f + h) * f32(0.125) + (a + c + g + i) * f32(0.0625)


def composite(mode, b, t, dst):
    return dst + b * t if mode == 1 else dst * (f32(1) - b) + b * t


def display(c, tonemapping):
    c = np.fmax(c, f32(0))
    if tonemapping == 0:
        return c
    y = luma(c)
    cb = c[..., 0] * f32(-0.1146) + c[..., 1] * f32(-0.3854) + c[..., 2] * f32(0.5)
    cr = c[..., 0] * f32(0.5) + c[..., 1] * f32(-0.4542) + c[..., 2] * f32(-0.0458)
    curve = lambda v: f32(1) - np.exp(-v)
    bt = curve(np.sqrt(cb * cb + cr * cr) * f32(2.4))
    desat = np.fmax((bt - f32(0.7)) * f32(0.8), f32(0))
    desat = desat * desat
    desat_col = lerp(c, y[..., None], desat[..., None])
    tm0 = c * np.fmax(f32(0), curve(y) / np.fmax(f32(1e-5), y))[..., None]
    tm1 = curve(desat_col)
    return lerp(tm0, tm1, (bt * bt)[..., None]) * f32(0.97)


def encode(rgb, alpha):
    v = clamp(rgb, 0, 1)
    e = np.where(v <= f32(0.0031308), f32(12.92) * v, f32(1.055) * np.power(v, f32(1) / f32(2.4)) - f32(0.055))
    out = np.empty(rgb.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.floor(clamp(e, 0, 1) * f32(255) + f32(0.5)).astype(np.uint8)
    out[..., 3] = np.floor(clamp(alpha, 0, 1) * f32(255) + f32(0.5)).astype(np.uint8)
    return out


def present(image, intensity, **kw):
    """image [H][W][4] -> (bytes uint8 [H][W][4], hdr float32 [H][W][4])"""
    s = settings_of(**kw)
    image = np.asarray(image, f32)
    Hh, W = image.shape[:2]
    rgb = image[..., :3].copy()
    with np.errstate(all="ignore"):
        if np.isfinite(f32(intensity)) and intensity > 0:
            sizes = mips(W, Hh, s["max_mip_dimension"])
            n = len(sizes)
            bf = blend_factors(s, intensity, n)
            chain = [down_first(rgb, sizes[0][0], sizes[0][1], s["threshold"], s["threshold_softness"])]
            for k in range(1, n):
                chain.append(down_plain(chain[k - 1], *sizes[k]))
            x, y = f32(0.004) / (f32(W) / f32(Hh)), f32(0.004)
            for k in range(n - 1, 0, -1):
                u, v = uv_grid(*sizes[k - 1])
                chain[k - 1] = composite(s["composite_mode"], bf[k], tent(chain[k], u, v, x, y), chain[k - 1])
            u, v = uv_grid(W, Hh)
            rgb = composite(s["composite_mode"], bf[0], tent(chain[0], u, v, x, y), rgb)
        hdr = np.concatenate([rgb, image[..., 3:]], -1).astype(f32)
        return encode(display(rgb, s["tonemapping"]), image[..., 3]), hdr
