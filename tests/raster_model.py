"""An independent NumPy float32 model of the pitch balls' picture, written from the behaviour of the viewer's ball material
(pitchvis_viewer/assets/shaders/noisy_color_rings_2d.wgsl:395-428), its camera and ball rectangle (setup.rs:359-365, :110-112) and
Bevy's alpha blend; it does not call the library.  Every value is rounded to f32 after every operation, components left to right;
sin, cos and atan2 are the double-precision functions of the C library rounded once to f32; sqrt and / are IEEE f32.  The model
has no pixel boxes and no tiles: every ball is tried on every pixel."""
import math

import numpy as np

f32 = np.float32
PI = f32(3.14159265359)
VIEWPORT_HEIGHT = f32(38.0) * f32(0.41421357)
GALAXY = 3


def _libm(fn, *xs):
    xs = [np.asarray(x, f32).astype(np.float64) for x in xs]
    shape = np.broadcast(*xs).shape
    flat = [np.broadcast_to(x, shape).ravel().tolist() for x in xs]
    return np.asarray(list(map(fn, *flat)), np.float64).astype(f32).reshape(shape)


def sin(x):
    return _libm(math.sin, x)


def cos(x):
    return _libm(math.cos, x)


def atan2(y, x):
    return _libm(math.atan2, y, x)


def arr(x):
    return np.asarray(x, f32)


# ---- the WGSL built-ins ----
def mod(x, y):
    return x - y * np.trunc(x / y)


def step(edge, x):
    return np.where(x >= edge, f32(1.0), f32(0.0)).astype(f32)


def clamp(x, lo, hi):
    return np.minimum(np.maximum(x, f32(lo)), f32(hi))


def mix(a, b, t):
    return a * (f32(1.0) - t) + b * t


def smoothstep(lo, hi, x):
    t = clamp((x - f32(lo)) / (f32(hi) - f32(lo)), 0.0, 1.0)
    return t * t * (f32(3.0) - f32(2.0) * t)


# ---- McEwan / Gustavson 3-D simplex noise, four corners as 4-vectors on a trailing axis ----
def permute(x):
    return mod((x * f32(34.0) + f32(1.0)) * x, f32(289.0))


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def simplex3(vx, vy, vz):
    vx, vy, vz = np.broadcast_arrays(arr(vx), arr(vy), arr(vz))
    v = [vx, vy, vz]
    c6, c3 = f32(1.0) / f32(6.0), f32(1.0) / f32(3.0)
    s = vx * c3 + vy * c3 + vz * c3
    i = [np.floor(c + s) for c in v]
    t = i[0] * c6 + i[1] * c6 + i[2] * c6
    x0 = [v[k] - i[k] + t for k in range(3)]
    g = [step(x0[1], x0[0]), step(x0[2], x0[1]), step(x0[0], x0[2])]          # step(x0.yzx, x0.xyz)
    l = [f32(1.0) - c for c in g]
    lz = [l[2], l[0], l[1]]                                                   # l.zxy
    i1 = [np.minimum(g[k], lz[k]) for k in range(3)]
    i2 = [np.maximum(g[k], lz[k]) for k in range(3)]
    x1 = [x0[k] - i1[k] + f32(1.0) * c6 for k in range(3)]
    x2 = [x0[k] - i2[k] + f32(2.0) * c6 for k in range(3)]
    x3 = [x0[k] - f32(1.0) + f32(3.0) * c6 for k in range(3)]
    i = [mod(c, f32(289.0)) for c in i]
    zero, one = np.zeros_like(vx), np.ones_like(vx)
    lanes = lambda k: np.stack([zero, i1[k], i2[k], one], -1)
    p = permute(permute(permute(i[2][..., None] + lanes(2)) + i[1][..., None] + lanes(1)) + i[0][..., None] + lanes(0))
    n_ = f32(1.0) / f32(7.0)
    ns = [n_ * f32(2.0) - f32(0.0), n_ * f32(0.5) - f32(1.0), n_ * f32(1.0) - f32(0.0)]
    j = p - f32(49.0) * np.floor(p * ns[2] * ns[2])
    x_ = np.floor(j * ns[2])
    y_ = np.floor(j - f32(7.0) * x_)
    x = x_ * ns[0] + ns[1]
    y = y_ * ns[0] + ns[1]
    h = f32(1.0) - np.abs(x) - np.abs(y)
    sh = -step(h, f32(0.0))
    ax = x + (np.floor(x) * f32(2.0) + f32(1.0)) * sh
    ay = y + (np.floor(y) * f32(2.0) + f32(1.0)) * sh
    norm = f32(1.79284291400159) - f32(0.85373472095314) * (ax * ax + ay * ay + h * h)
    grad = [ax * norm, ay * norm, h * norm]
    offs = [np.stack([x0[k], x1[k], x2[k], x3[k]], -1) for k in range(3)]
    m = np.maximum(f32(0.6) - dot3(offs, offs), f32(0.0))
    m = m * m
    mm, gd = m * m, dot3(grad, offs)
    return f32(42.0) * (mm[..., 0] * gd[..., 0] + mm[..., 1] * gd[..., 1] + mm[..., 2] * gd[..., 2] + mm[..., 3] * gd[..., 3])


# ---- the fragment ----
def shade(rgba, params, u, v):
    """rgba linear, params (calmness, time, pitch_accuracy, pitch_deviation), u / v arrays -> [..., 4]"""
    rgba, (calm, time, acc, dev) = arr(rgba), arr(params)
    u, v = np.broadcast_arrays(arr(u), arr(v))
    px, py = u * f32(2.0) - f32(1.0), v * f32(2.0) - f32(1.0)
    r = np.sqrt(px * px + py * py)
    noise = clamp(simplex3(u * f32(4.3), v * f32(4.3), time * f32(0.8)) - f32(0.15), 0.0, 1.0)
    f = sin(r * np.sqrt(r) * PI * f32(1.0))
    ring = f * f
    ring_rgb = [mix(rgba[c], f32(1.0), noise * calm * ring) for c in range(3)]
    ring_a = rgba[3] * ring
    dot = np.zeros_like(r)
    if acc >= f32(0.85):
        factor = (acc - f32(0.85)) / (f32(1.0) - f32(0.85))
        pulse = f32(0.85) + f32(0.15) * sin(time * f32(3.0))
        dot = f32(1.0) * smoothstep(0.08, 0.0, r) * factor * pulse
    star = np.zeros_like(r)
    on = ~((r > f32(0.25)) | (r < f32(0.01)))
    if on.any():
        ro = r[on]
        spiral_angle = atan2(py[on], px[on]) * f32(6.0) + ro * (dev * f32(4.0)) * PI * f32(4.0)
        intensity = np.maximum(f32(0.0), cos(spiral_angle)) * (f32(1.0) - smoothstep(0.15, 0.25, ro))
        brightness = mix(f32(0.3), f32(1.0), f32(1.0) - np.abs(dev) * f32(2.0)) * (f32(0.7) + f32(0.3) * sin(time * f32(3.0)))
        star[on] = f32(1.0) * intensity * brightness
    add = (dot + star) * f32(0.4)
    k = clamp(f32(1.0) - calm * f32(1.65), 0.0, 1.0)
    strength = k * k * k
    edge = smoothstep(0.96, 1.0, r)
    out = np.empty(r.shape + (4,), f32)
    for c in range(3):
        col = mix(rgba[c], ring_rgb[c] + add, strength)
        out[..., c] = mix(col, col, edge)
    out[..., 3] = mix(mix(rgba[3], ring_a, strength), f32(0.0), edge)
    return out


def touch(time, centers, elapsed, n_bins):
    """the balls' times after a frame with this peak list (update.rs:239); trunc(center) as the scene model takes it"""
    t = np.array(time, f32)
    for c in centers:
        c = float(f32(c))
        key = 0 if not c > 0.0 else (2 ** 63 if c >= 2.0 ** 63 else math.trunc(c))
        if key < n_bins:
            t[key] = f32(elapsed)
    return t


def srgb_to_linear(x):
    x = f32(x)
    if x <= f32(0.04045):
        return x / f32(12.92)
    return f32(math.pow(float((x + f32(0.055)) / f32(1.055)), float(f32(2.4))))


def clear_color(mode=0):
    c = (0.05, 0.0, 0.05) if mode == GALAXY else (0.23, 0.23, 0.25)
    return np.asarray([srgb_to_linear(v) for v in c] + [f32(1.0)], f32)


def drawing_order(xyzs, rgba, params, visible, time):
    """the bins that are drawn, back to front"""
    xyzs, rgba, params, time = arr(xyzs), arr(rgba), arr(params), arr(time)
    n = time.size
    bits = np.unpackbits(np.asarray(visible, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)
    ok = bits & (xyzs[:, 3] > 0) & np.isfinite(xyzs).all(1) & np.isfinite(rgba).all(1) & np.isfinite(params).all(1) & np.isfinite(time)
    return sorted(np.nonzero(ok)[0].tolist(), key=lambda b: (float(xyzs[b, 2]), b))


def frame(W, H, xyzs, rgba, params, visible, time, viewport_height=0.0, mode=0, background=None, coverage=None):
    """[H][W][4]; coverage: a list that receives the number of (pixel, ball) pairs shaded"""
    xyzs, rgba, params, time = arr(xyzs), arr(rgba), arr(params), arr(time)
    vh = VIEWPORT_HEIGHT if viewport_height == 0 else f32(viewport_height)
    s = vh / f32(H)
    wx = (np.arange(W, dtype=f32) + f32(0.5) - f32(0.5) * f32(W)) * s
    wy = (f32(0.5) * f32(H) - (np.arange(H, dtype=f32) + f32(0.5))) * s
    wx, wy = np.broadcast_arrays(wx[None, :], wy[:, None])
    img = np.array(background, f32) if background is not None else np.broadcast_to(clear_color(mode), (H, W, 4)).copy()
    pairs = 0
    with np.errstate(all="ignore"):
        for b in drawing_order(xyzs, rgba, params, visible, time):
            side = f32(20.0) * xyzs[b, 3]
            u = (wx - xyzs[b, 0]) / side + f32(0.5)
            v = f32(0.5) - (wy - xyzs[b, 1]) / side
            px, py = u * f32(2.0) - f32(1.0), v * f32(2.0) - f32(1.0)
            hit = np.sqrt(px * px + py * py) < f32(1.0)
            if not hit.any():
                continue
            pairs += int(hit.sum())
            src = shade(rgba[b], [params[b, 0], time[b], params[b, 1], params[b, 2]], u[hit], v[hit])
            dst = img[hit]
            k = f32(1.0) - src[:, 3]
            out = np.empty_like(dst)
            for c in range(3):
                out[:, c] = src[:, c] * src[:, 3] + dst[:, c] * k
            out[:, 3] = src[:, 3] + dst[:, 3] * k
            img[hit] = out
    if coverage is not None:
        coverage.append(pairs)
    return img
