"""An independent NumPy float32 model of the pitch-ball scene, written from pitchvis_viewer/src/display_system/update.rs:38-426
(with setup.rs:89-172 and util.rs:9-20) alone; it does not call the library.  Every value is rounded to f32 after every operation;
a libm call (powf, sin_cos, cosf / sinf) is the double-precision function rounded once to f32."""
import math

import numpy as np

from oracle.consumers import rgb_to_lch

f32 = np.float32
F = f32(1.0) / f32(305.0)            # update.rs:23
CUTOFF = f32(0.019)                  # update.rs:147
FULL, ZEN, PERFORMANCE, GALAXY = 0, 1, 2, 3
COLORS = [[0.85, 0.36, 0.36], [0.01, 0.52, 0.71], [0.97, 0.76, 0.05], [0.45, 0.34, 0.63], [0.47, 0.77, 0.22], [0.78, 0.32, 0.52],
          [0.00, 0.64, 0.56], [0.95, 0.54, 0.23], [0.30, 0.37, 0.64], [1.00, 0.96, 0.03], [0.57, 0.30, 0.55], [0.12, 0.71, 0.34]]
KAPPA, EPSILON, CBRT_EPSILON = f32(24389.0) / f32(27.0), f32(216.0) / f32(24389.0), f32(6.0) / f32(29.0)
S_0, WHITE_X, WHITE_Z = f32(0.003130668442500564), f32(0.9504492182750991), f32(1.0889166484304715)


def powf(x, y):
    x, y = float(x), float(y)
    if x != x or y != y:
        return f32(np.nan)
    try:
        return f32(math.pow(x, y))
    except (ValueError, OverflowError):
        return f32(np.nan) if x < 0 else f32(np.inf)


def rround(v):
    """f32::round: half away from zero"""
    v = f32(v)
    if not np.isfinite(v):
        return v
    return f32(math.floor(float(v) + 0.5)) if v >= 0 else f32(-math.floor(-float(v) + 0.5))


def as_usize(v):
    """Rust `as usize`: saturating, NaN -> 0"""
    v = float(v)
    if not v > 0.0:
        return 0
    return int(v) if v < 2.0 ** 63 else 2 ** 64 - 1


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def as_u8(v):
    v = float(v)
    return 0 if not v > 0.0 else (255 if v >= 255.0 else int(v))


def _compress(c):
    v = f32(f32(f32(1.055) * powf(c, f32(1.0) / f32(2.4))) - f32(0.055)) if c > S_0 else f32(f32(12.92) * c)
    return f32(max(min(v, f32(1.0)), f32(0.0)))


def lch_to_rgb(l, c, h):
    a, bb = f32(c * f32(math.cos(float(h)))), f32(c * f32(math.sin(float(h))))
    fy = f32(f32(l + f32(16.0)) / f32(116.0))
    fx = f32(f32(a / f32(500.0)) + fy)
    fz = f32(fy - f32(bb / f32(200.0)))
    xr = f32(f32(fx * fx) * fx) if fx > CBRT_EPSILON else f32(f32(f32(fx * f32(116.0)) - f32(16.0)) / KAPPA)
    yr = f32(f32(fy * fy) * fy) if l > f32(EPSILON * KAPPA) else f32(l / KAPPA)
    zr = f32(f32(fz * fz) * fz) if fz > CBRT_EPSILON else f32(f32(f32(fz * f32(116.0)) - f32(16.0)) / KAPPA)
    x, y, z = f32(xr * WHITE_X), yr, f32(zr * WHITE_Z)
    r = f32(f32(f32(x * f32(3.240812398895283)) - f32(y * f32(1.5373084456298136))) - f32(z * f32(0.4985865229069666)))
    g = f32(f32(f32(x * f32(-0.9692430170086407)) + f32(y * f32(1.8759663029085742))) + f32(z * f32(0.04155503085668564)))
    b = f32(f32(f32(x * f32(0.055638398436112804)) - f32(y * f32(0.20400746093241362))) + f32(z * f32(1.0571295702861434)))
    return [int(rround(f32(_compress(v) * f32(255.0)))) for v in (r, g, b)]


def calculate_color(bpo, bucket, colors, gray_level, easing_pow):
    """pitchvis_colors/src/lib.rs:86-117"""
    pc = f32(f32(f32(12.0) * f32(bucket)) / f32(bpo))
    rounded = rround(pc)
    base = [as_u8(f32(f32(c) * f32(255.0))) for c in colors[as_usize(rounded) % 12]]
    inacc = f32(abs(f32(pc - rounded)))
    l, c, h = rgb_to_lch(base)
    sat = f32(f32(1.0) - powf(f32(f32(2.0) * inacc), f32(easing_pow)))
    c = f32(c * sat)
    l = f32(f32(sat * l) + f32(f32(f32(1.0) - sat) * f32(gray_level)))
    return [f32(f32(v) / f32(255.0)) for v in lch_to_rgb(l, c, h)]


def to_linear(x):
    """bevy_color: LinearRgba::from(Srgba), one channel"""
    x = f32(x)
    return f32(x / f32(12.92)) if x <= f32(0.04045) else powf(f32(f32(x + f32(0.055)) / f32(1.055)), f32(2.4))


def bin_to_spiral(bpo, x):
    """util.rs:9-20"""
    x, b = f32(x), f32(bpo)
    radius = f32(f32(2.0) * f32(f32(0.3) + powf(f32(x / b), f32(0.75))))
    angle = f32(f32(f32(f32(x + b) / b) * f32(2.0)) * f32(math.pi))
    if not np.isfinite(angle):
        return f32(np.nan), f32(np.nan)
    return f32(f32(f32(-1.0) * f32(math.cos(float(angle)))) * radius), f32(f32(math.sin(float(angle))) * radius)


def secs_f32(ns):
    """core::time::Duration::as_secs_f32"""
    return f32(f32(ns // 1_000_000_000) + f32(f32(ns % 1_000_000_000) / f32(1e9)))


class SceneModel:
    def __init__(self, octaves, bpo, mode=FULL, enable_bloom=True, colors=COLORS, gray_level=60.0, easing_pow=1.3):
        self.n, self.bpo, self.mode, self.enable_bloom = octaves * bpo, bpo, mode, enable_bloom
        self.pal = (colors, gray_level, easing_pow)
        n = self.n
        self.n_segments = min(octaves * 72, 168) - 1                                   # setup.rs:134-137
        self.xyzs = np.zeros((n, 4), f32)
        self.rgba = np.zeros((n, 4), f32)
        self.params = np.zeros((n, 3), f32)
        self.visible = np.zeros(n, bool)
        for idx in range(n):                                                            # setup.rs:97-124
            x, y = bin_to_spiral(bpo, idx)
            intro = idx % 17 == 0
            self.xyzs[idx] = (x, y, f32(-0.01), f32(3.0) if intro else f32(0.0))
            self.visible[idx] = intro
            self.rgba[idx] = (to_linear(1.0), to_linear(0.7), to_linear(0.6), f32(1.0))
        self.bass_lit, self.bass_rgba, self.bloom = 0, np.array([0.8, 0.7, 0.6, 1.0], f32), f32(0.0)
        self.shift = f32(bpo - 3 * (bpo // 12))

    def _color(self, bucket):
        return calculate_color(self.bpo, float(f32(math.fmod(float(bucket), float(self.bpo)))), *self.pal)

    def update(self, peaks, calmness, accuracy, deviation, scene_calmness, dt_ns):
        n, dt = self.n, secs_f32(int(dt_ns))
        for idx in range(n):                                                            # update.rs:150-178
            size = f32(self.xyzs[idx, 3] / F)
            if f32(size * F) >= CUTOFF:
                self.visible[idx] = True
                dropoff = powf(f32(f32(0.85) - f32(f32(0.15) * f32(f32(idx) / f32(n)))), f32(f32(30.0) * dt))
                size = f32(size * dropoff)
                self.xyzs[idx, 3] = f32(size * F)
                self.rgba[idx, 3] = f32(np.fmax(f32(self.rgba[idx, 3] * dropoff), f32(0.7)))
                self.xyzs[idx, 2] = f32(self.xyzs[idx, 2] - f32(f32(f32(0.001) * f32(30.0)) * dt))
            if f32(size * F) < CUTOFF:
                self.visible[idx] = False
        if not peaks:                                                                   # update.rs:85-87
            return
        peaks = [(f32(c), f32(s)) for c, s in peaks]
        best, k_max = f32(np.finfo(np.float32).min), 0                                  # util.rs:48-57
        for k, (_, s) in enumerate(peaks):
            if s > best:
                best, k_max = s, k
        max_size = peaks[k_max][1]
        rounded = {}
        for c, s in peaks:                                                              # update.rs:208-212
            rounded[as_usize(np.trunc(c))] = (c, s)
        with np.errstate(all="ignore"):
            for idx, (c, s) in rounded.items():                                         # update.rs:214-304
                if idx >= n:
                    continue
                r, g, b = self._color(f32(c + self.shift))
                t = f32(f32(1.0) - f32(s / max_size))
                coef = f32(f32(1.0) - f32(t * t))
                x, y = bin_to_spiral(self.bpo, c)
                self.xyzs[idx, :3] = (x, y, f32(f32(f32(s / max_size) - f32(1.01)) * f32(12.5)))
                self.rgba[idx] = [clamp(to_linear(v), f32(0.0), f32(1.0)) for v in (r, g, b)] + [coef]
                calm = clamp(f32(f32(calmness[idx]) - f32(0.27)), f32(0.0), f32(1.0))
                self.params[idx] = (calm, accuracy[idx], deviation[idx])
                k = f32(0.7) if self.mode == PERFORMANCE else f32(1.0)
                scale = f32(f32(f32(s * k) * F) * f32(f32(1.0) + f32(f32(0.2) * calm)))
                self.xyzs[idx, 3] = scale
                if scale >= f32(0.002):
                    self.visible[idx] = True
            hide = np.zeros(n, bool)                                                    # update.rs:307-330
            radius = f32(f32(self.bpo // 12) * f32(0.23))
            for idx, (c, _) in rounded.items():
                if idx >= n:
                    continue
                lo = as_usize(np.fmax(rround(f32(c - radius)), f32(0.0)))
                hi = as_usize(np.fmin(rround(f32(c + radius)), f32(n - 1)))
                hide[lo:hi + 1] = True
            for idx in rounded:
                if idx < n:
                    hide[idx] = False
            self.visible[hide] = False
            if not self.enable_bloom or self.mode == PERFORMANCE:                       # update.rs:336-351
                self.bloom = f32(0.0)
            else:
                self.bloom = clamp(f32(f32(scene_calmness) * f32(1.3)), f32(0.0), f32(1.0))
            self.bass_lit = 0                                                           # update.rs:369-425
            if self.mode == GALAXY:
                return
            c0, s0 = peaks[0]
            rc = rround(f32(f32(c0 / f32(self.bpo)) * f32(12.0)))
            if as_usize(rc) * 6 >= self.n_segments:
                return
            self.bass_lit = as_usize(f32(rc * f32(6.0)))
            if self.bass_lit:
                r, g, b = self._color(f32(f32(f32(rc * f32(self.bpo)) / f32(12.0)) + self.shift))
                t = f32(f32(1.0) - f32(s0 / max_size))
                self.bass_rgba = np.array([r, g, b, f32(f32(1.0) - f32(t * t))], f32)

    def get(self):
        return {"ball_xyzs": self.xyzs.copy(), "ball_rgba": self.rgba.copy(), "ball_params": self.params.copy(),
                "ball_visible": pack_mask(self.visible), "bass_lit": int(self.bass_lit), "bass_rgba": self.bass_rgba.copy(),
                "bloom": f32(self.bloom)}


def pack_mask(visible):
    bits = np.zeros(((len(visible) + 31) // 32) * 32, np.uint8)
    bits[:len(visible)] = visible
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


EXACT = ("ball_visible", "ball_params", "bass_lit", "bloom")


def compare(got, want, rel):
    """The bars of tests/test_scene.py on two dicts of scene arrays (any leading dimensions): scale, z, mask, params, bass_lit and
    bloom bit-identical; x, y and the eight colour channels within rel * max(1, |want|), NaN where the other has NaN.  Returns the
    largest |difference| / max(1, |want|) seen."""
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=np.asarray(want[k]).dtype.kind == "f"), k
    g, w = np.asarray(got["ball_xyzs"]), np.asarray(want["ball_xyzs"])
    assert np.array_equal(g[..., 2:].view(np.uint32), w[..., 2:].view(np.uint32)), "z / scale"
    worst = 0.0
    for gg, ww in ((g[..., :2], w[..., :2]), (np.asarray(got["ball_rgba"]), np.asarray(want["ball_rgba"])),
                   (np.asarray(got["bass_rgba"]), np.asarray(want["bass_rgba"]))):
        gg, ww = gg.astype(np.float64), ww.astype(np.float64)
        assert np.array_equal(np.isnan(gg), np.isnan(ww))
        ok = ~np.isnan(ww)
        d = np.abs(gg[ok] - ww[ok]) / np.maximum(1.0, np.abs(ww[ok]))
        if d.size:
            worst = max(worst, float(d.max()))
    assert worst <= rel, worst
    return worst


# ---- inputs: frames of an oracle AnalysisState, and crafted frames ------------------------------------------------------------------
def oracle_frames(min_freq, octaves, bpo, n_frames, seed, db_frames=None):
    """Per frame (peaks, calmness, pitch_accuracy, pitch_deviation, scene_calmness) of oracle.analysis_state.OracleAnalysisState over
    n_frames consecutive frames at 1 / 30 s: the recipe of render_model.oracle_rows, extended to the fields the scene reads."""
    from oracle.analysis_state import OracleAnalysisState
    import render_model as RM
    n_bins = octaves * bpo
    if db_frames is None:
        rng = np.random.default_rng(seed)
        db_frames = (rng.random((n_frames, n_bins), dtype=np.float32) * 6.0).astype(f32)
        for _ in range(6):
            b0, t0 = int(rng.integers(3, n_bins - 3)), int(rng.integers(0, max(1, n_frames - 10)))
            t1 = min(n_frames, t0 + int(rng.integers(10, 60)))
            lvl = float(rng.uniform(18.0, 50.0))
            for t in range(t0, t1):
                b = int(np.clip(b0 + (t - t0) // 17, 2, n_bins - 3))
                db_frames[t, b] = lvl + 0.3 * np.sin(t / 7.0)
                db_frames[t, b - 1] = max(db_frames[t, b - 1], lvl - 9.0)
                db_frames[t, b + 1] = max(db_frames[t, b + 1], lvl - 11.0)
    del RM
    st = OracleAnalysisState(min_freq, octaves, bpo)
    out = []
    for f in range(n_frames):
        st.preprocess(db_frames[f], 33_333_333)
        out.append((list(zip(st.centers.astype(f32).tolist(), st.sizes.astype(f32).tolist())), np.array([e.y for e in st.calm], f32),
                    st.pitch_accuracy.astype(f32).copy(), st.pitch_deviation.astype(f32).copy(), f32(st.scene.y)))
    return out


def crafted_frames(n, bpo, seed):
    """Frames that exercise what a random stimulus rarely does; each is (name, peaks, calmness, accuracy, deviation, scene_calmness)."""
    rng = np.random.default_rng(seed)
    fields = lambda: (rng.random(n).astype(f32), rng.random(n).astype(f32), (rng.random(n).astype(f32) - f32(0.5)), f32(rng.random()))
    m = n // 2
    radius = (bpo // 12) * 0.23
    near = max(1.0, math.floor(radius))
    out = [("same_key_ab", [(m + 0.2, 9.0), (m + 0.7, 14.0)]), ("same_key_ba", [(m + 0.7, 14.0), (m + 0.2, 9.0)]),
           ("within_hide_radius", [(m + 0.1, 20.0), (m + 0.1 + near, 12.0), (5.5, 30.0)]),
           ("first_and_last_bin", [(0.4, 11.0), (n - 0.5, 25.0)]),
           ("seventy", [(float(f32((i * 7919) % n + 0.25)), float(f32(3.0 + (i * 37) % 23))) for i in range(70)]),
           ("all_zero_sizes", [(m - 3.5, 0.0), (m + 4.5, 0.0)]), ("full_a", [(m + 2.3, 18.0), (3.6, 8.0)]), ("empty", []),
           ("full_b", [(m - 6.4, 7.0), (m + 9.1, 16.0)])]
    return [(name, pk) + fields() for name, pk in out]
