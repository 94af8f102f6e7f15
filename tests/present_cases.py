"""Crafted inputs of the present stage, shared by the host tests (tests/test_present.py) and the device tests
(tests/test_present_gpu.py), and the bars both hold the results to.

Sizes: 1 x 1, 2 x 3, 5 x 4, 17 x 9, 129 x 33 (no multiple of the 16 x 16 tile or the 8 x 8 wave block, more than one tile), 4 x 130
(its mips are 1 wide long before the chain ends), 64 x 64; max_mip_dimension 4, 8, 16 and 64 (1, 2, 3 and 5 mips), one 33 x 17 case at
the default 512 (mip 0 is 994 x 512: the picture is magnified) and 1 x 1 at 16.  Content: a single lit pixel at a corner, on an edge
and in the middle, a constant, a checkerboard of 0.1 / 4.0 either side of the threshold's knee, an HDR ramp 0 .. 50, pixels that are
NaN, +-inf and negative, alpha 0, 0.5, 2 and NaN.  Both composite modes, both tone-mapping values, threshold 0, curvature 1 (the
infinite exponent) and 0.5.

Chain length and odd sides: 1 x 64 at 4096 (11 mips, 64 x 4096 down to 1 x 4: every table filled to MAX_MIPS) and at 4095 (10 mips of odd
heights), 40 x 24 at 100 (a ratio that is no integer, sides that halve unevenly), 4096 x 1 at 4 (one mip of 16 384 x 4, the widest the plan
admits: 1 024 tiles along x).  `forms` restates which kernel form the host picks for a picture's two passes; `stride_rows` makes the 61
patterns of the row-stride test (STRIDE_SHAPES)."""
import numpy as np

import present_model as M

f32 = np.float32


def constant(W, H, value=0.8):
    img = np.full((H, W, 4), value, f32)
    img[..., 3] = 1.0
    return img


def lit(W, H, where, value=30.0):
    img = np.zeros((H, W, 4), f32)
    img[..., :3] = 0.02
    img[..., 3] = 1.0
    j, i = {"corner": (0, W - 1), "edge": (H // 2, 0), "middle": (H // 2, W // 2)}[where]
    img[j, i, :3] = (value, 0.6 * value, 0.25 * value)
    return img


def checker(W, H):
    img = np.ones((H, W, 4), f32)
    jj, ii = np.mgrid[0:H, 0:W]
    img[..., :3] = np.where((ii + jj) % 2 == 0, f32(0.1), f32(4.0))[..., None]
    img[..., 1] *= f32(0.5)
    return img


def ramp(W, H):
    img = np.ones((H, W, 4), f32)
    t = np.linspace(0.0, 50.0, W * H).astype(f32).reshape(H, W)
    img[..., 0], img[..., 1], img[..., 2] = t, t[::-1] * f32(0.5), f32(50.0) - t
    return img


def random_hdr(W, H, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 1.0, (H, W, 4)).astype(f32) ** 4 * f32(8.0)
    img[..., 3] = rng.uniform(0.0, 1.0, (H, W)).astype(f32)
    return img


def specials(W, H, seed):
    """a random picture with NaN, +-inf and negative pixels strewn in, and alpha 0, 0.5, 2 and NaN"""
    img = random_hdr(W, H, seed)
    rng = np.random.default_rng(seed + 1)
    flat = img.reshape(-1, 4)
    for value in (np.nan, np.inf, -np.inf, -3.0):
        for at in rng.choice(W * H, max(1, W * H // 40), replace=False):
            flat[at, rng.integers(0, 3)] = value
    alphas = np.asarray([0.0, 0.5, 2.0, np.nan], f32)
    flat[:, 3] = alphas[np.arange(W * H) % 4]
    return img


EC, NONE = dict(composite_mode=0), dict(tonemapping=0)
# (name, image, intensity, settings)
CASES = [
    ("1x1-d16-constant", constant(1, 1), 0.5, dict(max_mip_dimension=16)),
    ("2x3-d4-corner", lit(2, 3, "corner"), 1.0, dict(max_mip_dimension=4)),
    ("5x4-d8-edge-ec", lit(5, 4, "edge"), 0.7, dict(max_mip_dimension=8, **EC)),
    ("17x9-d16-middle", lit(17, 9, "middle"), 0.3, dict(max_mip_dimension=16)),
    ("17x9-d16-specials", specials(17, 9, 11), 0.6, dict(max_mip_dimension=16)),
    ("129x33-d64-ramp", ramp(129, 33), 0.3, dict(max_mip_dimension=64)),
    ("129x33-d16-checker-none", checker(129, 33), 1.0, dict(max_mip_dimension=16, **NONE)),
    ("129x33-d4-ramp", ramp(129, 33), 0.6, dict(max_mip_dimension=4)),
    ("4x130-d64-ramp", ramp(4, 130), 0.8, dict(max_mip_dimension=64)),
    ("4x130-d64-corner-ec-curv", lit(4, 130, "corner"), 0.4, dict(max_mip_dimension=64, low_frequency_boost_curvature=0.5, **EC)),
    ("64x64-d64-specials", specials(64, 64, 21), 0.6, dict(max_mip_dimension=64)),
    ("64x64-d16-checker-ec-curv", checker(64, 64), 0.9, dict(max_mip_dimension=16, low_frequency_boost_curvature=0.5, low_frequency_boost=0.7, **EC)),
    ("64x64-d8-random-threshold0", random_hdr(64, 64, 31), 0.5, dict(max_mip_dimension=8, threshold=0.0)),
    ("64x64-d64-random-none-ec", random_hdr(64, 64, 32), 0.25, dict(max_mip_dimension=64, **NONE, **EC)),
    ("64x64-d4-constant", constant(64, 64, 1.7), 1.0, dict(max_mip_dimension=4)),
    ("33x17-d512-middle", lit(33, 17, "middle"), 0.5, dict()),
    ("5x4-d8-no-bloom", specials(5, 4, 41), 0.0, dict(max_mip_dimension=8)),
    ("17x9-d16-nan-intensity-none", random_hdr(17, 9, 42), float("nan"), dict(max_mip_dimension=16, **NONE)),
    ("1x64-d4096-random", random_hdr(1, 64, 51), 0.6, dict(max_mip_dimension=4096)),
    ("1x64-d4095-random", random_hdr(1, 64, 51), 0.6, dict(max_mip_dimension=4095)),
    ("40x24-d100-specials-ec", specials(40, 24, 52), 0.7, dict(max_mip_dimension=100, **EC)),
    ("4096x1-d4-ramp", ramp(4096, 1), 0.8, dict(max_mip_dimension=4)),
]
IDS = [c[0] for c in CASES]


# ---- the row-stride test's rows (tests/test_present_gpu.py) ----
# (W, H, max_mip_dimension, rows): every workgroup of the first makes 3 trips and rows 0 .. 2 a fourth; of the second 2 and a third
STRIDE_SHAPES = [(5, 4, 8, 3 * 65535 + 3), (24, 10, 8, 2 * 65535 + 3)]
STRIDE_PATTERNS = 61    # 65 535 % 61 = 21: a workgroup that starts on pattern p goes on to p + 21, then p + 42 (mod 61)
# pattern p's intensity is STRIDE_CYCLE[p % 9]: 0 and NaN skip bloom (14 of the 61 patterns), the rest are spread over (0, 1].  9 and 21
# share the factor 3, so the residues a workgroup meets are r, r + 3, r + 6: with the skips at 2 and 6 every run of three has at most
# one, and 8 -> 2 -> 5 and 3 -> 6 -> 0 are bloom -> skip -> bloom.
STRIDE_CYCLE = (0.3, 1.0, 0.0, 0.65, 0.12, 0.85, float("nan"), 0.5, 0.02)


def stride_rows(W, H, seed):
    """(images [61][H][W][4], intensities [61]): pattern p is random_hdr, specials at every fifth p, at STRIDE_CYCLE[p % 9]"""
    imgs = np.stack([(specials if p % 5 == 0 else random_hdr)(W, H, seed + p) for p in range(STRIDE_PATTERNS)])
    return imgs, np.asarray([STRIDE_CYCLE[p % len(STRIDE_CYCLE)] for p in range(STRIDE_PATTERNS)], f32)


# ---- which kernel form the host picks ----
TILE, FOOT = 16, 44 * 44    # present_batch.hip: a workgroup's target tile, the texels of its LDS footprint array


def _footprint(i0, wt, ws, margin):
    """present::footprint along one axis, in float32: the number of source texels that targets i0 .. i0 + 15 can sample"""
    last = min(i0 + TILE, wt) - 1
    a = (f32(i0) + f32(0.5)) / f32(wt) * f32(ws)
    b = (f32(last) + f32(0.5)) / f32(wt) * f32(ws)
    lo = int(np.floor(a - f32(margin))) - 2
    hi = int(np.floor(b + f32(margin))) + 2
    return min(max(hi, 0), ws - 1) - min(max(lo, 0), ws - 1) + 1


def _fit(wt, ht, ws, hs, mx, my):
    """footprints_fit: the widest and the highest footprint of any tile together"""
    fw = max(_footprint(i0, wt, ws, mx) for i0 in range(0, wt, TILE))
    fh = max(_footprint(j0, ht, hs, my) for j0 in range(0, ht, TILE))
    return fw * fh <= FOOT


def forms(W, H, d=512):
    """(first_staged, last_staged): whether the picture -> mip 0 pass and the mip 0 -> picture pass stage their footprints in LDS.
    Restates present::footprint, footprints_fit, tent_x and tent_reach (present_math.hpp, present_batch.hip) in NumPy float32."""
    w0, h0 = M.mips(W, H, d)[0]
    x = f32(0.004) / (f32(W) / f32(H))
    return _fit(w0, h0, W, H, 2.0, 2.0), _fit(W, H, w0, h0, x * f32(w0), f32(0.004) * f32(h0))


_models = {}


def model(name):
    """(bytes, hdr) of the model for a case, computed once"""
    if name not in _models:
        _, img, intensity, kw = CASES[IDS.index(name)]
        _models[name] = M.present(img, intensity, **kw)
    return _models[name]


def compare(tag, got_bytes, got_hdr, want_bytes, want_hdr, image):
    """The bars: out_hdr within 1e-5 of the image's largest finite value, with the same NaNs and infinities; bytes at
    most one level apart and at most 1 % of them different (the render stage's bar).  Prints what it saw."""
    finite = np.isfinite(image)
    scale = float(np.abs(image[finite]).max()) if finite.any() else 1.0
    both = np.isfinite(got_hdr) & np.isfinite(want_hdr)
    odd = ~both
    inf = np.isinf(want_hdr)
    same_odd = np.array_equal(np.isnan(got_hdr), np.isnan(want_hdr)) and np.array_equal(np.isinf(got_hdr), inf) and \
        np.array_equal(got_hdr[inf], want_hdr[inf])
    err = float(np.abs(got_hdr[both].astype(np.float64) - want_hdr[both]).max()) if both.any() else 0.0
    step = np.abs(got_bytes.astype(np.int32) - want_bytes.astype(np.int32))
    share = float((step != 0).mean())
    print(f"{tag}: max |hdr - want| = {err:.3e} (bar {1e-5 * scale:.3e}), {int(odd.sum())} non-finite, bytes differing {100 * share:.4f} %, "
          f"largest byte step {int(step.max())}")
    assert same_odd, (tag, "NaNs and infinities differ")
    assert err <= 1e-5 * scale, (tag, err, scale)
    assert step.max() <= 1, (tag, int(step.max()))
    assert share <= 0.01, (tag, share)
    return err, share
