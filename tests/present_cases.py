"""Crafted inputs of the present stage, shared by the host tests (tests/test_present.py) and the device tests
(tests/test_present_gpu.py), and the bars both hold the results to.

Sizes: 1 x 1, 2 x 3, 5 x 4, 17 x 9, 129 x 33 (no multiple of the 16 x 16 tile or the 8 x 8 wave block, more than one tile), 4 x 130
(its mips are 1 wide long before the chain ends), 64 x 64; max_mip_dimension 4, 8, 16 and 64 (1, 2, 3 and 5 mips), one 33 x 17 case at
the default 512 (mip 0 is 994 x 512: the picture is magnified) and 1 x 1 at 16.  Content: a single lit pixel at a corner, on an edge
and in the middle, a constant, a checkerboard of 0.1 / 4.0 either side of the threshold's knee, an HDR ramp 0 .. 50, pixels that are
NaN, +-inf and negative, alpha 0, 0.5, 2 and NaN.  Both composite modes, both tone-mapping values, threshold 0, curvature 1 (the
infinite exponent) and 0.5."""
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
]
IDS = [c[0] for c in CASES]

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
