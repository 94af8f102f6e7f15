"""The present stage (pvq_present_*: bloom, display transform and sRGB bytes) as far as it goes without a GPU: the symbols, the
argument checks and the host-only handle, what the compiler made of the kernels, known answers worked from the rule's statement
alone, and the host face against tests/present_model.py on every crafted case of tests/present_cases.py.

The bars, here and in tests/test_present_gpu.py (present_cases.compare): the bloomed linear picture within 1e-5 of the image's largest
finite value, bytes at most one level apart and at most 1 % of them different.  Host face and model share every operation but the powers
and exponentials (the host's first-pass power is taken in double arithmetic and rounded once to f32, the rest are libm's; the model's are
NumPy's); on the crafted cases they were seen to differ by at most 6.1e-5 at a largest value of 50 (bar 5e-4) and in no byte."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import present_cases as PC
import present_model as M
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import present as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32
NAMES = ["pvq_present_batch_create", "pvq_present_batch_destroy", "pvq_present_batch_rows_device", "pvq_present_batch_set_workspace_limit",
         "pvq_present_blend_factors", "pvq_present_default_settings", "pvq_present_frame", "pvq_present_mips"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. symbols and arguments ---------------------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    assert sorted(set(re.findall(r"\b(pvq_present_\w+)\s*\(", hdr))) == NAMES
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.PresentBatch is PP.PresentBatch and P.present_frame is PP.present_frame
    assert P.present_mips is PP.present_mips and P.present_blend_factors is PP.present_blend_factors


def test_default_settings_are_the_reference_cameras():
    s = P.present_settings()
    got = [getattr(s, k) for k in PP._FIELDS]
    assert got == [1.0, 1.0, f32(0.52), f32(0.17), f32(0.82), PP.ADDITIVE, 512, PP.TONEMAP_SOMEWHAT_BORING]
    _lib.load().pvq_present_default_settings(None)


def bad_settings():
    """(settings, word of the error text)"""
    out = []
    for k in PP._FIELDS[:5]:
        for v in (math.nan, math.inf, -math.inf):
            out.append((P.present_settings(**{k: v}), "finite"))
    out += [(P.present_settings(high_pass_frequency=0.0), "high_pass_frequency"), (P.present_settings(high_pass_frequency=-0.5), "high_pass_frequency")]
    out += [(P.present_settings(composite_mode=v), "composite_mode") for v in (-1, 2)]
    out += [(P.present_settings(tonemapping=v), "tonemapping") for v in (-1, 2)]
    out += [(P.present_settings(max_mip_dimension=v), "max_mip_dimension") for v in (1, 3, 4097, 1 << 31)]
    return out


def test_argument_ranges_and_host_only_handle():
    L = _lib.load()
    buf = np.zeros(4096, f32)
    p = buf.ctypes.data   # stands for device memory; a host-only handle never dereferences it
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    bp = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    up = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    ok = P.present_settings(max_mip_dimension=8)
    text = lambda: L.pvq_last_error().decode()
    # the pure queries
    n = C.c_uint32()
    assert L.pvq_present_mips(8, 8, 0, C.byref(n), None) == _lib.PVQ_OK and n.value == 8
    assert L.pvq_present_mips(8, 8, 4, None, up) == _lib.PVQ_OK
    for w, h in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert L.pvq_present_mips(w, h, 0, C.byref(n), None) == _lib.PVQ_ERR_INVALID_ARG and "4096" in text()
    for d in (1, 3, 4097):
        assert L.pvq_present_mips(8, 8, d, C.byref(n), None) == _lib.PVQ_ERR_INVALID_ARG and "max_mip_dimension" in text()
    assert L.pvq_present_mips(4096, 1, 512, C.byref(n), None) == _lib.PVQ_ERR_UNSUPPORTED and "16384" in text()
    assert L.pvq_present_blend_factors(None, 0.5, 8, fp) == _lib.PVQ_OK
    for nm in (0, 12):
        assert L.pvq_present_blend_factors(None, 0.5, nm, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_present_blend_factors(None, 0.5, 8, None) == _lib.PVQ_ERR_INVALID_ARG
    # the host face
    frame = L.pvq_present_frame
    assert frame(C.byref(ok), 8, 8, fp, 0.5, bp, None) == _lib.PVQ_OK
    assert frame(None, 8, 8, fp, 0.5, bp, fp) == _lib.PVQ_OK                       # NULL settings: the defaults; hdr over the image
    assert frame(C.byref(ok), 8, 8, None, 0.5, bp, None) == _lib.PVQ_ERR_INVALID_ARG
    assert frame(C.byref(ok), 8, 8, fp, 0.5, None, None) == _lib.PVQ_ERR_INVALID_ARG
    for w, h in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert frame(C.byref(ok), w, h, fp, 0.5, bp, None) == _lib.PVQ_ERR_INVALID_ARG and "4096" in text()
    assert frame(None, 4096, 1, fp, 0.5, bp, None) == _lib.PVQ_ERR_UNSUPPORTED
    # the batch handle: every range, rejected before any device is touched
    create = L.pvq_present_batch_create
    h = C.c_void_p()
    assert create(-1, C.byref(ok), 64, 64, None) == _lib.PVQ_ERR_INVALID_ARG
    for s, word in bad_settings():
        assert L.pvq_present_blend_factors(C.byref(s), 0.5, 4, fp) == _lib.PVQ_ERR_INVALID_ARG and word in text(), word
        assert frame(C.byref(s), 8, 8, fp, 0.5, bp, None) == _lib.PVQ_ERR_INVALID_ARG and word in text(), word
        for dev in (-1, 0):
            assert create(dev, C.byref(s), 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value and word in text(), word
    for dev in (-1, 0):
        for w, hh in ((0, 64), (64, 0), (4097, 64), (64, 4097)):
            assert create(dev, C.byref(ok), w, hh, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, None, 4096, 1, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
    for s, w, hh in ((None, 1, 1), (P.present_settings(max_mip_dimension=4096), 4096, 4096), (P.present_settings(max_mip_dimension=4), 129, 33)):
        assert create(-1, C.byref(s) if s is not None else None, w, hh, C.byref(h)) == _lib.PVQ_OK and h.value
        L.pvq_present_batch_destroy(h)
    assert create(-1, C.byref(ok), 64, 48, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        call = L.pvq_present_batch_rows_device
        assert call(None, 1, p, p, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, p, p, p, p, None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in text()
        assert call(h, 1, p, None, p, None, None) == _lib.PVQ_ERR_NO_DEVICE        # no intensities, no hdr
        assert call(h, 1, p, p, p, p + 16, None) == _lib.PVQ_ERR_NO_DEVICE
        assert call(h, 0, p, p, p, p, None) == _lib.PVQ_ERR_NO_DEVICE
        assert call(h, 1, None, p, p, p, None) == _lib.PVQ_ERR_INVALID_ARG          # no image
        assert call(h, 1, p, p, None, p, None) == _lib.PVQ_ERR_INVALID_ARG          # no bytes
        assert call(h, 1, p + 8, p, p, p, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in text()
        assert call(h, 1, p, p, p, p + 4, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in text()
        assert call(h, 1, p, p + 2, p, p, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in text()
        assert call(h, 1, p, p, p + 1, p, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in text()
        assert call(h, 1 << 31, p, p, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_present_batch_set_workspace_limit(h, 1 << 20) == _lib.PVQ_OK
        assert L.pvq_present_batch_set_workspace_limit(h, 0) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_present_batch_set_workspace_limit(None, 1) == _lib.PVQ_ERR_INVALID_ARG
    finally:
        L.pvq_present_batch_destroy(h)
    L.pvq_present_batch_destroy(None)
    # the Python face
    b = P.PresentBatch(64, 48, device=None, max_mip_dimension=16)
    assert (b.width, b.height, b.settings.max_mip_dimension) == (64, 48, 16)
    b.set_workspace_limit(1 << 20)
    with pytest.raises(ValueError):
        b.rows_device(p)
    with pytest.raises(ValueError):
        P.PresentBatch(64, 5000, device=None)
    with pytest.raises(ValueError):
        P.PresentBatch(64, 48, device=None, threshold=math.nan)
    with pytest.raises(TypeError):
        P.PresentBatch(64, 48, device=None, treshold=0.1)
    with pytest.raises(ValueError):
        P.present_frame(np.zeros((4, 4, 3), f32), 0.5)
    with pytest.raises(ValueError):
        P.present_mips(8, 8, 5000)


# ---- 2. kernel resources --------------------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """no kernel of the unit uses scratch; VGPRs, LDS and occupancy recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "present_batch.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "x.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(usage) == 6, list(usage)
    kinds = {"present_downILb1ELb1E": "first pass, staged", "present_downILb1ELb0E": "first pass", "present_downILb0ELb1E": "down, staged",
             "present_upILb0ELb1E": "up, staged", "present_upILb1ELb1E": "last pass, staged", "present_upILb1ELb0E": "last pass"}
    budget = {"first pass, staged": 256, "first pass": 288, "down, staged": 200, "up, staged": 136, "last pass, staged": 176, "last pass": 168}
    seen = set()
    for k, u in usage.items():
        kind = [v for key, v in kinds.items() if key in k]
        assert len(kind) == 1, k
        seen.add(kind[0])
        print(f"{kind[0]}: {u}")
        assert u["ScratchSize"] == 0, (k, u)
        assert u["LDS"] == (44 * 44 * 16 if "staged" in kind[0] else 0), (k, u)   # a tile's footprint of 16-byte texels
        # The taps of a texel are independent, and the compiler keeps as many in flight as registers allow: one or two waves a SIMD in
        # the first pass, whose fifteen double-precision powers are inlined, two or three elsewhere.
        assert u["VGPRs"] + u.get("AGPRs", 0) <= budget[kind[0]], (k, u)
        assert u["Occupancy"] >= (1 if kind[0] == "first pass" else 2), (k, u)
    assert seen == set(kinds.values())


# ---- 3. known answers -----------------------------------------------------------------------------------------------------------
def test_mips_known_answers():
    assert P.present_mips(1280, 720) == [(910, 512), (455, 256), (227, 128), (113, 64), (56, 32), (28, 16), (14, 8), (7, 4)]
    assert P.present_mips(1280, 720, 512) == P.present_mips(1280, 720, 0)
    assert P.present_mips(4, 130, 64) == [(2, 64), (1, 32), (1, 16), (1, 8), (1, 4)]
    assert P.present_mips(1, 1, 16) == [(16, 16), (8, 8), (4, 4)]
    assert [len(P.present_mips(64, 64, d)) for d in (4, 7, 8, 16, 64, 512, 4096)] == [1, 1, 2, 3, 5, 8, 11]
    assert P.present_mips(1, 4096, 4) == [(1, 4)]                    # round(1 * 4 / 4096) = 0: at least one texel
    # 11 mips, every table filled to MAX_MIPS; 10 mips of odd heights; a ratio that is no integer; the widest mip 0 the plan admits
    assert P.present_mips(1, 64, 4096) == [(64, 4096), (32, 2048), (16, 1024), (8, 512), (4, 256), (2, 128), (1, 64), (1, 32), (1, 16), (1, 8), (1, 4)]
    assert P.present_mips(1, 64, 4095) == [(64, 4095), (32, 2047), (16, 1023), (8, 511), (4, 255), (2, 127), (1, 63), (1, 31), (1, 15), (1, 7)]
    assert P.present_mips(40, 24, 100) == [(167, 100), (83, 50), (41, 25), (20, 12), (10, 6)]
    assert P.present_mips(4096, 1, 4) == [(16384, 4)]
    assert P.present_mips(5, 4, 8) == [(10, 8), (5, 4)] and P.present_mips(24, 10, 8) == [(19, 8), (9, 4)]   # the stride shapes
    for W, H, d in ((1280, 720, 512), (4, 130, 64), (129, 33, 16), (33, 17, 512), (5, 4, 8), (24, 10, 8), (1, 64, 4096), (1, 64, 4095),
                    (40, 24, 100), (4096, 1, 4)):
        assert P.present_mips(W, H, d) == M.mips(W, H, d)


def test_every_kernel_form_has_a_case():
    """The host picks each of the picture's two passes from two forms, staged in LDS or sampling device memory, by whether every tile's
    footprint fits 44 x 44 texels.  present_cases.forms restates that rule; this test holds the crafted cases and the stride shapes to
    it, so that a change to the footprint rule which leaves a form without a case fails here.  It is a mirror of the library and no
    more: it cannot see which kernel a call launched, only say which one the rule, as restated, picks."""
    shapes = {name: (img.shape[1], img.shape[0], kw.get("max_mip_dimension", 512)) for name, img, _, kw in PC.CASES}
    shapes.update({f"stride {W}x{H}-d{d}": (W, H, d) for W, H, d, _ in PC.STRIDE_SHAPES})
    got = {name: PC.forms(*s) for name, s in shapes.items()}
    for name, f in got.items():
        print(f"{name}: first pass {'staged' if f[0] else 'unstaged'}, last pass {'staged' if f[1] else 'unstaged'}")
    # A picture cannot have both passes unstaged: the first needs a mip 0 far smaller than the picture, the last one far larger.
    assert set(got.values()) == {(True, True), (False, True), (True, False)}
    for first_staged in (True, False):
        assert any(f[0] == first_staged for f in got.values())
    for last_staged in (True, False):
        assert any(f[1] == last_staged for f in got.values())
    named = {(64, 64, 4): (False, True), (64, 64, 8): (False, True), (129, 33, 4): (False, True),
             (33, 17, 512): (True, False), (40, 24, 100): (True, False), (1, 64, 4096): (True, False),
             (5, 4, 8): (True, True), (24, 10, 8): (True, True), (17, 9, 16): (True, True)}
    for s, want in named.items():
        assert s in shapes.values(), s
        assert PC.forms(*s) == want, (s, PC.forms(*s), want)
    assert all(PC.forms(W, H, d) == (True, True) for W, H, d, _ in PC.STRIDE_SHAPES)


@pytest.mark.parametrize("intensity", [0.0, 0.3, 1.0])
def test_blend_factors_at_the_reference_settings(intensity):
    """curvature 1: lf = 1 - powf(1 - r, inf) is 0 at r = 0 and 1 elsewhere, so B_0 = intensity and B_k = (intensity + 1) hp"""
    n = 8
    got = P.present_blend_factors(intensity, n)
    want = []
    for k in range(n):
        r = f32(k) / f32(n - 1)
        hp = f32(1) - min(max((r - f32(0.52)) / f32(0.52), f32(0)), f32(1))
        want.append(f32(intensity) * hp if k == 0 else (f32(intensity) + f32(1)) * hp)
    assert np.array_equal(bits(got), bits(np.asarray(want, f32)))
    assert got[0] == f32(intensity) and got[1] == f32(intensity) + f32(1)
    assert np.array_equal(bits(got), bits(M.blend_factors(M.settings_of(), intensity, n)))
    assert P.present_blend_factors(intensity, 1)[0] == f32(intensity)                      # r = 0 where there is one mip
    # energy conserving, curvature 0.5: lf = (1 - (1 - r)^2) * boost * (1 - intensity)
    kw = dict(composite_mode=0, low_frequency_boost_curvature=0.5, low_frequency_boost=0.7)
    got = P.present_blend_factors(intensity, 5, **kw)
    for k in range(5):
        r = k / 4.0
        want = (intensity + (1.0 - (1.0 - r) ** 2) * 0.7 * (1.0 - intensity)) * (1.0 - min(max((r - 0.52) / 0.52, 0.0), 1.0))
        assert abs(float(got[k]) - want) < 1e-6, (k, got[k], want)


def test_transform_and_encode_known_answers():
    srgb = lambda v: 12.92 * v if v <= 0.0031308 else 1.055 * v ** (1 / 2.4) - 0.055
    greys = [0.0, 0.05, 0.5, 1.0, 4.0, 50.0]
    img = np.zeros((1, len(greys), 4), f32)
    img[0, :, :3] = np.asarray(greys, f32)[:, None]
    img[0, :, 3] = [0.0, 0.5, 2.0, math.nan, 1.0, 0.25]
    out = P.present_frame(img, 0.0)                                                        # a grey has cb = cr = 0, hence bt = 0
    assert np.array_equal(out[0, 0], [0, 0, 0, 0])
    for i, v in enumerate(greys):
        want = 255.0 * srgb(0.97 * (1.0 - math.exp(-v)))
        assert np.all(out[0, i, :3] == out[0, i, 0]) and abs(float(out[0, i, 0]) - want) <= 0.5 + 1e-3, (v, out[0, i], want)
    assert out[0, :, 3].tolist() == [0, 128, 255, 0, 255, 64]                              # floor(a * 255 + 0.5); a NaN encodes as 0
    values = [0.0031308, 0.5, 1.0, 0.002, 7.0, -1.0, math.nan]
    img = np.ones((1, len(values), 4), f32)
    img[0, :, :3] = np.asarray(values, f32)[:, None]
    out = P.present_frame(img, 0.0, tonemapping=0)
    assert out[0, :, 0].tolist() == [10, 188, 255, 7, 255, 0, 0]                           # 10.31, 187.52, 255, 6.59


def test_below_the_knee_bloom_changes_nothing():
    """threshold - knee = 0.17 (1 - 0.82) = 0.0306: a constant 0.02 contributes nothing to mip 0, so every tent is 0"""
    img = PC.constant(17, 9, 0.02)
    out, hdr = P.present_frame(img, 1.0, hdr=True, max_mip_dimension=16)
    assert np.array_equal(bits(hdr), bits(img))
    assert np.array_equal(out, P.present_frame(img, 0.0, max_mip_dimension=16))
    above, hdr = P.present_frame(PC.constant(17, 9, 0.5), 1.0, hdr=True, max_mip_dimension=16)
    assert (hdr[..., :3] > 0.5).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_lit_pixel_blooms_symmetrically(mode):
    W, H = 17, 9
    img = PC.lit(W, H, "middle")
    _, hdr = P.present_frame(img, 0.8, hdr=True, max_mip_dimension=16, composite_mode=mode)
    glow = hdr[..., :3] - img[..., :3]
    assert np.abs(glow - glow[:, ::-1]).max() <= 1e-5 * 30.0 and np.abs(glow - glow[::-1]).max() <= 1e-5 * 30.0
    away = glow[H // 2, W // 2 + 2:, 0]
    assert (away > 0).all() if mode == 1 else (np.abs(away) > 0).all()                     # the light spreads
    if mode == 1:
        assert (np.diff(away) <= 1e-6).all()                                               # and falls off


# ---- 4. the host face against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.IDS)
def test_frames_match_model(name):
    _, img, intensity, kw = PC.CASES[PC.IDS.index(name)]
    out, hdr = P.present_frame(img, intensity, hdr=True, **kw)
    want_out, want_hdr = PC.model(name)
    PC.compare(name, out, hdr, want_out, want_hdr, img)
    assert np.array_equal(bits(hdr[..., 3]), bits(img[..., 3]))                             # alpha passes through
    if M.settings_of(**kw)["max_mip_dimension"] and np.isfinite(intensity) and intensity > 0:
        assert not np.array_equal(bits(hdr), bits(img))                                    # bloom did something
    else:
        assert np.array_equal(bits(hdr), bits(img))
    over = img.copy()                                                                      # hdr over the image
    L = _lib.load()
    s = P.present_settings(**kw)
    again = np.empty(img.shape, np.uint8)
    fp = over.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pvq_present_frame(C.byref(s), img.shape[1], img.shape[0], fp, intensity, again.ctypes.data_as(C.POINTER(C.c_uint8)), fp) == _lib.PVQ_OK
    assert np.array_equal(again, out) and np.array_equal(bits(over), bits(hdr))
