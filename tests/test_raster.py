"""The pitch balls as pixels (pvq_raster_*) as far as it goes without a GPU: the symbols, the argument checks and the host-only
handle, what the compiler made of the kernels, known answers worked from the formulas alone, and the host face against
tests/raster_model.py.

The bar, here and in tests/test_raster_gpu.py: no differing bit in any pixel channel.  Model, host face and device do the same f32
operations in the same order, and their libm calls are double-precision functions rounded once to f32."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pitchvis_amd as P
import raster_cases as RC
import raster_model as M
from pitchvis_amd import _lib
from pitchvis_amd import raster as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, want, tag):
    diff = bits(got) != bits(want)
    assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def host_frame(W, H, r, time, **kw):
    return P.raster_frame(W, H, r["ball_xyzs"], r["ball_rgba"], r["ball_params"], r["ball_visible"], time, **kw)


def model_frame(W, H, r, time, **kw):
    return M.frame(W, H, r["ball_xyzs"], r["ball_rgba"], r["ball_params"], r["ball_visible"], time, **kw)


def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    names = sorted(set(re.findall(r"\b(pvq_raster_\w+)\s*\(", hdr)))
    assert names == ["pvq_raster_batch_create", "pvq_raster_batch_destroy", "pvq_raster_batch_frames_device", "pvq_raster_batch_get_times",
                     "pvq_raster_frame", "pvq_raster_shade", "pvq_raster_touch"]
    for name in names:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4
    assert P.RasterBatch is PR.RasterBatch and P.raster_frame is PR.raster_frame and P.raster_shade is PR.raster_shade
    assert P.raster_touch is PR.raster_touch
    assert f32(PR.VIEWPORT_HEIGHT) == M.VIEWPORT_HEIGHT


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    h = C.c_void_p()
    create = L.pvq_raster_batch_create
    assert create(-1, 7, 36, 0, 0.0, 2, 64, 64, None) == _lib.PVQ_ERR_INVALID_ARG
    for dev in (-1, 0):   # rejected before any device is touched
        for o, b, ns in ((0, 36, 4), (7, 0, 4), (7, 36, 0)):
            assert create(dev, o, b, 0, 0.0, ns, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, 1, 2, 0, 0.0, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value       # 2 bins
        assert create(dev, 25, 41, 0, 0.0, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value     # 1025 bins
        assert "1024" in L.pvq_last_error().decode()
        for mode in (-1, 4):
            assert create(dev, 7, 36, mode, 0.0, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "mode" in L.pvq_last_error().decode()
        for w, hh in ((0, 64), (64, 0), (4097, 64), (64, 4097)):
            assert create(dev, 7, 36, 0, 0.0, 4, w, hh, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "4096" in L.pvq_last_error().decode()
        for vh in (-1.0, math.inf, math.nan):
            assert create(dev, 7, 36, 0, vh, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "viewport_height" in L.pvq_last_error().decode()
    for o, b, w, hh in ((1, 3, 1, 1), (7, 36, 4096, 4096), (16, 64, 129, 33)):
        assert create(-1, o, b, 3, 20.0, 2, w, hh, C.byref(h)) == _lib.PVQ_OK and h.value
        L.pvq_raster_batch_destroy(h)
    assert create(-1, 7, 36, 0, 0.0, 3, 64, 48, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        buf = np.zeros(4096, f32)
        p = buf.ctypes.data   # stands for device memory; a host-only handle never dereferences it
        el = (C.c_float * 1)(0.5)
        call = L.pvq_raster_batch_frames_device
        full = dict(ball_xyzs=p, ball_rgba=p, ball_params=p, ball_visible=p, center=p, peak_count=p, max_peaks=8, background=None)

        def ins(**kw):
            i = _lib.CRasterInputs()
            for k, v in {**full, **kw}.items():
                setattr(i, k, v)
            return C.byref(i)
        assert call(None, 1, ins(), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, ins(), el, p, p, None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
        assert call(h, 1, ins(), el, None, None, None) == _lib.PVQ_ERR_NO_DEVICE
        assert call(h, 1, None, el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG
        for name in ("center", "peak_count"):                                       # needed with or without an image
            assert call(h, 1, ins(**{name: None}), el, None, p, None) == _lib.PVQ_ERR_INVALID_ARG, name
        for name in ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible"):       # needed for an image only
            assert call(h, 1, ins(**{name: None}), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert call(h, 1, ins(**{name: None}), el, None, p, None) == _lib.PVQ_ERR_NO_DEVICE, name
        assert call(h, 1, ins(max_peaks=0), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert "max_peaks" in L.pvq_last_error().decode()
        for name in ("ball_xyzs", "ball_rgba", "background"):                        # 16-byte loads
            assert call(h, 1, ins(**{name: p + 4}), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG, name
        assert call(h, 1, ins(), el, p + 8, None, None) == _lib.PVQ_ERR_INVALID_ARG   # 16-byte stores
        assert "aligned" in L.pvq_last_error().decode()
        assert call(h, 1, ins(), None, p, None, None) == _lib.PVQ_ERR_INVALID_ARG     # no clock
        assert "elapsed" in L.pvq_last_error().decode()
        assert call(h, 1 << 31, ins(), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_raster_batch_get_times(h, 3, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_raster_batch_get_times(h, 0, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_raster_batch_get_times(h, 0, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.PVQ_ERR_NO_DEVICE
    finally:
        L.pvq_raster_batch_destroy(h)
    L.pvq_raster_batch_destroy(None)
    assert L.pvq_raster_batch_get_times(None, 0, None) == _lib.PVQ_ERR_INVALID_ARG
    # the host face's own checks
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    up = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.pvq_raster_shade(None, fp, 0.5, 0.5, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_raster_touch(4, None, 1, 0.5, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_raster_touch(4, None, 0, 0.5, fp) == _lib.PVQ_OK
    assert L.pvq_raster_frame(4, 8, 8, 0.0, 0, fp, fp, fp, up, fp, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_raster_frame(4, 0, 8, 0.0, 0, fp, fp, fp, up, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_raster_frame(4, 8, 4097, 0.0, 0, fp, fp, fp, up, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_raster_frame(4, 8, 8, -2.0, 0, fp, fp, fp, up, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_raster_frame(4, 8, 8, 0.0, 7, fp, fp, fp, up, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    b = P.RasterBatch(P.VqtRange(55.0, 7, 36), 5, 64, 48, device=None)
    assert (b.n_bins, b.width, b.height) == (252, 64, 48)
    with pytest.raises(P.PvqError) as e:
        b.frames_device(ball_xyzs=p, ball_rgba=p, ball_params=p, ball_visible=p, center=p, peak_count=p, elapsed=[0.0], image=p, max_peaks=4)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        b.frames_device(ball_xyzs=p, ball_rgba=p, ball_params=p, ball_visible=p, peak_count=p, elapsed=[0.0], image=p, max_peaks=4)
    with pytest.raises(TypeError):
        b.frames_device(size=p, elapsed=[0.0])
    with pytest.raises(ValueError):
        P.RasterBatch(P.VqtRange(55.0, 7, 36), 5, 64, 5000, device=None)


def test_kernel_resources(tmp_path):
    """no kernel of the unit uses scratch; VGPRs and LDS recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "raster_batch.hip")
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
    kern = {}
    for want in ("raster_marks", "raster_times", "raster_lists", "raster_tiles"):
        found = [u for k, u in usage.items() if want in k]
        assert len(found) == 1, (want, list(usage))
        kern[want] = found[0]
        print(f"{want}: {found[0]}")
    assert len(usage) == 4, list(usage)
    for k, u in kern.items():
        assert u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (k, u)
    assert kern["raster_tiles"]["LDS"] == 64 * 64          # a chunk of 64 ball records
    assert kern["raster_lists"]["LDS"] <= 8 * 1024 + 64    # a key per bin
    assert kern["raster_tiles"]["Occupancy"] >= 2


# ---- host face against the model ------------------------------------------------------------------------------------------------
PARAM_SETS = [   # rgba, (calmness, time, accuracy, deviation)
    ((0.5, 0.2, 0.1, 1.0), (0.3, 1.5, 0.9, 0.1)),
    ((0.9, 0.8, 0.7, 0.6), (0.0, 0.0, 0.0, 0.0)),          # Params::default(): no calmness, time 0
    ((0.1, 0.9, 0.3, 0.8), (0.7, 12.25, 1.0, -0.5)),       # flat disc, brightness mix at 0
    ((0.3, 0.3, 0.9, 1.0), (0.6, 123.456, 0.85, 0.49)),    # accuracy on the threshold, ring weight just above 0
    ((0.0, 1.0, 0.5, 0.3), (0.15, 3600.5, 0.849999, 0.6)), # under the threshold; |dev| > 0.5: a negative star brightness
    ((1.0, 1.0, 1.0, 1.0), (1.0, 86400.0, 1.05, -0.02)),   # a day on the clock: large noise coordinates
]


def test_shade_matches_model():
    g = np.concatenate([np.linspace(-0.05, 1.05, 45), [0.5, 0.505, 0.51, 0.625, 0.98, 1.0, 0.0]]).astype(f32)
    U, V = np.meshgrid(g, g)
    for rgba, par in PARAM_SETS:
        want = M.shade(rgba, par, U, V)
        got = np.asarray([P.raster_shade(rgba, par, u, v) for u, v in zip(U.ravel(), V.ravel())]).reshape(want.shape)
        same(got, want, par)
        r = np.hypot(2 * U - 1, 2 * V - 1)
        assert np.all(got[r >= 1.001][:, 3] == 0.0) and np.all(got[r < 0.95][:, 3] >= 0.0)


def test_touch_matches_model():
    n = 36
    t_host = t_model = np.zeros(n, f32)
    lists = RC.peak_lists(n, 1, 12, 5)[0]
    lists[11] = [f32(35.999), f32(36.0), f32(1e30), f32(np.inf), f32(-np.inf), f32(-0.0)]
    for f, centers in enumerate(lists):
        before = t_host.copy()
        t_host, t_model = P.raster_touch(t_host, centers, 0.25 * (f + 1)), M.touch(t_model, centers, 0.25 * (f + 1), n)
        same(t_host, t_model, f)
        if not centers:
            same(t_host, before, f)
    assert t_host[35] == f32(3.0) and len(set(t_host.tolist())) > 4


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (64, 64), (70, 50), (129, 33)])
def test_frames_match_model(size):
    W, H = size
    n = 252
    t = np.random.default_rng(3).uniform(0.0, 200.0, n).astype(f32)
    for seed, kw in ((11, {}), (12, dict(viewport_height=22.0)), (13, dict(mode=3))):
        r = RC.row(n, seed)
        cov = []
        want = model_frame(W, H, r, t, coverage=cov, **kw)
        hk = {("visuals_mode" if k == "mode" else k): v for k, v in kw.items()}
        same(host_frame(W, H, r, t, **hk), want, (size, seed))
        assert cov[0] > 0
    e = RC.edge_row()
    bg = np.random.default_rng(4).uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    same(host_frame(W, H, e, t[:36]), model_frame(W, H, e, t[:36]), "edges")
    same(host_frame(W, H, e, t[:36], background=bg), model_frame(W, H, e, t[:36], background=bg), "edges over a background")


def test_edge_row_rules():
    """the edge row's forbidden balls would show if drawn, and its equal-z pairs depend on the bin order"""
    W, H = 64, 64
    e = RC.edge_row()
    t = np.zeros(36, f32)
    img = host_frame(W, H, e, t)
    assert img[..., :3].max() < 2.0                                          # the invisible / non-finite balls are rgb 7 and 9
    assert M.drawing_order(e["ball_xyzs"], e["ball_rgba"], e["ball_params"], e["ball_visible"], t) == [0, 1, 5, 6, 7, 8, 9, 2, 3]
    t_bad = t.copy()
    t_bad[0] = np.nan                                                        # a time that is not finite: the ball is skipped
    assert not np.array_equal(host_frame(W, H, e, t_bad), img)
    same(host_frame(W, H, e, t_bad), model_frame(W, H, e, t_bad), "nan time")


# ---- known answers, from the formulas alone -------------------------------------------------------------------------------------
def one_ball(pos, z, scale, rgba, params):
    return {"ball_xyzs": np.asarray([[pos[0], pos[1], z, scale]], f32), "ball_rgba": np.asarray([rgba], f32),
            "ball_params": np.asarray([params], f32), "ball_visible": np.asarray([1], np.uint32)}


def join(*rows):
    out = {k: np.concatenate([r[k] for r in rows]) for k in ("ball_xyzs", "ball_rgba", "ball_params")}
    out["ball_visible"] = RC.pack_visible([True] * len(rows))
    return out


def radii(W, H, pos, scale):
    s = float(M.VIEWPORT_HEIGHT) / H
    wx = (np.arange(W) + 0.5 - 0.5 * W) * s
    wy = (0.5 * H - (np.arange(H) + 0.5)) * s
    return np.hypot((wx[None, :] - pos[0]) / (10.0 * scale), (wy[:, None] - pos[1]) / (10.0 * scale))


@pytest.mark.parametrize("who", ["host", "model"])
def test_known_answers(who):
    frame = host_frame if who == "host" else model_frame
    W, H = 64, 48
    clear = np.asarray([M.srgb_to_linear(0.23), M.srgb_to_linear(0.23), M.srgb_to_linear(0.25), 1.0], f32)
    assert abs(clear[0] - ((0.23 + 0.055) / 1.055) ** 2.4) < 1e-7 and abs(clear[2] - ((0.25 + 0.055) / 1.055) ** 2.4) < 1e-7
    galaxy = np.asarray([M.srgb_to_linear(0.05), 0.0, M.srgb_to_linear(0.05), 1.0], f32)
    t0 = np.zeros(1, f32)
    # calmness >= 0.61: ring weight clamp(1 - 1.65 calmness)^3 = 0, so a ball of alpha 1 is a flat disc
    rgb = (0.8, 0.25, 0.1)
    disc = one_ball((1.0, -0.5), -1.0, 0.3, rgb + (1.0,), (0.61, 0.99, 0.3))
    img = frame(W, H, disc, np.asarray([77.0], f32))
    r = radii(W, H, (1.0, -0.5), 0.3)
    inner, outer = r <= 0.9599, r >= 1.0001
    assert inner.sum() > 200 and outer.sum() > 200
    assert np.all(img[inner] == np.asarray(rgb + (1.0,), f32))                # exactly the material colour
    assert np.all(img[outer] == clear)                                        # exactly the clear colour
    gimg = frame(W, H, disc, t0, **({"visuals_mode": 3} if who == "host" else {"mode": 3}))
    assert np.all(gimg[outer] == galaxy) and np.all(gimg[inner] == np.asarray(rgb + (1.0,), f32))
    # the centre dot: at p = (0, 0) with accuracy 1, rgb gains 0.4 (0.85 + 0.15 sin 3t); ring and star are 0 there
    shade = P.raster_shade if who == "host" else (lambda c, p, u, v: M.shade(c, p, u, v))
    for t in (0.0, 0.7, 2.0):
        got = shade((0.2, 0.3, 0.4, 1.0), (0.0, t, 1.0, 0.25), 0.5, 0.5)
        gain = 0.4 * (0.85 + 0.15 * math.sin(3 * t))
        assert np.allclose(np.asarray(got)[:3], np.asarray([0.2, 0.3, 0.4]) + gain, rtol=0, atol=2e-7), (t, got)
        assert got[3] == 0.0                                                  # alpha a ring, and the ring is sin(0)^2
    # two overlapping flat discs of alpha 0.5: the blend equation in the stated order, and the other order differs
    a = one_ball((-0.4, 0.0), -2.0, 0.3, (1.0, 0.0, 0.0, 0.5), (0.7, 0.0, 0.0))
    b = one_ball((0.4, 0.0), -1.0, 0.3, (0.0, 1.0, 0.0, 0.5), (0.7, 0.0, 0.0))
    both = (radii(W, H, (-0.4, 0.0), 0.3) <= 0.9599) & (radii(W, H, (0.4, 0.0), 0.3) <= 0.9599)
    assert both.sum() > 50
    ca, cb = np.asarray([1.0, 0.0, 0.0], f32), np.asarray([0.0, 1.0, 0.0], f32)
    half = f32(0.5)
    under_a = ca * half + clear[:3] * half                                    # a first (z = -2), then b over it
    want_ab = np.concatenate([cb * half + under_a * half, [f32(0.5) + (f32(0.5) + f32(1.0) * half) * half]]).astype(f32)
    under_b = cb * half + clear[:3] * half
    want_ba = np.concatenate([ca * half + under_b * half, want_ab[3:]]).astype(f32)
    zeros2 = np.zeros(2, f32)
    img_ab = frame(W, H, join(a, b), zeros2)
    assert np.all(img_ab[both] == want_ab) and not np.array_equal(want_ab, want_ba)
    b["ball_xyzs"][0, 2] = -3.0                                               # now b lies under a
    assert np.all(frame(W, H, join(a, b), zeros2)[both] == want_ba)
    b["ball_xyzs"][0, 2] = -2.0                                               # equal z: the lower bin first
    assert np.all(frame(W, H, join(a, b), zeros2)[both] == want_ab)
    assert np.all(frame(W, H, join(b, a), zeros2)[both] == want_ba)


def test_intro_balls_cover_the_image():
    """a fresh scene's intro balls (scale 3: side 60, radius 30) lie within 9.2 of the origin; the view's corner is at 13.1"""
    s = P.SceneState(P.VqtRange(55.0, 7, 36)).get()
    W, H = 64, 48
    img = P.raster_frame(W, H, s["ball_xyzs"], s["ball_rgba"], s["ball_params"], s["ball_visible"], np.zeros(252, f32))
    clear = M.clear_color()
    assert not np.any(np.all(img == clear, axis=-1))
    cov = []
    same(img, M.frame(W, H, s["ball_xyzs"], s["ball_rgba"], s["ball_params"], s["ball_visible"], np.zeros(252, f32), coverage=cov), "intro")
    assert cov[0] == W * H * len(range(0, 252, 17))                           # every intro ball covers every pixel
