"""The backdrop stage (pvq_backdrop_*: spider net, debug panels and lit bass spiral as pixels, and the balls drawn over them) as far
as it goes without a GPU: the symbols, the argument checks and the host-only handle, what the compiler made of the kernels, known
answers of the coverage rule worked from its statement alone, and the host face against tests/backdrop_model.py.

The bar, here and in tests/test_backdrop_gpu.py: no differing bit in any pixel channel.  Model, host face and device evaluate the
same f32 expressions in the same order; the model tries every triangle on every pixel, so it also checks that the pixel boxes of
the other two lose nothing."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_cases as BC
import backdrop_model as M
import pitchvis_amd as P
import raster_cases as RC
import raster_model as RM
from pitchvis_amd import _lib
from pitchvis_amd import backdrop as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32
NAMES = ["pvq_backdrop_balls_over_device", "pvq_backdrop_batch_create", "pvq_backdrop_batch_destroy", "pvq_backdrop_batch_frames_device",
         "pvq_backdrop_draw_mesh", "pvq_backdrop_frame", "pvq_backdrop_geometry", "pvq_backdrop_panel_transforms"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, want, tag):
    diff = bits(got) != bits(want)
    assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ---- 1. symbols and arguments ---------------------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    assert sorted(set(re.findall(r"\b(pvq_backdrop_\w+)\s*\(", hdr))) == NAMES
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.BackdropBatch is PB.BackdropBatch and P.backdrop_frame is PB.backdrop_frame and P.backdrop_draw_mesh is PB.backdrop_draw_mesh
    assert P.backdrop_geometry is PB.backdrop_geometry and P.panel_transforms is PB.panel_transforms
    assert callable(P.RasterBatch.frames_over)
    assert (PB.NET_SPIRAL, PB.NET_RAYS, PB.BASS) == (M.NET_SPIRAL, M.NET_RAYS, M.BASS) == (0, 1, 2)


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    h = C.c_void_p()
    create = L.pvq_backdrop_batch_create
    assert create(-1, 7, 36, 0, 0.0, 2, 64, 64, None) == _lib.PVQ_ERR_INVALID_ARG
    for dev in (-1, 0):   # the raster stage's ranges, rejected before any device is touched
        for o, b, ns in ((0, 36, 4), (7, 0, 4), (7, 36, 0)):
            assert create(dev, o, b, 0, 0.0, ns, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, 1, 2, 0, 0.0, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
        assert create(dev, 25, 41, 0, 0.0, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
        assert "1024" in L.pvq_last_error().decode()
        for mode in (-1, 4):
            assert create(dev, 7, 36, mode, 0.0, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        for w, hh in ((0, 64), (64, 0), (4097, 64), (64, 4097)):
            assert create(dev, 7, 36, 0, 0.0, 4, w, hh, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "4096" in L.pvq_last_error().decode()
        for vh in (-1.0, math.inf, math.nan):
            assert create(dev, 7, 36, 0, vh, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "viewport_height" in L.pvq_last_error().decode()
    for o, b, w, hh in ((1, 3, 1, 1), (7, 36, 4096, 4096), (16, 64, 129, 33)):
        assert create(-1, o, b, 3, 20.0, 2, w, hh, C.byref(h)) == _lib.PVQ_OK and h.value
        L.pvq_backdrop_batch_destroy(h)
    assert create(-1, 7, 36, 0, 0.0, 3, 64, 48, C.byref(h)) == _lib.PVQ_OK and h.value
    buf = np.zeros(4096, f32)
    p = buf.ctypes.data   # stands for device memory; a host-only handle never dereferences it
    try:
        call = L.pvq_backdrop_batch_frames_device
        full = dict(bass_lit=p, bass_rgba=p, line_pos=p, line_rgba=p, disc_pos=p, disc_rgba=p, peak_count=p, max_peaks=8, hist_pos=p,
                    hist_rgba=p, graph_pos=p, graph_rgba=p, graph_capacity=300, background=None)

        def ins(**kw):
            i = _lib.CBackdropInputs()
            for k, v in {**full, **kw}.items():
                setattr(i, k, v)
            return C.byref(i)
        assert call(None, 1, ins(), p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, ins(), p, None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
        assert call(h, 1, None, p, None) == _lib.PVQ_ERR_NO_DEVICE                      # no inputs at all: net over clear
        assert call(h, 1, ins(), None, None) == _lib.PVQ_ERR_INVALID_ARG                # no image
        for name in ("bass_lit", "bass_rgba", "line_pos", "line_rgba", "disc_pos", "disc_rgba", "hist_pos", "hist_rgba", "graph_pos",
                     "graph_rgba"):                                                     # a half-given group
            assert call(h, 1, ins(**{name: None}), p, None) == _lib.PVQ_ERR_INVALID_ARG, name
        for group in (("bass_lit", "bass_rgba"), ("line_pos", "line_rgba"), ("disc_pos", "disc_rgba", "peak_count"), ("hist_pos", "hist_rgba"),
                      ("graph_pos", "graph_rgba")):                                     # a group left out whole
            assert call(h, 1, ins(**{k: None for k in group}), p, None) == _lib.PVQ_ERR_NO_DEVICE, group
        assert call(h, 1, ins(peak_count=None), p, None) == _lib.PVQ_ERR_INVALID_ARG    # discs without counts
        assert call(h, 1, ins(max_peaks=0), p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert "max_peaks" in L.pvq_last_error().decode()
        for cap in (0, 1, 1025):
            assert call(h, 1, ins(graph_capacity=cap), p, None) == _lib.PVQ_ERR_INVALID_ARG
        for name in ("bass_rgba", "line_rgba", "disc_rgba", "hist_rgba", "graph_rgba", "background"):   # 16-byte loads
            assert call(h, 1, ins(**{name: p + 4}), p, None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert "aligned" in L.pvq_last_error().decode()
        assert call(h, 1, ins(), p + 8, None) == _lib.PVQ_ERR_INVALID_ARG               # 16-byte stores
        assert call(h, 1, ins(line_pos=p + 2), p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1 << 31, ins(), p, None) == _lib.PVQ_ERR_INVALID_ARG
    finally:
        L.pvq_backdrop_batch_destroy(h)
    L.pvq_backdrop_batch_destroy(None)
    # the balls over a picture: the raster stage's checks, and its own two
    r = C.c_void_p()
    assert L.pvq_raster_batch_create(-1, 7, 36, 0, 0.0, 3, 64, 48, C.byref(r)) == _lib.PVQ_OK
    try:
        over = L.pvq_backdrop_balls_over_device
        i = _lib.CRasterInputs(p, p, p, p, p, p, 8, None)
        el = (C.c_float * 1)(0.5)
        assert over(None, 1, C.byref(i), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert over(r, 1, C.byref(i), el, p, None, None) == _lib.PVQ_ERR_NO_DEVICE
        assert over(r, 1, C.byref(i), el, None, p, None) == _lib.PVQ_ERR_INVALID_ARG and "d_image" in L.pvq_last_error().decode()
        assert over(r, 1, C.byref(i), el, p + 8, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert over(r, 1, C.byref(i), None, p, None, None) == _lib.PVQ_ERR_INVALID_ARG
        i.background = p
        assert over(r, 1, C.byref(i), el, p, None, None) == _lib.PVQ_ERR_INVALID_ARG and "background" in L.pvq_last_error().decode()
        assert L.pvq_raster_batch_frames_device(r, 1, C.byref(i), el, p, None, None) == _lib.PVQ_ERR_NO_DEVICE   # as before
    finally:
        L.pvq_raster_batch_destroy(r)
    # the host face's own checks
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    n = C.c_uint32()
    for o, what in ((0, 0), (1025, 0), (2, -1), (2, 3)):
        assert L.pvq_backdrop_geometry(o, what, None, C.byref(n)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_geometry(2, 1, None, None) == _lib.PVQ_OK
    assert L.pvq_backdrop_panel_transforms(252, 64, 64, 0.0, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_panel_transforms(252, 0, 64, 0.0, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_panel_transforms(252, 64, 64, -1.0, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_draw_mesh(8, 8, 8.0, 1, fp, fp, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_draw_mesh(8, 8, 8.0, 1, None, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_draw_mesh(8, 8, 8.0, 0, None, None, None, fp) == _lib.PVQ_OK
    assert L.pvq_backdrop_draw_mesh(8, 4097, 8.0, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_backdrop_draw_mesh(8, 8, math.nan, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    frame = L.pvq_backdrop_frame
    assert frame(2, 12, 8, 8, 0.0, 0, 0, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert frame(2, 12, 8, 8, 0.0, 0, 1, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG       # lit segments without a colour
    assert frame(0, 12, 8, 8, 0.0, 0, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert frame(2, 12, 0, 8, 0.0, 0, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert frame(2, 12, 8, 8, -1.0, 0, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert frame(2, 12, 8, 8, 0.0, 4, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    half = _lib.CBackdropPanels()
    half.line_pos = p
    assert frame(2, 12, 8, 8, 0.0, 0, 0, None, C.byref(half), None, fp) == _lib.PVQ_ERR_INVALID_ARG
    half.line_rgba, half.graph_pos, half.graph_rgba, half.graph_capacity = p, p, p, 1
    assert frame(2, 12, 8, 8, 0.0, 0, 0, None, C.byref(half), None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert frame(2, 12, 8, 8, 0.0, 0, 0, None, None, None, fp) == _lib.PVQ_OK
    b = P.BackdropBatch(P.VqtRange(55.0, 7, 36), 5, 64, 48, device=None)
    assert (b.n_bins, b.width, b.height) == (252, 64, 48)
    with pytest.raises(P.PvqError) as e:
        b.frames(1, bass_lit=p, bass_rgba=p, image=p)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        b.frames(1, bass_lit=p, image=p)
    with pytest.raises(TypeError):
        b.frames(1, size=p, image=p)
    with pytest.raises(ValueError):
        P.BackdropBatch(P.VqtRange(55.0, 7, 36), 5, 64, 5000, device=None)
    with pytest.raises(ValueError):
        P.RasterBatch(P.VqtRange(55.0, 7, 36), 5, 64, 48, device=None).frames_over(True, elapsed=[0.0])


# ---- 2. kernel resources --------------------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """no kernel of the unit uses scratch; VGPRs, LDS and occupancy recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "backdrop_batch.hip")
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
    for want in ("backdrop_lists", "backdrop_tiles"):
        found = [u for k, u in usage.items() if want in k]
        assert len(found) == 1, (want, list(usage))
        kern[want] = found[0]
        print(f"{want}: {found[0]}")
    assert len(usage) == 2, list(usage)
    for k, u in kern.items():
        assert u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (k, u)      # two workgroups of four waves a SIMD pair at the least
        assert u["Occupancy"] >= 2, (k, u)
    assert kern["backdrop_tiles"]["LDS"] == 0                     # the records come at wave-uniform addresses, not through LDS
    assert kern["backdrop_lists"]["LDS"] <= 64                    # the waves' counts and the running base


# ---- 3. known answers of the rule, from its statement alone ---------------------------------------------------------------------
CLEAR = np.asarray([0.25, 0.5, 0.75, 1.0], f32)
RED, HALF = np.asarray([1.0, 0.0, 0.0, 1.0], f32), np.asarray([0.0, 1.0, 0.0, 0.5], f32)


def blank(W=8, H=8):
    return np.broadcast_to(CLEAR, (H, W, 4)).copy()


def host_mesh(img, tri, rgba, **kw):
    return P.backdrop_draw_mesh(img, np.asarray(tri, f32).reshape(-1, 3, 2), np.asarray(rgba, f32).reshape(-1, 4), viewport_height=8.0, **kw)


def model_mesh(img, tri, rgba, **kw):
    return M.draw_mesh(img, np.asarray(tri, f32).reshape(-1, 3, 2), np.asarray(rgba, f32).reshape(-1, 4), viewport_height=8.0, **kw)


def quad(x0, y0, x1, y1):
    """the two triangles (2, 1, 0), (2, 0, 3) of the rectangle's corners taken counter-clockwise from (x1, y0)"""
    v = [(x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return [[v[2], v[1], v[0]], [v[2], v[0], v[3]]]


def once(img, colour):
    """the pixels that hold `colour` blended exactly once over CLEAR, and those that hold CLEAR"""
    k = f32(1.0) - colour[3]
    want = np.asarray([colour[c] * colour[3] + CLEAR[c] * k for c in range(3)] + [colour[3] + CLEAR[3] * k], f32)
    hit, clear = (img == want).all(-1), (img == CLEAR).all(-1)
    assert (hit | clear).all(), "a pixel is neither untouched nor blended exactly once"
    return hit


@pytest.mark.parametrize("draw", [host_mesh, model_mesh], ids=["host", "model"])
def test_rule_known_answers(draw):
    """8 x 8 pixels over 8 world units: the centres are at +-0.5, +-1.5, +-2.5, +-3.5; column i is x = i - 3.5, row j is y = 3.5 - j"""
    # an axis-aligned square between centres covers the centres strictly inside: x in (-2, 1) and y in (-1, 3)
    hit = once(draw(blank(), quad(-2.0, -1.0, 1.0, 3.0), [HALF, HALF]), HALF)
    want = np.zeros((8, 8), bool)
    want[1:5, 2:5] = True                                              # rows y = 2.5 .. -0.5, columns x = -1.5 .. 0.5
    assert np.array_equal(hit, want) and hit.sum() == 12
    # a square whose edges and whose diagonal — (-2.5, 2.5) - (2.5, -2.5), the corners 2 and 0 both triangles share — run through
    # centres, with alpha 0.5: every covered pixel is blended exactly once, the diagonal's (array entries [j][j]) too
    sq = quad(-2.5, -2.5, 2.5, 2.5)
    hit = once(draw(blank(), sq, [HALF, HALF]), HALF)
    assert all(hit[j, j] for j in range(2, 7))
    # both windings, and either order of the two triangles, give the same image
    ref = draw(blank(), sq, [HALF, HALF])
    flipped = [[t[0], t[2], t[1]] for t in sq]
    same(draw(blank(), flipped, [HALF, HALF]), ref, "winding")
    same(draw(blank(), sq[::-1], [HALF, HALF]), ref, "order")
    # an edge on a line of centres goes to one side only: the square's edges at x = +-2.5 and y = +-2.5.  A triangle's sign for an
    # edge is positive when its third vertex lies to the left of lo -> hi; lo -> hi runs upwards on a vertical edge and to the
    # right on a horizontal one, so the centres on the right and bottom edges belong to the square, those on the left and top do not
    assert hit[2:7, 6].all() and hit[6, 2:7].all() and not hit[:, 1].any() and not hit[1, :].any()
    assert hit[2:7, 2:7].all() and hit.sum() == 25
    # two squares side by side share the line x = 0.5, which runs through centres: every centre on it is covered exactly once
    pair = quad(-1.5, -1.5, 0.5, 1.5) + quad(0.5, -1.5, 2.5, 1.5)
    hit = once(draw(blank(), pair, [HALF] * 4), HALF)
    assert hit[:, 4].sum() == 3 and hit.sum() == 4 * 3
    # a 12-triangle fan centred on a pixel centre covers it, and every other pixel of the disc, exactly once
    c = np.asarray([0.5, -0.5], np.float64)
    ring = [c + 2.2 * np.asarray([math.cos(i * math.tau / 12), math.sin(i * math.tau / 12)]) for i in range(12)]
    fan = [[c, ring[i], ring[(i + 1) % 12]] for i in range(12)]
    hit = once(draw(blank(), fan, [HALF] * 12), HALF)
    assert hit[4, 4] and hit.sum() >= 12
    ys, xs = np.nonzero(hit)
    assert np.all(np.hypot(xs - 3.5 - 0.5, 3.5 - ys + 0.5) <= 2.2 + 1e-6)
    inner = np.hypot(np.arange(8)[None, :] - 3.5 - 0.5, 3.5 - np.arange(8)[:, None] + 0.5) <= 2.2 * math.cos(math.pi / 12) - 1e-6
    assert hit[inner].all()
    # triangles that draw nothing: zero area, a repeated vertex, NaN and Inf vertices, a non-finite colour, wholly off the image
    big = [(-3.9, -3.9), (3.9, -3.9), (0.0, 3.9)]
    nothing = [([(-3.0, -3.0), (0.0, 0.0), (3.0, 3.0)], RED), ([(1.0, 1.0), (1.0, 1.0), (2.0, 3.0)], RED),
               ([(math.nan, -3.9), (3.9, -3.9), (0.0, 3.9)], RED), ([(-3.9, -3.9), (math.inf, -3.9), (0.0, 3.9)], RED),
               ([(-3.9, -3.9), (3.9, -math.inf), (0.0, 3.9)], RED), (big, [1.0, math.nan, 0.0, 1.0]), (big, [1.0, 0.0, 0.0, math.inf]),
               ([(4.2, -3.0), (9.0, -3.0), (6.0, 3.0)], RED), ([(-3.0, 4.01), (3.0, 4.01), (0.0, 40.0)], RED),
               ([(-3.0e30, -1.0e30), (-2.0e30, -1.0e30), (-2.5e30, -3.0e30)], RED)]
    for tri, col in nothing:
        same(draw(blank(), [tri], [col]), blank(), tri)
    assert once(draw(blank(), [big], [RED]), RED).sum() > 20
    same(draw(blank(), [t for t, _ in nothing[:2]] + [big], [RED] * 3), draw(blank(), [big], [RED]), "degenerate beside a real one")
    # a transform with sy = -1 mirrors, and a translation moves by whole pixels
    tri = [(-2.2, 0.3), (1.7, 0.9), (0.4, 3.3)]
    up = draw(blank(), [tri], [RED])
    same(draw(blank(), [tri], [RED], transform=(0.0, 0.0, 1.0, -1.0)), up[::-1], "mirror")
    same(draw(blank(), [tri], [RED], transform=(1.0, -2.0, 1.0, 1.0))[2:, 1:], up[:-2, :-1], "shift")
    assert once(up, RED).sum() >= 3


def test_rule_host_matches_model_on_random_meshes():
    """slivers, needles, triangles far larger than the image and vertices on pixel centres, alpha 0.5 — so a pixel covered twice or
    not at all by one face alone would show"""
    rng = np.random.default_rng(5)
    for W, H, vh in ((8, 8, 8.0), (13, 7, 3.0), (33, 17, 50.0)):
        s = vh / H
        tri = (rng.random((160, 3, 2)) - 0.5) * [W * s * 1.6, vh * 1.6]
        tri[:40] = np.round(tri[:40] / s - 0.5) * s + 0.5 * s * (np.asarray([W, H]) % 2 == 0)      # on pixel centres
        tri[40:60, 2] = tri[40:60, 0] + (tri[40:60, 1] - tri[40:60, 0]) * 0.5 + rng.normal(size=(20, 2)) * 1e-4   # slivers
        tri[60:70] *= 400.0
        col = rng.random((160, 4))
        col[:, 3] = 0.5
        bg = rng.random((H, W, 4)).astype(f32)
        t = (0.3 * s, -0.2 * s, 1.25, -0.75)
        for kw in ({}, {"transform": t}):
            got = P.backdrop_draw_mesh(bg, tri.astype(f32), col.astype(f32), viewport_height=vh, **kw)
            want = M.draw_mesh(bg, tri.astype(f32), col.astype(f32), viewport_height=vh, **kw)
            same(got, want, (W, H, kw))
            assert not np.array_equal(got, bg)


# ---- 4. static geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("octaves", [1, 2, 3, 7])
def test_static_geometry(octaves):
    want = {M.NET_RAYS: 12, M.NET_SPIRAL: 72 * octaves - 1, M.BASS: min(72 * octaves, 168) - 1}
    assert M.counts(octaves) == want
    for what, n in want.items():
        got = P.backdrop_geometry(octaves, what)
        assert got.shape == (n, 4, 2)
        same(got, M.geometry(octaves, what), (octaves, what))
        assert np.isfinite(got).all()
    # the bass rectangle: 0.05 wide, |p - q| + 0.01 long, centred on the segment's midpoint (to a few ulp)
    b = P.backdrop_geometry(octaves, M.BASS).astype(np.float64)
    s = P.backdrop_geometry(octaves, M.NET_SPIRAL).astype(np.float64)[:len(b)]
    p, q = (s[:, 0] + s[:, 1]) / 2, (s[:, 2] + s[:, 3]) / 2                     # the thick-line quad's ends are p and q
    assert np.allclose(np.linalg.norm(b[:, 0] - b[:, 1], axis=1), 0.05, atol=1e-6)
    assert np.allclose(np.linalg.norm(b[:, 1] - b[:, 2], axis=1), np.linalg.norm(p - q, axis=1) + 0.01, atol=1e-5)
    assert np.allclose(b.mean(1), (p + q) / 2, atol=1e-5)
    r = P.backdrop_geometry(octaves, M.NET_RAYS).astype(np.float64)
    assert np.allclose(np.linalg.norm((r[:, 2] + r[:, 3]) / 2, axis=1), octaves * 2.2, atol=1e-5)


def test_panel_transforms():
    for n, W, H, vh in ((252, 1280, 720, 0.0), (36, 33, 17, 22.0), (1024, 1, 1, 3.0)):
        got = P.panel_transforms(n, W, H, vh)
        same(got, M.panel_transforms(n, W, H, vh), (n, W, H, vh))
    t = P.panel_transforms(252, 1280, 720).astype(np.float64)
    half = 38.0 * 0.41421357 / 2
    assert np.allclose(t[0], [half * 1280 / 720 - 252 * 0.011 - 0.2, half - 4.2, 1, 1], atol=1e-5)
    assert np.array_equal(t[1], t[0] * [1, 1, 1, -1]) and np.array_equal(t[2], [-5.0, -6.5, 3.0, 1.0])


# ---- 5. backdrop_frame against the model ----------------------------------------------------------------------------------------
_cases = {}


def host_case(W, H, top="spectrum"):
    if (W, H, top) not in _cases:
        _cases[(W, H, top)] = BC.host_case(W, H, top=top)
    return _cases[(W, H, top)]


@pytest.mark.parametrize("case", BC.frame_cases(), ids=lambda c: "%dx%d-mode%d-lit%d-%s-%s" % (c[0], c[1], c[2], c[3], "panels" if c[4] else "bare",
                                                                                                "bg" if c[5] else "clear"))
def test_frames_match_model(case):
    W, H, mode, lit, with_panels, with_bg = case
    # one pixel holds one opaque panel at most: the 1 x 1 cases take turns in which panel lies on it (backdrop_cases.transforms)
    top = "spectrum" if (W, H) != (1, 1) or mode == 0 else ("graph" if lit == 1 else "hist")
    vh, panels = host_case(W, H, top)
    bg = np.random.default_rng(4).uniform(0.0, 2.0, (H, W, 4)).astype(f32) if with_bg else None
    kw = dict(viewport_height=vh, bass_lit=lit, bass_rgba=BC.BASS_RGBA, panels=panels if with_panels else None, background=bg)
    want = M.frame(BC.OCTAVES, BC.BPO, W, H, mode=mode, **kw)
    same(P.backdrop_frame(BC.OCTAVES, BC.BPO, W, H, visuals_mode=mode, **kw), want, case)
    # every layer the case names changes at least one pixel against the same frame without it; in Galaxy mode net and bass are absent.
    # On 1 x 1 the only centre is the origin, which no bass segment (radius >= 0.6) reaches: that size can name no bass layer, and
    # of the panels it names the one that lies on the pixel.
    on_pixel = {"spectrum": ["line", "disc"], "graph": ["graph"], "hist": ["hist"]}[top]
    named = (["net"] if mode == 0 else []) + ((on_pixel if (W, H) == (1, 1) else ["line", "disc", "graph", "hist"]) if with_panels else [])
    named += ["bass"] if mode == 0 and lit and (W, H) != (1, 1) else []
    for layer in M.LAYERS:
        without = M.frame(BC.OCTAVES, BC.BPO, W, H, mode=mode, skip=(layer,), **kw)
        assert np.array_equal(without, want) != (layer in named), (case, layer)


# ---- 6. the balls over the backdrop ---------------------------------------------------------------------------------------------
def test_balls_over_backdrop_match_model():
    W, H = 33, 17
    vh, panels = host_case(W, H)
    n = BC.OCTAVES * BC.BPO
    r = RC.row(n, 31, spread=0.4 * vh)
    r["ball_xyzs"][:, 3] *= f32(vh / 16.0)                          # balls sized for the narrowed view
    t = np.random.default_rng(3).uniform(0.0, 20.0, n).astype(f32)
    balls = (r["ball_xyzs"], r["ball_rgba"], r["ball_params"], r["ball_visible"], t)
    kw = dict(viewport_height=vh, bass_lit=40, bass_rgba=BC.BASS_RGBA, panels=panels)
    back = P.backdrop_frame(BC.OCTAVES, BC.BPO, W, H, **kw)
    got = P.raster_frame(W, H, *balls, viewport_height=vh, background=back)
    cov = []
    want = RM.frame(W, H, *balls, viewport_height=vh, background=M.frame(BC.OCTAVES, BC.BPO, W, H, **kw), coverage=cov)
    same(got, want, "full composition")
    assert cov[0] > 0 and not np.array_equal(got, back)
    assert not np.array_equal(got, P.raster_frame(W, H, *balls, viewport_height=vh))
