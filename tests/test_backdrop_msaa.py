"""The multisampled backdrop (pvq_msaa_*: four samples a pixel, resolved at the end of the stage) as far as it goes without a GPU: the
symbols, the refusals, what the compiler made of the kernel, known answers worked from the statement of the rule alone, and the host
face against tests/backdrop_msaa_model.py.

The bar is tests/test_backdrop.py's: no differing bit in any pixel channel.  The model keeps [4][H][W][4], uses no pixel boxes and
tries every triangle on every sample, so it also checks that the one-sample rule's boxes lose no pixel that has a covered sample."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_cases as BC
import backdrop_model as M
import backdrop_msaa_model as MM
import pitchvis_amd as P
import raster_model as RM
from pitchvis_amd import _lib
from pitchvis_amd import backdrop as PB
from pitchvis_amd.consumers import _f
from test_backdrop import CLEAR, HALF, HIPCC, NAMES, RED, ROOT, bits, blank, quad, same

f32 = np.float32
MSAA_NAMES = ["pvq_msaa_batch_create", "pvq_msaa_batch_samples", "pvq_msaa_draw_mesh", "pvq_msaa_frame", "pvq_msaa_sample_positions"]
REFUSED = (0, 2, 3, 5, 8)


# ---- 1. symbols and refusals -------------------------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    assert sorted(set(re.findall(r"\b(pvq_backdrop_\w+)\s*\(", hdr))) == NAMES              # the backdrop's own set is unchanged
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(pvq_msaa_\w+)\s*\(", bare))) == MSAA_NAMES
    for name in MSAA_NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.msaa_sample_positions is PB.msaa_sample_positions
    b = P.BackdropBatch(P.VqtRange(55.0, 7, 36), 2, 64, 48, device=None)
    assert b.samples == 1 and L.pvq_msaa_batch_samples(b._h) == 1
    assert L.pvq_msaa_batch_samples(None) == 0


def test_sample_positions():
    want = np.asarray([[0.375, 0.125], [0.875, 0.375], [0.125, 0.625], [0.625, 0.875]], f32)
    same(P.msaa_sample_positions(4), want, "four samples")
    same(P.msaa_sample_positions(1), np.asarray([[0.5, 0.5]], f32), "one sample")
    same(np.asarray(MM.POSITIONS[4], f32), want, "the model's")
    assert np.abs(want - 0.5).max() == 0.375                       # what the pixel boxes rely on


def test_refusals_and_host_only_handle():
    L = _lib.load()
    buf = np.zeros(4096, f32)
    fp, p = _f(buf), buf.ctypes.data
    h = C.c_void_p()
    for s in REFUSED:
        calls = {"positions": L.pvq_msaa_sample_positions(s, fp),
                 "draw mesh": L.pvq_msaa_draw_mesh(s, 8, 8, 8.0, 0, None, None, None, fp),
                 "frame": L.pvq_msaa_frame(s, 2, 12, 8, 8, 0.0, 0, 0, None, None, None, fp)}
        for dev in (-1, 0):                                           # refused before any device is touched
            calls[f"create on {dev}"] = L.pvq_msaa_batch_create(s, dev, 7, 36, 0, 0.0, 2, 64, 48, C.byref(h))
            assert not h.value
        for who, st in calls.items():
            assert st == _lib.PVQ_ERR_INVALID_ARG, (s, who, st)
        assert "1 or 4" in L.pvq_last_error().decode(), s
        with pytest.raises(ValueError):
            P.backdrop_draw_mesh(blank(), np.zeros((0, 3, 2), f32), np.zeros((0, 4), f32), samples=s)
        with pytest.raises(ValueError):
            P.backdrop_frame(2, 12, 8, 8, samples=s)
        with pytest.raises(ValueError):
            P.BackdropBatch(P.VqtRange(55.0, 7, 36), 2, 64, 48, device=None, samples=s)
        with pytest.raises(ValueError):
            P.msaa_sample_positions(s)
    # the other checks are the one-sample faces'
    assert L.pvq_msaa_sample_positions(4, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_draw_mesh(4, 8, 8, 8.0, 1, None, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_draw_mesh(4, 8, 4097, 8.0, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_draw_mesh(4, 8, 8, 8.0, 0, None, None, None, fp) == _lib.PVQ_OK
    assert L.pvq_msaa_frame(4, 2, 12, 8, 8, 0.0, 0, 1, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_frame(4, 2, 12, 8, 8, 0.0, 4, 0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_frame(4, 2, 12, 8, 8, 0.0, 0, 0, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_batch_create(4, -1, 7, 36, 0, 0.0, 2, 64, 48, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_msaa_batch_create(4, -1, 25, 41, 0, 0.0, 2, 64, 48, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
    assert L.pvq_msaa_batch_create(4, -1, 7, 36, 0, 0.0, 2, 4097, 48, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    # a host-only handle made with four samples reports four and answers the frames call as a one-sample one does
    b = P.BackdropBatch(P.VqtRange(55.0, 7, 36), 3, 64, 48, device=None, samples=4)
    assert b.samples == 4 and L.pvq_msaa_batch_samples(b._h) == 4
    call = L.pvq_backdrop_batch_frames_device
    assert call(b._h, 1, None, p, None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
    assert call(b._h, 1, None, None, None) == _lib.PVQ_ERR_INVALID_ARG                  # its argument checks come first
    assert call(b._h, 1, None, p + 8, None) == _lib.PVQ_ERR_INVALID_ARG
    half = _lib.CBackdropInputs()
    half.line_pos = p
    assert call(b._h, 1, C.byref(half), p, None) == _lib.PVQ_ERR_INVALID_ARG
    with pytest.raises(P.PvqError) as e:
        b.frames(1, bass_lit=p, bass_rgba=p, image=p)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    one = C.c_void_p()
    assert L.pvq_msaa_batch_create(1, -1, 7, 36, 0, 0.0, 3, 64, 48, C.byref(one)) == _lib.PVQ_OK and one.value
    assert L.pvq_msaa_batch_samples(one) == 1
    L.pvq_backdrop_batch_destroy(one)


# ---- 2. kernel resources -----------------------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """the unit holds one kernel, within the budget the one-sample tile kernel is held to"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "backdrop_msaa.hip")
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
    print(usage)
    assert len(usage) == 1 and "backdrop_tiles_msaa" in next(iter(usage)), list(usage)
    u = next(iter(usage.values()))
    assert u["ScratchSize"] == 0 and u["LDS"] == 0, u
    assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, u
    assert u["Occupancy"] >= 2, u


# ---- 3. known answers of the rule, from its statement alone ------------------------------------------------------------------------
def host_mesh(img, tri, rgba, **kw):
    return P.backdrop_draw_mesh(img, np.asarray(tri, f32).reshape(-1, 3, 2), np.asarray(rgba, f32).reshape(-1, 4), viewport_height=8.0, samples=4, **kw)


def model_mesh(img, tri, rgba, **kw):
    return MM.draw_mesh(img, np.asarray(tri, f32).reshape(-1, 3, 2), np.asarray(rgba, f32).reshape(-1, 4), viewport_height=8.0, samples=4, **kw)


def over_clear(colour):
    """`colour` blended once over CLEAR, by the blend's formula in f32"""
    colour = np.asarray(colour, f32)
    k = f32(1.0) - colour[3]
    return np.asarray([colour[c] * colour[3] + CLEAR[c] * k for c in range(3)] + [colour[3] + CLEAR[3] * k], f32)


def resolved(covered, colour=RED):
    """a pixel over CLEAR whose samples listed in `covered` hold `colour` blended once: the resolve formula in f32"""
    s = [over_clear(colour) if k in covered else CLEAR for k in range(4)]
    return ((s[0] + s[1]) + (s[2] + s[3])) * f32(0.25)


FX, FY = (0.375, 0.875, 0.125, 0.625), (0.125, 0.375, 0.625, 0.875)


def expected(inside, colour=RED):
    """the 8 x 8 picture over 8 world units in which sample k of pixel (i, j), at x = i - 4 + FX[k], y = 4 - j - FY[k], is covered
    where inside(x, y)"""
    out = np.empty((8, 8, 4), f32)
    for j in range(8):
        for i in range(8):
            out[j, i] = resolved({k for k in range(4) if inside(i - 4 + FX[k], 4 - j - FY[k])}, colour)
    return out


@pytest.mark.parametrize("draw", [host_mesh, model_mesh], ids=["host", "model"])
def test_rule_known_answers(draw):
    """8 x 8 pixels over 8 world units, s = 1: column i spans x in [i - 4, i - 3], row j spans y in [3 - j, 4 - j], and every sample
    sits on a multiple of 1 / 8.  Opaque red over the clear colour."""
    c = -2.0                                                          # column 2 starts here; rows 2 .. 5 span y in [-2, 2]
    for offset, covered in ((0.5, {1, 3}), (0.25, {0, 1, 3}), (0.75, {1})):
        # a rectangle whose left edge lies inside column 2 and whose other edges lie on pixel borders, where no sample is
        img = draw(blank(), quad(c + offset, -2.0, 1.0, 2.0), [RED, RED])
        same(img, expected(lambda x, y: c + offset < x < 1.0 and -2.0 < y < 2.0), ("left edge at", offset))
        same(img[3, 2], resolved(covered), ("the edge's column", offset))
        assert len(covered) == {0.5: 2, 0.25: 3, 0.75: 1}[offset]
        same(img[3, 3], over_clear(RED), "a pixel inside")
        same(img[3, 1], CLEAR, "a pixel outside")
        same(img[1, 3], CLEAR, "a row above")
    # an edge exactly through sample 2 (x = c + 0.125): lo -> hi runs upwards on a vertical edge, the rectangle on its right has a
    # negative sign for it and loses the tie, the rectangle on its left has a positive sign and wins it
    right_of = draw(blank(), quad(c + 0.125, -2.0, 1.0, 2.0), [RED, RED])
    same(right_of, expected(lambda x, y: c + 0.125 < x < 1.0 and -2.0 < y < 2.0), "tie, rectangle on the right")
    same(right_of[3, 2], resolved({0, 1, 3}), "three samples")
    left_of = draw(blank(), quad(-3.0, -2.0, c + 0.125, 2.0), [RED, RED])
    same(left_of, expected(lambda x, y: -3.0 < x <= c + 0.125 and -2.0 < y < 2.0), "tie, rectangle on the left")
    same(left_of[3, 2], resolved({2}), "one sample")
    # ... and through sample 0 of row 3 (y = 4 - 3 - 0.125): lo -> hi runs to the right on a horizontal edge, so the rectangle above
    # it wins the tie and the one below it loses it
    y0 = 4.0 - 3.0 - 0.125
    above = draw(blank(), quad(-2.0, y0, 1.0, 3.0), [RED, RED])
    same(above, expected(lambda x, y: -2.0 < x < 1.0 and y0 <= y < 3.0), "tie, rectangle above")
    same(above[3, 3], resolved({0}), "one sample")
    below = draw(blank(), quad(-2.0, -2.0, 1.0, y0), [RED, RED])
    same(below, expected(lambda x, y: -2.0 < x < 1.0 and -2.0 < y < y0), "tie, rectangle below")
    same(below[3, 3], resolved({1, 2, 3}), "three samples")
    # the two together share that edge: every sample of the union is covered once
    both = draw(blank(), quad(-2.0, y0, 1.0, 3.0) + quad(-2.0, -2.0, 1.0, y0), [HALF] * 4)
    same(both, expected(lambda x, y: -2.0 < x < 1.0 and -2.0 < y < 3.0, HALF), "shared horizontal edge")
    # two alpha-0.5 triangles that share the diagonal x + y = 0.25, which runs through sample 0 of every pixel (j, j): every sample
    # of the square is blended exactly once — a pixel inside holds the once-blended value, none the twice-blended one or the clear colour
    sq = quad(-2.0, -2.0, 2.25, 2.25)
    assert sq[0][0] == (-2.0, 2.25) and sq[0][2] == (2.25, -2.0)      # the shared corners 2 and 0: the diagonal's ends
    assert all((j - 4 + FX[0]) + (4 - j - FY[0]) == 0.25 for j in range(8))
    img = draw(blank(), sq, [HALF, HALF])
    same(img, expected(lambda x, y: -2.0 < x < 2.25 and -2.0 < y < 2.25, HALF), "shared diagonal")
    once = over_clear(HALF)
    twice = over_clear(HALF) * f32(0.5) + np.asarray([0.0, 0.5, 0.0, 0.5], f32)
    assert not np.array_equal(once, twice)
    for j in range(2, 6):
        for i in range(2, 6):
            same(img[j, i], once, ("inside the union", i, j))
    assert not (img == twice).all(-1).any()
    flipped = [[t[0], t[2], t[1]] for t in sq]
    same(draw(blank(), flipped, [HALF, HALF]), img, "winding")
    same(draw(blank(), sq[::-1], [HALF, HALF]), img, "order")
    # a triangle thinner than the sample spacing: around a pixel centre it hits no sample and draws nothing (the one-sample rule
    # would colour the pixel); around sample 3 of pixel (3, 3) it moves that pixel by exactly a quarter
    def tiny(x, y):
        return [[(x - 0.05, y - 0.04), (x + 0.05, y - 0.04), (x, y + 0.06)]]
    same(draw(blank(), tiny(-0.5, 0.5), [RED]), blank(), "between the samples")
    assert not np.array_equal(P.backdrop_draw_mesh(blank(), np.asarray(tiny(-0.5, 0.5), f32), RED[None], viewport_height=8.0), blank())
    img = draw(blank(), tiny(3 - 4 + FX[3], 4 - 3 - FY[3]), [RED])
    want = blank()
    want[3, 3] = resolved({3})
    same(img, want, "one sample")
    same(img[3, 3] - CLEAR, (over_clear(RED) - CLEAR) * f32(0.25), "a quarter of the way")        # exact: every value is a multiple of 1 / 16
    # what draws nothing with one sample draws nothing with four
    big = [(-3.9, -3.9), (3.9, -3.9), (0.0, 3.9)]
    for tri, col in (([(-3.0, -3.0), (0.0, 0.0), (3.0, 3.0)], RED), ([(math.nan, -3.9), (3.9, -3.9), (0.0, 3.9)], RED),
                     ([(-3.9, -3.9), (math.inf, -3.9), (0.0, 3.9)], RED), (big, [1.0, math.nan, 0.0, 1.0]), (big, [1.0, 0.0, 0.0, math.inf]),
                     ([(4.2, -3.0), (9.0, -3.0), (6.0, 3.0)], RED), ([(-3.0e30, -1.0e30), (-2.0e30, -1.0e30), (-2.5e30, -3.0e30)], RED)):
        same(draw(blank(), [tri], [col]), blank(), tri)
    # an image_inout that is not constant: every sample starts from its own pixel, and an untouched pixel comes back bit for bit
    bg = np.random.default_rng(2).uniform(0.0, 2.0, (8, 8, 4)).astype(f32)
    img = draw(bg, quad(c + 0.5, -2.0, 1.0, 2.0), [RED, RED])
    same(img[0], bg[0], "untouched row")
    same(img[3, 3], RED, "opaque over anything")
    same(img[3, 2], ((bg[3, 2] + RED) + (bg[3, 2] + RED)) * f32(0.25), "two of four")


# ---- 4. the host face against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", BC.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_matches_model_on_random_meshes(size):
    """slivers, needles, vertices on sample positions and far off the image, a NaN vertex, a non-finite colour, zero-area triangles,
    both windings, alpha 0.5 — so a sample covered twice or not at all by one face alone would show"""
    W, H = size
    vh = BC.view(W, H)
    rng = np.random.default_rng(50 + W)
    s = vh / H
    tri = (rng.random((160, 3, 2)) - 0.5) * [W * s * 1.6, vh * 1.6]
    tri[:40] = np.round(tri[:40] / s * 8.0) * s / 8.0                                             # on the samples' grid of eighths
    tri[40:60, 2] = tri[40:60, 0] + (tri[40:60, 1] - tri[40:60, 0]) * 0.5 + rng.normal(size=(20, 2)) * 1e-4 * s   # slivers
    tri[60:70] *= 400.0                                                                           # far off the image
    tri[70:80, 2] = tri[70:80, 0] + (tri[70:80, 1] - tri[70:80, 0]) * 0.25                        # zero area (or nearly: f32)
    tri[80:120] = tri[80:120, [0, 2, 1]]                                                          # the other winding
    tri[120, 1, 0] = math.nan
    tri[121, 2, 1] = math.inf
    col = rng.random((160, 4))
    col[:, 3] = 0.5
    col[122, 1], col[123, 3] = math.inf, math.nan
    bg = rng.random((H, W, 4)).astype(f32)
    t = (0.3 * s, -0.2 * s, 1.25, -0.75)
    for kw in ({}, {"transform": t}):
        got = P.backdrop_draw_mesh(bg, tri.astype(f32), col.astype(f32), viewport_height=vh, samples=4, **kw)
        want = MM.draw_mesh(bg, tri.astype(f32), col.astype(f32), viewport_height=vh, **kw)
        print(f"{W} x {H} {kw and 'transformed'}: {int((bits(got) != bits(want)).sum())} of {got.size} channels differ from the model")
        same(got, want, (W, H, kw))
        assert not np.array_equal(got, bg) and np.isfinite(got).all()
        one = P.backdrop_draw_mesh(bg, tri.astype(f32), col.astype(f32), viewport_height=vh, **kw)
        assert W * H == 1 or not np.array_equal(got, one)


_cases = {}


def host_case(W, H, top="spectrum"):
    if (W, H, top) not in _cases:
        _cases[(W, H, top)] = BC.host_case(W, H, top=top)
    return _cases[(W, H, top)]


def case_kw(case):
    W, H, mode, lit, with_panels, with_bg = case
    top = "spectrum" if (W, H) != (1, 1) or mode == 0 else ("graph" if lit == 1 else "hist")
    vh, panels = host_case(W, H, top)
    bg = np.random.default_rng(4).uniform(0.0, 2.0, (H, W, 4)).astype(f32) if with_bg else None
    return dict(viewport_height=vh, bass_lit=lit, bass_rgba=BC.BASS_RGBA, panels=panels if with_panels else None, background=bg)


@pytest.mark.parametrize("case", BC.frame_cases(), ids=lambda c: "%dx%d-mode%d-lit%d-%s-%s" % (c[0], c[1], c[2], c[3], "panels" if c[4] else "bare",
                                                                                                "bg" if c[5] else "clear"))
def test_frames_match_model_and_the_one_sample_picture(case):
    """backdrop_frame(samples=4) equals the model bit for bit — both modes, with and without a background — and every pixel where the
    model finds the four samples and the centre covered alike by every triangle holds the one-sample picture's bits"""
    W, H, mode = case[:3]
    kw = case_kw(case)
    alike = np.ones((H, W), bool)
    want = MM.frame(BC.OCTAVES, BC.BPO, W, H, mode=mode, alike=alike, **kw)
    got = P.backdrop_frame(BC.OCTAVES, BC.BPO, W, H, visuals_mode=mode, samples=4, **kw)
    one = P.backdrop_frame(BC.OCTAVES, BC.BPO, W, H, visuals_mode=mode, **kw)
    start = kw["background"] if kw["background"] is not None else np.broadcast_to(RM.clear_color(mode), (H, W, 4))   # layer 0
    draws = not np.array_equal(bits(one), bits(start))
    differ = (bits(got) != bits(one)).any(-1)
    print(f"{case}: {int((bits(got) != bits(want)).sum())} of {got.size} channels differ from the model; {int((~alike).sum())} of {W * H} pixels "
          f"have a sample covered otherwise than the centre, {int(differ.sum())} differ from the one-sample picture")
    same(got, want, case)
    same(got[alike], one[alike], (case, "pixels whose samples agree"))
    assert (int((~alike).sum()) > 0) == draws, (case, draws)
    assert not differ[alike].any()
    if draws and W * H > 1:
        assert differ.any(), case


# ---- 5. one sample through the new entry points -----------------------------------------------------------------------------------
def test_one_sample_through_the_new_entry_points():
    L = _lib.load()
    rng = np.random.default_rng(9)
    for W, H in BC.SIZES[:3]:
        vh = BC.view(W, H)
        s = vh / H
        tri = ((rng.random((60, 3, 2)) - 0.5) * [W * s * 1.6, vh * 1.6]).astype(f32)
        col = rng.random((60, 4)).astype(f32)
        bg = rng.random((H, W, 4)).astype(f32)
        old = P.backdrop_draw_mesh(bg, tri, col, viewport_height=vh)
        new = bg.copy()
        assert L.pvq_msaa_draw_mesh(1, W, H, vh, len(tri), _f(tri), _f(col), None, _f(new)) == _lib.PVQ_OK
        same(new, old, ("draw mesh", W, H))
        assert not np.array_equal(old, bg)
    for case in [c for c in BC.frame_cases() if (c[0], c[1]) != (128, 96)]:
        W, H, mode, lit = case[:4]
        kw = case_kw(case)
        old = P.backdrop_frame(BC.OCTAVES, BC.BPO, W, H, visuals_mode=mode, **kw)
        keep = []
        o = PB._host_panels(BC.OCTAVES * BC.BPO, kw["panels"], keep) if kw["panels"] is not None else None
        new = np.empty((H, W, 4), f32)
        st = L.pvq_msaa_frame(1, BC.OCTAVES, BC.BPO, W, H, kw["viewport_height"], mode, lit, _f(BC.BASS_RGBA), C.byref(o) if o is not None else None,
                              _f(kw["background"]) if kw["background"] is not None else None, _f(new))
        assert st == _lib.PVQ_OK, case
        same(new, old, ("frame", case))
