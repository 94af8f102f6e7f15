"""The text stage (pvq_text_*: the pitch-name labels from font outlines, over the balls and under the overlay) as far as it goes
without a GPU: the symbols, the argument checks and the host-only handle, what the compiler made of the kernels, known answers of
the coverage and layout rules worked from their statement alone, the TrueType reader against fontTools, and the host face against
tests/text_model.py (float64, curves flattened to 1e-4 pixel, coverage by accumulation).

The bar of the host face against the model.  The library flattens to tol = 1 / 64 pixel, the model to 1e-4; an edge through a
pixel then errs by about tol * sqrt 2 in coverage, so the design fails above 2 sqrt 2 tol = 0.0442.  Seen on the crafted cases
(the twelve labels at 64 x 64, 256 x 256 and 301 x 173, views 15.74 and 40, and one em of 200 pixels): 0.01732 (the em of 200 pixels; 0.0126 among the
twelve labels); the bar is twice that, COVERAGE_BAR = 0.03464.  An image channel may differ by 1e-6 plus that bar times the colour."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pitchvis_amd as P
import text_cases as TC
import text_model as M
from pitchvis_amd import _lib
from pitchvis_amd import text as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32
COVERAGE_SEEN = 0.01732
COVERAGE_BAR = 2.0 * COVERAGE_SEEN
NAMES = ["pvq_text_batch_create", "pvq_text_batch_destroy", "pvq_text_batch_get_coverage", "pvq_text_batch_rows_device", "pvq_text_font_destroy",
         "pvq_text_font_from_outlines", "pvq_text_font_from_ttf", "pvq_text_font_glyph", "pvq_text_font_metrics", "pvq_text_frame",
         "pvq_text_layout_query", "pvq_text_pitch_labels"]


@pytest.fixture(scope="module")
def syn():
    return TC.font_of(TC.SYNTHETIC)


@pytest.fixture(scope="module")
def dejavu():
    fx = TC.fixture()
    return fx, TC.font_of(fx)


def cov_of(font, text, W, H, x=0.0, y=0.0):
    """coverage [H][W] of a one-label picture in the synthetic fonts' frame: a font unit is a pixel"""
    return PT.text_frame(font, [TC.unit_label(text, x, y)], width=W, height=H, viewport_height=float(H), coverage=True)[0]


# ---- 1. symbols and arguments ---------------------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(pvq_text_\w+)\s*\(", hdr))) == NAMES
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.TextFont is PT.TextFont and P.TextBatch is PT.TextBatch and P.text_frame is PT.text_frame
    assert P.text_layout is PT.text_layout and P.pitch_name_labels is PT.pitch_name_labels
    assert C.sizeof(_lib.CTextLabel) == 64 and C.sizeof(_lib.CTextLayout) == 36


def test_left_out_lists_no_longer_name_the_text():
    for path in ("include/pvq.h", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, path)).read()
        for item in re.findall(r"Left out[^\n]*:.*?(?:\*/|\n\n)", text, flags=re.S):
            flat = " ".join(item.split())
            assert "needs a font" not in flat, (path, flat[:200])
            if "pitch-name text" in flat:
                assert "text stage" in flat, (path, flat[:200])


def _label(text=b"s", x=0.0, y=0.0, font_px=64.0, scale=1.0, rgb=(1.0, 1.0, 1.0)):
    lab = _lib.CTextLabel()
    lab.text, lab.x, lab.y, lab.font_px, lab.scale = text, x, y, font_px, scale
    lab.rgb[:] = rgb
    return lab


BAD_LABELS = [dict(text=b""), dict(text=b"sssssssss"), dict(text=b"\xff"), dict(text=b"\xe2\x99"), dict(text=b"\xc0\xaf"), dict(x=math.nan),
              dict(y=math.inf), dict(font_px=0.0), dict(font_px=-1.0), dict(font_px=math.nan), dict(scale=0.0), dict(scale=math.inf),
              dict(rgb=(1.5, 0.0, 0.0)), dict(rgb=(0.0, -0.1, 0.0)), dict(rgb=(0.0, 0.0, math.nan)), dict(font_px=1025.0), dict(text=b"x")]


def test_argument_ranges_and_host_only_handle(syn):
    L = _lib.load()
    buf = np.zeros(64 * 64 * 4, f32)
    p = buf.ctypes.data   # stands for device memory; a host-only handle never dereferences it
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    font = syn._h
    good = (_lib.CTextLabel * 1)(_label())
    # the font constructors
    h = C.c_void_p()
    assert L.pvq_text_font_from_ttf(None, 100, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    raw = np.zeros(100, np.uint8)
    rp = raw.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.pvq_text_font_from_ttf(rp, 11, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    assert L.pvq_text_font_from_ttf(rp, 100, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and "offset" in L.pvq_last_error().decode()
    assert L.pvq_text_font_from_ttf(rp, 100, None) == _lib.PVQ_ERR_INVALID_ARG
    raw[:4] = list(b"ttcf")
    assert L.pvq_text_font_from_ttf(rp, 100, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
    sq = TC.SYNTHETIC["glyphs"][ord("s")]
    for upem, asc, desc in ((15, 1.0, 0.0), (16385, 1.0, 0.0), (64, math.nan, 0.0), (64, 0.0, math.inf), (64, 1e6, 0.0)):
        with pytest.raises(ValueError):
            P.TextFont.from_outlines({"s": sq}, upem, asc, desc)
    for bad in ((1.0, [3], sq[2], [1, 1, 1]),                      # flags shorter than points
                (1.0, [4], sq[2], sq[3]),                            # a contour end past the points
                (1.0, [1, 1, 3], sq[2], sq[3]),                      # ends that do not ascend
                (1.0, [2], sq[2], sq[3]),                            # the last contour stops short
                (-1.0, [3], sq[2], sq[3]), (math.nan, [3], sq[2], sq[3]),
                (1.0, [3], np.asarray(sq[2]) * 1e6, sq[3]), (1.0, [3], np.full((4, 2), np.nan), sq[3])):
        with pytest.raises(ValueError):
            P.TextFont.from_outlines({"s": bad}, 64, 32.0, -32.0)
    with pytest.raises(ValueError):
        P.TextFont.from_outlines({}, 64, 32.0, -32.0)
    with pytest.raises(ValueError):
        P.TextFont.from_outlines({0x110000: sq}, 64, 32.0, -32.0)
    assert L.pvq_text_font_metrics(None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_text_font_metrics(font, None, None, None) == _lib.PVQ_OK
    assert (syn.units_per_em, syn.ascent, syn.descent) == (64, 32.0, -32.0)
    n = C.c_uint32()
    assert L.pvq_text_font_glyph(None, ord("s"), None, None, None, 0, 0, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_text_font_glyph(font, ord("s"), None, None, C.byref(n), 0, 0, None, None, None) == _lib.PVQ_OK and n.value == 4
    assert L.pvq_text_font_glyph(font, ord("s"), None, None, None, 1, 3, None, fp, None) == _lib.PVQ_ERR_INVALID_ARG   # too small
    assert L.pvq_text_font_glyph(font, ord("x"), None, None, None, 0, 0, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert "U+0078" in L.pvq_last_error().decode()
    L.pvq_text_font_destroy(None)
    # the pitch labels
    out12 = (_lib.CTextLabel * 12)()
    for o in (0, 256):
        assert L.pvq_text_pitch_labels(o, None, out12) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_text_pitch_labels(7, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_text_pitch_labels(1, None, out12) == _lib.PVQ_OK and L.pvq_text_pitch_labels(255, None, out12) == _lib.PVQ_OK
    # the host face, the layout query and the batch handle take the same ranges; the handle checks them before any device is touched
    frame, query, create = L.pvq_text_frame, L.pvq_text_layout_query, L.pvq_text_batch_create
    lay = (_lib.CTextLayout * 64)()

    def each(labels, n, W, H, vh, with_frame=True):
        """the status of the entries, which must agree; a refusal comes before any device is touched, so device 0 refuses alike"""
        hh = C.c_void_p()
        got = [query(font, labels, n, W, H, vh, lay), create(-1, font, labels, n, vh, W, H, C.byref(hh))]
        if with_frame:                       # buf holds a 64 x 64 picture
            got.append(frame(font, labels, n, W, H, vh, fp, None))
        if got[0] == _lib.PVQ_OK:
            L.pvq_text_batch_destroy(hh)
        else:
            assert not hh.value
            got.append(create(0, font, labels, n, vh, W, H, C.byref(hh)))
            assert not hh.value
        assert len(set(got)) == 1, got
        return got[0], L.pvq_last_error().decode()

    assert each(good, 1, 64, 64, 64.0)[0] == _lib.PVQ_OK
    assert each(good, 1, 1, 1, 0.0, False)[0] == _lib.PVQ_OK and each(good, 1, 4096, 4096, 4096.0, False)[0] == _lib.PVQ_OK
    for W, H in ((0, 64), (64, 0), (4097, 64), (64, 4097)):
        st, msg = each(good, 1, W, H, 64.0)
        assert st == _lib.PVQ_ERR_INVALID_ARG and "4096" in msg
    for vh in (-1.0, math.inf, math.nan):
        st, msg = each(good, 1, 64, 64, vh)
        assert st == _lib.PVQ_ERR_INVALID_ARG and "viewport_height" in msg
    assert each(good, 0, 64, 64, 64.0)[0] == _lib.PVQ_ERR_INVALID_ARG
    assert each(None, 1, 64, 64, 64.0)[0] == _lib.PVQ_ERR_INVALID_ARG
    many = (_lib.CTextLabel * 65)(*[_label() for _ in range(65)])
    assert each(many, 64, 64, 64, 64.0)[0] == _lib.PVQ_OK
    st, msg = each(many, 65, 64, 64, 64.0)
    assert st == _lib.PVQ_ERR_INVALID_ARG and "64 labels" in msg
    for kw in BAD_LABELS:
        st, msg = each((_lib.CTextLabel * 2)(_label(), _label(**kw)), 2, 64, 64, 64.0)
        assert st == _lib.PVQ_ERR_INVALID_ARG and ("label 1" in msg or "U+0078" in msg), (kw, msg)
    assert each((_lib.CTextLabel * 1)(_label(font_px=1024.0)), 1, 64, 64, 64.0)[0] == _lib.PVQ_OK          # an em of exactly 1024 pixels
    assert each((_lib.CTextLabel * 1)(_label(b"ssssssss")), 1, 64, 64, 64.0)[0] == _lib.PVQ_OK            # eight codepoints
    assert each((_lib.CTextLabel * 1)(_label(x=3e38, y=-3e38)), 1, 64, 64, 64.0)[0] == _lib.PVQ_OK        # far off the image
    assert frame(font, good, 1, 64, 64, 64.0, None, None) == _lib.PVQ_ERR_INVALID_ARG                      # neither output
    assert frame(None, good, 1, 64, 64, 64.0, fp, None) == _lib.PVQ_ERR_INVALID_ARG
    assert query(font, good, 1, 64, 64, 64.0, None) == _lib.PVQ_ERR_INVALID_ARG
    assert create(-1, None, good, 1, 64.0, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    assert create(-1, font, good, 1, 64.0, 64, 64, None) == _lib.PVQ_ERR_INVALID_ARG
    assert create(-1, font, good, 1, 64.0, 64, 64, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        call = L.pvq_text_batch_rows_device
        assert call(None, 1, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, p, None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
        assert call(h, 0, p, None) == _lib.PVQ_ERR_NO_DEVICE
        assert call(h, 1, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, p + 8, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in L.pvq_last_error().decode()
        assert call(h, 1 << 31, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_text_batch_get_coverage(h, 0, fp) == _lib.PVQ_ERR_NO_DEVICE
        assert L.pvq_text_batch_get_coverage(h, -1, fp) == _lib.PVQ_ERR_NO_DEVICE
        for lab in (-2, 1):
            assert L.pvq_text_batch_get_coverage(h, lab, fp) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_text_batch_get_coverage(h, 0, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_text_batch_get_coverage(None, 0, fp) == _lib.PVQ_ERR_INVALID_ARG
    finally:
        L.pvq_text_batch_destroy(h)
    L.pvq_text_batch_destroy(None)
    # the Python face
    b = P.TextBatch(syn, [TC.unit_label("s")], 64, 48, viewport_height=48.0, device=None)
    assert (b.width, b.height, b.n_labels) == (64, 48, 1)
    with pytest.raises(P.PvqError) as e:
        b.rows(1, p)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(P.PvqError):
        b.coverage()
    with pytest.raises(ValueError):
        P.TextBatch(syn, [TC.unit_label("s")], 64, 5000, device=None)
    with pytest.raises(ValueError):
        P.TextBatch(syn, [TC.unit_label("sssssssss")], 64, 64, device=None)
    with pytest.raises(ValueError):
        P.text_frame(syn, [TC.unit_label("s")], np.zeros((4, 4, 3), f32))
    with pytest.raises(ValueError):
        P.text_frame(syn, [TC.unit_label("s")])
    with pytest.raises(ValueError):
        P.pitch_name_labels(7, colors=np.zeros((11, 3)))


# ---- 2. kernel resources --------------------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """no kernel of the unit uses scratch; the LDS is the one chunk of segments; VGPRs and occupancy recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "text_batch.hip")
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
    for want in ("text_coverage", "text_blend"):
        found = [u for k, u in usage.items() if want in k]
        assert len(found) == 1, (want, list(usage))
        kern[want] = found[0]
        print(f"{want}: {found[0]}")
    assert len(usage) == 2, list(usage)
    for k, u in kern.items():
        assert u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64, (k, u)       # a pixel's state is small: full occupancy
        assert u["Occupancy"] >= 8, (k, u)
    assert kern["text_coverage"]["LDS"] == 256 * 16               # one chunk of 256 segments of 16 bytes
    assert kern["text_blend"]["LDS"] == 0


# ---- 3. known answers from the coverage rule alone ------------------------------------------------------------------------------
def test_square_on_pixel_boundaries(syn):
    W = H = 16
    cov = cov_of(syn, "s", W, H)                     # the square spans pixels x 6 .. 10, y 4 .. 8
    want = np.zeros((H, W), f32)
    want[4:8, 6:10] = 1.0
    TC.same(cov, want, "square")


def test_square_shifted_by_a_quarter_pixel(syn):
    W = H = 16
    cov = cov_of(syn, "s", W, H, x=0.25, y=-0.25)    # x 6.25 .. 10.25, y 4.25 .. 8.25
    want = TC.rect_coverage(W, H, 6.25, 4.25, 10.25, 8.25)
    TC.same(cov, want, "shifted square")
    assert cov[5, 6] == 0.75 and cov[5, 10] == 0.25 and cov[4, 7] == 0.75 and cov[8, 7] == 0.25
    assert cov[4, 6] == 0.5625 and cov[4, 10] == 0.1875 and cov[8, 6] == 0.1875 and cov[8, 10] == 0.0625
    assert cov[5, 7] == 1.0 and cov.sum() == 16.0


def test_triangle_exact_areas(syn):
    W = H = 16
    cov = cov_of(syn, "t", W, H)                     # glyph (0,0) (6,0) (0,3): pixels (5,8) (11,8) (5,5)
    tri = [(5.0, 8.0), (11.0, 8.0), (5.0, 5.0)]
    want = np.asarray([[TC.clip_area(tri, i, j) for i in range(W)] for j in range(H)])
    assert np.abs(cov - want).max() <= 2.0 ** -22, np.abs(cov - want).max()
    assert abs(cov.sum() - 9.0) <= 1e-6                           # half of the 6 x 3 box
    assert cov[7, 5] == 1.0 and cov[5, 5] == 0.75 and cov[5, 6] == 0.25 and cov[5, 7] == 0.0 and cov[4, 5] == 0.0
    assert cov[6, 7] == 0.75 and cov[6, 8] == 0.25 and cov[7, 9] == 0.75 and cov[7, 10] == 0.25 and cov[6, 6] == 1.0
    assert not cov[:5].any() and not cov[8:].any() and not cov[:, :5].any() and not cov[:, 11:].any()


def test_hole_overlap_reversal_and_degenerate(syn):
    W = H = 16
    hole = cov_of(syn, "o", W, H)                    # 6 x 6 at x 5 .. 11, y 2 .. 8 with the hole x 7 .. 9, y 4 .. 6
    want = np.zeros((H, W), f32)
    want[2:8, 5:11] = 1.0
    want[4:6, 7:9] = 0.0
    TC.same(hole, want, "hole")
    both = cov_of(syn, "d", W, H)                    # squares x 5 .. 9, y 4 .. 8 and x 7 .. 11, y 2 .. 6
    want = np.zeros((H, W), f32)
    want[4:8, 5:9] = 1.0
    want[2:6, 7:11] = 1.0
    TC.same(both, want, "overlap counts once")
    TC.same(cov_of(syn, "r", W, H, 0.25, -0.25), cov_of(syn, "s", W, H, 0.25, -0.25), "reversed contour")
    assert not cov_of(syn, "h", W, H).any()
    bg = TC.images(1, W, H, 3)[0]
    TC.same(P.text_frame(syn, [TC.unit_label("h")], bg, viewport_height=float(H)), bg, "a horizontal contour draws nothing")
    lay = P.text_layout(syn, [TC.unit_label("h"), TC.unit_label("s")], W, H, float(H))
    assert not lay[0]["on_image"] and lay[0]["n_tiles"] == 0 and lay[0]["tiles"] == []
    assert lay[1]["on_image"] and (lay[1]["x0"], lay[1]["y0"], lay[1]["x1"], lay[1]["y1"]) == (6, 4, 9, 7) and lay[1]["n_segments"] == 2


def test_curves_and_implied_points_against_the_model(syn):
    W = H = 16
    for ch, area in (("q", 2.0 / 3.0 * 8.0 * 4.0), ("e", None)):
        lab = TC.unit_label(ch, 0.3, -0.4)
        got = P.text_frame(syn, [lab], width=W, height=H, viewport_height=float(H), coverage=True)[0]
        want = M.label_coverage(TC.SYNTHETIC, lab, W, H, float(H))
        assert np.abs(got - want).max() <= COVERAGE_BAR, (ch, np.abs(got - want).max())
        if area:
            # the parabola's segment is 2 / 3 base height; |p0 - 2 p1 + p2| = 16 gives 16 chords, whose polygon lacks 1 / 16^2 of it
            assert abs(got.sum() - area * (1.0 - 1.0 / 256.0)) <= 1e-4, (ch, got.sum())
    assert abs(want.sum() - 80.0 / 3.0) <= 0.01                       # 'e': a 4 x 4 square and four parabola segments of 2 / 3 * 4 * 1


@pytest.mark.parametrize("edge", ["left", "right", "top", "bottom", "corner"])
def test_glyph_hanging_off_an_edge(syn, edge):
    W, H = 21, 13
    x, y = {"left": (-W / 2.0 - 0.25, 0.0), "right": (W / 2.0 + 0.25, 0.0), "top": (0.5, H / 2.0 - 1.5), "bottom": (0.5, -H / 2.0 - 2.25),
            "corner": (W / 2.0, -H / 2.0 - 2.0)}[edge]
    x0, y1 = W / 2.0 + x - 2.0, H / 2.0 - y
    want = TC.rect_coverage(W, H, x0, y1 - 4.0, x0 + 4.0, y1)
    assert 0.0 < want.sum() < 16.0
    bg = TC.images(1, W, H, 5)[0]
    lab = P.TextLabel("s", x, y, 64.0, 1.0, (0.2, 0.5, 0.9))
    img, cov = P.text_frame(syn, [lab], bg, viewport_height=float(H), coverage=True)
    TC.same(cov[0], want, edge)
    changed = (TC.bits(img) != TC.bits(bg)).any(-1)
    assert np.array_equal(changed, want > 0)
    lay = P.text_layout(syn, [lab], W, H, float(H))[0]
    ys, xs = np.nonzero(want > 0)
    assert (lay["x0"], lay["y0"], lay["x1"], lay["y1"]) == (xs.min(), ys.min(), xs.max(), ys.max())


def test_blend_known_answer(syn):
    W = H = 16
    bg = TC.images(1, W, H, 7)[0]
    rgb = (0.2, 0.5, 0.9)
    img = P.text_frame(syn, [P.TextLabel("s", 0.25, -0.25, 64.0, 1.0, rgb)], bg, viewport_height=float(H))
    lin = M.srgb_to_linear(np.asarray(rgb, f32))
    for (j, i), a in (((5, 7), 1.0), ((5, 6), 0.75), ((8, 10), 0.0625)):
        a = f32(a)
        k = f32(1.0) - a
        want = [f32(lin[c]) * a + bg[j, i, c] * k for c in range(3)] + [a + bg[j, i, 3] * k]
        assert np.abs(img[j, i] - np.asarray(want, f32)).max() <= 2.0 ** -22, (j, i)   # the colour's pow is the library's own
    TC.same(img[0], bg[0], "a row the label does not reach")


# ---- 4. layout known answers ----------------------------------------------------------------------------------------------------
def test_layout_block_pen_and_baseline():
    font_m = {"glyphs": {ord("a"): TC.glyph(700, TC.rect(100, 0, 500, 600)), ord("b"): TC.glyph(300, TC.rect(50, -200, 250, 400))},
              "units_per_em": 1000, "ascent": 900.0, "descent": -300.0}
    font = TC.font_of(font_m)
    W, H, vh = 200, 120, 12.0
    lab = P.TextLabel("ab", 1.5, -0.75, 50.0, 0.04)
    s = float(f32(vh) / f32(H))
    k = 50.0 / 1000.0
    width, line = (700 + 300) * k, float(f32(1.2)) * 50.0
    baseline = -line / 2 + (line - (900 + 300) * k) / 2 + 900 * k          # the stated formula, font pixels below the label's y
    ox = (float(f32(1.5)) + (-width / 2) * float(f32(0.04))) / s + W / 2
    oy = H / 2 - (float(f32(-0.75)) - baseline * float(f32(0.04))) / s
    lay = P.text_layout(font, [lab], W, H, vh)[0]
    assert abs(lay["origin_x"] - ox) <= 1e-4 and abs(lay["baseline_y"] - oy) <= 1e-4
    assert abs(baseline - (900 - 300) * k / 2) <= 1e-9                        # the block's middle lies midway between ascent and descent
    cov = P.text_frame(font, [lab], width=W, height=H, viewport_height=vh, coverage=True)[0]
    z = float(f32(0.04)) / s                                                  # output pixels per font pixel
    a_box = (ox + 100 * k * z, oy - 600 * k * z, ox + 500 * k * z, oy)
    b_box = (ox + (700 + 50) * k * z, oy - 400 * k * z, ox + (700 + 250) * k * z, oy + 200 * k * z)   # pen advanced by a's advance
    want = TC.rect_coverage(W, H, *a_box) + TC.rect_coverage(W, H, *b_box)
    assert np.abs(cov - want).max() <= 1e-4
    # the block is centred: its middle, left + width / 2, is the label's x
    assert abs(ox + width * z / 2 - (float(f32(1.5)) / s + W / 2)) <= 1e-9
    assert lay["n_segments"] == 4 and lay["n_tiles"] == len(lay["tiles"]) > 0


def test_pitch_name_labels():
    for octaves in (1, 7, 9):
        labels = P.pitch_name_labels(octaves)
        assert [lab.text for lab in labels] == [M.PITCH_NAMES[(idx + 9) % 12] for idx in range(12)]
        assert labels[3].text == "C" and labels[4].text == "C♯" and labels[1].text == "B♭"
        for idx, lab in enumerate(labels):
            x, y = M.spiral_point_f32(12, 12 * octaves - 12 + idx)        # the last twelve of calculate_spiral_points(octaves, 12)
            f = f32(0.85) + f32(0.025) * abs(x)
            assert np.allclose([lab.x, lab.y], [x * f, y * f], rtol=3e-7, atol=1e-6), (octaves, idx, lab, x * f, y * f)
            xd, yd = M.spiral_point(12, float(12 * octaves - 12 + idx))
            assert abs(lab.x - xd * (0.85 + 0.025 * abs(xd))) <= 1e-4 and abs(lab.y - yd * (0.85 + 0.025 * abs(xd))) <= 1e-4
            assert (lab.font_px, lab.scale) == (40.0, float(f32(0.02)))
            assert np.array_equal(np.asarray(lab.rgb, f32), M.COLORS[(idx + 9) % 12])
    pal = np.random.default_rng(1).uniform(0, 1, (12, 3)).astype(f32)
    assert np.array_equal(np.asarray(P.pitch_name_labels(7, pal)[5].rgb, f32), pal[(5 + 9) % 12])
    # the squash: C (idx 3, the top of the spiral, x = 0) keeps 0.85; A (idx 0, far left) is pushed outwards
    top, left = P.pitch_name_labels(7)[3], P.pitch_name_labels(7)[0]
    assert abs(top.x) < 1e-4 and abs(top.y - 0.85 * M.spiral_point(12, 75.0)[1]) < 1e-4
    assert abs(left.x / M.spiral_point(12, 72.0)[0] - (0.85 + 0.025 * abs(M.spiral_point(12, 72.0)[0]))) < 1e-5


# ---- 5. the TrueType reader -----------------------------------------------------------------------------------------------------
def _same_glyphs(font, fx):
    assert (font.units_per_em, font.ascent, font.descent) == (fx["units_per_em"], fx["ascent"], fx["descent"])
    for cp, (adv, ends, pts, on) in fx["glyphs"].items():
        a, e, p, o = font.glyph(cp)
        assert a == adv and np.array_equal(e, ends) and np.array_equal(p, pts) and np.array_equal(o, on), hex(cp)


@pytest.mark.parametrize("cmap_format,long_loca", [(4, False), (12, False), (4, True), (12, True)])
def test_truetype_reader_point_for_point(tmp_path, cmap_format, long_loca):
    pytest.importorskip("fontTools")
    from fontTools.ttLib import TTFont
    path = tmp_path / "f.ttf"
    fx = TC.build_ttf(path, cmap_format, long_loca)
    tt = TTFont(str(path))
    assert tt["head"].indexToLocFormat == int(long_loca) and {t.format for t in tt["cmap"].tables} >= {cmap_format}
    assert cmap_format == 4 or {t.format for t in tt["cmap"].tables} == {12}
    font = P.TextFont.from_file(path)
    _same_glyphs(font, fx)
    _same_glyphs(TC.font_of(fx), fx)                                  # from_outlines gives back what it was given
    labels = P.pitch_name_labels(7)
    TC.same(P.text_frame(font, labels, width=64, height=64, coverage=True),
            P.text_frame(TC.font_of(fx), labels, width=64, height=64, coverage=True), "the file's font draws as the arrays'")
    with pytest.raises(ValueError) as e:
        font.glyph("x")
    assert "U+0078" in str(e.value)


def test_truetype_refusals(tmp_path, dejavu):
    pytest.importorskip("fontTools")
    path = tmp_path / "c.ttf"
    TC.build_ttf(path, composite=True)
    font = P.TextFont.from_file(path)
    font.glyph("C")
    with pytest.raises(P.PvqError) as e:
        font.glyph("Q")
    assert e.value.status == _lib.PVQ_ERR_UNSUPPORTED and "composite" in str(e.value)
    with pytest.raises(P.PvqError) as e:
        P.text_frame(font, [P.TextLabel("CQ", 0.0, 0.0)], width=64, height=64, coverage=True)
    assert e.value.status == _lib.PVQ_ERR_UNSUPPORTED
    with pytest.raises(ValueError) as e:                              # a codepoint the font lacks: named
        P.text_frame(dejavu[1], [P.TextLabel("CH", 0.0, 0.0)], width=64, height=64, coverage=True)
    assert "U+0048" in str(e.value)
    data = bytearray(open(path, "rb").read())
    with pytest.raises(ValueError) as e:
        P.TextFont.from_bytes(bytes(data[:200]))
    assert "table" in str(e.value)
    # a font without glyf outlines: the constructor takes it, a glyph is refused as unsupported
    from fontTools.ttLib import TTFont
    tt = TTFont(str(path))
    del tt["glyf"], tt["loca"]
    tt.sfntVersion = "OTTO"
    tt.save(str(tmp_path / "o.otf"))
    cff = P.TextFont.from_file(tmp_path / "o.otf")
    with pytest.raises(P.PvqError) as e:
        cff.glyph("C")
    assert e.value.status == _lib.PVQ_ERR_UNSUPPORTED and "CFF" in str(e.value)


def test_fixture_equals_a_system_dejavu(dejavu):
    """where matplotlib ships DejaVuSans.ttf, its nine glyphs are the fixture's (2.35 and 2.37 agree on them)"""
    mpl = pytest.importorskip("matplotlib")
    path = os.path.join(mpl.get_data_path(), "fonts", "ttf", "DejaVuSans.ttf")
    if not os.path.exists(path):
        pytest.skip("matplotlib ships no DejaVuSans.ttf here")
    _same_glyphs(P.TextFont.from_file(path), dejavu[0])


def test_fixture_contents(dejavu):
    fx = dejavu[0]
    assert sorted(fx["glyphs"]) == sorted(ord(c) for c in "CDEFGAB♯♭")
    assert (fx["units_per_em"], fx["ascent"], fx["descent"]) == (2048, 1901.0, -483.0)
    assert sum(len(g[3]) for g in fx["glyphs"].values()) == 207
    assert os.path.getsize(TC.GOLDEN) < 8192


# ---- 6. the host face against the model -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_results(dejavu):
    """the model's coverages and blends of every crafted case, computed once"""
    fx = dejavu[0]
    out = {}
    for case in TC.HOST_CASES:
        kind, W, H, vh = case
        labels = TC.case_labels(kind)
        bg = TC.images(1, W, H, 11)[0]
        img, covs = M.frame(fx, labels, bg, vh)
        out[case] = (labels, bg, (img, covs), M.frame(fx, labels, np.zeros((H, W, 4)), vh, covs)[0])
    return out


def test_bar_is_within_the_design():
    assert COVERAGE_BAR <= TC.BAR_LIMIT and abs(COVERAGE_BAR - 2.0 * COVERAGE_SEEN) < 1e-12


@pytest.mark.parametrize("case", TC.HOST_CASES, ids=lambda c: "%s-%dx%d-vh%g" % c)
def test_host_face_matches_model(dejavu, model_results, case):
    kind, W, H, vh = case
    labels, bg, (want_img, want_cov), want_black = model_results[case]
    img, cov = P.text_frame(dejavu[1], labels, bg, viewport_height=vh, coverage=True)
    err = TC.compare(cov, want_cov, COVERAGE_BAR, case)
    print(f"{case}: largest coverage difference {err:.5f}")
    assert cov.min() >= 0.0 and cov.max() <= 1.0 and cov.max() > 0.2
    shows = (cov > 0).any((1, 2))                                              # a square picture at the viewer's view cuts the outermost off
    assert np.array_equal(shows, (want_cov > 0).any((1, 2))) and shows.sum() >= (9 if kind == "pitch" else 1)
    # the picture: 1e-6 plus the coverage bar times the colour (over transparent black, where a channel is colour * coverage) ...
    black = P.text_frame(dejavu[1], labels, np.zeros((H, W, 4), f32), viewport_height=vh)
    lin = np.concatenate([M.srgb_to_linear(np.asarray([lab.rgb for lab in labels], f32)), np.ones((len(labels), 1))], 1)
    tol = 1e-6 + COVERAGE_BAR * lin.max(0)
    assert (np.abs(black - want_black) <= tol).all(), np.abs(black - want_black).max((0, 1))
    # ... and over a random picture, where a channel moves by (colour - what is there) per unit of coverage
    tol = 1e-6 + COVERAGE_BAR * np.maximum(lin.max(0), 1.0)
    assert (np.abs(img - want_img) <= tol).all(), np.abs(img - want_img).max((0, 1))
    untouched = (TC.bits(img) == TC.bits(bg)).all(-1)
    assert np.array_equal(untouched, ~(cov > 0).any(0))                        # coverage exactly 0: not touched
    lay = P.text_layout(dejavu[1], labels, W, H, vh)
    for c, d in zip(cov, lay):
        ys, xs = np.nonzero(c > 0)
        if not len(ys):
            continue
        assert d["on_image"] and d["x0"] <= xs.min() and xs.max() <= d["x1"] and d["y0"] <= ys.min() and ys.max() <= d["y1"]
        assert d["n_segments"] <= 3 * 400


def test_segment_counts_stay_small(dejavu):
    """a glyph of the fixture takes a few hundred chords at most at tol 1 / 64, also at an em of 200 pixels"""
    s = float(f32(M.VIEWPORT_HEIGHT) / f32(720))
    for ch in "CDEFGAB♯♭":
        for em in (13.0, 36.6, 200.0):
            lay = P.text_layout(dejavu[1], [P.TextLabel(ch, 0.0, 0.0, 40.0, em * s / 40.0)], 1280, 720)[0]
            assert 3 <= lay["n_segments"] <= (107 if em < 40 else 300), (ch, em, lay["n_segments"])
