"""CPU checks of the readout stage (include/pvq.h, "the readout"): the value's text and colour, the layout and the one-frame host
face against the NumPy model of tests/readout_model.py, bit for bit; the synthetic font's geometry against hand-computed pixel
sets; the argument checks; the kernels' resources; and that the cases tell five wrong rules from the right one."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import pitchvis_amd as P
import readout_cases as K
import readout_model as M
from pitchvis_amd import _lib
from text_cases import rect_coverage

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_readout_text", "pvq_readout_layout_query", "pvq_readout_frame", "pvq_readout_batch_create", "pvq_readout_batch_destroy",
           "pvq_readout_batch_rows_device", "pvq_readout_batch_get_atlas")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(L, name), name
    assert "common.rs:348-432" in hdr
    assert P.readout.CODEPOINTS == M.CODEPOINTS and P.readout.PREFIX == M.PREFIX


@pytest.mark.parametrize("value,want", list(zip(K.VALUES, K.EXPECTED_TEXT)), ids=[repr(v) for v in K.VALUES])
def test_text_and_colour(value, want):
    """pvq_readout_text against the stated strings, the model and, for finite values, Python's own format of the rounded value;
    the colour bit for bit against the model"""
    text, rgb = P.readout_text(value)
    assert text == want == M.value_text(value), (value, text, want, M.value_text(value))
    r = float(M.rounded(value))
    if math.isfinite(r):
        clamped = math.copysign(min(abs(r), float(M.CLAMP)), r)
        assert text == format(clamped, ">3.0f"), (value, text)
    else:
        assert text == {"nan": "NaN", "inf": "inf", "-inf": "-inf"}[str(r)]
    assert len(text) <= 11
    K.same(np.asarray(rgb, f32), M.value_srgb(value), value)


def test_colour_branches_by_hand():
    """common.rs:404-413: green to 10, yellow at 20, red from 30; a NaN fails every comparison"""
    for value, want in ((0.0, (0, 1, 0)), (10.0, (0, 1, 0)), (-10.4, (0, 1, 0)), (15.0, (0.5, 1, 0)), (20.0, (1, 1, 0)), (-25.0, (1, 0.5, 0)),
                        (30.0, (1, 0, 0)), (30.5, (1, 0, 0)), (float("nan"), (1, 0, 0)), (float("-inf"), (1, 0, 0))):
        assert P.readout_text(value)[1] == tuple(float(v) for v in want), value


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "%s-%dx%d-%g" % c)
def test_layout_against_the_model(case):
    """the box, the pen's end, the origins, the baseline row, the placed cells and the colours, every value of the list"""
    name, W, H, scale = case
    atlas = K.model_atlas(name, scale)
    for value in K.VALUES:
        got, want = P.readout_layout(K.lib_font(name), value, W, H, scale), M.layout(atlas, value, W, H)
        assert got["text"] == want["text"], value
        for key in ("xl", "xr", "yt", "yb", "text_width"):
            K.same(got[key], want[key], (case, value, key))
        K.same(got["font_px"], atlas.F, case)
        K.same(got["baseline"], atlas.baseline, case)
        assert got["origin_x"] == want["origin_x"] and got["baseline_row"] == want["baseline_row"], (case, value)
        for slot, ch in enumerate(want["text"]):
            x0, y0, cov = atlas.cells[ch]
            cell = (want["origin_x"][slot] + x0, want["baseline_row"] + y0, cov.shape[1], cov.shape[0])
            assert got["cells"][slot] == cell if cov.size else got["cells"][slot][2:] == (0, 0), (case, value, slot)
        K.same(got["value_srgb"], want["value_srgb"], (case, value))
        K.same(got["value_linear"], want["value_linear"], (case, value))


def test_synthetic_font_by_hand():
    """ui_scale 4 with 64 units per em: a font unit is a pixel.  On 301 x 173 the box edges and every glyph's rectangle are worked
    out here in exact fractions: xr = 301 - 0.01f * 301 and yb = 173 - 0.01f * 173 in f32, the line 1.2f * 64, advances in half
    pixels (the f32 sums are exact), baseline offset b = (76.8 - 64) / 2 + 48 = 54.4."""
    W, H, scale = 301, 173, 4.0
    font, model = K.lib_font("synthetic"), K.model_font("synthetic")
    host = P.ReadoutBatch(font, W, H, scale, device=None)
    # every atlas cell is the exact area of its rectangles
    for ch in M.CODEPOINTS:
        x0, y0, adv, cov = host.atlas(ch)
        assert adv == model["glyphs"][ord(ch)][0]
        rects = K.synthetic_rects(ch)
        if not rects:
            assert cov.size == 0
            continue
        want = sum(rect_coverage(cov.shape[1], cov.shape[0], r[0] - x0, -r[3] - y0, r[2] - x0, -r[1] - y0) for r in rects)
        assert x0 == math.floor(min(r[0] for r in rects)) and y0 == math.floor(-max(r[3] for r in rects))
        assert cov.shape == (math.ceil(-min(r[1] for r in rects)) - y0, math.ceil(max(r[2] for r in rects)) - x0)
        assert np.array_equal(cov.astype(np.float64), want), ch
    for value in (0.0, -99.5, 3e9):
        text = M.PREFIX + M.value_text(value)
        xr = Fraction(float(f32(W) - f32(0.01) * f32(W)))          # 297.99 and 171.27, as f32 has them
        yb = Fraction(float(f32(H) - f32(0.01) * f32(H)))
        advances = [Fraction(6) + Fraction(M.CODEPOINTS.index(c), 2) for c in text]
        xl, yt = xr - sum(advances), yb - Fraction(float(f32(1.2) * f32(64)))
        baseline_row = math.floor(yt + Fraction(float(f32(54.4))) + Fraction(1, 2))
        box_cols = [i for i in range(W) if xl <= Fraction(2 * i + 1, 2) < xr]
        box_rows = [j for j in range(H) if yt <= Fraction(2 * j + 1, 2) < yb]
        assert box_cols[-1] == 297 and box_rows == list(range(94, 171)), value   # 297.5 < 297.99; 94.5 >= 94.47, 170.5 < 171.27
        green = np.zeros((H, W))   # over a clear picture the green channel is the glyphs' coverage: white and the value's colour have G = 1
        pen = Fraction(0)
        for c, adv in zip(text, advances):
            origin = math.floor(xl + pen + Fraction(1, 2))
            for r in K.synthetic_rects(c):
                green += rect_coverage(W, H, origin + r[0], baseline_row - r[3], origin + r[2], baseline_row - r[1])
            pen += adv
        if M.value_srgb(value)[1] == 0:   # -99.5 and 3e9 are red: the value's glyphs add no green, take them out again
            pen = sum(advances[:len(M.PREFIX)])
            for c, adv in zip(text[len(M.PREFIX):], advances[len(M.PREFIX):]):
                origin = math.floor(xl + pen + Fraction(1, 2))
                for r in K.synthetic_rects(c):
                    green -= rect_coverage(W, H, origin + r[0], baseline_row - r[3], origin + r[2], baseline_row - r[1])
                pen += adv
        got = P.readout_frame(font, value, np.zeros((H, W, 4), f32), scale)
        assert np.array_equal(got[..., 1].astype(np.float64), green), value
        alpha_box = np.zeros((H, W), bool)
        alpha_box[np.ix_(box_rows, box_cols)] = True
        assert np.array_equal(got[..., 3] >= 0.5, alpha_box), value      # the box gives alpha 0.5, a glyph over it more, nothing else any
        assert (got[..., 3][~alpha_box] == 0).all()


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "%s-%dx%d-%g" % c)
def test_frame_against_the_model(case):
    """pvq_readout_frame bit for bit; outside the box and the cells' covered pixels every bit is kept, a NaN's payload included"""
    name, W, H, scale = case
    atlas, base = K.model_atlas(name, scale), K.background(W, H)
    for index, value in enumerate(K.VALUES):
        want, drawn = M.frame(atlas, value, base)
        K.compare(K.host_frame(name, W, H, scale, index), want, drawn, base, (case, value))
        assert drawn.any()


@pytest.mark.parametrize("name,scale", [("synthetic", 4.0), ("curved", 0.0), ("curved", 0.5), ("curved", 1.3)])
def test_host_atlas_against_the_model(name, scale):
    host, atlas = P.ReadoutBatch(K.lib_font(name), 64, 64, scale, device=None), K.model_atlas(name, scale)
    chords = 0
    for ch in M.CODEPOINTS:
        x0, y0, adv, cov = host.atlas(ch)
        mx0, my0, want = atlas.cells[ch]
        K.same(adv, atlas.advance[ch], ch)
        assert cov.shape == want.shape and (not cov.size or (x0, y0) == (mx0, my0)), ch
        K.same(cov, want, (name, scale, ch))
        chords += len(M.chords_of(K.model_font(name)["glyphs"][ord(ch)], float(atlas.F) / K.model_font(name)["units_per_em"]))
    firsts = [atlas.cells[ch][0] for ch in M.CODEPOINTS]
    if name == "curved":   # the curves take more than one chord, and the left bearings move the cells off their origins
        assert chords > 24 * 12 and (max(firsts) > 0 or atlas.F < 16)   # at 8 pixels an em the bearings stay within the first pixel
    else:                  # a negative left bearing: a cell that begins left of its origin
        assert min(firsts) < 0


WRONG = {"half_even": M.Rule(half_even=True), "minus_zero": M.Rule(drop_minus_zero=True), "pairwise_pen": M.Rule(pairwise_pen=True),
         "truncated_origin": M.Rule(truncate_origin=True), "closed_box": M.Rule(closed_box=True)}


@pytest.mark.parametrize("which", sorted(WRONG))
def test_the_cases_tell_a_wrong_rule_from_the_right_one(which):
    """each wrong variant, restated in the model, differs from the right rule (which the library equals bit for bit, above) in a
    text, a layout or a picture of the cases"""
    rule, told = WRONG[which], []
    for name, W, H, scale in K.CASES:
        atlas, base = K.model_atlas(name, scale), K.background(W, H)
        for value in K.VALUES:
            right, wrong = M.layout(atlas, value, W, H), M.layout(atlas, value, W, H, rule)
            if right["text"] != wrong["text"] or right["origin_x"] != wrong["origin_x"] or K.bits(right["xl"]) != K.bits(wrong["xl"]):
                told.append((name, W, H, scale, value))
            elif which == "closed_box" and (K.bits(M.frame(atlas, value, base)[0]) != K.bits(M.frame(atlas, value, base, rule)[0])).any():
                told.append((name, W, H, scale, value))
    assert told, which
    if which == "half_even":
        assert {v for *_, v in told} >= {0.5, -0.5, 10.5, 20.5, 30.5}
    if which == "minus_zero":
        assert {v for *_, v in told} == {-0.4}
    if which == "closed_box":
        assert {c[:4] for c in told} == {("curved", 50, 50, 0.0)}   # 50 - 0.01f * 50 == 49.5, a pixel's centre


def test_argument_checks():
    font = K.lib_font("synthetic")
    img = np.zeros((8, 8, 4), f32)
    lacking = dict(K.model_font("synthetic")["glyphs"])
    del lacking[ord("f")]
    short = P.TextFont.from_outlines(lacking, 64, 48.0, -16.0)
    for call in (lambda: P.readout_frame(short, 1.0, img), lambda: P.readout_layout(short, 1.0, 8, 8), lambda: P.ReadoutBatch(short, 8, 8, device=None)):
        with pytest.raises(Exception, match="U\\+0066"):
            call()
    for W, H in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        with pytest.raises(Exception, match="width and height"):
            P.ReadoutBatch(font, W, H, device=None)
        with pytest.raises(Exception, match="width and height"):
            P.readout_layout(font, 1.0, W, H)
    for scale in (-1.0, float("nan"), float("inf"), 64.5):
        with pytest.raises(Exception, match="ui_scale"):
            P.ReadoutBatch(font, 8, 8, scale, device=None)
        with pytest.raises(Exception, match="ui_scale"):
            P.readout_frame(font, 1.0, img, scale)
    P.ReadoutBatch(font, 8, 8, 64.0, device=None)   # F = 1024 is admitted
    L = _lib.load()
    host = P.ReadoutBatch(font, 8, 8, device=None)
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += -base % 16
    rows = lambda n, values, image: L.pvq_readout_batch_rows_device(host._h, n, values, image, None)
    assert rows(1, None, base) == _lib.PVQ_ERR_INVALID_ARG and rows(1, base, None) == _lib.PVQ_ERR_INVALID_ARG
    assert rows(1, base, base + 4) == _lib.PVQ_ERR_INVALID_ARG and b"16-byte aligned" in L.pvq_last_error()
    assert rows(2 ** 31, base, base) == _lib.PVQ_ERR_INVALID_ARG
    assert rows(1, base, base) == _lib.PVQ_ERR_NO_DEVICE           # after its checks: a host-only handle has no device
    assert L.pvq_readout_batch_get_atlas(host._h, ord("x"), None, None, None, None, None, 0, None) == _lib.PVQ_ERR_INVALID_ARG
    w, h = C.c_uint32(), C.c_uint32()
    assert L.pvq_readout_batch_get_atlas(host._h, ord("T"), None, None, C.byref(w), C.byref(h), None, 0, None) == _lib.PVQ_OK and w.value * h.value > 1
    assert L.pvq_readout_batch_get_atlas(host._h, ord("T"), None, None, None, None, None, 1, buf) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_readout_frame(font._h, 1.0, 8, 8, 0.0, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_readout_layout_query(font._h, 1.0, 8, 8, 0.0, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_readout_text(1.0, None, None) == _lib.PVQ_OK


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """every kernel of readout_batch.hip keeps its state in registers and LDS; the figures DESIGN 6k records are printed"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "readout_batch.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "x.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs|AGPRs): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(usage) == 2 and any("readout_atlas" in n for n in usage) and any("readout_draw" in n for n in usage), list(usage)
    for name, u in usage.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] <= 8192 and u["VGPRs"] <= 128, (name, u)   # several workgroups a CU
