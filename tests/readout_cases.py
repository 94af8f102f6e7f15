"""Shared by tests/test_readout.py and tests/test_readout_gpu.py: the two outline fonts (no font file is needed), the values, the
sizes, the pictures the readout is drawn over, the host face's pictures (made once a case and shared) and `compare`."""
import functools

import numpy as np

import pitchvis_amd as P
import readout_model as M
from text_cases import fixture, font_of, glyph, rect

f32 = np.float32

# The issue's list: every colour branch and its edges, the rounding ties, -0, three and four characters, the clamp, the smallest
# subnormal, NaN and the infinities.
VALUES = [0.0, 0.4, -0.4, 0.5, -0.5, 9.5, 10.0, 10.5, 15.0, 20.0, 20.5, 25.0, 30.0, 30.5, 99.5, -99.5, 999.0, -1000.0, 1e7, 2147483520.0, 3e9, -3e9,
          float(np.finfo(f32).smallest_subnormal), float("nan"), float("inf"), float("-inf")]
EXPECTED_TEXT = ["  0", "  0", " -0", "  1", " -1", " 10", " 10", " 11", " 15", " 20", " 21", " 25", " 30", " 31", "100", "-100", "999", "-1000",
                 "10000000", "2147483520", "2147483520", "-2147483520", "  0", "NaN", "inf", "-inf"]


def synthetic_font():
    """64 units per em: at ui_scale 4 a font unit is one output pixel.  Codepoint n of the atlas's order is a rectangle with
    quarter-pixel coordinates, at most 2.75 wide and ending at 4 at the latest, while the next glyph begins at 4.5 or later even with
    its left bearing, so no two glyphs of a string share a pixel; the advances 6, 6.5, 7, ... are distinct and every other one ends
    on half a pixel, so the origins' rounding is exercised.  'g' descends below the baseline, 'T' and 'N' have a second rectangle, the space has no outline."""
    glyphs = {}
    for n, ch in enumerate(M.CODEPOINTS):
        x0 = (-1.5, 0.0, 0.5, 1.25)[n % 4]
        y0 = -2.5 if ch == "g" else (0.0, 0.5)[n % 2]
        w, h = 1.0 + 0.75 * (n % 3) + 0.25 * (n % 2), 3.0 + (n % 7) + 0.75
        contours = [] if ch == " " else [rect(x0, y0, x0 + w, y0 + h)]
        if ch in "TN":
            contours.append(rect(x0, y0 + h + 1.0, x0 + w, y0 + h + 2.5))
        glyphs[ord(ch)] = glyph(6.0 + 0.5 * n, *contours)
    return {"glyphs": glyphs, "units_per_em": 64, "ascent": 48.0, "descent": -16.0}


def synthetic_rects(ch):
    """the rectangles (x0, y0, x1, y1), font units with y upwards, of a codepoint of the synthetic font"""
    n = M.CODEPOINTS.index(ch)
    x0 = (-1.5, 0.0, 0.5, 1.25)[n % 4]
    y0 = -2.5 if ch == "g" else (0.0, 0.5)[n % 2]
    w, h = 1.0 + 0.75 * (n % 3) + 0.25 * (n % 2), 3.0 + (n % 7) + 0.75
    out = [] if ch == " " else [(x0, y0, x0 + w, y0 + h)]
    if ch in "TN":
        out.append((x0, y0 + h + 1.0, x0 + w, y0 + h + 2.5))
    return out


def curved_font():
    """the fixture's nine DejaVuSans outlines given to the codepoints cyclically: more than one chord a curve, left bearings,
    advances that are no binary fractions of a pixel.  The shapes need not be legible."""
    fx = fixture()
    shapes = [fx["glyphs"][cp] for cp in sorted(fx["glyphs"])]
    return {"glyphs": {ord(ch): shapes[n % len(shapes)] for n, ch in enumerate(M.CODEPOINTS)}, "units_per_em": fx["units_per_em"],
            "ascent": fx["ascent"], "descent": fx["descent"]}


FONTS = {"synthetic": synthetic_font, "curved": curved_font}
# (font, width, height, ui_scale): the issue's three sizes — 64 x 64 cuts the box at the left edge — and 50 x 50, where
# xr = 50 - 0.01f * 50 is 49.5 exactly, the centre of pixel 49, which a closed box would take; and ui_scale 1.3, where the advances
# (font units times 20.8 / 2048) are no binary fractions, so that the order of the pen's sum shows in its roundings
CASES = [("synthetic", 301, 173, 4.0), ("curved", 301, 173, 0.0), ("synthetic", 64, 64, 4.0), ("curved", 64, 64, 0.0), ("synthetic", 160, 90, 0.5),
         ("curved", 160, 90, 0.5), ("curved", 50, 50, 0.0), ("curved", 301, 173, 1.3)]
GPU_CASES = [("curved", 301, 173, 0.0), ("synthetic", 64, 64, 4.0), ("curved", 160, 90, 0.5), ("curved", 50, 50, 0.0), ("curved", 301, 173, 1.3)]
NAN_PAYLOAD = np.uint32(0x7FC12345)


@functools.lru_cache(maxsize=None)
def model_font(name):
    return FONTS[name]()


@functools.lru_cache(maxsize=None)
def lib_font(name):
    return font_of(model_font(name))


@functools.lru_cache(maxsize=None)
def model_atlas(name, ui_scale):
    return M.Atlas(model_font(name), ui_scale)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, want, tag):
    diff = bits(got) != bits(want)
    assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@functools.lru_cache(maxsize=None)
def background(W, H):
    """a picture of finite values in 0 .. 1 (read-only); a NaN with a payload in the bottom right pixel, right of xr and
    below yb, which no readout of the cases reaches"""
    img = np.random.default_rng(W * 4099 + H).uniform(0.0, 1.0, (H, W, 4)).astype(f32)
    img.view(np.uint32)[H - 1, W - 1, 2] = NAN_PAYLOAD
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def host_frame(name, W, H, ui_scale, value_index):
    """the host face's picture of VALUES[value_index] over background(W, H) (read-only, shared)"""
    out = P.readout_frame(lib_font(name), VALUES[value_index], background(W, H), ui_scale)
    out.setflags(write=False)
    return out


def compare(got, want, drawn, base, tag):
    """no differing bit; outside `drawn` the picture keeps the bits of `base`, the NaN's payload included"""
    same(got, want, tag)
    keep = ~drawn
    assert (bits(got)[keep] == bits(base)[keep]).all(), (tag, "a pixel outside the box and the cells changed")
    assert bits(got)[-1, -1, 2] == NAN_PAYLOAD and not drawn[-1, -1], tag
