"""Shared by tests/test_text.py, tests/test_text_gpu.py and tests/test_sanitize_text.py: the glyph fixture, synthetic outline
fonts whose font unit is one output pixel, the crafted cases, a TrueType file built from the fixture, and `compare`."""
import os

import numpy as np

import pitchvis_amd as P
import text_model as M

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dejavu_pitch_glyphs.npz")
TOL = 1.0 / 64.0                       # the library's flattening tolerance, output pixels
BAR_LIMIT = 2.0 * np.sqrt(2.0) * TOL   # above this the design fails (an edge through a pixel errs by about tol * sqrt 2)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, want, tag):
    diff = bits(got) != bits(want)
    assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def fixture():
    """the nine DejaVuSans glyphs as a model font: {glyphs: {codepoint: (advance, ends, points, on)}, units_per_em, ascent, descent}"""
    d = np.load(GOLDEN)
    glyphs, c_at, p_at = {}, 0, 0
    for g, cp in enumerate(d["codepoints"]):
        nc, npts = int(d["n_contours"][g]), int(d["n_points"][g])
        glyphs[int(cp)] = (float(d["advances"][g]), d["contour_ends"][c_at:c_at + nc].copy(), d["points"][p_at:p_at + npts].copy(),
                           d["on_curve"][p_at:p_at + npts].copy())
        c_at, p_at = c_at + nc, p_at + npts
    return {"glyphs": glyphs, "units_per_em": int(d["units_per_em"]), "ascent": float(d["ascent"]), "descent": float(d["descent"])}


def font_of(model_font):
    return P.TextFont.from_outlines(model_font["glyphs"], model_font["units_per_em"], model_font["ascent"], model_font["descent"])


# ---- synthetic fonts: 64 units per em at font_px 64, scale 1 and viewport_height == height make a font unit one output pixel; with
# ascent 32 and descent -32 the baseline passes through the label's y, so a glyph point (gx, gy) of a one-glyph label at (x, y) lies
# at pixel (W / 2 + x - advance / 2 + gx, H / 2 - y - gy), all of it exact in f32
def glyph(advance, *contours):
    pts = [p for c in contours for p in c]
    ends = np.cumsum([len(c) for c in contours]) - 1
    return (float(advance), ends.astype(np.uint32), np.asarray([p[:2] for p in pts], f32).reshape(-1, 2),
            np.asarray([p[2] if len(p) > 2 else 1 for p in pts], np.uint8))


def rect(x0, y0, x1, y1, reverse=False):
    c = [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]
    return c[::-1] if reverse else c


def synthetic(glyphs):
    return {"glyphs": {ord(k): v for k, v in glyphs.items()}, "units_per_em": 64, "ascent": 32.0, "descent": -32.0}


SYNTHETIC = synthetic({
    "s": glyph(4, rect(0, 0, 4, 4)),                                        # a square
    "r": glyph(4, rect(0, 0, 4, 4, reverse=True)),                          # the same, wound the other way
    "t": glyph(6, [(0, 0), (6, 0), (0, 3)]),                                # a right triangle, hypotenuse of slope -1 / 2
    "o": glyph(6, rect(0, 0, 6, 6), rect(2, 2, 4, 4, reverse=True)),        # a square with an opposite-wound hole
    "d": glyph(6, rect(0, 0, 4, 4), rect(2, 2, 6, 6)),                      # two same-wound squares that overlap
    "h": glyph(4, [(0, 0), (4, 0)]),                                        # horizontal only: nothing
    "w": glyph(9, rect(0, 0, 2, 5)),                                        # a wide advance, for the pen
    "q": glyph(8, [(0, 0), (4, 8, 0), (8, 0)]),                             # a parabola over a chord: one off-curve point
    "e": glyph(8, [(0, 4, 0), (4, 8, 0), (8, 4, 0), (4, 0, 0)]),            # off-curve points only: every on-curve point implied
})


def unit_label(text, x=0.0, y=0.0, rgb=(1.0, 1.0, 1.0)):
    return P.TextLabel(text, x, y, 64.0, 1.0, rgb)


def rect_coverage(W, H, x0, y0, x1, y1):
    """area of the pixel-space rectangle inside every pixel, exact for quarter-pixel coordinates"""
    i, j = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    ox = np.clip(np.minimum(i + 1, x1) - np.maximum(i, x0), 0, None)
    oy = np.clip(np.minimum(j + 1, y1) - np.maximum(j, y0), 0, None)
    return oy[:, None] * ox[None, :]


def clip_area(poly, i, j):
    """area of a convex or concave simple polygon inside pixel (i, j): Sutherland-Hodgman against the four sides, then the shoelace"""
    pts = [np.asarray(p, np.float64) for p in poly]
    for axis, bound, keep_less in ((0, i, False), (0, i + 1, True), (1, j, False), (1, j + 1, True)):
        out = []
        for k in range(len(pts)):
            a, b = pts[k], pts[(k + 1) % len(pts)]
            ina = a[axis] <= bound if keep_less else a[axis] >= bound
            inb = b[axis] <= bound if keep_less else b[axis] >= bound
            if ina:
                out.append(a)
            if ina != inb:
                out.append(a + (bound - a[axis]) / (b[axis] - a[axis]) * (b - a))
        pts = out
        if not pts:
            return 0.0
    x, y = np.asarray(pts).T
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


# ---- the crafted cases of the host face against the model, and of the device against the host face
def pitch_labels(octaves=7):
    return P.pitch_name_labels(octaves)


def big_label():
    """one label whose em is 200 output pixels on a 301 x 173 image at the viewer's view"""
    s = float(f32(M.VIEWPORT_HEIGHT) / f32(173))
    return [P.TextLabel("B♭", 0.1, -0.05, 40.0, 200.0 * s / 40.0, (0.57, 0.30, 0.55))]


HOST_CASES = [("pitch", 64, 64, 0.0), ("pitch", 64, 64, 40.0), ("pitch", 256, 256, 0.0), ("pitch", 256, 256, 40.0), ("pitch", 301, 173, 0.0),
              ("pitch", 301, 173, 40.0), ("big", 301, 173, 0.0)]


def case_labels(kind):
    return pitch_labels() if kind == "pitch" else big_label()


def images(n, W, H, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, H, W, 4)).astype(f32)


def compare(got_cov, want_cov, bar, tag):
    """largest coverage difference, asserted against the bar"""
    err = float(np.abs(np.asarray(got_cov, np.float64) - want_cov).max())
    assert err <= bar, (tag, err, bar)
    return err


# ---- a TrueType file from the fixture's outlines (fontTools), point for point
def build_ttf(path, cmap_format=4, long_loca=False, composite=False):
    from array import array

    from fontTools.fontBuilder import FontBuilder
    from fontTools.ttLib.tables import ttProgram
    from fontTools.ttLib.tables._c_m_a_p import CmapSubtable
    from fontTools.ttLib.tables._g_l_y_f import Glyph, GlyphComponent, GlyphCoordinates

    fx = fixture()

    def simple(ends, pts, on):
        g = Glyph()
        g.numberOfContours = len(ends)
        g.endPtsOfContours = [int(e) for e in ends]
        g.coordinates = GlyphCoordinates([(int(x), int(y)) for x, y in pts])
        g.flags = array("B", [int(o) for o in on])
        g.program = ttProgram.Program()
        g.program.fromBytecode(b"\xb0\x00\x21" if len(ends) else b"")   # PUSHB[0] 0, POP: instructions the reader must skip
        return g

    names, glyphs, metrics, cmap = [".notdef"], {".notdef": simple([], [], [])}, {".notdef": (600, 0)}, {}
    if long_loca:   # a glyph large enough to push glyf past 128 KiB, where loca needs its long form
        n = 60000   # x swings by 6000 a point: two bytes each, so the glyph takes 180 KB or more
        names.append("filler")
        glyphs["filler"] = simple([n - 1], [(3000 if k & 1 else -3000, k % 2000 - 1000) for k in range(n)], [1] * n)
        metrics["filler"] = (600, 0)
    for cp, (adv, ends, pts, on) in fx["glyphs"].items():
        name = "uni%04X" % cp
        names.append(name)
        glyphs[name] = simple(ends, pts, on)
        metrics[name] = (int(adv), int(min(p[0] for p in pts)))
        cmap[cp] = name
    if composite:
        comp = GlyphComponent()
        comp.glyphName, comp.x, comp.y, comp.flags = "uni0043", 100, 0, 0x4
        g = Glyph()
        g.numberOfContours, g.components = -1, [comp]
        names.append("composite")
        glyphs["composite"], metrics["composite"], cmap[ord("Q")] = g, (1500, 0), "composite"
    fb = FontBuilder(fx["units_per_em"], isTTF=True)
    fb.setupGlyphOrder(names)
    fb.setupCharacterMap(cmap)
    fb.setupGlyf(glyphs)
    fb.setupHorizontalMetrics(metrics)
    fb.setupHorizontalHeader(ascent=int(fx["ascent"]), descent=int(fx["descent"]))
    fb.setupNameTable({"familyName": "PitchGlyphs", "styleName": "Regular"})
    fb.setupOS2()
    fb.setupPost()
    if cmap_format == 12:
        st = CmapSubtable.newSubtable(12)
        st.platformID, st.platEncID, st.language, st.cmap = 3, 10, 0, dict(cmap)
        fb.font["cmap"].tables = [st]
    fb.save(str(path))
    return fx
