"""A NumPy float32 restatement of the readout stage's rule (include/pvq.h, "the readout"), written from the statement of the rule and
pitchvis_viewer/src/app/common.rs:348-432, not from the C++: the value's text, its colour, the glyph atlas, the layout of a row and
the blend.  Every formula is f32 in the order the rule gives, without fused operations (NumPy fuses none), so the library's host
face must give these bits.  The coverage of a pixel is the text section's rule restated for whole cells at once.

`Rule` carries the five switches that tests/test_readout.py turns to show that its cases tell a wrong rule from the right one."""
import math
from dataclasses import dataclass

import numpy as np

f32 = np.float32
PREFIX = "Tuning drift: "
CODEPOINTS = " -0123456789:NTadfginrtu"
CLAMP = 2147483520          # the largest f32 below 2^31
TOL = 1.0 / 64.0            # flattening tolerance, output pixels
LINE_HEIGHT = f32(1.2)


@dataclass(frozen=True)
class Rule:
    half_even: bool = False        # wrong: round half to even instead of half away from zero
    drop_minus_zero: bool = False  # wrong: "-0" printed as "0"
    pairwise_pen: bool = False     # wrong: the pen summed pairwise instead of as a left fold
    truncate_origin: bool = False  # wrong: an origin by truncation instead of floorf(x + 0.5f)
    closed_box: bool = False       # wrong: the box closed on the right and at the bottom


RIGHT = Rule()


# ---- the text and its colour ------------------------------------------------------------------------------------------------------
def rounded(v, rule=RIGHT):
    """f32::round of an f32: half away from zero, the sign kept (so -0.4 gives -0.0)"""
    v = float(f32(v))
    if math.isnan(v) or math.isinf(v):
        return f32(v)
    if rule.half_even:
        return f32(math.copysign(float(round(abs(v))), v))
    return f32(math.copysign(math.floor(abs(v) + 0.5), v))   # exact in double for every f32


def value_text(v, rule=RIGHT):
    r = rounded(v, rule)
    if np.isnan(r):
        return "NaN"
    if np.isinf(r):
        return "inf" if r > 0 else "-inf"
    negative = bool(np.signbit(r)) and not (rule.drop_minus_zero and r == 0)
    digits = str(min(int(abs(float(r))), CLAMP))
    return (("-" if negative else "") + digits).rjust(3)


def value_srgb(v, rule=RIGHT):
    """common.rs:404-413 in f32"""
    a = np.abs(rounded(v, rule))
    if a <= f32(10):
        rgb = (f32(0), f32(1), f32(0))
    elif a <= f32(20):
        rgb = ((a - f32(10)) / (f32(20) - f32(10)), f32(1), f32(0))
    elif a <= f32(30):
        rgb = (f32(1), f32(1) - (a - f32(20)) / (f32(30) - f32(20)), f32(0))
    else:
        rgb = (f32(1), f32(0), f32(0))
    return np.asarray(rgb, f32)


def srgb_to_linear(x):
    """the scene section's curve, one channel: f32, the power taken in double and rounded once"""
    x = f32(x)
    if x <= f32(0.04045):
        return x / f32(12.92)
    return f32(np.float64((x + f32(0.055)) / f32(1.055)) ** np.float64(f32(2.4)))


# ---- the atlas --------------------------------------------------------------------------------------------------------------------
def chords_of(glyph, k):
    """a glyph (advance, contour_ends, points, on_curve) as directed chords [n][4] of f32: origin at (0, 0), y downwards, a point
    (gx, gy) at (gx k, -gy k) in double; implied points; a quadratic in ceil(sqrt(|p0 - 2 p1 + p2| / (4 tol))) chords of equal
    parameter; the ends rounded once to f32"""
    _, ends, pts, on = glyph
    out, first = [], 0
    for e in ends:
        p = [(float(x) * k, -(float(y) * k)) for x, y in pts[first:int(e) + 1]]
        o = [bool(v) for v in on[first:int(e) + 1]]
        first = int(e) + 1
        m = len(p)
        if m < 2:
            continue
        full = []
        for i in range(m):
            full.append((p[i], o[i]))
            nx = (i + 1) % m
            if not o[i] and not o[nx]:
                full.append(((0.5 * (p[i][0] + p[nx][0]), 0.5 * (p[i][1] + p[nx][1])), True))
        start = next(i for i, (_, flag) in enumerate(full) if flag)
        full = full[start:] + full[:start] + [full[start]]
        poly, i = [full[0][0]], 1
        while i < len(full):
            a, flag = full[i]
            if flag:
                poly.append(a)
                i += 1
                continue
            p0, p2 = poly[-1], full[i + 1][0]
            bend = math.hypot(p0[0] - 2.0 * a[0] + p2[0], p0[1] - 2.0 * a[1] + p2[1])
            n = max(1, min(int(math.ceil(math.sqrt(bend / (4.0 * TOL)))), 4096))
            for c in range(1, n):
                t = c / n
                u = 1.0 - t
                poly.append((u * u * p0[0] + 2.0 * u * t * a[0] + t * t * p2[0], u * u * p0[1] + 2.0 * u * t * a[1] + t * t * p2[1]))
            poly.append(p2)
            i += 2
        out.extend((f32(a[0]), f32(a[1]), f32(b[0]), f32(b[1])) for a, b in zip(poly[:-1], poly[1:]))
    return np.asarray(out, f32).reshape(-1, 4)


def chord_area(s, X, Y):
    """The text section's integral for one chord over the pixels (X, Y) (f32 arrays): the chord clipped to the rows Y .. Y + 1,
    clamp(x(y) - X, 0, 1) integrated over y, positive towards larger y"""
    x0, y0, x1, y1 = (f32(v) for v in s)
    zero, one, half = f32(0), f32(1), f32(0.5)
    if y0 == y1:
        return np.zeros_like(X)
    down = y1 > y0
    xa, ya, xb, yb = (x0, y0, x1, y1) if down else (x1, y1, x0, y0)
    with np.errstate(all="ignore"):
        top = Y + one
        ylo, yhi = np.where(ya > Y, ya, Y), np.where(yb < top, yb, top)
        slope = (xb - xa) / (yb - ya)
        xlo = np.where(ya >= Y, xa, xa + (Y - ya) * slope)
        xhi = np.where(yb <= top, xb, xa + (top - ya) * slope)
        h = yhi - ylo
        ua, ub = xlo - X, xhi - X
        ua, ub = np.where(ua > ub, ub, ua), np.where(ua > ub, ua, ub)
        d = ub - ua
        t0 = np.where(ua < zero, (zero - ua) / d, zero)
        t1 = np.where(ub > one, (one - ua) / d, one)
        c0, c1 = np.where(ua < zero, zero, ua), np.where(ub > one, one, ub)
        crossing = (t1 - t0) * (half * (c0 + c1)) + (one - t1)
        mean = np.where(ua >= one, one, np.where((ua >= zero) & (ub <= one), half * (ua + ub), crossing))
        area = (h * mean).astype(f32)
        area = area if down else -area
        return np.where((ylo < yhi) & ~(ub <= zero), area, zero).astype(f32)


class Atlas:
    """every codepoint's cell for a font (dict: glyphs, units_per_em, ascent, descent) at a UI scale"""

    def __init__(self, font, ui_scale=0.0):
        scale = f32(1) if ui_scale == 0 else f32(ui_scale)
        self.F = f32(16) * scale
        k = float(self.F) / font["units_per_em"]
        line, asc, desc = float(LINE_HEIGHT) * float(self.F), font["ascent"] * k, font["descent"] * k
        self.baseline = f32(0.5 * (line - (asc - desc)) + asc)
        self.advance, self.cells = {}, {}
        for ch in CODEPOINTS:
            glyph = font["glyphs"][ord(ch)]
            self.advance[ch] = f32(float(glyph[0]) * k)
            chords = chords_of(glyph, k)
            if len(chords) == 0:
                self.cells[ch] = (0, 0, np.zeros((0, 0), f32))
                continue
            lo_x, hi_x = float(chords[:, [0, 2]].min()), float(chords[:, [0, 2]].max())
            lo_y, hi_y = float(chords[:, [1, 3]].min()), float(chords[:, [1, 3]].max())
            chords = chords[chords[:, 1] != chords[:, 3]]
            if not (lo_x < hi_x and lo_y < hi_y) or len(chords) == 0:
                self.cells[ch] = (0, 0, np.zeros((0, 0), f32))
                continue
            x0, y0 = math.floor(lo_x), math.floor(lo_y)
            w, h = math.ceil(hi_x) - x0, math.ceil(hi_y) - y0
            X, Y = np.meshgrid(np.arange(x0, x0 + w).astype(f32), np.arange(y0, y0 + h).astype(f32))
            total = np.zeros((h, w), f32)
            for s in chords:
                total = total + chord_area(s, X, Y)
            a = np.abs(total)
            self.cells[ch] = (x0, y0, np.where(a < f32(1), np.where(a > f32(0), a, f32(0)), f32(1)).astype(f32))


# ---- a row ------------------------------------------------------------------------------------------------------------------------
def pen_positions(advances, rule=RIGHT):
    """p_0 .. p_n: the left fold in f32"""
    pens = [f32(0)]
    for a in advances:
        pens.append(pens[-1] + a)
    if rule.pairwise_pen:   # the total as a tree of pairs: the same sum in exact arithmetic, other roundings in f32
        level = list(advances)
        while len(level) > 1:
            level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        pens[-1] = level[0]
    return pens


def layout(atlas, v, W, H, rule=RIGHT):
    text = PREFIX + value_text(v, rule)
    pens = pen_positions([atlas.advance[c] for c in text], rule)
    Wf, Hf, wt = f32(W), f32(H), pens[-1]
    xr = Wf - f32(0.01) * Wf
    yb = Hf - f32(0.01) * Hf
    xl = xr - wt
    yt = yb - LINE_HEIGHT * atlas.F
    place = (lambda x: int(np.trunc(x))) if rule.truncate_origin else (lambda x: int(np.floor(x + f32(0.5))))
    srgb = value_srgb(v, rule)
    return {"text": text, "xl": xl, "xr": xr, "yt": yt, "yb": yb, "text_width": wt, "origin_x": [place(xl + p) for p in pens[:-1]],
            "baseline_row": int(np.floor(yt + atlas.baseline + f32(0.5))), "value_srgb": srgb,
            "value_linear": np.asarray([srgb_to_linear(c) for c in srgb], f32)}


def blend(src_rgb, alpha, dst):
    """the raster section's blend of (src_rgb, alpha) over dst [..][4], f32"""
    alpha = np.asarray(alpha, f32)
    k = f32(1) - alpha
    out = np.empty_like(dst)
    for c in range(3):
        out[..., c] = f32(src_rgb[c]) * alpha + dst[..., c] * k
    out[..., 3] = alpha + dst[..., 3] * k
    return out


def frame(atlas, v, image, rule=RIGHT):
    """(the picture, the mask of pixels the box or a glyph's non-zero coverage drew on)"""
    img = np.array(image, f32)
    H, W = img.shape[:2]
    lay = layout(atlas, v, W, H, rule)
    cx, cy = np.arange(W).astype(f32) + f32(0.5), np.arange(H).astype(f32) + f32(0.5)
    in_x = (cx >= lay["xl"]) & ((cx <= lay["xr"]) if rule.closed_box else (cx < lay["xr"]))
    in_y = (cy >= lay["yt"]) & ((cy <= lay["yb"]) if rule.closed_box else (cy < lay["yb"]))
    box = in_y[:, None] & in_x[None, :]
    img[box] = blend((0.0, 0.0, 0.0), f32(0.5), img[box])
    drawn = box.copy()
    white = np.ones(3, f32)
    for slot, ch in enumerate(lay["text"]):
        x0, y0, cov = atlas.cells[ch]
        x0, y0 = x0 + lay["origin_x"][slot], y0 + lay["baseline_row"]
        h, w = cov.shape
        i0, i1, j0, j1 = max(x0, 0), min(x0 + w, W), max(y0, 0), min(y0 + h, H)
        if i0 >= i1 or j0 >= j1:
            continue
        c = cov[j0 - y0:j1 - y0, i0 - x0:i1 - x0]
        part = img[j0:j1, i0:i1]
        mixed = blend(white if slot < len(PREFIX) else lay["value_linear"], c, part)
        part[c != 0] = mixed[c != 0]
        drawn[j0:j1, i0:i1] |= c != 0
    return img, drawn
