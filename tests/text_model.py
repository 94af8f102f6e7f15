"""An independent NumPy float64 restatement of the text stage's rule (include/pvq.h, "the text"), written from the rule's statement:
implied points, layout, the camera, curves flattened to 1e-4 pixel, exact signed-area coverage with min(|.|, 1), colour and blend.

The coverage is computed another way than the library's per-pixel integral: every chord is cut where it crosses a pixel boundary,
each piece adds its signed trapezoid to the one pixel it lies in and its full height to every pixel left of it in that row (the
accumulation of scan-line font rasterisers), so an error of the library's clipping or piecewise integral shows."""
import numpy as np

VIEWPORT_HEIGHT = float(np.float32(38.0) * np.float32(0.41421357))   # setup.rs:361, as the raster section takes it
LINE_HEIGHT = float(np.float32(1.2))
FLATTEN = 1e-4
COLORS = np.asarray([[0.85, 0.36, 0.36], [0.01, 0.52, 0.71], [0.97, 0.76, 0.05], [0.45, 0.34, 0.63], [0.47, 0.77, 0.22], [0.78, 0.32, 0.52],
                     [0.00, 0.64, 0.56], [0.95, 0.54, 0.23], [0.30, 0.37, 0.64], [1.00, 0.96, 0.03], [0.57, 0.30, 0.55], [0.12, 0.71, 0.34]], np.float32)
PITCH_NAMES = ["C", "C♯", "D", "E♭", "E", "F", "F♯", "G", "A♭", "A", "B♭", "B"]


def srgb_to_linear(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def contours_of(glyph):
    """a glyph (advance, contour_ends, points, on_curve) -> list of (points [m][2], on [m])"""
    _, ends, pts, on = glyph
    out, first = [], 0
    for e in ends:
        out.append((np.asarray(pts[first:e + 1], np.float64), np.asarray(on[first:e + 1], bool)))
        first = int(e) + 1
    return out


def polyline(pts, on, tol=FLATTEN):
    """a closed contour's chords as a closed polyline [k][2]; pts already in the space where tol is measured"""
    m = len(pts)
    if m < 2:
        return np.zeros((0, 2))
    full = []
    for k in range(m):
        full.append((pts[k], on[k]))
        nx = (k + 1) % m
        if not on[k] and not on[nx]:
            full.append(((pts[k] + pts[nx]) / 2.0, True))
    start = next(k for k, (_, o) in enumerate(full) if o)
    full = full[start:] + full[:start] + [full[start]]
    out, k = [full[0][0]], 1
    while k < len(full):
        p, o = full[k]
        if o:
            out.append(p)
            k += 1
            continue
        p0, p2 = out[-1], full[k + 1][0]
        n = max(1, int(np.ceil(np.sqrt(np.linalg.norm(p0 - 2.0 * p + p2) / (4.0 * tol)))))
        t = (np.arange(1, n + 1) / n)[:, None]
        out.extend((1 - t) ** 2 * p0 + 2 * (1 - t) * t * p + t ** 2 * p2)
        k += 2
    return np.asarray(out)


def layout(font, label, W, H, viewport_height=0.0):
    """font: dict with glyphs {codepoint: glyph}, units_per_em, ascent, descent.  Returns (origin pixel (x, y), list of closed
    polylines in output pixels, flattened to FLATTEN)"""
    vh = float(np.float32(viewport_height)) if viewport_height else VIEWPORT_HEIGHT
    s = float(np.float32(vh) / np.float32(H))
    px, scale = float(np.float32(label.font_px)), float(np.float32(label.scale))
    x, y = float(np.float32(label.x)), float(np.float32(label.y))
    k = px / font["units_per_em"]
    glyphs = [font["glyphs"][ord(c)] for c in label.text]
    width, line = sum(g[0] for g in glyphs) * k, LINE_HEIGHT * px
    asc, desc = font["ascent"] * k, font["descent"] * k
    left, top = -width / 2.0, -line / 2.0
    baseline = top + (line - (asc - desc)) / 2.0 + asc

    def to_pixel(p):   # p [.., 2] font pixels, y downwards
        wx, wy = x + p[..., 0] * scale, y - p[..., 1] * scale
        return np.stack([wx / s + W / 2.0, H / 2.0 - wy / s], -1)

    polys, pen = [], 0.0
    for g in glyphs:
        for pts, on in contours_of(g):
            q = np.stack([left + pen + pts[:, 0] * k, baseline - pts[:, 1] * k], -1)
            poly = polyline(to_pixel(q), on)
            if len(poly):
                polys.append(poly)
        pen += g[0] * k
    return to_pixel(np.asarray([left, baseline])), polys


def coverage(polys, W, H):
    """exact area of the outline inside every pixel square, by accumulation: [H][W] float64 in 0 .. 1"""
    area, full = np.zeros((H, W)), np.zeros((H, W + 1))
    for poly in polys:
        a, b = poly[:-1], poly[1:]
        # cut every chord at the pixel boundaries it crosses: parameters of the integer x and y between its ends
        pieces_a, pieces_b = [], []
        same = (np.floor(a) == np.floor(b)).all(1) | ((a == b).all(1))
        pieces_a.append(a[same])
        pieces_b.append(b[same])
        for p, q in zip(a[~same], b[~same]):
            ts = [0.0, 1.0]
            for c in (0, 1):
                lo, hi = sorted((p[c], q[c]))
                for v in range(int(np.floor(lo)) + 1, int(np.ceil(hi))):
                    ts.append((v - p[c]) / (q[c] - p[c]))
            ts = np.unique(np.clip(ts, 0.0, 1.0))[:, None]
            cut = p + ts * (q - p)
            pieces_a.append(cut[:-1])
            pieces_b.append(cut[1:])
        a, b = np.concatenate(pieces_a), np.concatenate(pieces_b)
        mid = (a + b) / 2.0
        i, j = np.floor(mid[:, 0]).astype(np.int64), np.floor(mid[:, 1]).astype(np.int64)
        dy = b[:, 1] - a[:, 1]
        rows = (j >= 0) & (j < H) & (i >= 0) & (dy != 0.0)
        inside = rows & (i < W)
        np.add.at(area, (j[inside], i[inside]), dy[inside] * (mid[inside, 0] - i[inside]))
        np.add.at(full, (j[rows], np.minimum(i[rows], W)), dy[rows])
    left_of = np.cumsum(full[:, ::-1], 1)[:, ::-1]          # inclusive sum over i' >= i
    total = area + left_of[:, 1:]                           # pieces strictly right of the pixel count in full
    return np.minimum(np.abs(total), 1.0)


def label_coverage(font, label, W, H, viewport_height=0.0):
    return coverage(layout(font, label, W, H, viewport_height)[1], W, H)


def frame(font, labels, image, viewport_height=0.0, coverages=None):
    """the labels over image [H][W][4] in label order, float64; also the coverages [n][H][W] (computed unless given)"""
    img = np.array(image, np.float64)
    H, W = img.shape[:2]
    covs = []
    for n, lab in enumerate(labels):
        c = label_coverage(font, lab, W, H, viewport_height) if coverages is None else coverages[n]
        covs.append(c)
        lin = srgb_to_linear(np.asarray(lab.rgb, np.float32))
        a = c[..., None]
        img[..., :3] = np.where(a > 0, lin * a + img[..., :3] * (1 - a), img[..., :3])
        img[..., 3] = np.where(c > 0, c + img[..., 3] * (1 - c), img[..., 3])
    return img, np.asarray(covs)


def spiral_point(bpo, x):
    """util.rs:9-20 in float64"""
    radius = 2.0 * (0.3 + (x / bpo) ** 0.75)
    angle = (x + bpo) / bpo * 2.0 * np.pi
    return -np.cos(angle) * radius, np.sin(angle) * radius


def spiral_point_f32(bpo, i):
    """the same in f32, operation for operation, the libm calls in double and rounded once (the scene section's convention)"""
    f32 = np.float32
    b, x = f32(bpo), f32(i)
    radius = f32(2.0) * (f32(0.3) + f32(np.float64(x / b) ** 0.75))
    angle = (x + b) / b * f32(2.0) * f32(np.pi)
    return f32(-1.0) * f32(np.cos(np.float64(angle))) * radius, f32(np.sin(np.float64(angle))) * radius
