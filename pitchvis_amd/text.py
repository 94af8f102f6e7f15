"""The viewer's twelve pitch-name labels, drawn from font outlines over the pitch balls and under the overlay (include/pvq.h, "the
text", has the rule: layout, exact-area coverage at output resolution, blend).  The image is linear float32 [height][width][4], as
``backdrop_frame`` / ``raster_frame(background=...)`` leave it.  The library embeds no font: bring one (the viewer's is DejaVuSans).

* ``TextFont`` — ``from_file`` / ``from_bytes`` (TrueType, simple glyphs) or ``from_outlines`` (the same data as arrays)
* ``TextLabel``, ``pitch_name_labels`` — a label; the reference's twelve
* ``text_layout``, ``text_frame`` — what the layout makes of labels; one picture on the host
* ``TextBatch`` — many rows on the GPU (pvq_text_batch_*): the handle owns the labels' coverage layer, ``rows`` blends it over
  every row's picture.  The caller runs it in the Full and Performance visuals modes only, after the balls and before the overlay.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .consumers import _f
from .raster import _checked

FONT_PX, SCALE = 40.0, 0.02   # setup.rs:394, :412
MAX_LABELS, MAX_CODEPOINTS = 64, 8
_bp, _up = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


def _u(a):
    return a.ctypes.data_as(_up)


def _b(a):
    return a.ctypes.data_as(_bp)


@dataclass
class TextLabel:
    """``text`` (1 .. 8 codepoints) centred on (``x``, ``y``) in world units; ``scale`` world units per font pixel; ``rgb`` sRGB"""
    text: str
    x: float
    y: float
    font_px: float = FONT_PX
    scale: float = SCALE
    rgb: Tuple[float, float, float] = (1.0, 1.0, 1.0)


def _labels(labels: Sequence[TextLabel]):
    labels = list(labels)
    arr = (_lib.CTextLabel * max(len(labels), 1))()
    for o, lab in zip(arr, labels):
        raw = lab.text.encode("utf-8")
        if len(raw) > 35 or b"\0" in raw:
            raise ValueError("a label's text is 1 .. 8 codepoints")
        o.text, o.x, o.y, o.font_px, o.scale = raw, float(lab.x), float(lab.y), float(lab.font_px), float(lab.scale)
        rgb = [float(v) for v in lab.rgb]
        if len(rgb) != 3:
            raise ValueError("rgb holds three values")
        o.rgb[:] = rgb
    return arr, len(labels)


class TextFont:
    """Outlines and advances per codepoint, units per em, hhea ascent and descent.  Not to be used from two threads at once."""

    def __init__(self, handle):
        self._L = _lib.load()
        self._h = handle
        u, a, d = C.c_uint32(), C.c_float(), C.c_float()
        _checked(self._L, self._L.pvq_text_font_metrics(self._h, C.byref(u), C.byref(a), C.byref(d)))
        self.units_per_em, self.ascent, self.descent = u.value, a.value, d.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_text_font_destroy(h)
            self._h = None

    @classmethod
    def from_bytes(cls, data: bytes) -> "TextFont":
        """A TrueType font: simple glyphs, cmap format 4 or 12; hinting, kern and GPOS are not read"""
        L = _lib.load()
        buf = np.frombuffer(bytes(data), np.uint8)
        h = C.c_void_p()
        _checked(L, L.pvq_text_font_from_ttf(_b(buf) if buf.size else None, buf.size, C.byref(h)))
        return cls(h)

    @classmethod
    def from_file(cls, path) -> "TextFont":
        with open(path, "rb") as fh:
            return cls.from_bytes(fh.read())

    @classmethod
    def from_outlines(cls, glyphs: dict, units_per_em: int, ascent: float, descent: float) -> "TextFont":
        """``glyphs``: codepoint (int or one-character str) -> (advance, contour_ends, points [n][2], on_curve [n]), as ``glyph``
        returns them"""
        L = _lib.load()
        cps, adv, n_c, n_p, ends, pts, on = [], [], [], [], [], [], []
        for cp, (advance, contour_ends, points, on_curve) in glyphs.items():
            p = np.asarray(points, np.float32).reshape(-1, 2)
            o = np.asarray(on_curve, np.uint8).reshape(-1)
            e = np.asarray(contour_ends, np.int64).reshape(-1)
            if len(p) != len(o) or (e < 0).any():
                raise ValueError("a glyph's points and flags differ in length, or a contour end is negative")
            cps.append(ord(cp) if isinstance(cp, str) else int(cp))
            adv.append(float(advance))
            n_c.append(len(e))
            n_p.append(len(p))
            ends.append(e)
            pts.append(p)
            on.append(o)
        cat = lambda parts, dtype, shape: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(shape, dtype), dtype)
        cps, n_c, n_p = (np.asarray(v, np.uint32) for v in (cps, n_c, n_p))
        adv = np.asarray(adv, np.float32)
        ends, pts, on = cat(ends, np.uint32, (0,)), cat(pts, np.float32, (0, 2)), cat(on, np.uint8, (0,))
        h = C.c_void_p()
        _checked(L, L.pvq_text_font_from_outlines(len(cps), _u(cps), _f(adv), _u(n_c), _u(ends), _u(n_p), _f(pts), _b(on), int(units_per_em),
                                                  float(ascent), float(descent), C.byref(h)))
        return cls(h)

    def glyph(self, codepoint):
        """(advance, contour_ends uint32 [c], points float32 [n][2] in font units with y upwards, on_curve uint8 [n])"""
        cp = ord(codepoint) if isinstance(codepoint, str) else int(codepoint)
        a, nc, npts = C.c_float(), C.c_uint32(), C.c_uint32()
        _checked(self._L, self._L.pvq_text_font_glyph(self._h, cp, C.byref(a), C.byref(nc), C.byref(npts), 0, 0, None, None, None))
        ends, pts, on = np.zeros(nc.value, np.uint32), np.zeros((npts.value, 2), np.float32), np.zeros(npts.value, np.uint8)
        _checked(self._L, self._L.pvq_text_font_glyph(self._h, cp, None, None, None, nc.value, npts.value, _u(ends), _f(pts), _b(on)))
        return a.value, ends, pts, on


def pitch_name_labels(octaves: int, colors=None):
    """The reference's twelve labels (setup.rs:386-416) for a range of ``octaves``; ``colors`` 12 RGB triples, None: the palette"""
    L = _lib.load()
    pal = None
    if colors is not None:
        pal = np.ascontiguousarray(colors, np.float32)
        if pal.shape != (12, 3):
            raise ValueError("colors: 12 RGB triples")
    arr = (_lib.CTextLabel * 12)()
    _checked(L, L.pvq_text_pitch_labels(int(octaves), _f(pal) if pal is not None else None, arr))
    return [TextLabel(o.text.decode("utf-8"), o.x, o.y, o.font_px, o.scale, tuple(o.rgb)) for o in arr]


def text_layout(font: TextFont, labels: Sequence[TextLabel], width: int, height: int, viewport_height: float = 0.0):
    """Per label a dict: ``on_image``, the pixel box ``x0 y0 x1 y1`` (first and last column and row), ``n_segments``, ``n_tiles``,
    ``tiles`` (row-major numbers of the 16 x 16 tiles the box meets) and the first glyph's origin ``origin_x``, ``baseline_y`` in
    output pixels"""
    L = _lib.load()
    arr, n = _labels(labels)
    out = (_lib.CTextLayout * max(n, 1))()
    _checked(L, L.pvq_text_layout_query(font._h, arr, n, int(width), int(height), float(viewport_height), out))
    tiles_x = (int(width) + 15) // 16
    res = []
    for o in out[:n]:
        d = {k: getattr(o, k) for k, _ in _lib.CTextLayout._fields_}
        d["on_image"] = bool(o.on_image)
        d["tiles"] = [ty * tiles_x + tx for ty in range(o.y0 // 16, o.y1 // 16 + 1) for tx in range(o.x0 // 16, o.x1 // 16 + 1)] if o.on_image else []
        res.append(d)
    return res


def text_frame(font: TextFont, labels: Sequence[TextLabel], image=None, *, width: Optional[int] = None, height: Optional[int] = None,
               viewport_height: float = 0.0, coverage: bool = False):
    """``image`` [height][width][4] with the labels blended over it in label order (a new array).  ``coverage=True``: also every
    label's coverage, float32 [n][height][width] — returned alone when ``image`` is None and ``width``, ``height`` are given."""
    L = _lib.load()
    img = None
    if image is not None:
        img = np.array(image, np.float32)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError("image [height][width][4]")
        height, width = img.shape[:2]
    elif width is None or height is None or not coverage:
        raise ValueError("an image, or width and height with coverage=True")
    arr, n = _labels(labels)
    cov = np.zeros((n, int(height), int(width)), np.float32) if coverage else None
    _checked(L, L.pvq_text_frame(font._h, arr, n, int(width), int(height), float(viewport_height), _f(img) if img is not None else None,
                                 _f(cov) if cov is not None else None))
    if img is None:
        return cov
    return (img, cov) if coverage else img


class TextBatch:
    """The labels for MANY rows on the GPU.  ``device=None``: a host-only handle (the argument checks work; the device calls raise:
    no CPU fallback).  The font is not needed after the handle is made."""

    def __init__(self, font: TextFont, labels: Sequence[TextLabel], width: int, height: int, viewport_height: float = 0.0,
                 device: Optional[int] = 0):
        self._L = _lib.load()
        self.width, self.height, self.device = int(width), int(height), device
        arr, self.n_labels = _labels(labels)
        self._h = C.c_void_p()
        _checked(self._L, self._L.pvq_text_batch_create(-1 if device is None else int(device), font._h, arr, self.n_labels, float(viewport_height),
                                                        self.width, self.height, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_text_batch_destroy(h)
            self._h = None

    def rows(self, n_rows: int, image, stream=None):
        """Blend the labels over ``n_rows`` pictures, ``image`` a contiguous float32 device tensor [n_rows][height][width][4] (any
        leading shape with that many rows), in place.  Returns the image.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        n = int(n_rows) * self.height * self.width * 4
        if hasattr(image, "numel") and (image.numel() != n or not image.is_contiguous() or image.element_size() != 4):
            raise ValueError(f"image must be a contiguous float32 tensor of {int(n_rows)} rows [{self.height}][{self.width}][4]")
        _checked(self._L, self._L.pvq_text_batch_rows_device(self._h, int(n_rows), _ptr(image), _stream_handle(stream)))
        return image

    def coverage(self, label: Optional[int] = None) -> np.ndarray:
        """The coverage layer as a full float32 [height][width] image: one label's, or (None) the largest over the labels
        (synchronises)"""
        out = np.zeros((self.height, self.width), np.float32)
        _checked(self._L, self._L.pvq_text_batch_get_coverage(self._h, -1 if label is None else int(label), _f(out)))
        return out
