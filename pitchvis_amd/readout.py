"""The viewer's tuning-drift readout, "Tuning drift: NNN" in a half-transparent box at the bottom right, drawn over the finished
picture in the Debugging display mode (include/pvq.h, "the readout", has the rule: text, colour, glyph atlas, layout, blend).  The
image is linear float32 [height][width][4], as ``OverlayBatch.frames`` leaves it; the present stage follows.  The library embeds no
font: bring a ``TextFont``.

* ``readout_text`` — a value's text and sRGB colour
* ``readout_layout``, ``readout_frame`` — what the layout makes of a value; one picture on the host
* ``ReadoutBatch`` — many rows on the GPU (pvq_readout_batch_*), each row its own value read from device memory: the handle owns the
  glyph atlas, ``rows`` formats, lays out and draws.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .consumers import _f
from .raster import _checked
from .text import TextFont

PREFIX = "Tuning drift: "
CODEPOINTS = " -0123456789:NTadfginrtu"   # every codepoint the stage can emit, in the atlas's order


def readout_text(value: float) -> Tuple[str, Tuple[float, float, float]]:
    """The value text (Rust's ``format!("{:>3.0}", value.round())``) and its sRGB colour"""
    L = _lib.load()
    text, rgb = C.create_string_buffer(12), (C.c_float * 3)()
    _checked(L, L.pvq_readout_text(float(value), text, rgb))
    return text.value.decode("ascii"), tuple(rgb)


def readout_layout(font: TextFont, value: float, width: int, height: int, ui_scale: float = 0.0) -> dict:
    """A dict: the box ``xl xr yt yb``, ``text_width``, ``font_px``, ``baseline``, ``baseline_row``, ``text`` (the whole string),
    per glyph slot ``origin_x`` and the placed cell ``cells`` as (x0, y0, w, h) on the image (not clipped), and the value text's
    colour ``value_srgb``, ``value_linear`` (float32 [3])"""
    L = _lib.load()
    o = _lib.CReadoutLayout()
    _checked(L, L.pvq_readout_layout_query(font._h, float(value), int(width), int(height), float(ui_scale), C.byref(o)))
    n = o.n_slots
    d = {k: getattr(o, k) for k in ("xl", "xr", "yt", "yb", "text_width", "font_px", "baseline", "baseline_row")}
    d.update(text=o.text.decode("ascii"), origin_x=list(o.origin_x[:n]),
             cells=[(o.cell_x0[s], o.cell_y0[s], o.cell_w[s], o.cell_h[s]) for s in range(n)],
             value_srgb=np.array(o.value_srgb[:], np.float32), value_linear=np.array(o.value_linear[:], np.float32))
    return d


def readout_frame(font: TextFont, value: float, image, ui_scale: float = 0.0) -> np.ndarray:
    """``image`` [height][width][4] with the readout of ``value`` blended over it (a new array)"""
    L = _lib.load()
    img = np.array(image, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image [height][width][4]")
    _checked(L, L.pvq_readout_frame(font._h, float(value), img.shape[1], img.shape[0], float(ui_scale), _f(img)))
    return img


class ReadoutBatch:
    """The readout for MANY rows on the GPU.  ``device=None``: a host-only handle (the argument checks work, ``atlas`` gives the host
    face's cells; ``rows`` raises: no CPU fallback).  The font is not needed after the handle is made."""

    def __init__(self, font: TextFont, width: int, height: int, ui_scale: float = 0.0, device: Optional[int] = 0):
        self._L = _lib.load()
        self.width, self.height, self.device = int(width), int(height), device
        self._h = C.c_void_p()
        _checked(self._L, self._L.pvq_readout_batch_create(-1 if device is None else int(device), font._h, self.width, self.height, float(ui_scale),
                                                           C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_readout_batch_destroy(h)
            self._h = None

    def rows(self, values, image, stream=None):
        """Draw the readout of ``values`` (a contiguous float32 device tensor, one value a row: ``tuning_grid_inaccuracy`` as
        ``AnalysisBatch`` filled it, any shape) over as many pictures, ``image`` a contiguous float32 device tensor
        [...][height][width][4], in place.  Returns the image.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        n_rows = int(values.numel())
        if not values.is_contiguous() or values.element_size() != 4 or not values.is_floating_point():
            raise ValueError("values must be a contiguous float32 tensor")
        if image.numel() != n_rows * self.height * self.width * 4 or not image.is_contiguous() or image.element_size() != 4:
            raise ValueError(f"image must be a contiguous float32 tensor of {n_rows} rows [{self.height}][{self.width}][4]")
        _checked(self._L, self._L.pvq_readout_batch_rows_device(self._h, n_rows, _ptr(values), _ptr(image), _stream_handle(stream)))
        return image

    def atlas(self, codepoint):
        """A codepoint's cell: (x0, y0, advance, coverage float32 [h][w]) — the cell's first column and row relative to (origin
        column, baseline row), the advance in pixels (synchronises)"""
        cp = ord(codepoint) if isinstance(codepoint, str) else int(codepoint)
        x0, y0, w, h, adv = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_float()
        _checked(self._L, self._L.pvq_readout_batch_get_atlas(self._h, cp, C.byref(x0), C.byref(y0), C.byref(w), C.byref(h), C.byref(adv), 0, None))
        out = np.zeros((h.value, w.value), np.float32)
        if out.size:
            _checked(self._L, self._L.pvq_readout_batch_get_atlas(self._h, cp, None, None, None, None, None, out.size, _f(out)))
        return x0.value, y0.value, adv.value, out
