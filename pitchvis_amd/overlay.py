"""What the viewer's debug picture draws in front of the pitch balls: the scrolling spectrogram quad and the twelve chroma boxes,
blended in place over a finished image (include/pvq.h, "the overlay", has the rule).  The image is linear float32
[height][width][4], as ``backdrop_frame`` / ``raster_frame(background=...)`` leave it.

* ``overlay_quad`` — the reference's quad; ``OverlayState`` — one stream's ring of spectrogram rows, kept literally as the
  viewer keeps its texture; ``overlay_frame`` — one frame on the host
* ``OverlayBatch`` — many streams on the GPU (pvq_overlay_batch_*), fed with what ``RenderBatch.rows_device`` leaves in device
  memory; the handle keeps every stream's last ``history_rows`` rows
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .consumers import _f
from .raster import _checked

HISTORY_ROWS = 200   # setup.rs:430
_bp, _up = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


def _b(a):
    return a.ctypes.data_as(_bp)


def _quad(quad):
    if quad is None:
        return None
    q = np.ascontiguousarray(quad, np.float32)
    if q.shape != (4,):
        raise ValueError("a quad is (cx, cy, ex, ey)")
    return q


def _palette(colors):
    if colors is None:
        return None
    pal = np.ascontiguousarray(colors, np.float32)
    if pal.shape != (12, 3):
        raise ValueError("colors: 12 RGB triples")
    return pal


def overlay_quad(n_bins: int, history_rows: int = HISTORY_ROWS) -> np.ndarray:
    """(cx, cy, ex, ey) of the viewer's spectrogram quad: centre, extent along x (time) and along y (frequency)"""
    L = _lib.load()
    out = np.empty(4, np.float32)
    _checked(L, L.pvq_overlay_quad(int(n_bins), int(history_rows), _f(out)))
    return out


class OverlayState:
    """One stream's spectrogram texture on the host: ``push`` a frame's row (``spectrogram_row``), then ``overlay_frame`` draws it"""

    def __init__(self, n_bins: int, history_rows: int = HISTORY_ROWS):
        self._L = _lib.load()
        self._h = C.c_void_p()
        _checked(self._L, self._L.pvq_overlay_state_create(int(n_bins), int(history_rows), C.byref(self._h)))
        self.n_bins, self.history_rows = int(n_bins), int(history_rows) or HISTORY_ROWS

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_overlay_state_destroy(h)
            self._h = None

    def push(self, row_rgba) -> None:
        row = np.ascontiguousarray(row_rgba, np.uint8)
        if row.shape != (self.n_bins, 4):
            raise ValueError("a row is uint8 [n_bins][4]")
        _checked(self._L, self._L.pvq_overlay_state_push(self._h, _b(row)))

    def texture(self):
        """(texture uint8 [history_rows][n_bins][4], write index) as they stand"""
        out = np.empty((self.history_rows, self.n_bins, 4), np.uint8)
        w = C.c_uint32()
        _checked(self._L, self._L.pvq_overlay_state_texture(self._h, _b(out), C.byref(w)))
        return out, w.value


def overlay_frame(image, state: Optional[OverlayState] = None, chroma=None, *, viewport_height: float = 0.0, ui_scale: float = 1.0, quad=None,
                  colors=None) -> np.ndarray:
    """``image`` [height][width][4] with the quad of ``state`` (the frame pushed last) and the boxes of ``chroma`` (twelve
    strengths, ``chroma_row``) blended over it (a new array).  ``quad`` None: the reference's."""
    L = _lib.load()
    img = np.array(image, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image [height][width][4]")
    q, pal = _quad(quad), _palette(colors)
    c = None
    if chroma is not None:
        c = np.ascontiguousarray(chroma, np.float32)
        if c.shape != (12,):
            raise ValueError("chroma holds twelve strengths")
    _checked(L, L.pvq_overlay_frame(state._h if state is not None else None, img.shape[1], img.shape[0], float(viewport_height), float(ui_scale),
                                    _f(q) if q is not None else None, _f(c) if c is not None else None, _f(pal) if pal is not None else None,
                                    _f(img)))
    return img


class OverlayBatch:
    """The overlay for MANY streams on the GPU.  ``device=None``: a host-only handle (the argument checks work; the device calls
    raise: no CPU fallback)."""

    def __init__(self, range, n_streams: int, width: int, height: int, history_rows: int = HISTORY_ROWS, viewport_height: float = 0.0,
                 ui_scale: float = 1.0, quad=None, colors=None, device: Optional[int] = 0):
        self._L = _lib.load()
        self.range, self.n_streams, self.device = range, int(n_streams), device
        self.width, self.height = int(width), int(height)
        self.n_bins = range.octaves * range.buckets_per_octave
        self.history_rows = int(history_rows) or HISTORY_ROWS
        self._h = C.c_void_p()
        q, pal = _quad(quad), _palette(colors)
        _checked(self._L, self._L.pvq_overlay_batch_create(-1 if device is None else int(device), range.octaves, range.buckets_per_octave,
                                                           int(history_rows), float(viewport_height), float(ui_scale),
                                                           _f(q) if q is not None else None, _f(pal) if pal is not None else None,
                                                           self.n_streams, self.width, self.height, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_overlay_batch_destroy(h)
            self._h = None

    def frames(self, n_frames: int, image, rows=None, chroma=None, stream=None):
        """Blend ``n_frames`` frames of every stream over ``image`` (device tensor [n_streams][n_frames][height][width][4], float32)
        in place.  ``rows``: a uint8 device tensor [n_streams][n_frames][n_bins][4] (either spectrogram output of
        ``RenderBatch.rows_device``), or the dict that call returned — its ``spectrogram_vqt``, else its ``spectrogram_peaks``, and
        its ``chroma`` unless ``chroma`` is given; None: no quad, and the rings do not advance.  ``chroma``: a float32 device tensor
        [n_streams][n_frames][12]; None: no boxes.  Returns the image.  Asynchronous on ``stream``; one handle's calls are
        stream-ordered."""
        from . import _ptr, _stream_handle
        if isinstance(rows, dict):
            if chroma is None:
                chroma = rows.get("chroma")
            rows = rows.get("spectrogram_vqt", rows.get("spectrogram_peaks"))
        n = self.n_streams * int(n_frames)
        if hasattr(rows, "numel") and (rows.numel() != n * self.n_bins * 4 or not rows.is_contiguous() or rows.element_size() != 1):
            raise ValueError("rows is not a contiguous uint8 tensor [n_streams][n_frames][n_bins][4]")
        if hasattr(chroma, "numel") and (chroma.numel() != n * 12 or not chroma.is_contiguous() or chroma.element_size() != 4):
            raise ValueError("chroma is not a contiguous float32 tensor [n_streams][n_frames][12]")
        shape = (self.n_streams, int(n_frames), self.height, self.width, 4)
        if hasattr(image, "numel") and (image.numel() != int(np.prod(shape)) or not image.is_contiguous() or image.element_size() != 4):
            raise ValueError(f"image must be a contiguous float32 tensor of shape {shape}")
        _checked(self._L, self._L.pvq_overlay_batch_frames_device(self._h, int(n_frames), _ptr(rows), _ptr(chroma), _ptr(image),
                                                                  _stream_handle(stream)))
        return image

    def texture(self, stream_index: int):
        """(texture uint8 [history_rows][n_bins][4], write index): one stream's ring as the viewer's texture would stand after the
        frames seen (synchronises)"""
        out = np.empty((self.history_rows, self.n_bins, 4), np.uint8)
        w = C.c_uint32()
        _checked(self._L, self._L.pvq_overlay_batch_get_texture(self._h, int(stream_index), _b(out), C.byref(w)))
        return out, w.value
