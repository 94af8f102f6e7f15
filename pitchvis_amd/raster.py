"""The pitch balls as pixels: what the viewer's renderer makes of the ball records of ``scene`` — the ball material's fragment
(pitchvis_viewer/assets/shaders/noisy_color_rings_2d.wgsl:395-428) over a 20 x 20 rectangle per ball, the orthographic camera of
setup.rs:359-365, the balls blended back to front over the clear colour.  The output is the linear HDR target before bloom and tone
mapping, float32 [height][width][4].

* ``raster_shade`` — one fragment, ``raster_touch`` — a frame's update of the balls' times, ``raster_frame`` — one frame on the
  host (pvq_raster_shade / _touch / _frame), the one-frame face
* ``RasterBatch`` — many streams on the GPU (pvq_raster_batch_*), fed with what ``SceneBatch.frames_device`` leaves in device
  memory; the handle keeps every ball's time between calls.  ``RasterBatch.frames_over`` draws the balls over the picture
  ``backdrop.BackdropBatch`` leaves (pvq_backdrop_balls_over_device)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .consumers import _check, _f
from .scene import FULL

_up = C.POINTER(C.c_uint32)
VIEWPORT_HEIGHT = float(np.float32(38.0) * np.float32(0.41421357))   # setup.rs:361
BALLS = ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible")
INPUTS = BALLS + ("center", "peak_count")


def _checked(L, st):
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((L.pvq_last_error() or b"").decode())
    _check(st)


def raster_shade(rgba, params, u: float, v: float) -> np.ndarray:
    """The fragment of a ball of linear ``rgba`` and ``params`` = (calmness, time, pitch_accuracy, pitch_deviation) at mesh uv"""
    L = _lib.load()
    c, p = np.ascontiguousarray(rgba, np.float32), np.ascontiguousarray(params, np.float32)
    if c.shape != (4,) or p.shape != (4,):
        raise ValueError("rgba and params hold four values each")
    out = np.empty(4, np.float32)
    _checked(L, L.pvq_raster_shade(_f(c), _f(p), float(u), float(v), _f(out)))
    return out


def raster_touch(ball_time, centers, elapsed: float) -> np.ndarray:
    """``ball_time`` [n_bins] after a frame whose peak list has these centers, at clock ``elapsed`` (a new array)"""
    L = _lib.load()
    t = np.array(ball_time, np.float32)
    c = np.ascontiguousarray(centers, np.float32).ravel()
    _checked(L, L.pvq_raster_touch(t.size, _f(c) if c.size else None, c.size, float(elapsed), _f(t)))
    return t


def raster_frame(width: int, height: int, ball_xyzs, ball_rgba, ball_params, ball_visible, ball_time, *, viewport_height: float = 0.0,
                 visuals_mode: int = FULL, background=None) -> np.ndarray:
    """One frame on the host from the arrays ``SceneState.get`` gives and the balls' times; ``background`` [height][width][4] or
    None: the clear colour of ``visuals_mode``.  ``viewport_height`` 0: the viewer's."""
    L = _lib.load()
    xyzs, rgba = np.ascontiguousarray(ball_xyzs, np.float32), np.ascontiguousarray(ball_rgba, np.float32)
    par, vis = np.ascontiguousarray(ball_params, np.float32), np.ascontiguousarray(ball_visible, np.uint32)
    t = np.ascontiguousarray(ball_time, np.float32)
    n = t.size
    if xyzs.shape != (n, 4) or rgba.shape != (n, 4) or par.shape != (n, 3) or vis.shape != ((n + 31) // 32,):
        raise ValueError("ball_xyzs / ball_rgba [n_bins][4], ball_params [n_bins][3], ball_visible [ceil(n_bins / 32)], ball_time [n_bins]")
    bg = None
    if background is not None:
        bg = np.ascontiguousarray(background, np.float32)
        if bg.shape != (height, width, 4):
            raise ValueError("background: [height][width][4]")
    if not (1 <= width <= 4096 and 1 <= height <= 4096):
        raise ValueError("width and height are 1 .. 4096")
    out = np.empty((height, width, 4), np.float32)
    _checked(L, L.pvq_raster_frame(n, width, height, float(viewport_height), int(visuals_mode), _f(xyzs), _f(rgba), _f(par),
                                   vis.ctypes.data_as(_up), _f(t), _f(bg) if bg is not None else None, _f(out)))
    return out


class RasterBatch:
    """The picture for MANY streams on the GPU: one call draws n_frames frames of every stream; the balls' times stay in the handle
    between calls.  ``device=None``: a host-only handle (the argument checks work; ``frames_device`` raises: no CPU fallback)."""

    def __init__(self, range, n_streams: int, width: int, height: int, visuals_mode: int = FULL, viewport_height: float = 0.0,
                 device: Optional[int] = 0):
        self._L = _lib.load()
        self.range, self.n_streams, self.device = range, int(n_streams), device
        self.width, self.height = int(width), int(height)
        self.n_bins = range.octaves * range.buckets_per_octave
        self._h = C.c_void_p()
        _checked(self._L, self._L.pvq_raster_batch_create(-1 if device is None else int(device), range.octaves, range.buckets_per_octave,
                                                          int(visuals_mode), float(viewport_height), self.n_streams, self.width, self.height,
                                                          C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_raster_batch_destroy(h)
            self._h = None

    def frames_device(self, balls=None, peaks=None, *, elapsed, image=True, ball_time=False, background=None, n_frames: Optional[int] = None,
                      max_peaks: Optional[int] = None, stream=None, **inputs) -> dict:
        """Draw every stream's frames.  Inputs: torch device tensors [n_streams][n_frames][...] by keyword, or as the dicts
        ``SceneBatch.frames_device`` returned (``balls``) and ``AnalysisBatch.preprocess_device`` filled (``peaks``: center and
        peak_count are read); the keys of ``raster.INPUTS``.  ``elapsed``: the clock of every frame in seconds (host sequence,
        shared by all streams).  ``image`` / ``ball_time``: True to allocate, a device tensor to fill, False / None to leave out.
        ``background``: a device tensor [height][width][4].  Returns {"image": ..., "ball_time": ...} of what was asked for.
        The kernels run asynchronously on ``stream``."""
        return self._frames(False, balls, peaks, elapsed, image, ball_time, background, n_frames, max_peaks, stream, inputs)

    def _frames(self, over, balls, peaks, elapsed, image, ball_time, background, n_frames, max_peaks, stream, inputs) -> dict:
        """frames_device (over False) and frames_over (over True): the same checks, one of the two C calls"""
        from . import _ptr, _stream_handle
        unknown = set(inputs) - set(INPUTS)
        if unknown:
            raise TypeError(f"unknown input {sorted(unknown)}")
        t = {k: (balls or {}).get(k) for k in BALLS}
        t.update({k: (peaks or {}).get(k) for k in ("center", "peak_count")})
        t.update({k: v for k, v in inputs.items() if v is not None})
        el = np.ascontiguousarray(elapsed, np.float32).ravel()
        if n_frames is None:
            n_frames = el.size
        if el.size != n_frames:
            raise ValueError("elapsed: one clock value per frame")
        if max_peaks is None:
            max_peaks = int(t["center"].shape[-1]) if hasattr(t["center"], "shape") else 0
        rows, n = self.n_streams * n_frames, self.n_bins
        per_row = {"ball_xyzs": 4 * n, "ball_rgba": 4 * n, "ball_params": 3 * n, "ball_visible": (n + 31) // 32, "center": max_peaks, "peak_count": 1}
        for k, v in t.items():
            if hasattr(v, "numel") and (v.numel() != rows * per_row[k] or not v.is_contiguous() or v.element_size() != 4):
                raise ValueError(f"input {k!r} is not a contiguous 32-bit tensor [n_streams][n_frames][...]")
        if hasattr(background, "numel") and (background.numel() != self.height * self.width * 4 or not background.is_contiguous()
                                             or background.element_size() != 4):
            raise ValueError("background must be a contiguous float32 tensor [height][width][4]")
        shapes = {"image": (self.n_streams, n_frames, self.height, self.width, 4), "ball_time": (self.n_streams, n_frames, n)}
        out = {}
        for name, want in (("image", image), ("ball_time", ball_time)):
            if want is None or want is False:
                continue
            if want is True:
                import torch
                dev = next(v.device for v in t.values() if hasattr(v, "device"))
                want = torch.empty(shapes[name], dtype=torch.float32, device=dev)
            elif hasattr(want, "numel") and (want.numel() != int(np.prod(shapes[name])) or not want.is_contiguous() or want.element_size() != 4):
                raise ValueError(f"output {name!r} must be a contiguous float32 tensor of shape {shapes[name]}")
            out[name] = want
        i = _lib.CRasterInputs(_ptr(t["ball_xyzs"]), _ptr(t["ball_rgba"]), _ptr(t["ball_params"]), _ptr(t["ball_visible"]), _ptr(t["center"]),
                               _ptr(t["peak_count"]), int(max_peaks), _ptr(background))
        call = self._L.pvq_backdrop_balls_over_device if over else self._L.pvq_raster_batch_frames_device
        _checked(self._L, call(self._h, int(n_frames), C.byref(i), _f(el) if el.size else None, _ptr(out.get("image")),
                               _ptr(out.get("ball_time")), _stream_handle(stream)))
        return out

    def frames_over(self, image, balls=None, peaks=None, *, elapsed, ball_time=False, n_frames: Optional[int] = None,
                    max_peaks: Optional[int] = None, stream=None, **inputs) -> dict:
        """``frames_device``, except that every row's balls are blended over what ``image`` (a device tensor
        [n_streams][n_frames][height][width][4], as ``BackdropBatch.frames`` fills it) already holds for that row, in place.
        Returns {"image": image, "ball_time": ...}."""
        if image is None or image is True or image is False:
            raise ValueError("frames_over draws into an image that is given")
        return self._frames(True, balls, peaks, elapsed, image, ball_time, None, n_frames, max_peaks, stream, inputs)

    def times(self, stream_index: int) -> np.ndarray:
        """One stream's ball times after the last call (synchronises)"""
        out = np.empty(self.n_bins, np.float32)
        _checked(self._L, self._L.pvq_raster_batch_get_times(self._h, int(stream_index), _f(out)))
        return out
