"""The picture behind the pitch balls: the spider net, the debug panels and the lit bass spiral as pixels — every layer a list of
flat-coloured triangles in world units, blended back to front under one coverage rule (include/pvq.h has the table of layers and
the rule).  The output is linear float32 [height][width][4]; ``raster_frame(background=...)`` / ``RasterBatch.frames_over`` put the
balls on it.

* ``backdrop_geometry`` — the static quads of the net spiral, the rays or the bass spiral; ``panel_transforms`` — the reference's
  placement of the three panels; ``backdrop_draw_mesh`` — the rule's one-mesh face; ``backdrop_frame`` — one frame on the host
* ``BackdropBatch`` — many streams on the GPU (pvq_backdrop_batch_*), fed with what ``SceneBatch.frames_device``,
  ``PanelsBatch.rows_device`` and ``PanelsBatch.graph_device(first_emitted=0)`` leave in device memory
* ``samples=4`` on ``backdrop_draw_mesh``, ``backdrop_frame`` and ``BackdropBatch`` draws with four samples a pixel, resolved at the
  end of the stage (pvq_msaa_*; the reference's desktop setting, Msaa::Sample4); ``samples=1``, the default, is the one-sample rule
  through the one-sample entry points; ``msaa_sample_positions`` — where the samples lie
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .consumers import _f
from .raster import _checked
from .scene import FULL

NET_SPIRAL, NET_RAYS, BASS = 0, 1, 2
MESHES = ("line", "disc", "hist", "graph")
IDENTITY = (0.0, 0.0, 1.0, 1.0)


def backdrop_geometry(octaves: int, what: int) -> np.ndarray:
    """[n][4][2]: the quads v0 .. v3 of ``what`` (NET_SPIRAL, NET_RAYS, BASS); their triangles are (2, 1, 0) and (2, 0, 3)"""
    L = _lib.load()
    n = C.c_uint32()
    _checked(L, L.pvq_backdrop_geometry(int(octaves), int(what), None, C.byref(n)))
    out = np.empty((n.value, 4, 2), np.float32)
    _checked(L, L.pvq_backdrop_geometry(int(octaves), int(what), _f(out), None))
    return out


def panel_transforms(n_bins: int, width: int, height: int, viewport_height: float = 0.0) -> np.ndarray:
    """[3][4]: (tx, ty, sx, sy) of the spectrum, the histogram and the graph as the viewer places them"""
    L = _lib.load()
    out = np.empty((3, 4), np.float32)
    _checked(L, L.pvq_backdrop_panel_transforms(int(n_bins), int(width), int(height), float(viewport_height), _f(out)))
    return out


def _samples(samples) -> int:
    if samples not in (1, 4):
        raise ValueError("samples is 1 or 4")
    return int(samples)


def msaa_sample_positions(samples: int) -> np.ndarray:
    """[samples][2]: (x, y) of every sample in pixel units from the pixel's top-left corner"""
    L = _lib.load()
    out = np.empty((_samples(samples), 2), np.float32)
    _checked(L, L.pvq_msaa_sample_positions(int(samples), _f(out)))
    return out


def _transform(t):
    t = np.ascontiguousarray(IDENTITY if t is None else t, np.float32)
    if t.shape != (4,):
        raise ValueError("a transform is (tx, ty, sx, sy)")
    return t


def backdrop_draw_mesh(image, pos, rgba, *, viewport_height: float = 0.0, transform=None, samples: int = 1) -> np.ndarray:
    """``image`` [height][width][4] with the triangles ``pos`` [n][3][2] of linear colours ``rgba`` [n][4] blended over it in index
    order (a new array).  ``samples=4``: every sample of a pixel starts from the pixel, and the result is resolved."""
    L = _lib.load()
    samples = _samples(samples)
    img = np.array(image, np.float32)
    p, c = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(rgba, np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or p.shape[1:] != (3, 2) or c.shape != (p.shape[0], 4):
        raise ValueError("image [height][width][4], pos [n][3][2], rgba [n][4]")
    t = None if transform is None else _transform(transform)
    args = (img.shape[1], img.shape[0], float(viewport_height), p.shape[0], _f(p) if p.size else None, _f(c) if c.size else None,
            _f(t) if t is not None else None, _f(img))
    _checked(L, L.pvq_backdrop_draw_mesh(*args) if samples == 1 else L.pvq_msaa_draw_mesh(samples, *args))
    return img


def _host_panels(n_bins: int, panels: dict, keep: list) -> _lib.CBackdropPanels:
    """``panels``: line_pos / line_rgba, disc_pos / disc_rgba, hist_pos / hist_rgba, graph_pos / graph_rgba (as the mesh functions of
    ``panels`` give them) and spectrum_transform / histogram_transform / graph_transform"""
    known = {f"{m}_{k}" for m in MESHES for k in ("pos", "rgba")} | {"spectrum_transform", "histogram_transform", "graph_transform"}
    if set(panels) - known:
        raise TypeError(f"unknown panel entry {sorted(set(panels) - known)}")
    o = _lib.CBackdropPanels()
    for m in MESHES:
        pos, col = panels.get(m + "_pos"), panels.get(m + "_rgba")
        if pos is None and col is None:
            continue
        if pos is None or col is None:
            raise ValueError(f"{m}: positions and colours go together")
        pos, col = np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(col, np.float32).reshape(-1, 4)
        per = 13 if m == "disc" else 4
        if pos.shape[0] != col.shape[0] or pos.shape[0] % per or (m in ("line", "hist") and pos.shape[0] != 4 * (n_bins - 1)):
            raise ValueError(f"{m}: [vertices][3] and [vertices][4], as the panels stage lays them out")
        if m == "disc":
            o.n_peaks = pos.shape[0] // 13
            if o.n_peaks == 0:
                continue
        if m == "graph":
            o.graph_capacity = pos.shape[0] // 4 + 1
        keep += [pos, col]
        setattr(o, m + "_pos", pos.ctypes.data)
        setattr(o, m + "_rgba", col.ctypes.data)
    for name in ("spectrum_transform", "histogram_transform", "graph_transform"):
        getattr(o, name)[:] = _transform(panels.get(name)).tolist()
    return o


def backdrop_frame(octaves: int, buckets_per_octave: int, width: int, height: int, *, viewport_height: float = 0.0, visuals_mode: int = FULL,
                   bass_lit: int = 0, bass_rgba=None, panels: Optional[dict] = None, background=None, samples: int = 1) -> np.ndarray:
    """One frame on the host: clear colour or ``background``, net, panels (see ``_host_panels``), lit bass segments; with
    ``samples=4`` drawn per sample and resolved"""
    L = _lib.load()
    samples = _samples(samples)
    if not (1 <= width <= 4096 and 1 <= height <= 4096):
        raise ValueError("width and height are 1 .. 4096")
    bg = None
    if background is not None:
        bg = np.ascontiguousarray(background, np.float32)
        if bg.shape != (height, width, 4):
            raise ValueError("background: [height][width][4]")
    col = None
    if bass_rgba is not None:
        col = np.ascontiguousarray(bass_rgba, np.float32)
        if col.shape != (4,):
            raise ValueError("bass_rgba holds four values")
    keep: list = []
    o = _host_panels(int(octaves) * int(buckets_per_octave), panels, keep) if panels is not None else None
    out = np.empty((height, width, 4), np.float32)
    args = (int(octaves), int(buckets_per_octave), width, height, float(viewport_height), int(visuals_mode), int(bass_lit),
            _f(col) if col is not None else None, C.byref(o) if o is not None else None, _f(bg) if bg is not None else None, _f(out))
    _checked(L, L.pvq_backdrop_frame(*args) if samples == 1 else L.pvq_msaa_frame(samples, *args))
    return out


class BackdropBatch:
    """The backdrop for MANY streams on the GPU; stateless.  ``device=None``: a host-only handle (the argument checks work;
    ``frames`` raises: no CPU fallback).  ``samples=4``: four samples a pixel, kept in registers and resolved by the tile kernel;
    the image ``frames`` returns has the shape and the meaning it has with one sample."""

    INPUTS = ("bass_lit", "bass_rgba", "line_pos", "line_rgba", "disc_pos", "disc_rgba", "peak_count", "hist_pos", "hist_rgba", "graph_pos",
              "graph_rgba")

    def __init__(self, range, n_streams: int, width: int, height: int, visuals_mode: int = FULL, viewport_height: float = 0.0,
                 device: Optional[int] = 0, samples: int = 1):
        self._L = _lib.load()
        self.samples = _samples(samples)
        self.range, self.n_streams, self.device = range, int(n_streams), device
        self.width, self.height = int(width), int(height)
        self.n_bins = range.octaves * range.buckets_per_octave
        self._h = C.c_void_p()
        args = (-1 if device is None else int(device), range.octaves, range.buckets_per_octave, int(visuals_mode), float(viewport_height),
                self.n_streams, self.width, self.height, C.byref(self._h))
        _checked(self._L, self._L.pvq_backdrop_batch_create(*args) if self.samples == 1 else self._L.pvq_msaa_batch_create(self.samples, *args))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_backdrop_batch_destroy(h)
            self._h = None

    def frames(self, n_frames: int, scene=None, panels=None, graph=None, *, image=True, background=None, max_peaks: Optional[int] = None,
               graph_capacity: Optional[int] = None, spectrum_transform=None, histogram_transform=None, graph_transform=None,
               stream=None, **inputs):
        """Draw ``n_frames`` frames of every stream.  Inputs: torch device tensors [n_streams][n_frames][...] by keyword (the names of
        ``INPUTS``), or as the dicts ``SceneBatch.frames_device`` (``scene``: bass_lit, bass_rgba), ``PanelsBatch.rows_device``
        (``panels``; peak_count by keyword) and ``PanelsBatch.graph_device(first_emitted=0)`` (``graph``) returned.  Every group is
        optional.  The transforms default to the identity (``panel_transforms`` gives the viewer's).  ``image``: True to allocate, or
        a device tensor [n_streams][n_frames][height][width][4] to fill.  ``background``: a device tensor [height][width][4].
        Returns the image.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        unknown = set(inputs) - set(self.INPUTS)
        if unknown:
            raise TypeError(f"unknown input {sorted(unknown)}")
        t = {k: None for k in self.INPUTS}
        for d in (scene, panels, graph):
            t.update({k: v for k, v in (d or {}).items() if k in t})
        t.update({k: v for k, v in inputs.items() if v is not None})
        rows, n = self.n_streams * int(n_frames), self.n_bins
        if max_peaks is None:
            max_peaks = int(t["disc_pos"].shape[-3]) if hasattr(t["disc_pos"], "shape") and len(t["disc_pos"].shape) >= 3 else 0
        if graph_capacity is None:
            graph_capacity = int(t["graph_pos"].shape[-2]) // 4 + 1 if hasattr(t["graph_pos"], "shape") else 0
        v, c = 4 * (n - 1), 4 * max(graph_capacity - 1, 0)
        per_row = {"bass_lit": 1, "bass_rgba": 4, "line_pos": 3 * v, "line_rgba": 4 * v, "hist_pos": 3 * v, "hist_rgba": 4 * v,
                   "disc_pos": 39 * max_peaks, "disc_rgba": 52 * max_peaks, "peak_count": 1, "graph_pos": 3 * c, "graph_rgba": 4 * c}
        for k, x in t.items():
            if hasattr(x, "numel") and (x.numel() != rows * per_row[k] or not x.is_contiguous() or x.element_size() != 4):
                raise ValueError(f"input {k!r} is not a contiguous 32-bit tensor [n_streams][n_frames][...]")
        if hasattr(background, "numel") and (background.numel() != self.height * self.width * 4 or not background.is_contiguous()
                                             or background.element_size() != 4):
            raise ValueError("background must be a contiguous float32 tensor [height][width][4]")
        shape = (self.n_streams, int(n_frames), self.height, self.width, 4)
        if image is True:
            import torch
            dev = next((x.device for x in list(t.values()) + [background] if hasattr(x, "device")), None)
            image = torch.empty(shape, dtype=torch.float32, device=dev if dev is not None else f"cuda:{self.device or 0}")
        elif hasattr(image, "numel") and (image.numel() != int(np.prod(shape)) or not image.is_contiguous() or image.element_size() != 4):
            raise ValueError(f"image must be a contiguous float32 tensor of shape {shape}")
        i = _lib.CBackdropInputs()
        for k in self.INPUTS:
            setattr(i, k, _ptr(t[k]))
        if t["disc_pos"] is None:   # the counts are the discs' alone
            i.peak_count = 0
        i.max_peaks, i.graph_capacity, i.background = int(max_peaks), int(graph_capacity), _ptr(background)
        for name, tr in (("spectrum_transform", spectrum_transform), ("histogram_transform", histogram_transform), ("graph_transform", graph_transform)):
            getattr(i, name)[:] = _transform(tr).tolist()
        _checked(self._L, self._L.pvq_backdrop_batch_frames_device(self._h, int(n_frames), C.byref(i), _ptr(image), _stream_handle(stream)))
        return image
