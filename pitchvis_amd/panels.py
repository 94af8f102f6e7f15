"""The viewer's debug panels (pitchvis_viewer/src/display_system/update.rs:474-869, DisplayMode::Debugging): the smoothed spectrum as
a thick line with a disc on every continuous peak, the per-bin calmness as a thick line, and the last values of the scene calmness as
a thick line.  A mesh is positions ``[vertices][3]`` and colours ``[vertices][4]``; indices and UVs come from ``panel_topology``.

* ``spectrum_mesh`` / ``calmness_histogram_mesh`` / ``CalmnessGraph`` — one stream on the host, the one-stream face
* ``PanelsBatch`` — many streams on the GPU (pvq_panels_batch_*), fed with what ``AnalysisBatch.preprocess_device`` leaves in device
  memory: ``rows_device`` is stateless, ``graph_device`` keeps every stream's history in the handle

The reference's transforms, visibility toggles and the concatenation of line and discs into one mesh stay with the caller.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .consumers import COLORS, GRAY_LEVEL, _check, _f

_up = C.POINTER(C.c_uint32)
DISC_VERTICES, DISC_SEGMENTS = 13, 12
GRAPH_CAPACITY = 300   # app/common.rs:2037


def _checked(L, st):
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((L.pvq_last_error() or b"").decode())
    _check(st)


def spectrum_mesh(n_buckets: int, buckets_per_octave: int, x_vqt_smoothed, peaks_continuous: Sequence[Tuple[float, float]] = (),
                  colors: np.ndarray = COLORS, gray_level: float = GRAY_LEVEL) -> dict:
    """update_spectrum (update.rs:474-638): ``line_pos [4 (n - 1)][3]``, ``line_rgba [4 (n - 1)][4]``, ``disc_pos [n_peaks][13][3]``,
    ``disc_rgba [n_peaks][13][4]`` (float32); ``peaks_continuous``: (center, size) pairs in list order."""
    colors = np.ascontiguousarray(colors, np.float32)
    x = np.ascontiguousarray(x_vqt_smoothed, np.float32)
    if x.size != n_buckets:
        raise ValueError("x_vqt_smoothed must hold n_buckets values")
    k = len(peaks_continuous)
    ctr = np.asarray([p[0] for p in peaks_continuous] or [0.0], np.float32)
    sz = np.asarray([p[1] for p in peaks_continuous] or [0.0], np.float32)
    segs = max(n_buckets - 1, 0)
    out = {"line_pos": np.zeros((4 * segs, 3), np.float32), "line_rgba": np.zeros((4 * segs, 4), np.float32),
           "disc_pos": np.zeros((k, DISC_VERTICES, 3), np.float32), "disc_rgba": np.zeros((k, DISC_VERTICES, 4), np.float32)}
    L = _lib.load()
    _checked(L, L.pvq_spectrum_mesh(n_buckets, buckets_per_octave, _f(x), _f(ctr), _f(sz), k, _f(colors), gray_level, _f(out["line_pos"]),
                                    _f(out["line_rgba"]), _f(out["disc_pos"]) if k else None, _f(out["disc_rgba"]) if k else None))
    return out


def calmness_histogram_mesh(n_buckets: int, calmness) -> dict:
    """update_calmness_histogram (update.rs:744-869): ``pos [4 (n - 1)][3]``, ``rgba [4 (n - 1)][4]``"""
    c = np.ascontiguousarray(calmness, np.float32)
    if c.size != n_buckets:
        raise ValueError("calmness must hold n_buckets values")
    segs = max(n_buckets - 1, 0)
    out = {"pos": np.zeros((4 * segs, 3), np.float32), "rgba": np.zeros((4 * segs, 4), np.float32)}
    L = _lib.load()
    _checked(L, L.pvq_calmness_histogram_mesh(n_buckets, _f(c), _f(out["pos"]), _f(out["rgba"])))
    return out


def panel_topology(n_quads: int, n_circles: int = 0):
    """(indices uint32 ``[6 n_quads + 36 n_circles]``, uvs ``[4 n_quads + 13 n_circles][2]``) of n_quads quads followed by
    n_circles discs; every normal is (0, 0, 1)."""
    idx = np.zeros(6 * n_quads + 3 * DISC_SEGMENTS * n_circles, np.uint32)
    uvs = np.zeros((4 * n_quads + DISC_VERTICES * n_circles, 2), np.float32)
    L = _lib.load()
    _checked(L, L.pvq_panel_topology(n_quads, n_circles, idx.ctypes.data_as(_up), _f(uvs)))
    return idx, uvs


class CalmnessGraph:
    """update_scene_calmness_graph (update.rs:640-742) for one stream on the host: the history ring and its mesh"""

    def __init__(self, capacity: int = GRAPH_CAPACITY):
        self._L = _lib.load()
        self._h = C.c_void_p()
        _checked(self._L, self._L.pvq_calmness_graph_create(int(capacity), C.byref(self._h)))
        self.capacity = int(self._L.pvq_calmness_graph_capacity(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_calmness_graph_destroy(h)
            self._h = None

    def push(self, value: float) -> None:
        _check(self._L.pvq_calmness_graph_push(self._h, float(value)))

    def mesh(self) -> dict:
        """``pos [4 (C - 1)][3]``, ``rgba [4 (C - 1)][4]`` and ``history [C]`` (oldest first) as they stand"""
        c = self.capacity
        out = {"pos": np.zeros((4 * (c - 1), 3), np.float32), "rgba": np.zeros((4 * (c - 1), 4), np.float32), "history": np.zeros(c, np.float32)}
        _check(self._L.pvq_calmness_graph_mesh(self._h, _f(out["pos"]), _f(out["rgba"]), _f(out["history"])))
        return out


class PanelsBatch:
    """The debug panels for MANY streams on the GPU.  ``device=None``: a host-only handle (the argument checks work; the device calls
    raise: no CPU fallback)."""

    OUTPUTS = ("line_pos", "line_rgba", "disc_pos", "disc_rgba", "hist_pos", "hist_rgba")
    GRAPH_OUTPUTS = ("graph_pos", "graph_rgba")

    def __init__(self, range, n_streams: int, graph_capacity: int = GRAPH_CAPACITY, colors: Optional[np.ndarray] = None,
                 gray_level: float = GRAY_LEVEL, device: Optional[int] = 0):
        self._L = _lib.load()
        self.range, self.n_streams, self.device = range, int(n_streams), device
        self.n_bins = range.octaves * range.buckets_per_octave
        self._h = C.c_void_p()
        pal = None if colors is None else np.ascontiguousarray(colors, np.float32)
        if pal is not None and pal.shape != (12, 3):
            raise ValueError("colors: 12 RGB triples")
        _checked(self._L, self._L.pvq_panels_batch_create(-1 if device is None else int(device), range.octaves, range.buckets_per_octave,
                                                          _f(pal) if pal is not None else None, gray_level, self.n_streams,
                                                          int(graph_capacity), C.byref(self._h)))
        self.graph_capacity = int(self._L.pvq_panels_batch_graph_capacity(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_panels_batch_destroy(h)
            self._h = None

    def output_shape(self, name: str, n_rows: int, max_peaks: int = 0):
        """shape of an output of ``rows_device`` for n_rows rows, or of ``graph_device`` for n_rows emitted frames of every stream"""
        v, c = 4 * (self.n_bins - 1), 4 * (self.graph_capacity - 1)
        return {"line_pos": (n_rows, v, 3), "line_rgba": (n_rows, v, 4), "hist_pos": (n_rows, v, 3), "hist_rgba": (n_rows, v, 4),
                "disc_pos": (n_rows, max_peaks, DISC_VERTICES, 3), "disc_rgba": (n_rows, max_peaks, DISC_VERTICES, 4),
                "graph_pos": (self.n_streams, n_rows, c, 3), "graph_rgba": (self.n_streams, n_rows, c, 4)}[name]

    def rows_device(self, fields=None, outputs=None, *, x_vqt_smoothed=None, center=None, size=None, peak_count=None, calmness=None,
                    n_rows: Optional[int] = None, max_peaks: Optional[int] = None, stream=None) -> dict:
        """Spectrum and histogram meshes of every row.  Inputs: torch device tensors, by keyword or as the dict
        ``AnalysisBatch.preprocess_device`` fills (``fields``; keys ``x_vqt_smoothed``, ``center``, ``size``, ``peak_count``,
        ``calmness``; leading dimensions are flattened to rows, nothing is copied).  ``outputs``: a dict name -> device tensor to
        fill, or a sequence of names to allocate (default: every output the given inputs allow).  ``n_rows`` / ``max_peaks`` default
        to what the tensors' shapes say (raw pointers need them).  Returns the dict of output tensors.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        f = dict(fields or {})
        x = x_vqt_smoothed if x_vqt_smoothed is not None else f.get("x_vqt_smoothed")
        ctr = center if center is not None else f.get("center")
        sz = size if size is not None else f.get("size")
        cnt = peak_count if peak_count is not None else f.get("peak_count")
        calm = calmness if calmness is not None else f.get("calmness")
        if max_peaks is None:
            max_peaks = int(ctr.shape[-1]) if hasattr(ctr, "shape") else 0
        if n_rows is None:
            t = next((t for t in (x, calm) if hasattr(t, "numel")), None)
            if t is not None:
                n_rows = t.numel() // self.n_bins
            elif hasattr(cnt, "numel"):
                n_rows = cnt.numel()
            else:
                raise ValueError("n_rows is needed with raw pointers")
        for t, per_row in ((x, self.n_bins), (calm, self.n_bins), (ctr, max_peaks), (sz, max_peaks), (cnt, 1)):
            if hasattr(t, "numel"):
                if t.numel() != n_rows * per_row or not t.is_contiguous() or t.element_size() != 4:
                    raise ValueError("an input tensor is not contiguous 32-bit [n_rows][...]")
        if outputs is None:
            have = {"line": x is not None, "hist": calm is not None, "disc": ctr is not None and sz is not None and cnt is not None}
            outputs = [n for n in self.OUTPUTS if have[n.split("_")[0]]]
        if not isinstance(outputs, dict):
            import torch
            dev = next(t.device for t in (x, calm, ctr, cnt) if hasattr(t, "device"))
            outputs = {name: torch.empty(self.output_shape(name, n_rows, max_peaks), dtype=torch.float32, device=dev) for name in outputs}
        o = _lib.CPanelsOutputs()
        for name, t in outputs.items():
            if name not in self.OUTPUTS:
                raise ValueError(f"unknown output {name!r}")
            if hasattr(t, "numel"):
                shape = self.output_shape(name, n_rows, max_peaks)
                if t.numel() != int(np.prod(shape)) or not t.is_contiguous() or t.element_size() != 4:
                    raise ValueError(f"output {name!r} must be a contiguous float32 tensor of shape {shape}")
            setattr(o, name, _ptr(t))
        _checked(self._L, self._L.pvq_panels_batch_rows_device(self._h, int(n_rows), _ptr(x), _ptr(ctr), _ptr(sz), _ptr(cnt), int(max_peaks),
                                                               _ptr(calm), C.byref(o), _stream_handle(stream)))
        return outputs

    def graph_device(self, scene_calmness, outputs=None, *, first_emitted: Optional[int] = None, n_frames: Optional[int] = None,
                     stream=None) -> dict:
        """Advance every stream's history by the ``n_frames`` values of ``scene_calmness`` (device tensor ``[n_streams][n_frames]``)
        and write the graph meshes of frames ``first_emitted .. n_frames - 1`` (default: the newest frame alone).  ``outputs``: a dict
        name -> device tensor, or a sequence of names of ``GRAPH_OUTPUTS`` to allocate (default: both; an empty sequence only advances
        the history).  Returns the dict of output tensors.  Asynchronous on ``stream``; one handle's calls are stream-ordered."""
        from . import _ptr, _stream_handle
        if n_frames is None:
            if not hasattr(scene_calmness, "numel"):
                raise ValueError("n_frames is needed with a raw pointer")
            n_frames = scene_calmness.numel() // self.n_streams
        if hasattr(scene_calmness, "numel") and (scene_calmness.numel() != self.n_streams * n_frames or not scene_calmness.is_contiguous()
                                                 or scene_calmness.element_size() != 4):
            raise ValueError("scene_calmness is not a contiguous 32-bit tensor [n_streams][n_frames]")
        if first_emitted is None:
            first_emitted = max(n_frames - 1, 0)
        emitted = max(n_frames - first_emitted, 0)
        if outputs is None:
            outputs = self.GRAPH_OUTPUTS
        if not isinstance(outputs, dict):
            import torch
            outputs = {name: torch.empty(self.output_shape(name, emitted), dtype=torch.float32, device=scene_calmness.device) for name in outputs}
        for name, t in outputs.items():
            if name not in self.GRAPH_OUTPUTS:
                raise ValueError(f"unknown output {name!r}")
            if hasattr(t, "numel"):
                shape = self.output_shape(name, emitted)
                if t.numel() != int(np.prod(shape)) or not t.is_contiguous() or t.element_size() != 4:
                    raise ValueError(f"output {name!r} must be a contiguous float32 tensor of shape {shape}")
        _checked(self._L, self._L.pvq_panels_batch_graph_device(self._h, int(n_frames), _ptr(scene_calmness), int(first_emitted),
                                                                _ptr(outputs.get("graph_pos")), _ptr(outputs.get("graph_rgba")),
                                                                _stream_handle(stream)))
        return outputs

    def history(self, stream_index: int) -> np.ndarray:
        """one stream's last ``graph_capacity`` values after the last call, oldest first (synchronises)"""
        out = np.zeros(self.graph_capacity, np.float32)
        _checked(self._L, self._L.pvq_panels_batch_get_history(self._h, int(stream_index), _f(out)))
        return out
