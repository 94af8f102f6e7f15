"""The viewer's main picture (pitchvis_viewer/src/display_system/update.rs:38-426): a pitch ball per bin that lights on a peak, fades
between frames and hides beside a stronger neighbour; the bass spiral lit up to the lowest note; the bloom driven by scene calmness.

* ``SceneState`` — one stream on the host (pvq_scene_state_*), the one-stream face
* ``SceneBatch`` — many streams on the GPU (pvq_scene_batch_*), state kept in the handle between calls, fed with what
  ``AnalysisBatch.preprocess_device`` leaves in device memory
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .consumers import EASING_POW, GRAY_LEVEL, _check, _f

FULL, ZEN, PERFORMANCE, GALAXY = _lib.VISUALS_FULL, _lib.VISUALS_ZEN, _lib.VISUALS_PERFORMANCE, _lib.VISUALS_GALAXY   # VisualsMode
_up = C.POINTER(C.c_uint32)
INPUTS = ("center", "size", "peak_count", "calmness", "pitch_accuracy", "pitch_deviation", "scene_calmness")


def midi_pitch(buckets_per_octave: int, bin: int) -> Optional[int]:
    """The MIDI pitch the ``ml`` branch looks a bin's ball up at (display_system/util.rs:23-31), ``None`` above 127"""
    out = C.c_uint32()
    st = _lib.load().pvq_ml_midi_pitch(int(buckets_per_octave), int(bin), C.byref(out))
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((_lib.load().pvq_last_error() or b"").decode())
    _check(st)
    return None if out.value == 0xFFFFFFFF else int(out.value)


def _settings(visuals_mode, enable_bloom, colors, gray_level, easing_pow):
    pal = None if colors is None else np.ascontiguousarray(colors, np.float32)
    if pal is not None and pal.shape != (12, 3):
        raise ValueError("colors: 12 RGB triples")
    cfg = _lib.CSceneSettings(int(visuals_mode), int(bool(enable_bloom)), _f(pal) if pal is not None else None, gray_level, easing_pow)
    return cfg, pal


def _state_arrays(n_bins):
    return {"ball_xyzs": np.empty((n_bins, 4), np.float32), "ball_rgba": np.empty((n_bins, 4), np.float32),
            "ball_params": np.empty((n_bins, 3), np.float32), "ball_visible": np.empty((n_bins + 31) // 32, np.uint32),
            "bass_lit": np.empty(1, np.uint32), "bass_rgba": np.empty(4, np.float32), "bloom": np.empty(1, np.float32)}


def _state_args(a):
    return (_f(a["ball_xyzs"]), _f(a["ball_rgba"]), _f(a["ball_params"]), a["ball_visible"].ctypes.data_as(_up),
            a["bass_lit"].ctypes.data_as(_up), _f(a["bass_rgba"]), _f(a["bloom"]))


def _finish(a):
    a["bass_lit"] = int(a["bass_lit"][0])
    a["bloom"] = np.float32(a["bloom"][0])
    return a


class SceneState:
    """update_display (update.rs:38-134) for one stream on the host.  Settings are fixed at create."""

    def __init__(self, range, visuals_mode: int = FULL, enable_bloom: bool = True, colors: Optional[np.ndarray] = None,
                 gray_level: float = GRAY_LEVEL, easing_pow: float = EASING_POW):
        self._L = _lib.load()
        self.range = range
        self._h = C.c_void_p()
        cfg, _pal = _settings(visuals_mode, enable_bloom, colors, gray_level, easing_pow)
        st = self._L.pvq_scene_state_create(range.octaves, range.buckets_per_octave, C.byref(cfg), C.byref(self._h))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        self.n_bins = int(self._L.pvq_scene_state_n_bins(self._h))
        self.n_segments = int(self._L.pvq_scene_state_n_segments(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_scene_state_destroy(h)
            self._h = None

    def update(self, peaks_continuous, calmness, pitch_accuracy, pitch_deviation, scene_calmness: float, frame_time: float,
               ml_prob=None) -> None:
        """One frame: ``peaks_continuous`` (center, size) pairs in list order, three per-bin fields, the smoothed scene calmness and
        the frame's duration in seconds (``frame_time``; an int is taken as nanoseconds).  ``ml_prob``: the frame's 128 note
        probabilities for the viewer's ``ml`` branch (update.rs:247-255, pvq_ml_scene_state_update); ``None``: the branch is off."""
        ctr = np.asarray([p[0] for p in peaks_continuous] or [0.0], np.float32)
        sz = np.asarray([p[1] for p in peaks_continuous] or [0.0], np.float32)
        per_bin = [np.ascontiguousarray(a, np.float32) for a in (calmness, pitch_accuracy, pitch_deviation)]
        if any(a.size != self.n_bins for a in per_bin):
            raise ValueError("calmness, pitch_accuracy and pitch_deviation must hold n_bins values")
        ns = frame_time if isinstance(frame_time, (int, np.integer)) else int(round(frame_time * 1e9))
        if ml_prob is not None:
            ml = np.ascontiguousarray(ml_prob, np.float32)
            if ml.size != 128:
                raise ValueError("ml_prob must hold 128 values")
            _check(self._L.pvq_ml_scene_state_update(self._h, _f(ctr), _f(sz), len(peaks_continuous), _f(per_bin[0]), _f(per_bin[1]),
                                                     _f(per_bin[2]), float(scene_calmness), int(ns), _f(ml)))
            return
        _check(self._L.pvq_scene_state_update(self._h, _f(ctr), _f(sz), len(peaks_continuous), _f(per_bin[0]), _f(per_bin[1]), _f(per_bin[2]),
                                              float(scene_calmness), int(ns)))

    def get(self) -> dict:
        """The scene as it stands: the arrays of ``SceneBatch.OUTPUTS`` for one frame (bass_lit an int, bloom a float32)"""
        a = _state_arrays(self.n_bins)
        _check(self._L.pvq_scene_state_get(self._h, *_state_args(a)))
        return _finish(a)


class SceneBatch:
    """The same scene for MANY streams on the GPU: one call advances every stream by n_frames frames, the state stays in the handle
    between calls.  ``device=None``: a host-only handle (the argument checks work; ``frames_device`` raises: no CPU fallback)."""

    OUTPUTS = ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible", "bass_lit", "bass_rgba", "bloom")

    def __init__(self, range, n_streams: int, visuals_mode: int = FULL, enable_bloom: bool = True, colors: Optional[np.ndarray] = None,
                 gray_level: float = GRAY_LEVEL, easing_pow: float = EASING_POW, device: Optional[int] = 0):
        self._L = _lib.load()
        self.range, self.n_streams, self.device = range, int(n_streams), device
        self.n_bins = range.octaves * range.buckets_per_octave
        self._h = C.c_void_p()
        cfg, _pal = _settings(visuals_mode, enable_bloom, colors, gray_level, easing_pow)
        st = self._L.pvq_scene_batch_create(-1 if device is None else int(device), range.octaves, range.buckets_per_octave, C.byref(cfg),
                                            self.n_streams, C.byref(self._h))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        self.n_segments = int(self._L.pvq_scene_batch_n_segments(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_scene_batch_destroy(h)
            self._h = None

    def output_shape(self, name: str, n_frames: int):
        """(shape, numpy dtype) of an output for n_frames frames of every stream"""
        s, f, n = self.n_streams, n_frames, self.n_bins
        return {"ball_xyzs": ((s, f, n, 4), np.float32), "ball_rgba": ((s, f, n, 4), np.float32), "ball_params": ((s, f, n, 3), np.float32),
                "ball_visible": ((s, f, (n + 31) // 32), np.uint32), "bass_lit": ((s, f), np.uint32), "bass_rgba": ((s, f, 4), np.float32),
                "bloom": ((s, f), np.float32)}[name]

    def frames_device(self, fields=None, outputs=None, *, frame_time: float = 1.0 / 30.0, frame_times=None, n_frames: Optional[int] = None,
                      max_peaks: Optional[int] = None, stream=None, ml_prob=None, ml_stride_frames: Optional[int] = None, **inputs) -> dict:
        """Advance every stream.  Inputs: torch device tensors [n_streams][n_frames][...], by keyword or as the dict
        ``AnalysisBatch.preprocess_device(outputs=...)`` filled (``fields``; the keys of ``scene.INPUTS``).  ``outputs``: a dict
        name -> device tensor to fill, or a sequence of names to allocate (default: all of ``OUTPUTS``).  ``frame_time`` in seconds,
        or ``frame_times``: per-frame seconds (host sequence).  ``n_frames`` / ``max_peaks`` default to what the tensors' shapes
        say (raw pointers need them).  ``ml_prob``: the note probabilities ``[n_streams][ml_stride_frames][128]`` for the viewer's
        ``ml`` branch, a device tensor (``NoteModel.rows_device``'s ``d_prob``, taken where it lies) or a raw pointer;
        ``ml_stride_frames`` defaults to the tensor's second dimension; ``None``: the branch is off.  Returns the dict of output
        tensors.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        f = dict(fields or {})
        f.update({k: v for k, v in inputs.items() if v is not None})
        unknown = set(inputs) - set(INPUTS)
        if unknown:
            raise TypeError(f"unknown input {sorted(unknown)}")
        t = {k: f.get(k) for k in INPUTS}
        if max_peaks is None:
            max_peaks = int(t["center"].shape[-1]) if hasattr(t["center"], "shape") else 0
        if n_frames is None:
            cnt = t["peak_count"]
            if not hasattr(cnt, "numel"):
                raise ValueError("n_frames is needed with raw pointers")
            n_frames = cnt.numel() // self.n_streams
        rows = self.n_streams * n_frames
        per_row = {"center": max_peaks, "size": max_peaks, "peak_count": 1, "scene_calmness": 1}
        for k, v in t.items():
            if hasattr(v, "numel") and (v.numel() != rows * per_row.get(k, self.n_bins) or not v.is_contiguous() or v.element_size() != 4):
                raise ValueError(f"input {k!r} is not a contiguous 32-bit tensor [n_streams][n_frames][...]")
        if outputs is None:
            outputs = self.OUTPUTS
        if not isinstance(outputs, dict):
            import torch
            dev = next(v.device for v in t.values() if hasattr(v, "device"))
            made = {}
            for name in outputs:
                shape, dt = self.output_shape(name, n_frames)
                made[name] = torch.empty(shape, dtype=torch.int32 if dt == np.uint32 else torch.float32, device=dev)
            outputs = made
        o = _lib.CSceneOutputs()
        for name, v in outputs.items():
            if name not in self.OUTPUTS:
                raise ValueError(f"unknown output {name!r}")
            if hasattr(v, "numel"):
                shape, _ = self.output_shape(name, n_frames)
                if v.numel() != int(np.prod(shape)) or not v.is_contiguous() or v.element_size() != 4:
                    raise ValueError(f"output {name!r} must be a contiguous 32-bit tensor of shape {shape}")
            setattr(o, name, _ptr(v))
        i = _lib.CSceneInputs(_ptr(t["center"]), _ptr(t["size"]), _ptr(t["peak_count"]), int(max_peaks), _ptr(t["calmness"]),
                              _ptr(t["pitch_accuracy"]), _ptr(t["pitch_deviation"]), _ptr(t["scene_calmness"]))
        ft = None
        if frame_times is not None:
            if len(frame_times) != n_frames:
                raise ValueError("frame_times: one entry per frame")
            ft = (C.c_uint64 * n_frames)(*[int(round(x * 1e9)) for x in frame_times])
        if ml_prob is not None:
            if hasattr(ml_prob, "shape"):
                if ml_prob.dim() != 3 or ml_prob.shape[0] != self.n_streams or ml_prob.shape[2] != 128 or not ml_prob.is_contiguous() \
                        or ml_prob.element_size() != 4:
                    raise ValueError("ml_prob must be a contiguous f32 tensor [n_streams][ml_stride_frames][128]")
                if ml_stride_frames is None:
                    ml_stride_frames = int(ml_prob.shape[1])
                if ml_stride_frames > ml_prob.shape[1]:
                    raise ValueError("ml_prob is smaller than n_streams * ml_stride_frames rows")
            if ml_stride_frames is None:
                raise ValueError("ml_stride_frames is needed with a raw pointer")
            st = self._L.pvq_ml_scene_batch_frames_device(self._h, int(n_frames), C.byref(i), _ptr(ml_prob), int(ml_stride_frames),
                                                          int(round(frame_time * 1e9)), ft, C.byref(o), _stream_handle(stream))
        else:
            st = self._L.pvq_scene_batch_frames_device(self._h, int(n_frames), C.byref(i), int(round(frame_time * 1e9)), ft, C.byref(o),
                                                       _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        return outputs

    def state(self, stream_index: int) -> dict:
        """One stream's scene after the last call, as ``SceneState.get`` (synchronises)"""
        a = _state_arrays(self.n_bins)
        _check(self._L.pvq_scene_batch_get_state(self._h, int(stream_index), *_state_args(a)))
        return _finish(a)
