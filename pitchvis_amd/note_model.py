"""The trainer's note model (pitchvis_train/train.py:67-99), which the viewer runs per rendered frame through TorchScript
(pitchvis_viewer/src/ml_system.rs:24-69): pvq_note_model_* of include/pvq.h.  ``NoteModel.infer`` is the one-row host face,
``NoteModel.rows_device`` runs every frame of many streams on the GPU, reading the ``[n_streams][stride_frames][n_bins]`` dB buffer
``Vqt.batch_streams_device`` writes, in place.  With a ``NoteCarry`` the windows continue from call to call (pvq_note_carry_*): a
caller that feeds frames as they arrive gets a model row per frame, and the rows of all streams share tiles."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib

N_OUT = 128   # ml_system.rs:7
_fp = C.POINTER(C.c_float)


@dataclass
class NoteModelParams:
    """train.py:67-75; kernel 5, stride 2, 16 channels, pool 2 and 128 outputs are fixed"""
    n_bins: int = 252
    t_frames: int = 5
    mlp_size: int = 1024
    mlp_layers: int = 2

    def sizes(self):
        """(L, O_conv, O_pool, n_features)"""
        L = self.t_frames * self.n_bins
        o_conv = (L - 5) // 2 + 1
        return L, o_conv, o_conv // 2, 16 * (o_conv // 2)


def _weights_dict(sd) -> dict:
    """state_dict (tensors or arrays) -> contiguous f32 arrays"""
    out = {}
    for k, v in sd.items():
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        out[k] = np.ascontiguousarray(v, np.float32)
    return out


def _c_weights(params: "NoteModelParams", weights):
    """(CNoteModelWeights over the arrays of a state_dict-named dict, what must stay alive while it is used)"""
    w = _weights_dict(weights)
    L, _, _, n_feat = params.sizes()
    want = {"conv1.weight": 16 * 5, "conv1.bias": 16, "fc1.weight": params.mlp_size * n_feat, "fc1.bias": params.mlp_size,
            "output.weight": N_OUT * params.mlp_size, "output.bias": N_OUT}
    for i in range(params.mlp_layers):
        want[f"layers.{i}.weight"] = params.mlp_size * params.mlp_size
        want[f"layers.{i}.bias"] = params.mlp_size
    cw = _lib.CNoteModelWeights()
    in_range = (3 <= params.n_bins <= 1024 and 1 <= params.t_frames <= 8 and L >= 8 and 16 <= params.mlp_size <= 4096
                and params.mlp_size % 16 == 0 and 0 <= params.mlp_layers <= 8)
    if in_range:   # (sizes the library refuses are left to it: it reads no weight before its checks)
        for name, n in want.items():
            if name not in w or w[name].size != n:
                raise ValueError(f"weights: {name} must have {n} elements")
    nl = max(params.mlp_layers, 1)
    lw, lb = (_fp * nl)(), (_fp * nl)()
    for i in range(params.mlp_layers):
        lw[i] = w[f"layers.{i}.weight"].ctypes.data_as(_fp) if f"layers.{i}.weight" in w else None
        lb[i] = w[f"layers.{i}.bias"].ctypes.data_as(_fp) if f"layers.{i}.bias" in w else None
    for field, name in (("conv_weight", "conv1.weight"), ("conv_bias", "conv1.bias"), ("fc1_weight", "fc1.weight"),
                        ("fc1_bias", "fc1.bias"), ("output_weight", "output.weight"), ("output_bias", "output.bias")):
        if name in w:
            setattr(cw, field, w[name].ctypes.data_as(_fp))
    cw.layer_weight, cw.layer_bias = lw, lb
    return cw, (w, lw, lb)


PRECISIONS = {"f32": 0, "bf16": 1, "f16": 2}   # pvq_note_precision


def _precision(precision) -> int:
    if precision not in PRECISIONS:
        raise ValueError(f"precision: one of {sorted(PRECISIONS)}, not {precision!r}")
    return PRECISIONS[precision]


def note_round(x, precision: str) -> np.ndarray:
    """pvq_note_round: ``x`` rounded to nearest even to "bf16" or "f16" ("f32": unchanged), as an f32 array of its shape"""
    from . import _check
    a = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(a)
    _check(_lib.load().pvq_note_round(_precision(precision), a.ctypes.data_as(_fp), a.size, out.ctypes.data_as(_fp)))
    return out


class NoteModel:
    """``weights``: PyTorch ``state_dict`` names -> arrays (conv1.weight [16][1][5], conv1.bias, fc1.weight [mlp][n_features],
    fc1.bias, layers.i.weight / .bias, output.weight [128][mlp], output.bias).  ``device=None``: a host-only handle (``infer`` works;
    ``rows_device`` raises: no CPU fallback)."""

    OUTPUTS = ("d_prob", "d_logits", "d_mask")

    def __init__(self, params: NoteModelParams, weights, device: Optional[int] = 0, precision: str = "f32"):
        """``precision``: "f32" (the default, pvq_note_model_create), "bf16" or "f16": the dense layers on the 16-bit matrix
        instructions under the rule of include/pvq.h (pvq_note_model_create_precision); the outputs stay f32."""
        from . import _check
        self._L = _lib.load()
        self.params = params
        self.device = device
        self.precision = str(precision)
        self._h = C.c_void_p()
        cw, keep = _c_weights(params, weights)   # (keep: alive until the library has copied them)
        cp = _lib.CNoteModelParams(params.n_bins, params.t_frames, params.mlp_size, params.mlp_layers)
        dev = -1 if device is None else int(device)
        if self.precision == "f32":
            st = self._L.pvq_note_model_create(dev, C.byref(cp), C.byref(cw), C.byref(self._h))
        else:
            st = self._L.pvq_note_model_create_precision(dev, C.byref(cp), C.byref(cw), _precision(self.precision), C.byref(self._h))
        del keep
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        s4 = (C.c_uint32 * 4)()
        _check(self._L.pvq_note_model_sizes(self._h, s4))
        self.window_len, self.o_conv, self.o_pool, self.n_features = (int(x) for x in s4)

    @classmethod
    def from_state_dict(cls, sd, n_bins: int, t_frames: int, device: Optional[int] = 0, precision: str = "f32") -> "NoteModel":
        """mlp_size and mlp_layers are read off the shapes.  Takes the module's ``state_dict()`` as well as
        ``torch.jit.load(path).state_dict()``, what train.py:205-208 saves."""
        w = _weights_dict(sd)
        if "fc1.weight" not in w or w["fc1.weight"].ndim != 2:
            raise ValueError("state_dict: fc1.weight [mlp_size][n_features] is missing")
        layers = 0
        while f"layers.{layers}.weight" in w:
            layers += 1
        return cls(NoteModelParams(int(n_bins), int(t_frames), int(w["fc1.weight"].shape[0]), layers), w, device, precision)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_note_model_destroy(h)
            self._h = None

    def infer(self, window) -> np.ndarray:
        """one row on the host (ml_system.rs::infer): window [t_frames][n_bins] or flat [L], oldest frame first -> 128 probabilities"""
        from . import _check
        x = np.ascontiguousarray(window, np.float32).reshape(-1)
        if x.size != self.window_len:
            raise ValueError(f"window: {self.window_len} values")
        out = np.empty(N_OUT, np.float32)
        _check(self._L.pvq_note_model_infer(self._h, x.ctypes.data_as(_fp), out.ctypes.data_as(_fp)))
        return out

    def set_workspace_limit(self, n_bytes: int) -> None:
        from . import _check
        _check(self._L.pvq_note_model_set_workspace_limit(self._h, int(n_bytes)))

    def output_shape(self, name: str, n_streams: int, stride_frames: int):
        """(shape, numpy dtype) of an output"""
        return {"d_prob": ((n_streams, stride_frames, N_OUT), np.float32), "d_logits": ((n_streams, stride_frames, N_OUT), np.float32),
                "d_mask": ((n_streams, stride_frames, 4), np.uint32)}[name]

    def rows_device(self, d_db, n_frames=None, stride_frames: Optional[int] = None, outputs=None, *, n_streams: Optional[int] = None,
                    stream=None, carry: Optional["NoteCarry"] = None) -> dict:
        """Every row of every stream.  With ``carry`` (pvq_note_model_rows_carry_device) ``n_frames`` counts the NEW frames of each
        stream, which continue what the carry has seen: row (s, f) is a model row once the stream has seen ``t_frames - 1`` frames
        before it, and carries the bits this call without a carry gives the same window.  ``d_db``: device tensor ``[n_streams][stride_frames][n_bins]`` (or a raw pointer, with
        ``n_streams`` and ``stride_frames``); ``n_frames``: one count per stream (default: ``stride_frames`` each).  ``outputs``: a
        dict name -> device tensor to fill, or a sequence of names to allocate (default: all three; ``d_mask`` is an int32 tensor
        holding the uint32 words).  Returns the dict of output tensors.  Asynchronous on ``stream``."""
        from . import _check, _ptr, _stream_handle
        if hasattr(d_db, "shape"):
            if d_db.dim() != 3 or d_db.shape[2] != self.params.n_bins or not d_db.is_contiguous() or d_db.element_size() != 4:
                raise ValueError("d_db must be a contiguous f32 tensor [n_streams][stride_frames][n_bins]")
            if n_streams is None:
                n_streams = int(d_db.shape[0])
            if stride_frames is None:
                stride_frames = int(d_db.shape[1])
            if n_streams * stride_frames * self.params.n_bins > d_db.numel():
                raise ValueError("d_db is smaller than n_streams * stride_frames rows")
        if n_streams is None or stride_frames is None:
            raise ValueError("n_streams and stride_frames are needed with a raw pointer")
        nf = None
        if n_frames is not None:
            n_frames = [int(x) for x in n_frames]
            if len(n_frames) != n_streams:
                raise ValueError("one frame count per stream")
            nf = (C.c_size_t * max(n_streams, 1))(*n_frames)
        if outputs is None:
            outputs = self.OUTPUTS
        if not isinstance(outputs, dict):
            import torch
            made = {}
            for name in outputs:
                if name not in self.OUTPUTS:
                    raise ValueError(f"unknown output {name!r}")
                shape, dt = self.output_shape(name, n_streams, stride_frames)
                made[name] = torch.empty(shape, dtype=torch.float32 if dt == np.float32 else torch.int32, device=d_db.device)
            outputs = made
        o = _lib.CNoteModelOutputs()
        for name, t in outputs.items():
            if name not in self.OUTPUTS:
                raise ValueError(f"unknown output {name!r}")
            if hasattr(t, "numel"):
                shape, _ = self.output_shape(name, n_streams, stride_frames)
                if t.numel() != int(np.prod(shape)) or not t.is_contiguous() or t.element_size() != 4:
                    raise ValueError(f"output {name!r} must be a contiguous 32-bit tensor of shape {shape}")
            setattr(o, name, _ptr(t))
        if carry is not None:
            st = self._L.pvq_note_model_rows_carry_device(self._h, carry._h, _ptr(d_db), nf, int(n_streams), int(stride_frames), C.byref(o),
                                                          _stream_handle(stream))
        else:
            st = self._L.pvq_note_model_rows_device(self._h, _ptr(d_db), nf, int(n_streams), int(stride_frames), C.byref(o), _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        return outputs


class NoteCarry:
    """What continues a model's windows across ``NoteModel.rows_device(..., carry=...)`` calls for ``n_streams`` streams: the last
    ``t_frames - 1`` frames of each on the device, and the host count of the frames each has been given.  Belongs to the model's
    ``n_bins``, ``t_frames`` and device; a host-only model gives a host-only carry."""

    def __init__(self, model: NoteModel, n_streams: int):
        from . import _check
        self._L = _lib.load()
        self.model, self.n_streams = model, int(n_streams)
        self._h = C.c_void_p()
        st = self._L.pvq_note_carry_create(model._h, self.n_streams, C.byref(self._h))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_note_carry_destroy(h)
            self._h = None

    def reset(self, stream_index: Optional[int] = None, stream=None) -> None:
        """forget one stream's frames, or (``None``) every stream's"""
        from . import _check, _stream_handle
        st = self._L.pvq_note_carry_reset(self._h, -1 if stream_index is None else int(stream_index), _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def frames_seen(self, s: int) -> int:
        """frames stream ``s`` has been given since create or reset"""
        from . import _check
        out = C.c_uint64()
        st = self._L.pvq_note_carry_frames_seen(self._h, int(s), C.byref(out))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        return int(out.value)
