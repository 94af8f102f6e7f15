"""What turns the picture chain's linear HDR target into displayable bytes: bloom over a mip pyramid, the display transform and the
sRGB encode (include/pvq.h, "the present stage", has the rule).  The picture is linear float32 [height][width][4], as
``backdrop_frame`` / ``raster_frame`` / ``overlay_frame`` leave it; the intensity is the scene stage's ``bloom``.

* ``present_mips`` — the mip sizes; ``present_blend_factors`` — a level's share of the bloom; ``present_frame`` — one picture on
  the host
* ``PresentBatch`` — many pictures on the GPU (pvq_present_batch_*), fed with the image the picture chain leaves in device memory
  and ``SceneBatch``'s ``bloom`` buffer where it lies
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .consumers import _f
from .raster import _checked

ENERGY_CONSERVING, ADDITIVE = 0, 1              # composite_mode
TONEMAP_NONE, TONEMAP_SOMEWHAT_BORING = 0, 1    # tonemapping
_FIELDS = ("low_frequency_boost", "low_frequency_boost_curvature", "high_pass_frequency", "threshold", "threshold_softness", "composite_mode",
           "max_mip_dimension", "tonemapping")


def present_settings(**settings) -> _lib.CPresentSettings:
    """the reference camera's settings (setup.rs:347-383) with the given fields replaced"""
    s = _lib.CPresentSettings()
    _lib.load().pvq_present_default_settings(C.byref(s))
    for k, v in settings.items():
        if k not in _FIELDS:
            raise TypeError(f"unknown present setting {k!r}")
        setattr(s, k, v)
    return s


def present_mips(width: int, height: int, max_mip_dimension: int = 0) -> list:
    """[(w, h)] of mip 0 .. n_mips - 1"""
    L = _lib.load()
    n = C.c_uint32()
    sizes = np.zeros((11, 2), np.uint32)
    _checked(L, L.pvq_present_mips(int(width), int(height), int(max_mip_dimension), C.byref(n), sizes.ctypes.data_as(C.POINTER(C.c_uint32))))
    return [(int(w), int(h)) for w, h in sizes[:n.value]]


def present_blend_factors(intensity: float, n_mips: int, **settings) -> np.ndarray:
    """B_0 .. B_{n_mips - 1}"""
    L = _lib.load()
    out = np.empty(max(int(n_mips), 0), np.float32)
    s = present_settings(**settings)
    _checked(L, L.pvq_present_blend_factors(C.byref(s), float(intensity), int(n_mips), _f(out)))
    return out


def present_frame(image, intensity: float, hdr: bool = False, **settings):
    """``image`` [height][width][4] -> uint8 [height][width][4]; with ``hdr`` also the bloomed linear picture before the display
    transform: (bytes, float32 [height][width][4])"""
    L = _lib.load()
    img = np.ascontiguousarray(image, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image [height][width][4]")
    out = np.empty(img.shape, np.uint8)
    lin = np.empty(img.shape, np.float32) if hdr else None
    s = present_settings(**settings)
    _checked(L, L.pvq_present_frame(C.byref(s), img.shape[1], img.shape[0], _f(img), float(intensity), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    _f(lin) if hdr else None))
    return (out, lin) if hdr else out


class PresentBatch:
    """The present stage for MANY pictures on the GPU.  ``device=None``: a host-only handle (the argument checks work; the device
    call raises: no CPU fallback)."""

    def __init__(self, width: int, height: int, device: Optional[int] = 0, **settings):
        self._L = _lib.load()
        self.width, self.height, self.device = int(width), int(height), device
        self.settings = present_settings(**settings)
        self._h = C.c_void_p()
        _checked(self._L, self._L.pvq_present_batch_create(-1 if device is None else int(device), C.byref(self.settings), self.width, self.height,
                                                           C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_present_batch_destroy(h)
            self._h = None

    def set_workspace_limit(self, n_bytes: int) -> None:
        """upper bound of the mip-chain workspace (default 1 GiB): a call whose rows need more runs in pieces, with the same bits"""
        _checked(self._L, self._L.pvq_present_batch_set_workspace_limit(self._h, int(n_bytes)))

    def rows_device(self, image, intensity=None, out=None, hdr=None, stream=None):
        """Present every row of ``image`` (a float32 device tensor [...][height][width][4]; the leading dimensions are the rows).
        ``intensity``: a float32 device tensor with one value a row (``SceneBatch``'s ``bloom``), None: no bloom.  ``out``: a uint8
        device tensor of the image's shape, made when None; ``hdr``: a float32 device tensor of the image's shape for the bloomed
        linear picture (it may be ``image``), or None.  Returns ``out``.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        per = self.height * self.width * 4
        if not hasattr(image, "numel"):
            raise ValueError("image is a device tensor")
        if image.numel() % per or not image.is_contiguous() or image.element_size() != 4:
            raise ValueError("image must be a contiguous float32 tensor [...][height][width][4]")
        n = image.numel() // per
        if intensity is not None and (intensity.numel() != n or not intensity.is_contiguous() or intensity.element_size() != 4):
            raise ValueError("intensity is not a contiguous float32 tensor with one value a row")
        if out is None:
            import torch
            out = torch.empty(tuple(image.shape), dtype=torch.uint8, device=image.device)
        if out.numel() != n * per or not out.is_contiguous() or out.element_size() != 1:
            raise ValueError("out must be a contiguous uint8 tensor of the image's shape")
        if hdr is not None and (hdr.numel() != n * per or not hdr.is_contiguous() or hdr.element_size() != 4):
            raise ValueError("hdr must be a contiguous float32 tensor of the image's shape")
        _checked(self._L, self._L.pvq_present_batch_rows_device(self._h, n, _ptr(image), _ptr(intensity), _ptr(out), _ptr(hdr), _stream_handle(stream)))
        return out
