"""The synth stage (include/pvq.h, "the synth stage"): rustysynth_fork's voices from a sound bank and MIDI-style event lists — by
default the dry path, ``enable_reverb_and_chorus = false``; with ``effects=True`` its reverb and chorus too (reverb.rs, chorus.rs,
synthesizer.rs:393-475), which is what pitchvis_train renders.

* ``SynthBank.from_arrays``  — SoundFont::new after parsing (soundfont.rs, instrument_region.rs, preset_region.rs): arrays in
* ``SynthState``             — Synthesizer + MidiFileSequencer for one stream on the host (synthesizer.rs, midifile_sequencer.rs:52-104)
* ``SynthBatch``             — the same for many streams: the control rate planned on the host, the audio rate replayed on the GPU,
                               left / right rows left in device memory for ``AgcBatch.condition_device``
* ``SynthEffects``           — Reverb + Chorus alone on the host, fed with chosen inputs; ``chorus_table`` is Chorus::new's delay table

Events are a 5-tuple of arrays ``(time_s float64, channel, command, data1, data2)``, sorted by time: a stream's WHOLE list.  A handle
keeps how many it has consumed, so successive calls continue one another.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

GENERATORS = 61   # generator_type.rs:71
BLOCK = 64        # SynthesizerSettings::DEFAULT_BLOCK_SIZE
F_START, F_LOOP, F_FILTER, F_ENDS = 1, 2, 4, 8   # pvq_synth_record.flags

RECORD_DTYPE = np.dtype([("voice", "<u4"), ("flags", "<u4"), ("ratio_lo", "<u4"), ("ratio_hi", "<u4"), ("a", "<f4", (5,)), ("gain", "<f4", (4,)),
                         ("desc", "<u4"), ("key", "<i4"), ("stage", "<u4")])
assert RECORD_DTYPE.itemsize == 64
SENDS_DTYPE = np.dtype([("chorus", "<f4", (4,)), ("reverb", "<f4", (2,)), ("pad", "<u4", (2,))])   # pvq_synth_sends
assert SENDS_DTYPE.itemsize == 32
PVQ_SYNTH_EFFECTS = 1

_i16p, _i32p, _u32p, _u64p = C.POINTER(C.c_int16), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _check(st: int):
    if st == _lib.PVQ_OK:
        return
    msg = (_lib.load().pvq_last_error() or b"").decode()
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError(msg)
    from . import PvqError
    raise PvqError(st, msg)


def instrument_generator_defaults() -> np.ndarray:
    """the 61 values an instrument region starts from (instrument_region.rs:39-58)"""
    gs = np.zeros(GENERATORS, np.int16)
    gs[8] = 13500
    gs[[21, 23, 25, 26, 27, 28, 30, 33, 34, 35, 36, 38]] = -12000
    gs[43] = gs[44] = 0x7F00
    gs[46] = gs[47] = -1
    gs[56] = 100
    gs[58] = -1
    return gs


def preset_generator_defaults() -> np.ndarray:
    """preset_region.rs:32-34"""
    gs = np.zeros(GENERATORS, np.int16)
    gs[43] = gs[44] = 0x7F00
    return gs


class SynthBank:
    """A SoundFont after parsing (pvq_synth_bank_*)."""

    def __init__(self):
        raise TypeError("use SynthBank.from_arrays")

    @classmethod
    def from_arrays(cls, wave_data, samples, instrument_regions, instruments, preset_regions, presets) -> "SynthBank":
        """``wave_data`` int16; ``samples`` [n][7] = start, end, start_loop, end_loop, sample_rate, original_pitch, pitch_correction;
        ``instrument_regions`` = (gs int16 [n][61], sample index [n]): a region's generators after the defaults and its zones;
        ``instruments`` [n][2] = first region, regions; ``preset_regions`` = (gs int16 [n][61], instrument index [n]);
        ``presets`` [n][4] = bank, patch, first region, regions.  ValueError names the first bad index."""
        self = object.__new__(cls)
        self._L = _lib.load()
        self._h = C.c_void_p()
        wave = np.ascontiguousarray(wave_data, np.int16).reshape(-1)
        smp = np.ascontiguousarray(samples, np.int32).reshape(-1, 7)
        igs = np.ascontiguousarray(instrument_regions[0], np.int16).reshape(-1, GENERATORS)
        ismp = np.ascontiguousarray(instrument_regions[1], np.uint32).reshape(-1)
        ins = np.ascontiguousarray(instruments, np.uint32).reshape(-1, 2)
        pgs = np.ascontiguousarray(preset_regions[0], np.int16).reshape(-1, GENERATORS)
        pins = np.ascontiguousarray(preset_regions[1], np.uint32).reshape(-1)
        pre = np.ascontiguousarray(presets, np.int32).reshape(-1, 4)
        if igs.shape[0] != ismp.size or pgs.shape[0] != pins.size:
            raise ValueError("one sample / instrument index per region")
        _check(self._L.pvq_synth_bank_create(wave.ctypes.data_as(_i16p), wave.size, smp.ctypes.data_as(_i32p), smp.shape[0],
                                             igs.ctypes.data_as(_i16p), ismp.ctypes.data_as(_u32p), igs.shape[0], ins.ctypes.data_as(_u32p),
                                             ins.shape[0], pgs.ctypes.data_as(_i16p), pins.ctypes.data_as(_u32p), pgs.shape[0],
                                             pre.ctypes.data_as(_i32p), pre.shape[0], C.byref(self._h)))
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_synth_bank_destroy(h)
            self._h = None

    def counts(self) -> Tuple[int, int, int, int]:
        """wave values, instrument regions, preset regions, presets"""
        out = (C.c_uint64 * 4)()
        _check(self._L.pvq_synth_bank_counts(self._h, out))
        return tuple(int(x) for x in out)


def _events(ev):
    if ev is None:
        ev = ((), (), (), (), ())
    t = np.ascontiguousarray(ev[0], np.float64).reshape(-1)
    rest = [np.ascontiguousarray(a, np.int32).reshape(-1) for a in ev[1:5]]
    if any(a.size != t.size for a in rest):
        raise ValueError("the five event arrays have one length")
    return [t] + rest


def _snapshots(getter) -> List[List[Tuple[int, float, float]]]:
    counts = (C.c_uint32 * 2)()
    _check(getter(counts, None, 0, None, None, None, 0))
    n_snap, n_voices = int(counts[0]), int(counts[1])
    ptr = np.zeros(n_snap + 1, np.uint32)
    key = np.zeros(max(n_voices, 1), np.int32)
    gl = np.zeros(max(n_voices, 1), np.float32)
    gr = np.zeros(max(n_voices, 1), np.float32)
    _check(getter(counts, ptr.ctypes.data_as(_u32p), ptr.size, key.ctypes.data_as(_i32p), gl.ctypes.data_as(_fp), gr.ctypes.data_as(_fp), key.size))
    return [[(int(key[k]), float(gl[k]), float(gr[k])) for k in range(int(ptr[f]), int(ptr[f + 1]))] for f in range(n_snap)]


class SynthState:
    """One stream on the host (pvq_synth_state_*): the planner, then the replay of its plan."""

    def __init__(self, bank: SynthBank, sample_rate: int, maximum_polyphony: int = 64, effects: bool = False):
        self._L = _lib.load()
        self._bank = bank
        self.effects = bool(effects)
        self._h = C.c_void_p()
        if effects:
            _check(self._L.pvq_synth_state_create_ex(bank._h, int(sample_rate), int(maximum_polyphony), PVQ_SYNTH_EFFECTS, C.byref(self._h)))
        else:
            _check(self._L.pvq_synth_state_create(bank._h, int(sample_rate), int(maximum_polyphony), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_synth_state_destroy(h)
            self._h = None

    def render(self, events, n_blocks: int, snapshot_blocks: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """MidiFileSequencer::render over the next ``n_blocks`` blocks: (left, right), float32 ``[n_blocks * 64]``"""
        t, ch, cmd, d1, d2 = _events(events)
        snap = np.ascontiguousarray(snapshot_blocks if snapshot_blocks is not None else [], np.uint32)
        left = np.zeros(max(int(n_blocks) * BLOCK, 1), np.float32)
        right = np.zeros_like(left)
        _check(self._L.pvq_synth_state_render(self._h, t.ctypes.data_as(_dp), ch.ctypes.data_as(_i32p), cmd.ctypes.data_as(_i32p),
                                              d1.ctypes.data_as(_i32p), d2.ctypes.data_as(_i32p), t.size, int(n_blocks),
                                              snap.ctypes.data_as(_u32p) if snap.size else None, snap.size, left.ctypes.data_as(_fp),
                                              right.ctypes.data_as(_fp)))
        return left[:int(n_blocks) * BLOCK], right[:int(n_blocks) * BLOCK]

    def snapshots(self) -> List[List[Tuple[int, float, float]]]:
        """(key, current_mix_gain_left, current_mix_gain_right) of the active voices after each snapshot block of the last render"""
        return _snapshots(lambda *a: self._L.pvq_synth_state_get_snapshots(self._h, *a))

    def plan(self) -> Tuple[np.ndarray, np.ndarray]:
        """the last render's plan: (block_ptr uint32 [n_blocks + 1], records RECORD_DTYPE [n_records])"""
        counts = (C.c_uint32 * 2)()
        _check(self._L.pvq_synth_state_get_plan(self._h, counts, None, 0, None, 0))
        ptr = np.zeros(int(counts[0]) + 1, np.uint32)
        rec = np.zeros(max(int(counts[1]), 1), RECORD_DTYPE)
        _check(self._L.pvq_synth_state_get_plan(self._h, counts, ptr.ctypes.data_as(_u32p), ptr.size,
                                                C.cast(rec.ctypes.data, C.POINTER(_lib.CSynthRecord)), rec.size))
        return ptr, rec[:int(counts[1])]

    def sends(self) -> Tuple[np.ndarray, np.ndarray]:
        """the last render's effect gains: (block_ptr uint32 [n_blocks + 1], sends SENDS_DTYPE, one per record of ``plan()``); a state
        without effects has none: ([0], empty)"""
        counts = (C.c_uint32 * 2)()
        _check(self._L.pvq_synth_state_get_sends(self._h, counts, None, 0, None, 0))
        ptr = np.zeros(int(counts[0]) + 1, np.uint32)
        snd = np.zeros(max(int(counts[1]), 1), SENDS_DTYPE)
        _check(self._L.pvq_synth_state_get_sends(self._h, counts, ptr.ctypes.data_as(_u32p), ptr.size,
                                                 C.cast(snd.ctypes.data, C.POINTER(_lib.CSynthSends)), snd.size))
        return ptr, snd[:int(counts[1])]

    @property
    def active_voices(self) -> int:
        return int(self._L.pvq_synth_state_active_voices(self._h))


class SynthBatch:
    """Many streams (pvq_synth_batch_*): a wavefront per stream, a lane per voice object.  ``device=None``: a host-only handle (the
    argument checks work; rendering raises: no CPU fallback)."""

    def __init__(self, bank: SynthBank, n_streams: int, sample_rate: int, maximum_polyphony: int = 64, device: Optional[int] = 0,
                 effects: bool = False):
        self._L = _lib.load()
        self._bank = bank
        self.n_streams = int(n_streams)
        self.device = device
        self.effects = bool(effects)
        self._h = C.c_void_p()
        if effects:   # the handle then owns every stream's reverb buffers and chorus rings on the device
            _check(self._L.pvq_synth_batch_create_ex(-1 if device is None else int(device), bank._h, self.n_streams, int(sample_rate),
                                                     int(maximum_polyphony), PVQ_SYNTH_EFFECTS, C.byref(self._h)))
        else:
            _check(self._L.pvq_synth_batch_create(-1 if device is None else int(device), bank._h, self.n_streams, int(sample_rate),
                                                  int(maximum_polyphony), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_synth_batch_destroy(h)
            self._h = None

    def render(self, events, n_blocks, d_left, d_right, snapshot_blocks: Optional[Sequence[int]] = None, stream=None) -> None:
        """``events[s]``: stream s's 5-tuple (or None: no events); ``n_blocks``: one count, or one per stream; ``d_left`` / ``d_right``:
        sequences of device tensors (or raw pointers), rows of ``n_blocks[s] * 64`` float32.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        n = self.n_streams
        if np.isscalar(n_blocks):
            n_blocks = [int(n_blocks)] * n
        if len(events) != n or len(n_blocks) != n or len(d_left) != n or len(d_right) != n:
            raise ValueError("one entry per stream of the batch")
        for s in range(n):
            for t in (d_left[s], d_right[s]):
                if hasattr(t, "numel") and (t.numel() < int(n_blocks[s]) * BLOCK or t.element_size() != 4 or not t.is_contiguous()):
                    raise ValueError(f"stream {s}: a row must be a contiguous float32 tensor of at least n_blocks * 64 values")
        evs = [_events(e) for e in events]
        ptr = np.zeros(n + 1, np.uint64)
        ptr[1:] = np.cumsum([e[0].size for e in evs])
        cat = [np.ascontiguousarray(np.concatenate([e[k] for e in evs])) if n else np.zeros(0) for k in range(5)]
        cat[0] = cat[0].astype(np.float64, copy=False)
        cat[1:] = [a.astype(np.int32, copy=False) for a in cat[1:]]
        snap = np.ascontiguousarray(snapshot_blocks if snapshot_blocks is not None else [], np.uint32)
        tab = lambda ts: (C.c_void_p * n)(*[_ptr(t) for t in ts])
        _check(self._L.pvq_synth_batch_render_device(self._h, ptr.ctypes.data_as(_u64p), cat[0].ctypes.data_as(_dp), cat[1].ctypes.data_as(_i32p),
                                                     cat[2].ctypes.data_as(_i32p), cat[3].ctypes.data_as(_i32p), cat[4].ctypes.data_as(_i32p),
                                                     (C.c_size_t * n)(*[int(x) for x in n_blocks]), tab(d_left), tab(d_right),
                                                     snap.ctypes.data_as(_u32p) if snap.size else None, snap.size, _stream_handle(stream)))

    def last_times(self) -> dict:
        """the last render's cost in ms (waits for it): planner and layout on the host, upload and replay kernel on the device"""
        out, n = (C.c_float * 4)(), C.c_uint64()
        _check(self._L.pvq_synth_batch_last_times(self._h, out, C.byref(n)))
        return dict(plan_ms=float(out[0]), stage_ms=float(out[1]), upload_ms=float(out[2]), replay_ms=float(out[3]), records=int(n.value))

    def snapshots(self, stream_index: int) -> List[List[Tuple[int, float, float]]]:
        """``SynthState.snapshots`` for one stream of the last render (host data: does not wait for the device)"""
        return _snapshots(lambda *a: self._L.pvq_synth_batch_get_snapshots(self._h, int(stream_index), *a))


def chorus_table(sample_rate: int) -> np.ndarray:
    """Chorus::new's delay table (chorus.rs:24-29): float32 ``[round(sample_rate / 0.4)]``, delays in samples"""
    L = _lib.load()
    n = int(L.pvq_synth_chorus_table(int(sample_rate), None, 0))
    if n == 0:
        raise ValueError((L.pvq_last_error() or b"").decode())
    out = np.zeros(n, np.float32)
    L.pvq_synth_chorus_table(int(sample_rate), out.ctypes.data_as(_fp), out.size)
    return out


class SynthEffects:
    """Reverb + Chorus alone on the host (pvq_synth_effects_*), fed with chosen inputs: the code ``SynthState(effects=True)`` runs."""

    def __init__(self, sample_rate: int):
        self._L = _lib.load()
        self._h = C.c_void_p()
        _check(self._L.pvq_synth_effects_create(int(sample_rate), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_synth_effects_destroy(h)
            self._h = None

    def process(self, chorus_in_left, chorus_in_right, reverb_in) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """three inputs of ``n_blocks * 64`` float32 -> (chorus out left, chorus out right, reverb out left, reverb out right); the
        state goes on from call to call"""
        ins = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (chorus_in_left, chorus_in_right, reverb_in)]
        n = ins[0].size
        if n % BLOCK or any(a.size != n for a in ins):
            raise ValueError("three inputs of one length, a multiple of 64")
        outs = [np.zeros(max(n, 1), np.float32) for _ in range(4)]
        _check(self._L.pvq_synth_effects_process(self._h, n // BLOCK, *[a.ctypes.data_as(_fp) for a in ins], *[a.ctypes.data_as(_fp) for a in outs]))
        return tuple(a[:n] for a in outs)
