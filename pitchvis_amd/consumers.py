"""Callers either side of the VQT path, mirroring the reference's own items:

* ``MonoAgc``                        — dagc_fork/src/lib.rs:19-87
* ``train_dataset`` / ``write_npy``  — pitchvis_train/src/train.rs:252-351, 443-460, 192-208 (frames on the GPU)
* ``AgcBatch`` / ``train_dataset_streams`` — the same for many rendered streams at once (train.rs:146-163), conditioned on the device
* ``train_dataset_from_events``      — the same from MIDI-style events on: the voices rendered on the device too (synth.py)
* ``Stream``                         — the pitchvis_audio RingBuffer contract with a device-resident ring
* ``calculate_color`` / ``led_frame``— pitchvis_colors/src/lib.rs:86-117, pitchvis_serial/src/main.rs:122-175
* ``spectrogram_row`` / ``chroma_row`` — pitchvis_viewer/src/display_system/update.rs:961-1065, 1102-1131 (one AnalysisState, host)
* ``RenderBatch``                    — both, and the LED frame, for many rows at once on the device
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib

_fp = C.POINTER(C.c_float)


def _f(a: np.ndarray):
    return a.ctypes.data_as(_fp)


def _check(st: int):
    if st != _lib.PVQ_OK:
        L = _lib.load()
        from . import PvqError
        raise PvqError(st, (L.pvq_last_error() or b"").decode())


class MonoAgc:
    """dagc::MonoAgc (dagc_fork/src/lib.rs:19-87)"""

    def __init__(self, desired_output_rms: float, distortion_factor: float):
        self._L = _lib.load()
        self._h = C.c_void_p()
        st = self._L.pvq_mono_agc_create(desired_output_rms, distortion_factor, C.byref(self._h))
        if st != _lib.PVQ_OK:
            raise ValueError((self._L.pvq_last_error() or b"").decode())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_mono_agc_destroy(h)
            self._h = None

    def freeze_gain(self, freeze: bool) -> None:
        self._L.pvq_mono_agc_freeze_gain(self._h, int(bool(freeze)))

    def is_gain_frozen(self) -> bool:
        return bool(self._L.pvq_mono_agc_is_gain_frozen(self._h))

    def gain(self) -> float:
        return float(self._L.pvq_mono_agc_gain(self._h))

    def process(self, samples: np.ndarray) -> None:
        """in place, like the reference (lib.rs:76)"""
        assert samples.dtype == np.float32 and samples.flags.c_contiguous
        self._L.pvq_mono_agc_process(self._h, _f(samples), samples.size)


STEP_SIZE_IN_CHUNKS = 3   # train.rs:44


def train_chunk_samples(vqt) -> int:
    """train.rs:128-129"""
    return int(_lib.load().pvq_train_chunk_samples(vqt._h))


def train_dataset(vqt, left: np.ndarray, right: Optional[np.ndarray], voices: Sequence[Sequence[Tuple[int, float, float]]],
                  step: int = STEP_SIZE_IN_CHUNKS, agc: Optional[MonoAgc] = None, chunk: Optional[int] = None) -> np.ndarray:
    """The body of pitchvis_train::synthesize_midi_to_wav + generate_data for one rendered stream
    (train.rs:252-351, 443-460).  ``left``/``right``: the synthesizer's output, a whole number of chunks;
    ``voices[f]``: (key, mix_gain_left, mix_gain_right) of the voices sounding at analysed chunk f.
    Returns the flat float32 rows ``[n_frames * (n_bins + 128)]`` that train() concatenates into data.npy."""
    L = _lib.load()
    chunk = train_chunk_samples(vqt) if chunk is None else int(chunk)
    left = np.ascontiguousarray(left, np.float32)
    n_chunks = left.size // chunk
    assert n_chunks * chunk == left.size, "the stream must be a whole number of chunks"
    if right is not None:
        right = np.ascontiguousarray(right, np.float32)
        assert right.size == left.size
    agc = agc or MonoAgc(0.07, 0.001)   # train.rs:265
    mono = np.empty(n_chunks * chunk, np.float32)
    gains = np.empty(n_chunks, np.float32)
    _check(L.pvq_train_condition_stream(agc._h, _f(left), _f(right) if right is not None else None, n_chunks, chunk,
                                        _f(mono), _f(gains)))
    n_frames = n_chunks // step
    db = np.empty((n_frames, vqt.n_bins), np.float32)
    _check(L.pvq_train_frames_db(vqt._h, _f(mono), n_chunks, chunk, step, _f(db)))
    return _train_rows(L, vqt.n_bins, db, gains, voices, step)


def _train_rows(L, n_bins: int, db: np.ndarray, gains: np.ndarray, voices, step: int) -> np.ndarray:
    """train.rs:317-337, 347, 443-460 for one stream: db [n_frames][n_bins], gains [n_chunks] -> flat rows"""
    n_frames = db.shape[0]
    assert len(voices) == n_frames
    ptr = np.zeros(n_frames + 1, np.uint32)
    keys, gl, gr = [], [], []
    for f, vs in enumerate(voices):
        for k, a, b in vs:
            keys.append(k); gl.append(a); gr.append(b)
        ptr[f + 1] = len(keys)
    keys = np.asarray(keys if keys else [0], np.int32)
    gl = np.asarray(gl if gl else [0], np.float32)
    gr = np.asarray(gr if gr else [0], np.float32)
    agc_gain = np.ascontiguousarray(gains[step - 1::step][:n_frames])   # agc.gain() at the analysed chunks (train.rs:326)
    rows = np.empty((n_frames, n_bins + 128), np.float32)
    _check(L.pvq_train_rows(_f(db), n_frames, n_bins, ptr.ctypes.data_as(C.POINTER(C.c_uint32)),
                            keys.ctypes.data_as(C.POINTER(C.c_int32)), _f(gl), _f(gr), _f(agc_gain), _f(rows)))
    return rows.reshape(-1)


class AgcBatch:
    """One dagc::MonoAgc per stream for MANY streams on the GPU (pvq_agc_batch_*): the trainer's conditioning (train.rs:286-301:
    downmix, silence gate, AGC) with a lane per stream, the bits of ``pvq_train_condition_stream``; gains kept between calls.
    ``device=None``: a host-only handle (the argument checks work; conditioning raises: no CPU fallback)."""

    def __init__(self, n_streams: int, desired_output_rms: float, distortion_factor: float, device: Optional[int] = 0):
        self._L = _lib.load()
        self.n_streams = int(n_streams)
        self._h = C.c_void_p()
        st = self._L.pvq_agc_batch_create(-1 if device is None else int(device), self.n_streams, desired_output_rms, distortion_factor,
                                          C.byref(self._h))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_agc_batch_destroy(h)
            self._h = None

    def condition_device(self, d_lefts, d_rights, n_chunks, chunk: int, d_outs=None, d_gain_out=None, gain_stride: Optional[int] = None,
                         stream=None) -> None:
        """d_lefts / d_rights / d_outs: sequences of device tensors (or raw pointers), one per stream; d_rights None, or an entry
        None: mono; d_outs None: in place over d_lefts.  d_gain_out: device tensor [n_streams][gain_stride] (default stride: its
        second dimension).  Asynchronous on `stream`."""
        from . import _ptr, _stream_handle
        n = self.n_streams
        if len(d_lefts) != n or len(n_chunks) != n or (d_rights is not None and len(d_rights) != n) or (d_outs is not None and len(d_outs) != n):
            raise ValueError("one entry per stream of the batch")
        tab = lambda ts: (C.c_void_p * n)(*[_ptr(t) for t in ts])
        lefts = tab(d_lefts)
        if gain_stride is None:
            gain_stride = int(d_gain_out.shape[1]) if d_gain_out is not None else 0
        _check(self._L.pvq_agc_batch_condition_device(self._h, lefts, tab(d_rights) if d_rights is not None else None,
                                                      (C.c_size_t * n)(*[int(x) for x in n_chunks]), int(chunk),
                                                      tab(d_outs) if d_outs is not None else lefts, _ptr(d_gain_out), int(gain_stride),
                                                      _stream_handle(stream)))

    def gains(self) -> np.ndarray:
        """MonoAgc::gain of every stream after the last call (synchronises)"""
        out = np.empty(self.n_streams, np.float32)
        _check(self._L.pvq_agc_batch_get_gains(self._h, _f(out)))
        return out


def train_dataset_streams(vqt, lefts, rights, voices, step: int = STEP_SIZE_IN_CHUNKS):
    """``train_dataset`` for MANY rendered streams at once, the trainer's par_iter over files (train.rs:146-163): every stream is
    uploaded once, conditioned on the device (one MonoAgc(0.07, 0.001) each, train.rs:265), all frames of all streams come from ONE
    many-streams transform call, and only dB rows and per-chunk gains come back.  ``lefts[s]`` / ``rights[s]`` (``rights`` or an
    entry None: mono) / ``voices[s]`` as ``train_dataset``'s arguments.  Returns one flat row array per stream, laid out as
    ``train_dataset``'s."""
    import torch
    L = _lib.load()
    n = len(lefts)
    if n == 0:
        return []
    chunk = train_chunk_samples(vqt)
    dev = torch.device("cuda", vqt.device)
    n_chunks, d_l, d_r = [], [], []
    for s in range(n):
        left = np.ascontiguousarray(lefts[s], np.float32)
        nc = left.size // chunk
        assert nc * chunk == left.size, "every stream must be a whole number of chunks"
        n_chunks.append(nc)
        d_l.append(torch.from_numpy(left).to(dev))
        right = rights[s] if rights is not None else None
        if right is not None:
            right = np.ascontiguousarray(right, np.float32)
            assert right.size == left.size
            d_r.append(torch.from_numpy(right).to(dev))
        else:
            d_r.append(None)
    n_frames = [nc // step for nc in n_chunks]
    max_chunks, max_frames = max(max(n_chunks), 1), max(max(n_frames), 1)
    with torch.cuda.device(dev):
        agc = AgcBatch(n, 0.07, 0.001, device=vqt.device)   # train.rs:265
        d_gain = torch.zeros((n, max_chunks), dtype=torch.float32, device=dev)
        agc.condition_device(d_l, d_r, n_chunks, chunk, d_gain_out=d_gain)   # in place: d_l now holds the conditioned mono streams
        d_db = torch.empty((n, max_frames, vqt.n_bins), dtype=torch.float32, device=dev)
        vqt.batch_streams_device(d_l, chunk * step, n_frames, d_db, out_stride_frames=max_frames)   # the ring buffer of train.rs:268-269: zeros before the stream
        vqt.input_status()   # (waits; raises on a non-finite sample like pvq_train_frames_db)
        db = d_db.cpu().numpy()
        gains = d_gain.cpu().numpy()
    return [_train_rows(L, vqt.n_bins, np.ascontiguousarray(db[s, :n_frames[s]]), gains[s, :n_chunks[s]], voices[s], step) for s in range(n)]


def train_dataset_from_events(vqt, bank, events, n_chunks, step: int = STEP_SIZE_IN_CHUNKS, maximum_polyphony: int = 64, effects: bool = False):
    """``train_dataset_streams`` with the first link on the device too (train.rs:252-351 from the MIDI events on): every stream's
    events are planned on the host and its voices rendered on the device (``SynthBatch``, the synthesizer's dry path) into left /
    right rows that go straight to ``AgcBatch.condition_device``; the active voices after every analysed chunk (train.rs:317-337)
    become the targets.  No PCM crosses to the host.  ``events[s]``: stream s's ``(time_s, channel, command, data1, data2)``;
    ``n_chunks``: chunks to render, one count or one per stream.  Returns one flat row array per stream, laid out as
    ``train_dataset``'s.  ``effects=True``: the synthesizer's reverb and chorus too, the trainer's own setting (train.rs:264)."""
    import torch
    from .synth import BLOCK, SynthBatch
    L = _lib.load()
    n = len(events)
    if n == 0:
        return []
    chunk = train_chunk_samples(vqt)
    assert chunk % BLOCK == 0   # train.rs:128-129
    n_chunks = [int(n_chunks)] * n if np.isscalar(n_chunks) else [int(x) for x in n_chunks]
    n_frames = [nc // step for nc in n_chunks]
    max_chunks, max_frames = max(max(n_chunks), 1), max(max(n_frames), 1)
    per_chunk = chunk // BLOCK
    dev = torch.device("cuda", vqt.device)
    with torch.cuda.device(dev):
        synth = SynthBatch(bank, n, int(vqt.params().sr), maximum_polyphony, device=vqt.device, effects=effects)
        d_l = [torch.empty(max(nc * chunk, 1), dtype=torch.float32, device=dev) for nc in n_chunks]
        d_r = [torch.empty(max(nc * chunk, 1), dtype=torch.float32, device=dev) for nc in n_chunks]
        snapshot_blocks = [(f + 1) * step * per_chunk - 1 for f in range(max_frames)]
        synth.render(events, [nc * per_chunk for nc in n_chunks], d_l, d_r, snapshot_blocks=snapshot_blocks)
        agc = AgcBatch(n, 0.07, 0.001, device=vqt.device)   # train.rs:265
        d_gain = torch.zeros((n, max_chunks), dtype=torch.float32, device=dev)
        agc.condition_device(d_l, d_r, n_chunks, chunk, d_gain_out=d_gain)   # in place: d_l now holds the conditioned mono streams
        d_db = torch.empty((n, max_frames, vqt.n_bins), dtype=torch.float32, device=dev)
        vqt.batch_streams_device(d_l, chunk * step, n_frames, d_db, out_stride_frames=max_frames)
        vqt.input_status()
        db = d_db.cpu().numpy()
        gains = d_gain.cpu().numpy()
    voices = [synth.snapshots(s)[:n_frames[s]] for s in range(n)]
    return [_train_rows(L, vqt.n_bins, np.ascontiguousarray(db[s, :n_frames[s]]), gains[s, :n_chunks[s]], voices[s], step) for s in range(n)]


def write_npy(path: str, data: np.ndarray) -> None:
    """train.rs:192-208: flat '<f4' .npy"""
    data = np.ascontiguousarray(data, np.float32).reshape(-1)
    _check(_lib.load().pvq_npy_write_f32(str(path).encode(), _f(data), data.size))


class Stream:
    """pitchvis_audio::RingBuffer (lib.rs:17-22) fed like audio_desktop.rs:88-131, ring on the device"""

    def __init__(self, vqt, buf_size: int, with_agc: bool = True):
        self._L = _lib.load()
        self._vqt = vqt
        self._h = C.c_void_p()
        self.buf_size = int(buf_size)
        _check(self._L.pvq_stream_create(vqt._h, buf_size, int(with_agc), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_stream_destroy(h)
            self._h = None

    def push(self, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, np.float32)
        _check(self._L.pvq_stream_push(self._h, _f(data), data.size))

    @property
    def gain(self) -> float:
        return float(self._L.pvq_stream_gain(self._h))

    @property
    def chunk_size_ms(self) -> float:
        return float(self._L.pvq_stream_chunk_size_ms(self._h))

    def frame_db(self) -> np.ndarray:
        out = np.empty(self._vqt.n_bins, np.float32)
        _check(self._L.pvq_stream_frame_db(self._h, _f(out)))
        return out

    def read(self, n_last: Optional[int] = None) -> np.ndarray:
        n = self.buf_size if n_last is None else int(n_last)
        out = np.empty(n, np.float32)
        _check(self._L.pvq_stream_read(self._h, _f(out), n))
        return out


class PinnedArray:
    """float32 NumPy view of page-locked host memory (pvq_host_alloc): hand `.array` to the host-buffer entry points"""

    def __init__(self, shape):
        self._L = _lib.load()
        n = int(np.prod(shape))
        self._p = self._L.pvq_host_alloc(4 * max(n, 1))
        if not self._p:
            raise MemoryError((self._L.pvq_last_error() or b"").decode())
        buf = (C.c_float * max(n, 1)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=np.float32, count=n).reshape(shape)

    def __del__(self):
        p = getattr(self, "_p", None)
        if p:
            self.array = None
            self._L.pvq_host_free(p)
            self._p = None


# pitchvis_colors/src/lib.rs:19-36
COLORS = np.array([
    [0.85, 0.36, 0.36], [0.01, 0.52, 0.71], [0.97, 0.76, 0.05], [0.45, 0.34, 0.63], [0.47, 0.77, 0.22], [0.78, 0.32, 0.52],
    [0.00, 0.64, 0.56], [0.95, 0.54, 0.23], [0.30, 0.37, 0.64], [1.00, 0.96, 0.03], [0.57, 0.30, 0.55], [0.12, 0.71, 0.34],
], np.float32)
GRAY_LEVEL, EASING_POW = 60.0, 1.3                       # lib.rs:56-57
# pitchvis_serial/src/main.rs:44-59
SERIAL_COLORS = np.array([
    [0.95, 0.10, 0.10], [0.01, 0.52, 0.71], [0.97, 0.79, 0.00], [0.45, 0.34, 0.63], [0.47, 0.99, 0.02], [0.88, 0.02, 0.52],
    [0.00, 0.80, 0.55], [0.99, 0.54, 0.03], [0.25, 0.30, 0.64], [0.95, 0.99, 0.00], [0.52, 0.00, 0.60], [0.05, 0.80, 0.15],
], np.float32)
SERIAL_GRAY_LEVEL, SERIAL_EASING_POW = 5.0, 2.3


def calculate_color(buckets_per_octave: int, bucket: float, colors: np.ndarray = COLORS, gray_level: float = GRAY_LEVEL,
                    easing_pow: float = EASING_POW) -> Tuple[float, float, float]:
    colors = np.ascontiguousarray(colors, np.float32)
    out = np.empty(3, np.float32)
    _lib.load().pvq_calculate_color(buckets_per_octave, bucket, _f(colors), gray_level, easing_pow, _f(out))
    return float(out[0]), float(out[1]), float(out[2])


def led_frame(n_buckets: int, buckets_per_octave: int, peaks_continuous: Sequence[Tuple[float, float]],
              colors: np.ndarray = SERIAL_COLORS, gray_level: float = SERIAL_GRAY_LEVEL,
              easing_pow: float = SERIAL_EASING_POW) -> bytes:
    """pitchvis_serial::update_serial (main.rs:122-175): the bytes written to the serial port"""
    colors = np.ascontiguousarray(colors, np.float32)
    ctr = np.asarray([p[0] for p in peaks_continuous] or [0.0], np.float32)
    sz = np.asarray([p[1] for p in peaks_continuous] or [0.0], np.float32)
    out = np.zeros(3 + 3 * n_buckets, np.uint8)
    n = _lib.load().pvq_led_frame(n_buckets, buckets_per_octave, _f(ctr), _f(sz), len(peaks_continuous), _f(colors), gray_level,
                                  easing_pow, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out[:n].tobytes()


SPECTROGRAM_VQT, SPECTROGRAM_PEAKS = _lib.SPECTROGRAM_VQT, _lib.SPECTROGRAM_PEAKS   # SpectrogramMode (update.rs:959-961)


def spectrogram_row(mode: int, n_buckets: int, buckets_per_octave: int, x_vqt_smoothed=None,
                    peaks_continuous: Sequence[Tuple[float, float]] = (), colors: np.ndarray = COLORS, gray_level: float = GRAY_LEVEL,
                    easing_pow: float = EASING_POW) -> np.ndarray:
    """update_spectrogram_system's match (update.rs:961-1065): the RGBA row written at write_index, uint8 ``[n_buckets][4]``.
    SPECTROGRAM_VQT reads ``x_vqt_smoothed``, SPECTROGRAM_PEAKS ``peaks_continuous`` ((center, size) in list order).  The texture
    ring, its flip and the clearing of the next line stay with the caller."""
    colors = np.ascontiguousarray(colors, np.float32)
    x = None if x_vqt_smoothed is None else np.ascontiguousarray(x_vqt_smoothed, np.float32)
    if x is not None and x.size != n_buckets:
        raise ValueError("x_vqt_smoothed must hold n_buckets values")
    ctr = np.asarray([p[0] for p in peaks_continuous] or [0.0], np.float32)
    sz = np.asarray([p[1] for p in peaks_continuous] or [0.0], np.float32)
    out = np.zeros((n_buckets, 4), np.uint8)
    L = _lib.load()
    st = L.pvq_spectrogram_row(int(mode), n_buckets, buckets_per_octave, _f(x) if x is not None else None, _f(ctr), _f(sz),
                               len(peaks_continuous), _f(colors), gray_level, easing_pow, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((L.pvq_last_error() or b"").decode())
    _check(st)
    return out


def chroma_row(min_freq: float, n_buckets: int, buckets_per_octave: int, x_vqt_smoothed) -> np.ndarray:
    """update_chroma_system's chroma (update.rs:1102-1131): twelve strengths, the largest 1.0 (float32)"""
    x = np.ascontiguousarray(x_vqt_smoothed, np.float32)
    if x.size != n_buckets:
        raise ValueError("x_vqt_smoothed must hold n_buckets values")
    out = np.zeros(12, np.float32)
    L = _lib.load()
    st = L.pvq_chroma_row(min_freq, n_buckets, buckets_per_octave, _f(x), _f(out))
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((L.pvq_last_error() or b"").decode())
    _check(st)
    return out


class RenderBatch:
    """The viewer's spectrogram row (both modes), its chroma strengths and the serial LED frame for MANY rows on the GPU
    (pvq_render_batch_*): a row is one frame of one stream, a wavefront renders it from the fields ``AnalysisBatch`` leaves in device
    memory.  Stateless; one geometry and one palette per object (the LED strip's own: ``colors=SERIAL_COLORS,
    gray_level=SERIAL_GRAY_LEVEL, easing_pow=SERIAL_EASING_POW``).  ``device=None``: a host-only handle (the argument checks work;
    rendering raises: no CPU fallback)."""

    OUTPUTS = ("spectrogram_vqt", "spectrogram_peaks", "chroma", "led")

    def __init__(self, range, colors: Optional[np.ndarray] = None, gray_level: float = GRAY_LEVEL, easing_pow: float = EASING_POW,
                 device: Optional[int] = 0):
        self._L = _lib.load()
        self.range = range
        self.n_bins = range.octaves * range.buckets_per_octave
        self.device = device
        self._h = C.c_void_p()
        pal = None if colors is None else np.ascontiguousarray(colors, np.float32)
        if pal is not None and pal.shape != (12, 3):
            raise ValueError("colors: 12 RGB triples")
        st = self._L.pvq_render_batch_create(-1 if device is None else int(device), range.min_freq, range.octaves, range.buckets_per_octave,
                                             _f(pal) if pal is not None else None, gray_level, easing_pow, C.byref(self._h))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_render_batch_destroy(h)
            self._h = None

    def output_shape(self, name: str, n_rows: int):
        """(shape, numpy dtype) of an output for n_rows rows"""
        return {"spectrogram_vqt": ((n_rows, self.n_bins, 4), np.uint8), "spectrogram_peaks": ((n_rows, self.n_bins, 4), np.uint8),
                "chroma": ((n_rows, 12), np.float32), "led": ((n_rows, 3 + 3 * self.n_bins), np.uint8)}[name]

    def rows_device(self, fields=None, outputs=None, *, x_vqt_smoothed=None, center=None, size=None, peak_count=None,
                    n_rows: Optional[int] = None, max_peaks: Optional[int] = None, stream=None) -> dict:
        """Render every row.  Inputs: torch device tensors, by keyword or as the dict ``AnalysisBatch.preprocess_device`` fills
        (``fields``; keys ``x_vqt_smoothed``, ``center``, ``size``, ``peak_count``; leading dimensions are flattened to rows, nothing
        is copied).  ``outputs``: a dict name -> device tensor to fill, or a sequence of names to allocate (default: every output the
        given inputs allow).  ``n_rows`` / ``max_peaks`` default to what the tensors' shapes say (raw pointers need them).
        Returns the dict of output tensors.  Asynchronous on ``stream``."""
        from . import _ptr, _stream_handle
        f = dict(fields or {})
        x = x_vqt_smoothed if x_vqt_smoothed is not None else f.get("x_vqt_smoothed")
        ctr = center if center is not None else f.get("center")
        sz = size if size is not None else f.get("size")
        cnt = peak_count if peak_count is not None else f.get("peak_count")
        if max_peaks is None:
            max_peaks = int(ctr.shape[-1]) if hasattr(ctr, "shape") else 0
        if n_rows is None:
            if hasattr(x, "numel"):
                n_rows = x.numel() // self.n_bins
            elif hasattr(cnt, "numel"):
                n_rows = cnt.numel()
            else:
                raise ValueError("n_rows is needed with raw pointers")
        for t, per_row in ((x, self.n_bins), (ctr, max_peaks), (sz, max_peaks), (cnt, 1)):
            if hasattr(t, "numel"):
                if t.numel() != n_rows * per_row or not t.is_contiguous() or t.element_size() != 4:
                    raise ValueError("an input tensor is not contiguous 32-bit [n_rows][...]")
        if outputs is None:
            outputs = [n for n in self.OUTPUTS if (x is not None if n in ("spectrogram_vqt", "chroma") else
                                                   (ctr is not None and sz is not None and cnt is not None))]
        if not isinstance(outputs, dict):
            import torch
            dev = next(t.device for t in (x, ctr, cnt) if hasattr(t, "device"))
            made = {}
            for name in outputs:
                shape, dt = self.output_shape(name, n_rows)
                made[name] = torch.empty(shape, dtype=torch.uint8 if dt == np.uint8 else torch.float32, device=dev)
            outputs = made
        o = _lib.CRenderOutputs()
        for name, t in outputs.items():
            if name not in self.OUTPUTS:
                raise ValueError(f"unknown output {name!r}")
            if hasattr(t, "numel"):
                shape, dt = self.output_shape(name, n_rows)
                if t.numel() != int(np.prod(shape)) or not t.is_contiguous() or t.element_size() != np.dtype(dt).itemsize:
                    raise ValueError(f"output {name!r} must be a contiguous {np.dtype(dt).name} tensor of shape {shape}")
            setattr(o, name, _ptr(t))
        st = self._L.pvq_render_batch_rows_device(self._h, int(n_rows), _ptr(x), _ptr(ctr), _ptr(sz), _ptr(cnt), int(max_peaks), C.byref(o),
                                                  _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        return outputs
