"""The many-streams conditioning on the GPU (pvq_agc_batch_*: downmix, silence gate, MonoAgc, a lane per stream) against the host code it
batches: pvq_train_condition_stream / pvq_mono_agc_process, themselves pinned bit for bit to the oracle's MonoAgc / train_loop in
test_consumers.py.  Every equality below is on the uint32 view of the f32 values: no tolerance (the one stated exception: NaNs in
test_odd_values)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pitchvis_amd as P
from pitchvis_amd import _lib

pytestmark = pytest.mark.gpu

_fp = C.POINTER(C.c_float)
SENTINEL = np.float32(-12345.5)


def _train_params():
    # pitchvis_train/src/train.rs:30-42 (tests/test_consumers_gpu.py::_train_params)
    q = 10.0
    return P.VqtParameters(sr=22050.0, n_fft=32768, range=P.VqtRange(55.0, 7, 36), sparsity_quantile=0.999, quality=q, gamma=5.3 * q)


def _trainer_chunk():
    return P.train_chunk_samples(P.Vqt.new(_train_params(), None))   # 1 984 = 31 x 64


def _render(n, sr, seed, n_notes=5):
    """the seeded piano-roll stand-in of tests/test_consumers_gpu.py::_render (fewer notes and partials: 200 streams are rendered)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    left = np.zeros(n)
    right = np.zeros(n)
    notes = []
    for _ in range(n_notes):
        key = int(rng.integers(40, 90))
        t0 = float(rng.uniform(0, t[-1] * 0.8))
        f0 = 440.0 * 2 ** ((key - 69) / 12)
        env = np.where(t >= t0, np.exp(-(t - t0) * 3.0), 0.0)
        tone = sum(np.sin(2 * np.pi * f0 * h * t) / h ** 2 for h in range(1, 4)) * env * 0.2
        pan = rng.uniform(0.2, 0.8)
        left += tone * pan
        right += tone * (1 - pan)
        notes.append((key, t0, pan))
    return left.astype(np.float32), right.astype(np.float32), notes


def _noise(n, seed, amp=0.2):
    """a tone with noise on it: no sample is exactly zero, cheap to make"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    f = rng.uniform(100.0, 2000.0)
    left = (amp * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    right = (amp * 0.7 * np.sin(2 * np.pi * 1.5 * f * t) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    return left, right


def _host(rms, d, left, right, n_chunks, chunk, agc=None):
    """the yardstick: pvq_train_condition_stream on one MonoAgc -> (mono, gain after each chunk, the agc)"""
    L = _lib.load()
    agc = agc or P.MonoAgc(rms, d)
    mono = np.empty(n_chunks * chunk, np.float32)
    gains = np.empty(n_chunks, np.float32)
    f = lambda a: a.ctypes.data_as(_fp)
    st = L.pvq_train_condition_stream(agc._h, f(left), f(right) if right is not None else None, n_chunks, chunk, f(mono), f(gains))
    assert st == _lib.PVQ_OK
    return mono, gains, agc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), float(np.asarray(got).reshape(-1)[bad[0]]), float(np.asarray(want).reshape(-1)[bad[0]]))


def _device(batch, lefts, rights, n_chunks, chunk, in_place=False, pad=0, gain_pad=0):
    """one condition call on fresh uploads -> (outs [tensor incl. pad], gains [n][max + gain_pad] numpy)"""
    d_l = [torch.from_numpy(x).cuda() for x in lefts]
    d_r = None if rights is None else [None if x is None else torch.from_numpy(x).cuda() for x in rights]
    if in_place:
        d_o = None
    else:
        d_o = [torch.full((n_chunks[s] * chunk + pad,), float(SENTINEL), device="cuda") for s in range(len(lefts))]
    d_g = torch.full((len(lefts), max(n_chunks) + gain_pad), float(SENTINEL), device="cuda")
    batch.condition_device(d_l, d_r, n_chunks, chunk, d_outs=d_o, d_gain_out=d_g)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (d_l if in_place else d_o)], d_g.cpu().numpy()


# ---- 200 streams at the trainer geometry ---------------------------------------------------------------------------------------
N_MANY = 200


@pytest.fixture(scope="module")
def many():
    chunk = _trainer_chunk()
    rng = np.random.default_rng(2024)
    n_chunks = [int(x) for x in rng.integers(3, 41, N_MANY)]
    n_chunks[0], n_chunks[1] = 40, 3
    lefts, rights = [], []
    for s in range(N_MANY):
        left, right, _ = _render(n_chunks[s] * chunk, 22050.0, 1000 + s)
        if s % 4 == 0:      # exact zeros over whole chunks: the silence gate
            a = min(1, n_chunks[s] - 2)
            b = min(a + 2, n_chunks[s])
            left[a * chunk:b * chunk] = 0.0
            right[a * chunk:b * chunk] = 0.0
        if s % 7 == 0:      # a burst of amplitude 20: the clamp g = d
            o = (n_chunks[s] - 1) * chunk + 777
            left[o:o + 10] = 20.0
            right[o:o + 10] = 20.0
        lefts.append(left)
        rights.append(right)
    return chunk, n_chunks, lefts, rights


@pytest.mark.parametrize("table", ["stereo", "mono", "mixed"])
def test_bit_identity_many_streams(many, table):
    chunk, n_chunks, lefts, rights = many
    rms, d = 0.07, 0.001   # train.rs:265
    if table == "stereo":
        rs = list(rights)
    elif table == "mono":
        rs = None
    else:
        rs = [rights[s] if s % 3 else None for s in range(N_MANY)]
    want = [_host(rms, d, lefts[s], rs[s] if rs is not None else None, n_chunks[s], chunk) for s in range(N_MANY)]
    # the stimulus reaches all three branches ON THE HOST: a frozen chunk (gain equal before and after it), an unfrozen one, and the clamp
    # g = d (a conditioned sample x of an unfrozen chunk with x^2 / rms > 1 / d, i.e. |x| > sqrt(rms / d) = 8.37)
    frozen = unfrozen = clamped = 0
    for s in range(N_MANY):
        mono, gains, _ = want[s]
        before = np.concatenate([[np.float32(1.0)], gains[:-1]])
        fz = _bits(before) == _bits(gains)
        frozen += int(fz.sum())
        unfrozen += int((~fz).sum())
        for c in np.nonzero(~fz)[0]:
            clamped += int((np.abs(mono[c * chunk:(c + 1) * chunk]) > np.sqrt(rms / d)).sum())
    assert frozen >= 1 and unfrozen >= 1 and clamped >= 1, (frozen, unfrozen, clamped)
    batch = P.AgcBatch(N_MANY, rms, d)
    outs, gains = _device(batch, lefts, rs, n_chunks, chunk, gain_pad=2)
    final = batch.gains()
    for s in range(N_MANY):
        _assert_bits(outs[s], want[s][0], ("samples", table, s))
        _assert_bits(gains[s, :n_chunks[s]], want[s][1], ("gains", table, s))
        assert np.all(gains[s, n_chunks[s]:] == SENTINEL), s
        _assert_bits([final[s]], [want[s][2].gain()], ("final gain", table, s))


@pytest.mark.parametrize("chunk", [64, "trainer", 1000])   # 1 000: no multiple of 64, nor of the tile
@pytest.mark.parametrize("rms,d", [(0.07, 0.0001),    # audio_desktop.rs:93
                                   (0.001, 0.0001),   # the crate's own test
                                   (0.5, 0.0), (0.07, 1.0)])
def test_other_parameters(rms, d, chunk):
    chunk = _trainer_chunk() if chunk == "trainer" else chunk
    n = 64
    rng = np.random.default_rng(7)
    n_chunks = [int(x) for x in rng.integers(2, 9, n)]
    lefts, rights = [], []
    for s in range(n):
        left, right = _noise(n_chunks[s] * chunk, 50 + s)
        if s % 5 == 0:
            left[:chunk] = 0.0
            right[:chunk] = 0.0
        lefts.append(left)
        rights.append(right if s % 2 else None)
    batch = P.AgcBatch(n, rms, d)
    outs, gains = _device(batch, lefts, rights, n_chunks, chunk)
    final = batch.gains()
    for s in range(n):
        mono, g, agc = _host(rms, d, lefts[s], rights[s], n_chunks[s], chunk)
        _assert_bits(outs[s], mono, ("samples", s))
        _assert_bits(gains[s, :n_chunks[s]], g, ("gains", s))
        _assert_bits([final[s]], [agc.gain()], ("final gain", s))


@pytest.mark.parametrize("chunk", [999, 7])
def test_any_chunk_and_rows_off_the_16_byte_grid(chunk):
    """a chunk that is no multiple of 4 (the recurrence then looks at the chunk boundary after every sample) and rows that start 4, 8 or
    12 bytes off a 16-byte boundary (the tiles are then filled and drained dword by dword)"""
    n = 66
    rng = np.random.default_rng(13)
    n_chunks = [int(x) for x in rng.integers(1, 12, n)]
    lefts, rights = [], []
    for s in range(n):
        left, right = _noise(n_chunks[s] * chunk, 500 + s)
        if s % 5 == 0:
            left[:chunk] = 0.0
            right[:chunk] = 0.0
        lefts.append(left)
        rights.append(right if s % 2 else None)
    batch = P.AgcBatch(n, 0.07, 0.001)
    off = lambda s, x: torch.cat([torch.full((s % 4,), float(SENTINEL)), torch.from_numpy(x), torch.full((5,), float(SENTINEL))]).cuda()
    d_l = [off(s, x)[s % 4:] for s, x in enumerate(lefts)]
    d_r = [None if x is None else off(s + 1, x)[(s + 1) % 4:] for s, x in enumerate(rights)]
    hold = [torch.full((n_chunks[s] * chunk + 9,), float(SENTINEL), device="cuda") for s in range(n)]
    d_o = [hold[s][(s + 2) % 4:] for s in range(n)]
    d_g = torch.full((n, 12), float(SENTINEL), device="cuda")
    batch.condition_device(d_l, d_r, n_chunks, chunk, d_outs=d_o, d_gain_out=d_g)
    torch.cuda.synchronize()
    gains = d_g.cpu().numpy()
    for s in range(n):
        mono, g, _ = _host(0.07, 0.001, lefts[s], rights[s], n_chunks[s], chunk)
        m, lead = n_chunks[s] * chunk, (s + 2) % 4
        got = hold[s].cpu().numpy()
        _assert_bits(got[lead:lead + m], mono, ("samples", s))
        assert np.all(got[:lead] == SENTINEL) and np.all(got[lead + m:] == SENTINEL), s
        _assert_bits(gains[s, :n_chunks[s]], g, ("gains", s))
        assert np.all(gains[s, n_chunks[s]:] == SENTINEL), s


def test_state_across_calls():
    """one call over 30 chunks equals three calls over 10 + 1 + 19 chunks (every stream's gain persists like one MonoAgc's)"""
    chunk, n, total = _trainer_chunk(), 70, 30
    lefts, rights = zip(*[_noise(total * chunk, 300 + s) for s in range(n)])
    for s in range(0, n, 6):
        lefts[s][9 * chunk:12 * chunk] = 0.0
        rights[s][9 * chunk:12 * chunk] = 0.0
    one = P.AgcBatch(n, 0.07, 0.001)
    outs1, gains1 = _device(one, list(lefts), list(rights), [total] * n, chunk)
    three = P.AgcBatch(n, 0.07, 0.001)
    d_l = [torch.from_numpy(x).cuda() for x in lefts]
    d_r = [torch.from_numpy(x).cuda() for x in rights]
    d_o = [torch.full((total * chunk,), float(SENTINEL), device="cuda") for _ in range(n)]
    d_g = torch.full((n, total), float(SENTINEL), device="cuda")
    at = 0
    for part in (10, 1, 19):   # back to back on one stream, no synchronisation between the calls
        cut = lambda ts: [t[at * chunk:] for t in ts]
        three.condition_device(cut(d_l), cut(d_r), [part] * n, chunk, d_outs=cut(d_o), d_gain_out=d_g[:, at:], gain_stride=total)
        at += part
    torch.cuda.synchronize()
    gains3 = d_g.cpu().numpy()
    for s in range(n):
        _assert_bits(d_o[s].cpu().numpy(), outs1[s], ("samples", s))
        _assert_bits(gains3[s], gains1[s], ("gains", s))
        mono, g, _ = _host(0.07, 0.001, lefts[s], rights[s], total, chunk)
        _assert_bits(outs1[s], mono, ("host samples", s))
        _assert_bits(gains1[s], g, ("host gains", s))
    _assert_bits(three.gains(), one.gains(), "final gains")


def test_in_place_and_nothing_written_past_the_end():
    chunk, n = 1000, 67
    rng = np.random.default_rng(11)
    n_chunks = [int(x) for x in rng.integers(0, 7, n)]   # (some streams have no chunk at all)
    n_chunks[3] = 6
    lefts, rights = [], []
    for s in range(n):
        left, right = _noise(n_chunks[s] * chunk + 300, 700 + s)   # 300 samples past the end: not the call's to touch
        lefts.append(left)
        rights.append(right if s % 3 else None)
    a = P.AgcBatch(n, 0.07, 0.001)
    outs, gains = _device(a, lefts, rights, n_chunks, chunk, pad=300, gain_pad=3)
    b = P.AgcBatch(n, 0.07, 0.001)
    ins, gains_ip = _device(b, lefts, rights, n_chunks, chunk, in_place=True, gain_pad=3)
    for s in range(n):
        m = n_chunks[s] * chunk
        _assert_bits(ins[s][:m], outs[s][:m], ("in place", s))
        _assert_bits(ins[s][m:], lefts[s][m:], ("in place: past the end", s))
        assert np.all(outs[s][m:] == SENTINEL), s
        assert np.all(gains[s, n_chunks[s]:] == SENTINEL) and np.all(gains_ip[s, n_chunks[s]:] == SENTINEL), s
        mono, g, _ = _host(0.07, 0.001, lefts[s][:m], None if rights[s] is None else rights[s][:m], n_chunks[s], chunk)
        _assert_bits(outs[s][:m], mono, ("host samples", s))
        _assert_bits(gains[s, :n_chunks[s]], g, ("host gains", s))
    _assert_bits(gains_ip, gains, "gains")
    _assert_bits(a.gains(), b.gains(), "final gains")


def test_odd_values():
    """inf, nan, a subnormal (1e-41) and 1e30 in the streams.  The ONE relaxation of this file: an x86 host and the GPU give a NaN they
    produce themselves a different sign / payload (0 x inf: 0xffc00000 on SSE, 0x7fc00000 on the GPU), so where the host value is a NaN
    the device value must be a NaN, and everywhere else the bits are equal."""
    chunk, n, nc = 1000, 64, 5
    odd = [np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), np.float32(1e-41), np.float32(-1e-41), np.float32(1e30)]
    rng = np.random.default_rng(5)
    lefts, rights = [], []
    for s in range(n):
        left, right = _noise(nc * chunk, 900 + s)
        if s % 4 == 1:
            left[2 * chunk:3 * chunk] = np.float32(1e-41)     # a whole chunk of subnormals: its sum of squares is 0, the gate closes
            right[2 * chunk:3 * chunk] = np.float32(1e-41)
        for _ in range(3):
            o = int(rng.integers(0, nc * chunk))
            left[o] = odd[int(rng.integers(0, len(odd)))]
            if s % 2:
                right[int(rng.integers(0, nc * chunk))] = odd[int(rng.integers(0, len(odd)))]
        lefts.append(left)
        rights.append(right if s % 3 else None)
    batch = P.AgcBatch(n, 0.07, 0.001)
    outs, gains = _device(batch, lefts, rights, [nc] * n, chunk)
    final = batch.gains()
    n_nan = 0
    for s in range(n):
        mono, g, agc = _host(0.07, 0.001, lefts[s], rights[s], nc, chunk)
        for got, want, what in ((outs[s], mono, "samples"), (gains[s], g, "gains"), (final[s:s + 1], np.float32([agc.gain()]), "final gain")):
            nan = np.isnan(want)
            n_nan += int(nan.sum())
            assert np.array_equal(np.isnan(got), nan), (what, s)
            _assert_bits(got[~nan], want[~nan], (what, s))
    assert n_nan >= 1


def _voices(notes, n_frames, step, chunk):
    out = []
    for f in range(n_frames):
        tt = (f + 1) * step * chunk / 22050.0
        out.append([(k, float(np.exp(-(tt - t0) * 3.0) * pan * 4), float(np.exp(-(tt - t0) * 3.0) * (1 - pan) * 4)) for k, t0, pan in notes if tt >= t0])
    return out


def test_train_dataset_streams_end_to_end():
    v = P.Vqt.new(_train_params(), 0)
    chunk, step, nb = P.train_chunk_samples(v), 3, v.n_bins
    n_chunks = [42, 30, 9, 36, 21, 45]
    lefts, rights, voices = [], [], []
    for s, nc in enumerate(n_chunks):
        left, right, notes = _render(nc * chunk, 22050.0, 40 + s, n_notes=8)
        if s == 0:
            left[10 * chunk:12 * chunk] = 0.0
            right[10 * chunk:12 * chunk] = 0.0
        lefts.append(left)
        rights.append(right if s != 2 else None)
        voices.append(_voices(notes, nc // step, step, chunk))
    # the algorithm fixed: pvq.h promises the streams call the single-stream call's bits
    v.set_algo(P.ALGO_FFT)
    got = P.train_dataset_streams(v, lefts, rights, voices, step=step)
    assert len(got) == len(n_chunks)
    for s, nc in enumerate(n_chunks):
        want = P.train_dataset(v, lefts[s], rights[s], voices[s], step=step).reshape(nc // step, nb + 128)
        rows = got[s].reshape(nc // step, nb + 128)
        assert np.array_equal(rows[:, nb:], want[:, nb:]), s
        _assert_bits(rows[:, :nb].reshape(-1), want[:, :nb].reshape(-1), ("dB", s))
    assert sum(float(g.reshape(-1, nb + 128)[:, nb:].sum()) for g in got) > 0
    # left to itself each call picks its own path: the bars of test_train_dataset_vs_reference_loop
    v.set_algo(P.ALGO_AUTO)
    got = P.train_dataset_streams(v, lefts, rights, voices, step=step)
    for s in (0, 3):
        nc = n_chunks[s]
        want = P.train_dataset(v, lefts[s], rights[s], voices[s], step=step).reshape(nc // step, nb + 128)
        rows = got[s].reshape(nc // step, nb + 128)
        assert np.array_equal(rows[:, nb:], want[:, nb:]), s
        err = np.abs(rows[:, :nb] - want[:, :nb])
        loud = want[:, :nb] > 1.0
        print(f"stream {s}: max {err[loud].max():.3e} median {np.median(err[loud]):.3e} everywhere {err.max():.3e}")
        assert err[loud].max() <= 2e-2 and np.median(err[loud]) <= 2e-4, (err[loud].max(), np.median(err[loud]))
        assert err.max() <= 0.5


def test_nan_reaches_input_status():
    """a conditioned stream that carries a NaN makes input_status() raise after the streams call, as for any device-pointer call"""
    v = P.Vqt.new(_train_params(), 0)
    chunk, step, n, nc = P.train_chunk_samples(v), 3, 4, 18
    lefts = [_noise(nc * chunk, 60 + s)[0] for s in range(n)]
    assert v.window_union > 1000
    lefts[2][nc * chunk - 1000] = np.nan   # inside the last frame's windows
    d_l = [torch.from_numpy(x).cuda() for x in lefts]
    batch = P.AgcBatch(n, 0.07, 0.001)
    batch.condition_device(d_l, None, [nc] * n, chunk)
    d_db = torch.empty((n, nc // step, v.n_bins), device="cuda")
    v.batch_streams_device(d_l, chunk * step, [nc // step] * n, d_db)
    with pytest.raises(P.PvqError) as e:
        v.input_status()
    assert e.value.status == _lib.PVQ_ERR_NONFINITE_INPUT
    v.input_status()   # cleared
    with pytest.raises(P.PvqError):
        P.train_dataset_streams(v, lefts, None, [[[] for _ in range(nc // step)]] * n, step=step)
