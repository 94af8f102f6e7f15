"""GPU checks of the synth stage's effects: the device replay with reverb and chorus (synth_fx_batch.hip) carries the host face's bits —
every case of tests/synth_fx_cases.py, streams of different cases and lengths side by side, several uneven calls against one, rows at
an offset inside a wider buffer, a handle of its own at 16 kHz (chorus ring = one block, all-pass slots reused in the next block) and
at 48 kHz — and the trainer's chain from events on with effects equals the chain fed with the host face's effect PCM."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pitchvis_amd as P
import synth_cases as SC
import synth_fx_cases as FC
from pitchvis_amd import _lib
from pitchvis_amd import synth as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
NAMES = FC.AT_22050
SR = 22050


@pytest.fixture(scope="module")
def bank():
    return S.SynthBank.from_arrays(**FC.bank_arrays())


@pytest.fixture(scope="module")
def host(bank):
    """every case on the host face with effects at polyphony 64, rendered once: name -> (left, right, snapshots after every 16th block)"""
    out = {}
    for name, (events, n_blocks, _, sr) in FC.CASES.items():
        st = S.SynthState(bank, sr, 64, effects=True)
        left, right = st.render(events, n_blocks, list(range(15, n_blocks, 16)))
        left.setflags(write=False)
        right.setflags(write=False)
        out[name] = (left, right, st.snapshots())
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _streams(n):
    """n streams over the 22 050 Hz cases in turn, later rounds shorter: [(name, n_blocks)]"""
    return [(NAMES[s % len(NAMES)], max(FC.CASES[NAMES[s % len(NAMES)]][1] - 7 * (s // len(NAMES)) - (s % 3), 1)) for s in range(n)]


@pytest.mark.parametrize("n_streams", [1, 3, 70])
def test_device_rows_equal_the_host_face_bit_for_bit(bank, host, n_streams):
    streams = {1: [("chorus_cc", 150)], 3: [("mixed", 340), ("silence", 40), ("flush", 700)]}.get(n_streams) or _streams(n_streams)
    batch = S.SynthBatch(bank, n_streams, SR, 64, device=0, effects=True)
    d_l = [torch.full((nb * 64,), 7.0, device="cuda") for _, nb in streams]
    d_r = [torch.full((nb * 64,), 7.0, device="cuda") for _, nb in streams]
    batch.render([FC.CASES[name][0] for name, _ in streams], [nb for _, nb in streams], d_l, d_r, snapshot_blocks=list(range(15, 700, 16)))
    torch.cuda.synchronize()
    for s, (name, nb) in enumerate(streams):
        left, right, snaps = host[name]
        assert np.array_equal(_bits(d_l[s].cpu().numpy()), _bits(left[:nb * 64])), (s, name)
        assert np.array_equal(_bits(d_r[s].cpu().numpy()), _bits(right[:nb * 64])), (s, name)
        assert batch.snapshots(s) == snaps[:len(range(15, nb, 16))], (s, name)
        if name == "silence":
            assert not d_l[s].any() and not d_r[s].any()   # a stream with no events: rows of zeros
    assert {name for name, _ in streams} == set(NAMES) or n_streams < len(NAMES)


def test_three_uneven_calls_equal_one_and_rows_may_sit_inside_a_wider_buffer(bank, host):
    streams = [("chorus_cc", 150), ("reverb_default", 120), ("mixed", 340), ("silence", 40), ("instrument_sends", 80)]
    n = len(streams)
    batch = S.SynthBatch(bank, n, SR, 64, device=0, effects=True)
    stride, offset = 340 * 64 + 24, 8   # a row stride larger than any length, rows 8 values into their line
    buf_l = torch.full((n, stride), -3.0, device="cuda")
    buf_r = torch.full((n, stride), -3.0, device="cuda")
    done = [0] * n
    for part in ([37, 1, 150, 40, 0], [1, 64, 1, 0, 79], None):   # 0 and 1 block for some: sample counts and ring positions diverge
        counts = [nb - done[s] for s, (_, nb) in enumerate(streams)] if part is None else part
        d_l = [buf_l[s, offset + done[s] * 64: offset + (done[s] + counts[s]) * 64] if counts[s] else None for s in range(n)]
        d_r = [buf_r[s, offset + done[s] * 64: offset + (done[s] + counts[s]) * 64] if counts[s] else None for s in range(n)]
        batch.render([FC.CASES[name][0] for name, _ in streams], counts, d_l, d_r)
        done = [done[s] + counts[s] for s in range(n)]
    got_l, got_r = buf_l.cpu().numpy(), buf_r.cpu().numpy()
    for s, (name, nb) in enumerate(streams):
        left, right, _ = host[name]
        for got, want in ((got_l[s], left), (got_r[s], right)):
            assert np.array_equal(_bits(got[offset:offset + nb * 64]), _bits(want[:nb * 64])), (s, name)
            assert np.all(got[:offset] == -3.0) and np.all(got[offset + nb * 64:] == -3.0), (s, name)   # nothing outside the rows is written


def test_low_polyphony_batch_steals_under_the_extra_sums(bank):
    names = ["steal", "mixed"]
    batch = S.SynthBatch(bank, 2, SR, 8, device=0, effects=True)
    n_blocks = [FC.CASES[n][1] for n in names]
    d_l = [torch.empty(nb * 64, device="cuda") for nb in n_blocks]
    d_r = [torch.empty(nb * 64, device="cuda") for nb in n_blocks]
    batch.render([FC.CASES[n][0] for n in names], n_blocks, d_l, d_r)
    for s, name in enumerate(names):   # (eight voice objects: `steal` steals from its ninth note on)
        left, right = S.SynthState(bank, SR, 8, effects=True).render(FC.CASES[name][0], n_blocks[s])
        assert np.array_equal(_bits(d_l[s].cpu().numpy()), _bits(left)) and np.array_equal(_bits(d_r[s].cpu().numpy()), _bits(right)), name


@pytest.mark.parametrize("name", ["sr16k", "sr48k"])
def test_other_sample_rates_in_two_calls(bank, host, name):
    events, n_blocks, _, sr = FC.CASES[name]
    batch = S.SynthBatch(bank, 2, sr, 64, device=0, effects=True)   # the second stream: silence beside it
    d_l = [torch.full((n_blocks * 64,), 7.0, device="cuda") for _ in range(2)]
    d_r = [torch.full((n_blocks * 64,), 7.0, device="cuda") for _ in range(2)]
    cut = 7
    batch.render([events, None], cut, [t[:cut * 64] for t in d_l], [t[:cut * 64] for t in d_r])
    batch.render([events, None], n_blocks - cut, [t[cut * 64:] for t in d_l], [t[cut * 64:] for t in d_r])
    left, right, _ = host[name]
    assert np.array_equal(_bits(d_l[0].cpu().numpy()), _bits(left)) and np.array_equal(_bits(d_r[0].cpu().numpy()), _bits(right))
    assert not d_l[1].any() and not d_r[1].any()


def test_batch_made_with_flags_zero_equals_the_dry_host_face():
    L = _lib.load()
    plain = S.SynthBank.from_arrays(**SC.bank_arrays())
    batch = S.SynthBatch.__new__(S.SynthBatch)
    batch._L, batch._bank, batch.n_streams, batch.device, batch._h = L, plain, 2, 0, C.c_void_p()
    assert L.pvq_synth_batch_create_ex(0, plain._h, 2, SC.SR, 64, 0, C.byref(batch._h)) == _lib.PVQ_OK
    names = ["mixed", "wobble"]
    n_blocks = [SC.CASES[n][1] for n in names]
    d_l = [torch.empty(nb * 64, device="cuda") for nb in n_blocks]
    d_r = [torch.empty(nb * 64, device="cuda") for nb in n_blocks]
    batch.render([SC.CASES[n][0] for n in names], n_blocks, d_l, d_r)
    for s, name in enumerate(names):
        left, right = S.SynthState(plain, SC.SR, 64).render(SC.CASES[name][0], n_blocks[s])
        assert np.array_equal(_bits(d_l[s].cpu().numpy()), _bits(left)) and np.array_equal(_bits(d_r[s].cpu().numpy()), _bits(right)), name


def test_planner_refusal_launches_nothing_and_ends_the_handle(bank):
    batch = S.SynthBatch(bank, 2, SR, 64, device=0, effects=True)
    d_l = [torch.full((30 * 64,), 5.0, device="cuda") for _ in range(2)]
    d_r = [torch.full((30 * 64,), 5.0, device="cuda") for _ in range(2)]
    with pytest.raises(ValueError) as e:
        batch.render([FC.CASES["reverb_default"][0], SC.RUNAWAY[0]], 30, d_l, d_r)
    assert "stream 1" in str(e.value) and "block 11" in str(e.value) and "key 100" in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((t == 5.0).all()) for t in d_l + d_r)
    with pytest.raises(ValueError, match="cannot go on"):
        batch.render([None, None], 1, d_l, d_r)


def test_train_dataset_from_events_with_effects_equals_the_chain_fed_with_the_host_faces_pcm(bank):
    q = 10.0   # pitchvis_train/src/train.rs:30-42
    v = P.Vqt.new(P.VqtParameters(sr=22050.0, n_fft=32768, range=P.VqtRange(55.0, 7, 36), sparsity_quantile=0.999, quality=q, gamma=5.3 * q), 0)
    v.set_algo(P.ALGO_FFT)   # one path for both chains: the streams call promises its own bits per path
    chunk, step, nb = P.train_chunk_samples(v), 3, v.n_bins
    per_chunk = chunk // 64
    names = ["mixed", "chorus_cc", "silence", "instrument_sends"]
    n_chunks = [max(3, min(9, FC.CASES[n][1] // per_chunk)) - i % 2 for i, n in enumerate(names)]
    events = [FC.CASES[n][0] for n in names]
    got = P.train_dataset_from_events(v, bank, events, n_chunks, step=step, effects=True)
    dry = P.train_dataset_from_events(v, bank, events, n_chunks, step=step)
    lefts, rights, voices = [], [], []
    for s, name in enumerate(names):
        st = S.SynthState(bank, SR, 64, effects=True)
        n_frames = n_chunks[s] // step
        left, right = st.render(events[s], n_chunks[s] * per_chunk, [(f + 1) * step * per_chunk - 1 for f in range(n_frames)])
        lefts.append(left)
        rights.append(right)
        voices.append(st.snapshots())
    want = P.train_dataset_streams(v, lefts, rights, voices, step=step)
    assert len(got) == len(want) == len(names)
    for s in range(len(names)):
        assert got[s].size == (n_chunks[s] // step) * (nb + 128)
        assert np.array_equal(_bits(got[s]), _bits(want[s])), names[s]
    assert any(not np.array_equal(_bits(g), _bits(d)) for g, d in zip(got, dry))   # the effects reach the rows
