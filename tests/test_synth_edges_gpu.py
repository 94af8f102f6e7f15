"""GPU checks of the effects replay (synth_fx_batch.hip) at its edges, on the inputs of tests/synth_edge_cases.py, which
tests/test_synth_edges.py has checked on the host: a whole cycle of the chorus LFO with signal in the ring (blocks in which 125 of
128 taps read the block's own sums from LDS, blocks in which at most 3 do, the delay table's wrap in either channel, two laps of
the table in one call), a ring of 65 slots whose index takes every residue, hard-left and hard-right voices with the chorus on, the rates from 44 100 Hz up, and all
thirteen dry cases under the quarter-block walk.  Every comparison is device rows against the host face on the uint32 view."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth_edge_cases as EC
from pitchvis_amd import synth as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bank():
    return S.SynthBank.from_arrays(**EC.bank_arrays())


@pytest.fixture(scope="module")
def host(bank):
    """every case on the host face with effects at polyphony 64, rendered once: name -> (left, right, snapshots after every 16th block)"""
    out = {}
    for name, (events, n_blocks, sr) in list(EC.CASES.items()) + list(EC.DRY.items()):
        st = S.SynthState(bank, sr, EC.POLYPHONY, effects=True)
        left, right = st.render(events, n_blocks, list(range(15, n_blocks, 16)))
        left.setflags(write=False)
        right.setflags(write=False)
        out[name] = (left, right, st.snapshots())
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(n_blocks, fill=7.0):
    return [torch.full((nb * 64,), fill, device="cuda") for nb in n_blocks]


def _assert_rows(d_left, d_right, want, what):
    assert np.array_equal(_bits(d_left.cpu().numpy()), _bits(want[0])), what
    assert np.array_equal(_bits(d_right.cpu().numpy()), _bits(want[1])), what


@pytest.mark.parametrize("name", EC.LONG)
def test_long_chorus_beside_a_silent_stream(bank, host, name):
    events, n_blocks, sr = EC.CASES[name]
    batch = S.SynthBatch(bank, 2, sr, EC.POLYPHONY, device=0, effects=True)
    d_l, d_r = _rows([n_blocks] * 2), _rows([n_blocks] * 2)
    batch.render([events, None], n_blocks, d_l, d_r)
    _assert_rows(d_l[0], d_r[0], host[name], name)
    assert not d_l[1].any() and not d_r[1].any()   # the stream without events: rows of zeros
    dry = S.SynthState(bank, sr, EC.POLYPHONY).render(events, n_blocks)
    got = d_l[0].cpu().numpy(), d_r[0].cpu().numpy()
    for c in range(2):   # the effects reach the rows up to the last block
        assert not np.array_equal(_bits(got[c][-64:]), _bits(dry[c][-64:])), (name, c)


def test_long_chorus_at_16200_hz_in_five_uneven_calls_beside_one_run(bank, host):
    """each wrap of the delay table (right: block 474, left: block 632) alone in a one-block call, no synchronisation between the
    calls; the second stream renders all 650 blocks in the first call and 0 blocks in the later ones"""
    name = "long_chorus_16200"
    events, n_blocks, sr = EC.CASES[name]
    batch = S.SynthBatch(bank, 2, sr, EC.POLYPHONY, device=0, effects=True)
    d_l, d_r = _rows([n_blocks] * 2), _rows([n_blocks] * 2)
    done = 0
    for i, nb in enumerate(EC.SPLIT_16200):
        part = slice(done * 64, (done + nb) * 64)
        batch.render([events, events], [nb, n_blocks if i == 0 else 0], [d_l[0][part], d_l[1] if i == 0 else None],
                     [d_r[0][part], d_r[1] if i == 0 else None])
        done += nb
    assert done == n_blocks
    for s in range(2):
        _assert_rows(d_l[s], d_r[s], host[name], (name, s))


def test_two_laps_of_the_delay_table_in_one_call(bank, host):
    """the per-block table index has to wrap: the per-lane wrap alone is right for one lap of a call, and this call makes two"""
    events, n_blocks, sr = EC.CASES[EC.TWO_LAPS]
    batch = S.SynthBatch(bank, 1, sr, EC.POLYPHONY, device=0, effects=True)
    d_l, d_r = _rows([n_blocks]), _rows([n_blocks])
    batch.render([events], n_blocks, d_l, d_r)
    _assert_rows(d_l[0], d_r[0], host[EC.TWO_LAPS], EC.TWO_LAPS)


@pytest.mark.parametrize("name", ["pan_edges"] + EC.HIGH_RATES)
def test_pan_edges_and_high_rates_in_two_calls(bank, host, name):
    events, n_blocks, sr = EC.CASES[name]
    batch = S.SynthBatch(bank, 2, sr, EC.POLYPHONY, device=0, effects=True)   # a handle of its own per rate; the second stream: silence
    d_l, d_r = _rows([n_blocks] * 2), _rows([n_blocks] * 2)
    cut = 7
    batch.render([events, None], cut, [t[:cut * 64] for t in d_l], [t[:cut * 64] for t in d_r])
    batch.render([events, None], n_blocks - cut, [t[cut * 64:] for t in d_l], [t[cut * 64:] for t in d_r])
    _assert_rows(d_l[0], d_r[0], host[name], name)
    assert not d_l[1].any() and not d_r[1].any()


def test_the_thirteen_dry_cases_with_effects_in_one_batch(bank, host):
    names = list(EC.DRY)
    assert len(names) == 13
    n_blocks = [EC.DRY[n][1] for n in names]
    batch = S.SynthBatch(bank, len(names), EC.SR, EC.POLYPHONY, device=0, effects=True)
    d_l, d_r = _rows(n_blocks), _rows(n_blocks)
    batch.render([EC.DRY[n][0] for n in names], n_blocks, d_l, d_r, snapshot_blocks=list(range(15, max(n_blocks), 16)))
    torch.cuda.synchronize()
    for s, name in enumerate(names):
        left, right, snaps = host[name]
        _assert_rows(d_l[s], d_r[s], (left, right), name)
        assert len(snaps) == len(range(15, n_blocks[s], 16)) and batch.snapshots(s) == snaps, name
        if name == "silence":
            assert not d_l[s].any() and not d_r[s].any()


def test_dry_cases_with_effects_at_polyphony_8(bank):
    names = ["noloop_end", "sweep", "steal"]
    n_blocks = [EC.DRY[n][1] for n in names]
    batch = S.SynthBatch(bank, len(names), EC.SR, 8, device=0, effects=True)
    d_l, d_r = _rows(n_blocks), _rows(n_blocks)
    batch.render([EC.DRY[n][0] for n in names], n_blocks, d_l, d_r)
    for s, name in enumerate(names):   # (eight voice objects: `steal` steals from its ninth note on)
        want = S.SynthState(bank, EC.SR, 8, effects=True).render(EC.DRY[name][0], n_blocks[s])
        _assert_rows(d_l[s], d_r[s], want, name)


def test_rows_inside_a_nan_guard_band_and_nothing_outside_them_changes(bank, host):
    streams = ["pan_edges", "noloop_end", "silence"]
    n_blocks = [(EC.CASES.get(n) or EC.DRY[n])[1] for n in streams]
    events = [(EC.CASES.get(n) or EC.DRY[n])[0] for n in streams]
    n = len(streams)
    batch = S.SynthBatch(bank, n, EC.SR, EC.POLYPHONY, device=0, effects=True)
    stride, offset = max(n_blocks) * 64 + 24, 8   # a row stride larger than any length, rows 8 values into their line
    buf_l = torch.full((n, stride), float("nan"), device="cuda")
    buf_r = torch.full((n, stride), float("nan"), device="cuda")
    fill = _bits(buf_l[0, :1].cpu().numpy())[0]
    batch.render(events, n_blocks, [buf_l[s, offset:offset + n_blocks[s] * 64] for s in range(n)],
                 [buf_r[s, offset:offset + n_blocks[s] * 64] for s in range(n)])
    got_l, got_r = buf_l.cpu().numpy(), buf_r.cpu().numpy()
    for s, name in enumerate(streams):
        end = offset + n_blocks[s] * 64
        for got, want in ((got_l[s], host[name][0]), (got_r[s], host[name][1])):
            assert np.array_equal(_bits(got[offset:end]), _bits(want)), (s, name)
            assert np.all(_bits(got[:offset]) == fill) and np.all(_bits(got[end:]) == fill), (s, name)   # the guard band keeps its bits
