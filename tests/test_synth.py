"""CPU checks of the synth stage (include/pvq.h, "the synth stage"): the C ABI's names and argument checks, the planner's decisions
and control values against the independent float64 model (tests/synth_model.py), the audio rate in NumPy float32 fed with the host's
plan (bit for bit), analytic checks on a looped sine, and the behaviour cases of tests/synth_cases.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth_cases as SC
import synth_model as SM
from pitchvis_amd import PvqError, _lib
from pitchvis_amd import synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ["pvq_synth_bank_create", "pvq_synth_bank_destroy", "pvq_synth_bank_counts", "pvq_synth_state_create", "pvq_synth_state_destroy",
         "pvq_synth_state_render", "pvq_synth_state_get_snapshots", "pvq_synth_state_get_plan", "pvq_synth_state_active_voices",
         "pvq_synth_batch_create", "pvq_synth_batch_destroy", "pvq_synth_batch_render_device", "pvq_synth_batch_get_snapshots",
         "pvq_synth_batch_last_times"]


@pytest.fixture(scope="module")
def bank():
    return S.SynthBank.from_arrays(**SC.bank_arrays())


@pytest.fixture(scope="module")
def rendered(bank):
    """every case rendered once on the host: name -> dict(left, right, ptr, rec, snaps, snap_blocks)"""
    out = {}
    for name, (events, n_blocks, poly) in SC.CASES.items():
        st = S.SynthState(bank, SC.SR, poly)
        snap_blocks = list(range(5, n_blocks, 17))
        left, right = st.render(events, n_blocks, snap_blocks)
        ptr, rec = st.plan()
        for a in (left, right, ptr, rec):
            a.setflags(write=False)
        out[name] = dict(left=left, right=right, ptr=ptr, rec=rec, snaps=st.snapshots(), snap_blocks=snap_blocks)
    return out


@pytest.fixture(scope="module")
def models():
    """the model of every case, evaluated in float64 and in float32: name -> (Model, blocks, snapshots), and the same under name + "/f32" added"""
    out = {}
    arrays = SC.bank_arrays()
    for name, (events, n_blocks, poly) in SC.CASES.items():
        for f32 in (False, True):
            m = SM.Model(arrays, SC.SR, poly, float32=f32)
            blocks, snaps = m.run(events, n_blocks, set(range(5, n_blocks, 17)))
            out[name + ("/f32" if f32 else "")] = (m, blocks, snaps)
    return out


def test_symbols_exported_and_abi():
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.pvq_abi_version() == 4
    assert S.RECORD_DTYPE.itemsize == 64 == __import__("ctypes").sizeof(_lib.CSynthRecord)
    assert "enable_reverb_and_chorus = false" in hdr   # what is left out is said where the entries are declared


def test_bank_argument_checks(bank):
    assert bank.counts() == (700, 10, 8, 8)
    good = SC.bank_arrays()

    def bad(**kw):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError) as e:
            S.SynthBank.from_arrays(**a)
        return str(e.value)

    smp = good["samples"].copy(); smp[1, 1] = 701
    assert "instrument region 1" in bad(samples=smp) and "end" in bad(samples=smp)
    smp = good["samples"].copy(); smp[0, 2] = -1
    assert "start_loop" in bad(samples=smp)
    smp = good["samples"].copy(); smp[2, 4] = 0
    assert "sample rate" in bad(samples=smp)
    gs, idx = good["instrument_regions"]
    assert "names sample 5" in bad(instrument_regions=(gs, np.array([0, 1, 1, 1, 2, 2, 0, 1, 3, 5], np.uint32)))
    g2 = gs.copy(); g2[0, 12] = 1   # END_ADDRESS_COARSE_OFFSET: 32768 values further
    assert "instrument region 0" in bad(instrument_regions=(g2, idx))
    ins = good["instruments"].copy(); ins[6] = (9, 2)
    assert "instrument 6" in bad(instruments=ins)
    pgs, pidx = good["preset_regions"]
    assert "names instrument 8" in bad(preset_regions=(pgs, np.array([0, 1, 2, 3, 4, 5, 6, 8], np.uint32)))
    pre = good["presets"].copy(); pre[3, 3] = 6
    assert "preset 3" in bad(presets=pre)
    assert "must not be empty" in bad(wave_data=np.zeros(0, np.int16))
    with pytest.raises(ValueError):
        S.SynthBank.from_arrays(good["wave_data"], good["samples"], (gs, idx[:-1]), good["instruments"], good["preset_regions"], good["presets"])
    with pytest.raises(TypeError):
        S.SynthBank()


def test_state_and_batch_argument_checks(bank):
    L = _lib.load()
    for sr in (15999, 192001):
        with pytest.raises(ValueError, match="sample rate"):
            S.SynthState(bank, sr)
    for poly in (7, 257):
        with pytest.raises(ValueError, match="polyphony"):
            S.SynthState(bank, SC.SR, poly)
    with pytest.raises(PvqError) as e:
        S.SynthState(bank, SC.SR, 65)
    assert e.value.status == _lib.PVQ_ERR_UNSUPPORTED
    with pytest.raises(PvqError) as e:
        S.SynthBatch(bank, 2, SC.SR, 128, device=None)
    assert e.value.status == _lib.PVQ_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="zero streams"):
        S.SynthBatch(bank, 0, SC.SR, device=None)
    assert L.pvq_synth_state_create(None, SC.SR, 64, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_state_render(None, None, None, None, None, None, 0, 0, None, 0, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_batch_get_snapshots(None, 0, None, None, 0, None, None, None, 0) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_bank_counts(None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_state_active_voices(None) == 0
    st = S.SynthState(bank, SC.SR)
    with pytest.raises(ValueError, match="outside 0 .. 255"):
        st.render(SC.ev((0.0, 0, SC.ON, 256, 100)), 1)
    with pytest.raises(ValueError, match="outside 0 .. 255"):
        st.render(SC.ev((0.0, -1, SC.ON, 60, 100)), 1)
    with pytest.raises(ValueError, match="earlier than"):
        st.render((np.array([0.2, 0.1]), [0, 0], [SC.ON, SC.ON], [60, 61], [100, 100]), 1)
    with pytest.raises(ValueError, match="NaN"):
        st.render((np.array([np.nan]), [0], [SC.ON], [60], [100]), 1)
    with pytest.raises(ValueError, match="ascend"):
        st.render(SC.ev(), 8, snapshot_blocks=[3, 3])
    with pytest.raises(ValueError, match="one length"):
        st.render((np.zeros(2), [0], [0], [0], [0]), 1)
    left, right = st.render(SC.ev((0.0, 0, SC.ON, 57, 100)), 4, snapshot_blocks=[1, 3, 9])   # (a snapshot block past the call is not taken)
    assert st.active_voices == 1 and len(st.snapshots()) == 2 and np.any(left != 0)
    with pytest.raises(ValueError, match="shorter than"):
        st.render(SC.ev(), 1)   # one event has been consumed
    counts = (__import__("ctypes").c_uint32 * 2)()
    ptr = (__import__("ctypes").c_uint32 * 1)()
    assert L.pvq_synth_state_get_plan(st._h, counts, ptr, 1, None, 0) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_state_get_snapshots(st._h, counts, ptr, 1, None, None, None, 0) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_state_render(st._h, None, None, None, None, None, 1, 1, None, 0, left.ctypes.data_as(S._fp),
                                    right.ctypes.data_as(S._fp)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_state_render(st._h, None, None, None, None, None, 0, 1, None, 0, None, None) == _lib.PVQ_ERR_INVALID_ARG


def test_host_only_handle_checks_arguments_then_reports_no_device(bank):
    b = S.SynthBatch(bank, 2, SC.SR, device=None)
    events = [SC.CASES["sine_root"][0], None]
    with pytest.raises(ValueError, match="one entry per stream"):
        b.render(events[:1], 4, [16, 16], [16, 16])
    with pytest.raises(ValueError, match="null left or right"):
        b.render(events, 4, [0, 16], [16, 16])
    with pytest.raises(ValueError, match="4-byte aligned"):
        b.render(events, 4, [18, 16], [16, 16])
    with pytest.raises(PvqError) as e:
        b.render(events, [4, 0], [16, 0], [16, 0])
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    assert b.last_times()["records"] == 0 and b.last_times()["replay_ms"] == 0.0
    with pytest.raises(ValueError, match="stream_index"):
        b.snapshots(2)
    assert b.snapshots(1) == []


def test_read_outside_wave_data_is_refused_with_stream_block_and_key(bank):
    st = S.SynthState(bank, SC.SR)
    with pytest.raises(ValueError) as e:
        st.render(*SC.RUNAWAY[:2])
    msg = str(e.value)
    assert "stream 0" in msg and "block 11" in msg and "key 100" in msg, msg
    assert "outside wave_data" in (_lib.load().pvq_last_error() or b"").decode()
    with pytest.raises(ValueError, match="cannot go on"):
        st.render(SC.RUNAWAY[0], 1)


# ---- the audio rate in NumPy float32, fed with the host's plan ---------------------------------------------------------
def numpy_replay(arrays, ptr, rec, n_blocks):
    """oscillator.rs:112-176, bi_quad_filter.rs:77-99, synthesizer.rs:363-391 / 478-495 with NumPy's int64 and float32 (IEEE, unfused):
    the records of a block are independent voices, so a block is walked sample by sample over vectors of its records"""
    f32 = np.float32
    wave = arrays["wave_data"].astype(np.int64)
    gs, smp_idx = arrays["instrument_regions"]
    desc = np.zeros((len(smp_idx), 4), np.int64)
    for i in range(len(smp_idx)):
        s, g = arrays["samples"][int(smp_idx[i])].astype(np.int64), gs[i].astype(np.int64)
        desc[i] = (s[0] + 32768 * g[4] + g[0], s[1] + 32768 * g[12] + g[1], s[2] + 32768 * g[45] + g[2], s[3] + 32768 * g[50] + g[3])
    pos = np.zeros(64, np.int64)
    mem = np.zeros((64, 4), f32)   # x1 x2 y1 y2
    lane_desc = np.zeros(64, np.int64)
    left, right = np.zeros(n_blocks * 64, f32), np.zeros(n_blocks * 64, f32)
    fp_to_sample = f32(1.0) / f32(32768 * (1 << 24))
    for b in range(n_blocks):
        r = rec[ptr[b]:ptr[b + 1]]
        n = r.size
        if n == 0:
            continue
        v = r["voice"].astype(np.int64)
        started = (r["flags"] & S.F_START) != 0
        lane_desc[v[started]] = r["desc"][started]
        d = desc[lane_desc[v]]
        p = np.where(started, d[:, 0] << 24, pos[v])
        x1, x2, y1, y2 = (np.where(started, f32(0), mem[v, k]) for k in range(4))
        looping, active = (r["flags"] & S.F_LOOP) != 0, (r["flags"] & S.F_FILTER) != 0
        ratio = (r["ratio_hi"].astype(np.int64) << 32) | r["ratio_lo"].astype(np.int64)
        end_loop, length = d[:, 3], d[:, 3] - d[:, 2]
        a = r["a"]
        block = np.zeros((n, 64), f32)
        for t in range(64):
            p = np.where(looping & (p >= (end_loop << 24)), p - (length << 24), p)
            i1 = p >> 24
            live = looping | (i1 < d[:, 1])
            i2 = np.where(looping & (i1 + 1 >= end_loop), i1 + 1 - length, i1 + 1)
            w1, w2 = wave[np.where(live, i1, 0)], wave[np.where(live, i2, 0)]
            x = fp_to_sample * np.where(live, (w1 << 24) + (p & ((1 << 24) - 1)) * (w2 - w1), 0).astype(f32)
            p = np.where(live, p + ratio, p)
            y = a[:, 0] * x + a[:, 1] * x1 + a[:, 2] * x2 - a[:, 3] * y1 - a[:, 4] * y2
            out = np.where(active, y, x).astype(f32)
            x2, x1, y2, y1 = np.where(active, x1, x2), np.where(active, x, x1), np.where(active, y1, y2), np.where(active, y, y1)
            block[:, t] = out
        ina = ~active   # bi_quad_filter.rs:93-98
        x2, x1 = np.where(ina, block[:, 62], x2), np.where(ina, block[:, 63], x1)
        y2, y1 = np.where(ina, x2, y2), np.where(ina, x1, y1)
        pos[v] = p
        mem[v] = np.stack([x1, x2, y1, y2], axis=1)
        for dst, (ip, ic) in ((left, (0, 1)), (right, (2, 3))):
            o = dst[b * 64:(b + 1) * 64]
            for k in range(n):   # record order is the order of the sum
                prev, cur = r["gain"][k, ip], r["gain"][k, ic]
                if max(prev, cur) < f32(1.0e-3):
                    continue
                if abs(cur - prev) < f32(1.0e-3):
                    o += cur * block[k]
                else:
                    step = f32(1.0 / 64.0) * (cur - prev)
                    g = np.empty(64, f32)
                    acc = f32(prev)
                    for t in range(64):
                        g[t] = acc
                        acc = f32(acc + step)
                    o += g * block[k]
    return left, right


@pytest.mark.parametrize("name", list(SC.CASES))
def test_numpy_audio_rate_equals_the_host_face_bit_for_bit(rendered, name):
    h = rendered[name]
    n_blocks = SC.CASES[name][1]
    left, right = numpy_replay(SC.bank_arrays(), h["ptr"], h["rec"], n_blocks)
    assert np.array_equal(left.view(np.uint32), h["left"].view(np.uint32))
    assert np.array_equal(right.view(np.uint32), h["right"].view(np.uint32))
    if name != "silence":
        assert np.any(h["left"] != 0)
    else:
        assert not h["left"].any() and not h["right"].any() and h["rec"].size == 0


# ---- the planner against the model --------------------------------------------------------------------------------------------
ULP = 2.0 ** -24


def _deviation(want, got_gain, got_coef, got_ratio_fp):
    """(gain error / mix_gain, coefficient error, pitch_ratio_fp error / max(1, ratio)) of one record against a model record"""
    gain = max(abs(got_gain[k] - want["gain"][k]) for k in range(4)) / max(want["mix"], 1e-30)
    coef = max(abs(got_coef[k] - want["coef"][k]) for k in range(5)) if want["filter"] else 0.0
    return gain, coef, abs(got_ratio_fp - (1 << 24) * want["ratio"]) / max(1.0, want["ratio"])


@pytest.mark.parametrize("name", list(SC.CASES))
def test_planner_decisions_equal_the_models_and_values_lie_within_rounding(rendered, models, name):
    """DECISIONS equal the float64 model's exactly.  VALUES: the bounds from the rounding chains are 16 * 2^-24 of the voice's mix_gain
    for a gain, 16 * 2^-24 of 1 for a coefficient and 8 * max(1, ratio) units for pitch_ratio_fp.  They hold against the model
    EVALUATED IN FLOAT32 (the same expressions, rounded where the reference holds an f32).  Against the float64 evaluation they are
    too tight for voices with an LFO: the reference derives the LFO's f64 period from an f32 frequency (lfo.rs:37), so one rounding
    of the frequency grows with the number of periods played (20 Hz for 1 s: 20 x 2^-24 of a period, times 6000 cents of cutoff
    depth).  That is the reference's own error, not the product's, so the float64 comparison allows, value by value, what the
    float32 evaluation of the model itself deviates from the float64 one, plus the bound.  DESIGN.md 6j records both figures."""
    h = rendered[name]
    m, blocks, snaps = models[name]
    m32, blocks32, _ = models[name + "/f32"]
    for mm in (m, m32):
        assert mm.undecided == 0
        assert min(mm.margins, default=1.0) > 1e-6, min(mm.margins)   # no threshold within rounding of a compared value, over every block
    ptr, rec = h["ptr"], h["rec"]
    assert len(blocks) == len(ptr) - 1
    worst = dict(vs_f32=[0.0, 0.0, 0.0], vs_f64=[0.0, 0.0, 0.0], f32_vs_f64=[0.0, 0.0, 0.0], excess=[0.0, 0.0, 0.0])
    for b, (want, want32) in enumerate(zip(blocks, blocks32)):
        got = rec[ptr[b]:ptr[b + 1]]
        for model_block in (want, want32):
            assert [w["voice"] for w in model_block] == got["voice"].tolist(), (name, b)
            assert [w["key"] for w in model_block] == got["key"].tolist(), (name, b)
            assert [w["stage"] for w in model_block] == got["stage"].tolist(), (name, b)
            assert [w["looping"] for w in model_block] == ((got["flags"] & S.F_LOOP) != 0).tolist(), (name, b)
            assert [w["filter"] for w in model_block] == ((got["flags"] & S.F_FILTER) != 0).tolist(), (name, b)
        assert [w["region"] for w, g in zip(want, got) if g["flags"] & S.F_START] == [int(g["desc"]) for g in got if g["flags"] & S.F_START]
        for w, w32, g in zip(want, want32, got):
            fp = (int(g["ratio_hi"]) << 32) | int(g["ratio_lo"])
            gain, coef = [float(x) for x in g["gain"]], [float(x) for x in g["a"]]
            d64, d32 = _deviation(w, gain, coef, fp), _deviation(w32, gain, coef, fp)
            own = _deviation(w, w32["gain"], w32["coef"] if w32["filter"] else [0.0] * 5, int((1 << 24) * w32["ratio"]))
            for k in range(3):
                worst["vs_f64"][k] = max(worst["vs_f64"][k], d64[k])
                worst["vs_f32"][k] = max(worst["vs_f32"][k], d32[k])
                worst["f32_vs_f64"][k] = max(worst["f32_vs_f64"][k], own[k])
                worst["excess"][k] = max(worst["excess"][k], d64[k] - own[k])
    print("synth model figures", name, {k: ["%.3g" % (v[0] / ULP), "%.3g" % (v[1] / ULP), "%.3g" % v[2]] for k, v in worst.items()},
          "(gain and coefficient in units of 2^-24, pitch_ratio_fp in units per max(1, ratio))")
    bounds = (16 * ULP, 16 * ULP, 8.0)
    for k in range(3):
        assert worst["vs_f32"][k] <= bounds[k], (k, worst)
        assert worst["excess"][k] <= bounds[k], (k, worst)
    assert len(snaps) == len(h["snaps"])
    for want, got in zip(snaps, h["snaps"]):
        assert [w[0] for w in want] == [g[0] for g in got]
    for want, got in zip(models[name + "/f32"][2], h["snaps"]):
        for w, g in zip(want, got):
            assert abs(w[1] - g[1]) <= 16 * ULP * max(w[1] + w[2], 1e-30) and abs(w[2] - g[2]) <= 16 * ULP * max(w[1] + w[2], 1e-30)


# ---- analytic ----------------------------------------------------------------------------------------------------------------
def test_looped_sine_at_its_root_key_is_a_sine_of_the_expected_frequency_and_amplitude(rendered):
    h = rendered["sine_root"]
    rec = h["rec"]
    assert np.all((rec["flags"] & S.F_FILTER) == 0) and np.all(rec["ratio_lo"][:200] == 1 << 24) and np.all(rec["ratio_hi"] == 0)
    note_gain = 10.0 ** (0.05 * 2.0 * 20.0 * np.log10(100 / 127.0))
    channel_gain = ((100 << 7) / 16383.0 * (127 << 7) / 16383.0) ** 2
    angle = np.pi / 200.0 * ((100.0 / 16383.0) * (64 << 7) - 50.0 + 50.0)   # the centre of channel.rs:58 is 0.003 right of pi / 4
    assert abs(angle - np.pi / 4) < 1e-4
    t = np.arange(1024, 9216)   # hold / sustain: the envelope is 1
    table = np.round(30000 * np.sin(2 * np.pi * np.arange(SC.SINE_N) / SC.SINE_N)) / 32768.0
    for chan, trig in (("left", np.cos), ("right", np.sin)):
        amp = note_gain * channel_gain * 0.5 * trig(angle)
        want = amp * table[t % SC.SINE_N]                      # pitch ratio 1: the table itself, period 100 samples = 220.5 Hz
        assert np.max(np.abs(h[chan][t] - want)) <= 8 * 2.0 ** -24 * amp
        assert abs(np.max(np.abs(h[chan][t])) - amp * 30000 / 32768.0) <= 1e-6
    spec = np.abs(np.fft.rfft(h["left"][1024:1024 + 8000] * np.hanning(8000)))
    assert abs(np.argmax(spec) * SC.SR / 8000.0 - SC.SR / SC.SINE_N) <= SC.SR / 8000.0


def test_strongest_vqt_bin_of_the_sine_is_its_keys(rendered):
    import oracle as O
    from helpers import get_geom
    _, op = get_geom("serial_22k_180")   # 22 050 Hz, 55 Hz upwards, 36 bins an octave
    ov = O.OracleVqt(op)
    h = rendered["sine_root"]
    mono = 0.5 * (h["left"][:16384] + h["right"][:16384])
    db = ov.calculate_batch(mono, 16384, 1)[0]
    assert int(np.argmax(db)) == 36 * 2   # key 57 = A3 = 220 Hz = two octaves above 55 Hz


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cuts", [("steal", [77]), ("hold_pedal", [1, 150, 151]), ("wobble", [33, 200]), ("noloop_end", list(range(1, 60))),
                                        ("mixed", [100, 101, 230])])
def test_split_renders_are_bit_equal(bank, rendered, name, cuts):
    events, n_blocks, poly = SC.CASES[name]
    st = S.SynthState(bank, SC.SR, poly)
    parts = [st.render(e, n) for e, n in SC.chunked(events, n_blocks, cuts)]
    left, right = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert np.array_equal(left.view(np.uint32), rendered[name]["left"].view(np.uint32))
    assert np.array_equal(right.view(np.uint32), rendered[name]["right"].view(np.uint32))


def _per_block(h):
    return [h["rec"][h["ptr"][b]:h["ptr"][b + 1]] for b in range(len(h["ptr"]) - 1)]


def test_sixty_five_notes_steal_the_voice_the_reference_steals(rendered, models):
    blocks = _per_block(rendered["steal"])
    assert max(len(b) for b in blocks) == 64
    m = models["steal"][0]
    assert m.steals >= 3   # the 65th note and the three late ones; the record-by-record comparison above says WHICH voice each took
    full = next(i for i, b in enumerate(blocks) if len(b) == 64)
    stolen = [b for b in blocks[full + 1:] if len(b) == 64 and np.any(b["flags"] & S.F_START)]
    assert stolen, "a started record among 64: a voice object was taken over"


def test_exclusive_class_restarts_the_channels_voice(rendered, models):
    blocks = _per_block(rendered["exclusive"])
    assert models["exclusive"][0].reuses == 2   # 75 over 60 and 62 over 75 on channel 0; channel 1 gets a voice of its own
    assert max(len(b) for b in blocks) == 2
    starts = [(int(r["voice"]), int(r["key"])) for b in blocks for r in b if r["flags"] & S.F_START]
    assert [k for _, k in starts] == [60, 75, 62, 64] and len({v for v, _ in starts[:3]}) == 1 and starts[3][0] != starts[0][0]


def test_hold_pedal_delays_the_release(rendered):
    blocks = _per_block(rendered["hold_pedal"])
    block_of = lambda t: int(np.ceil(t * SC.SR / 64.0))
    first_release = next(i for i, b in enumerate(blocks) if len(b) and b["stage"][0] == 4)
    assert first_release == block_of(0.5001)   # note off at 0.2 s, pedal up at 0.5 s
    assert all(((b["flags"] & S.F_LOOP) != 0).all() for b in blocks[:first_release] if len(b))
    assert not (blocks[first_release]["flags"][0] & S.F_LOOP)   # LOOP_UNTIL_NOTE_OFF ends with the release (oscillator.rs:90-94)


def test_pitch_bend_changes_the_ratio_mid_note(rendered):
    rec = rendered["pitch_bend"]["rec"]
    ratio = ((rec["ratio_hi"].astype(np.int64) << 32) | rec["ratio_lo"]) / float(1 << 24)
    block_of = lambda t: int(np.ceil(t * SC.SR / 64.0))
    assert ratio[block_of(0.05)] == 1.0
    assert abs(ratio[block_of(0.15)] - 2.0 ** (2.0 * (96 * 128 - 8192) / 8192.0 / 12.0)) < 1e-6     # range 2 semitones
    assert abs(ratio[block_of(0.22)] - 2.0 ** (2.0 * (16383 - 8192) / 8192.0 / 12.0)) < 1e-6
    assert abs(ratio[block_of(0.32)] - 2.0 ** (-12.5 / 12.0)) < 1e-6                                 # RPN 0: 12.50 semitones, bend -1
    assert abs(ratio[block_of(0.42)] - 2.0 ** ((-12.5 + 6.0) / 12.0)) < 1e-6                         # RPN 2: coarse tune + 6
    wheel = ratio[block_of(0.475):block_of(0.5)]                                                     # modulation wheel: the vibrato LFO reaches the pitch
    assert np.ptp(wheel) > 1e-3 and np.ptp(ratio[block_of(0.455):block_of(0.47)]) == 0.0
    assert abs(ratio[-1] - 2.0 ** ((6.0 + (((80 << 7) | 3) - 8192) / 8192.0) / 12.0)) < 1e-6         # RPN 1 fine tune; controllers reset


def test_all_sound_off_kills_the_channels_voices_at_once(rendered):
    blocks = _per_block(rendered["all_sound_off"])
    k = int(np.ceil(0.2001 * SC.SR / 64.0))
    assert sorted(blocks[k - 1]["key"].tolist()) == [57, 60, 67] and blocks[k]["key"].tolist() == [57]
    assert sorted(blocks[-1]["key"].tolist()) == [57, 62]


def test_sample_without_loop_ends_inside_a_block_and_the_voice_leaves_at_the_next(rendered):
    h = rendered["noloop_end"]
    blocks = _per_block(h)
    ends = [i for i, b in enumerate(blocks) if len(b) and (b["flags"][0] & S.F_ENDS)]
    assert len(ends) == 3
    for i in ends:
        assert len(blocks[i + 1]) == 0 or (blocks[i + 1]["flags"][0] & S.F_START)
        tail = h["left"][i * 64:(i + 1) * 64]
        assert tail[0] != 0 and tail[-1] == 0   # sound, then the zeros of oscillator.rs:120-122


def test_loop_until_note_off_voice_plays_to_the_samples_end_after_release(rendered):
    blocks = _per_block(rendered["loop_until_off"])
    by_key = {48: [], 84: []}
    for b in blocks:
        for r in b:
            by_key[int(r["key"])].append(r)
    for key, t_off in ((48, 0.3001), (84, 0.3501)):
        flags = np.array([r["flags"] for r in by_key[key]])
        n_loop = int(((flags & S.F_LOOP) != 0).sum())
        # (the note starts with block 1; the block that applies the note off releases the voice before its oscillator runs)
        assert n_loop == int(np.ceil(t_off * SC.SR / 64.0)) - 1 and not np.any(flags[n_loop:] & S.F_LOOP)
    for key in (48, 84):   # out of the loop the position runs to the sample's end, long before the release has faded
        assert by_key[key][-1]["flags"] & S.F_ENDS and by_key[key][-1]["stage"] == 4


def test_filter_goes_inactive_and_active_again_and_the_clamp_is_hit(rendered, models):
    active = (rendered["sweep"]["rec"]["flags"] & S.F_FILTER) != 0
    edges = np.flatnonzero(np.diff(active.astype(int)))
    assert len(edges) >= 4 and active[0]   # on, off, on, off, on: bi_quad_filter.rs:93-98 decides what the filter resumes from
    assert models["wobble"][0].clamped > 10 and models["sweep"][0].clamped == 0


def test_gain_slope_constant_and_skipped_all_occur(rendered):
    g = rendered["gains"]["rec"]["gain"]
    for ip, ic in ((0, 1), (2, 3)):
        skip = np.maximum(g[:, ip], g[:, ic]) < np.float32(1e-3)
        const = ~skip & (np.abs(g[:, ic] - g[:, ip]) < np.float32(1e-3))
        assert skip.sum() > 10 and const.sum() > 10 and (~skip & ~const).sum() >= 4
    both = (np.maximum(g[:, 0], g[:, 1]) < np.float32(1e-3)) & (np.maximum(g[:, 2], g[:, 3]) < np.float32(1e-3))
    assert both.sum() > 5   # channel volume 0: the voice still walks its samples


# ---- the kernel's resources --------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_replay_kernel_uses_no_scratch_and_whole_lds_granules(tmp_path):
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "synth_batch.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "x.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(usage) == 1 and "synth_replay" in next(iter(usage))
    u = next(iter(usage.values()))
    assert u["ScratchSize"] == 0 and u["LDS"] % 16 == 0 and 0 < u["LDS"] <= 40960 and u["VGPRs"] <= 128, u   # four workgroups a CU
