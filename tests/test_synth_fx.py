"""CPU checks of the synth stage's effects (include/pvq.h: PVQ_SYNTH_EFFECTS, pvq_synth_effects_*): the new names, flags 0 against
today's entries, the sends against the formula of voice.rs and synthesizer.rs, the delay table, the host face against the
sample-by-sample NumPy model (tests/synth_fx_model.py) bit for bit, split renders, and analytic checks through the effects-only face."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth_cases as SC
import synth_fx_cases as FC
import synth_fx_model as FM
from pitchvis_amd import PvqError, _lib
from pitchvis_amd import synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pvq_synth_state_create_ex", "pvq_synth_batch_create_ex", "pvq_synth_state_get_sends", "pvq_synth_effects_create",
         "pvq_synth_effects_destroy", "pvq_synth_effects_process", "pvq_synth_chorus_table"]
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def bank():
    return S.SynthBank.from_arrays(**FC.bank_arrays())


@pytest.fixture(scope="module")
def rendered(bank):
    """every case on the host face with effects, once: name -> dict(left, right, ptr, rec, sends)"""
    out = {}
    for name, (events, n_blocks, poly, sr) in FC.CASES.items():
        st = S.SynthState(bank, sr, poly, effects=True)
        left, right = st.render(events, n_blocks)
        ptr, rec = st.plan()
        sptr, sends = st.sends()
        assert np.array_equal(ptr, sptr) and sends.size == rec.size
        for a in (left, right, ptr, rec, sends):
            a.setflags(write=False)
        out[name] = dict(left=left, right=right, ptr=ptr, rec=rec, sends=sends)
    return out


@pytest.fixture(scope="module")
def modelled(rendered):
    """the model of every case, fed with the host's plan, sends and delay table, once"""
    arrays, tables, out = FC.bank_arrays(), {}, {}
    for name, (events, n_blocks, poly, sr) in FC.CASES.items():
        if sr not in tables:
            tables[sr] = S.chorus_table(sr)
        h = rendered[name]
        out[name] = FM.render(arrays, sr, h["ptr"], h["rec"], h["sends"], tables[sr], n_blocks)
    return out


def test_new_names_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.pvq_abi_version() == 4
    assert S.SENDS_DTYPE.itemsize == 32 == C.sizeof(_lib.CSynthSends)
    assert re.search(r"#define\s+PVQ_SYNTH_EFFECTS\s+1u", hdr)


def test_flags_zero_is_todays_create_and_unknown_flags_are_refused(bank):
    L = _lib.load()
    plain = S.SynthBank.from_arrays(**SC.bank_arrays())
    for name, (events, n_blocks, poly) in SC.CASES.items():
        old = S.SynthState(plain, SC.SR, poly)
        new = S.SynthState.__new__(S.SynthState)
        new._L, new._bank, new._h = L, plain, C.c_void_p()
        assert L.pvq_synth_state_create_ex(plain._h, SC.SR, poly, 0, C.byref(new._h)) == _lib.PVQ_OK
        a, b = old.render(events, n_blocks), new.render(events, n_blocks)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), name
        pa, pb = old.plan(), new.plan()
        assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes(), name
        ptr, sends = new.sends()
        assert ptr.tolist() == [0] and sends.size == 0   # a dry state has no sends
    for flags in (2, 3, 0x80000000):
        h = C.c_void_p()
        assert L.pvq_synth_state_create_ex(plain._h, SC.SR, 64, flags, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h
        assert b"flag" in L.pvq_last_error()
        assert L.pvq_synth_batch_create_ex(-1, plain._h, 2, SC.SR, 64, flags, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h
    assert L.pvq_synth_effects_create(22050, None) == _lib.PVQ_ERR_INVALID_ARG and L.pvq_last_error() == b"null handle"
    assert L.pvq_synth_effects_process(None, 0, None, None, None, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_synth_state_get_sends(None, None, None, 0, None, 0) == _lib.PVQ_ERR_INVALID_ARG
    L.pvq_synth_effects_destroy(None)
    with pytest.raises(ValueError, match="between 16000 and 192000"):
        S.SynthEffects(15999)
    with pytest.raises(ValueError, match="between 16000 and 192000"):
        S.chorus_table(192001)


def test_effects_change_the_rows_and_the_dry_plan_stays(bank):
    events, n_blocks, poly, sr = FC.CASES["reverb_default"]
    dry, wet = S.SynthState(bank, sr, poly), S.SynthState(bank, sr, poly, effects=True)
    dl, _ = dry.render(events, n_blocks)
    wl, _ = wet.render(events, n_blocks)
    assert dry.plan()[1].tobytes() == wet.plan()[1].tobytes()   # the 64-byte records do not change with effects
    assert np.any(dl != wl) and np.any(wl[-64 * 20:] != 0) and not np.any(dl[-64 * 20:] != 0)   # the tail is the reverb's


@pytest.mark.parametrize("name", list(FC.CASES))
def test_sends_follow_voice_rs_and_synthesizer_rs(rendered, name):
    """send = clamp((1 / 127) cc + 0.01 (0.1 gs), 0, 1) per voice and block (voice.rs:257-266, channel.rs:197-203, voice.rs:159-160);
    previous = the block before's current, or the current in a voice's first block (voice.rs:231-232, 269-272); chorus[k] = send *
    mix gain, reverb = (0.015 send) (mix left + mix right).  The record's gains are the mix gains times master_volume = 0.5, so
    2 * gain is the mix gain exactly unless a gain is subnormal, which is asserted not to happen."""
    events, n_blocks, poly, sr = FC.CASES[name]
    h = rendered[name]
    rev_cc, cho_cc = FC.channel_sends(events, n_blocks, sr)
    gs = FC.bank_arrays()["instrument_regions"][0]
    pgs = FC.bank_arrays()["preset_regions"][0]
    assert not pgs[:, 15].any() and not pgs[:, 16].any()   # the preset regions add nothing to the sends
    tiny = np.finfo(f32).tiny
    current = {}   # voice object -> (reverb send, chorus send) of its last block
    compared = 0
    for b in range(n_blocks):
        for k in range(h["ptr"][b], h["ptr"][b + 1]):
            r, s = h["rec"][k], h["sends"][k]
            ch = FC.REGION_CHANNEL[name][int(r["desc"])]
            inst_r = f32(0.01) * (f32(0.1) * f32(gs[r["desc"], 16]))
            inst_c = f32(0.01) * (f32(0.1) * f32(gs[r["desc"], 15]))
            cur_r = np.clip((f32(1.0) / f32(127.0)) * f32(rev_cc[b, ch]) + inst_r, f32(0), f32(1))
            cur_c = np.clip((f32(1.0) / f32(127.0)) * f32(cho_cc[b, ch]) + inst_c, f32(0), f32(1))
            prev_r, prev_c = (cur_r, cur_c) if r["flags"] & S.F_START else current[int(r["voice"])]
            current[int(r["voice"])] = (cur_r, cur_c)
            g = r["gain"]
            assert all(x == 0 or abs(x) >= tiny for x in g), (b, k)
            mix = [f32(2.0) * x for x in g]
            want_c = [prev_c * mix[0], cur_c * mix[1], prev_c * mix[2], cur_c * mix[3]]
            want_r = [(f32(0.015) * prev_r) * (mix[0] + mix[2]), (f32(0.015) * cur_r) * (mix[1] + mix[3])]
            assert _bits(s["chorus"]).tolist() == _bits(np.array(want_c, f32)).tolist(), (name, b, k)
            assert _bits(s["reverb"]).tolist() == _bits(np.array(want_r, f32)).tolist(), (name, b, k)
            compared += 1
    assert compared == h["rec"].size and (compared > 0 or name == "silence")


def test_the_send_cases_reach_the_clamp_and_every_write_block_branch(rendered, modelled):
    h = rendered["instrument_sends"]
    mix = f32(2.0) * h["rec"]["gain"][:, 1]
    on = mix > 0
    assert np.any(h["sends"]["chorus"][on, 1] == mix[on])       # a send clamped to exactly 1
    assert np.any((h["sends"]["chorus"][on, 1] < f32(0.05) * mix[on]) & (h["sends"]["chorus"][on, 1] > 0))   # and the small one
    br = modelled["chorus_cc"]["branches"]
    assert all(br["chorus"].get(k, 0) > 0 for k in ("constant", "slope")), br
    assert all(br["reverb"].get(k, 0) > 0 for k in ("constant", "slope", "skip")), br


@pytest.mark.parametrize("sr", [16000, 22050, 48000, 192000])
def test_delay_table_and_lengths(sr):
    table = S.chorus_table(sr)
    want = FM.delay_table(sr)
    comb, allpass, ring, n = FM.lengths(sr)
    assert table.size == want.size == n == {16000: 40000, 22050: 55125, 48000: 120000, 192000: 480000}[sr]
    assert ring == {16000: 64, 22050: 87, 48000: 189, 192000: 750}[sr]
    assert int(comb.sum() + allpass.sum()) == {16000: 9233, 22050: 12731, 48000: 27702, 192000: 110805}[sr]
    assert comb.min() > 64 and allpass.min() > 64 and ring >= 64
    assert np.all(np.abs(table.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))), sr   # one f32 unit in the last place
    assert table.min() >= 1.0 and table.max() < ring - 1   # what lets the kernel index the ring without a test


def test_reverb_constants_are_the_issues():
    fb, d1, d2, w1, w2 = FM.reverb_constants()
    assert (fb, d1, d2, w1, w2) == (f32(0.84), f32(0.2), f32(0.8), f32(1.0), f32(0.0))


@pytest.mark.parametrize("name", list(FC.CASES))
def test_model_equals_the_host_face_bit_for_bit(rendered, modelled, name):
    h, m = rendered[name], modelled[name]
    assert np.array_equal(_bits(m["left"]), _bits(h["left"])), name
    assert np.array_equal(_bits(m["right"]), _bits(h["right"])), name
    if name == "silence":
        assert not h["left"].any() and not h["right"].any()
    else:
        assert m["reverb_out"].any() and h["left"].any()
    if name in ("chorus_cc", "instrument_sends", "sr16k", "sr48k"):
        assert m["chorus_out"][0].any() and m["chorus_out"][1].any()


def test_flush_case_takes_each_of_the_three_flush_branches(modelled):
    flushed = modelled["flush"]["flushed"]
    assert flushed["comb"] > 0 and flushed["store"] > 0 and flushed["allpass"] > 0, flushed


@pytest.mark.parametrize("name", ["chorus_cc", "sr16k", "sr48k", "flush"])
def test_effects_only_face_fed_with_the_models_sums_gives_the_models_outputs(modelled, name):
    m, sr = modelled[name], FC.CASES[name][3]
    fx = S.SynthEffects(sr)
    n = m["reverb_in"].size
    cut = 64 * 3   # two calls: the state goes on
    a = fx.process(m["chorus_in"][0][:cut], m["chorus_in"][1][:cut], m["reverb_in"][:cut])
    b = fx.process(m["chorus_in"][0][cut:], m["chorus_in"][1][cut:], m["reverb_in"][cut:])
    got = [np.concatenate([x, y]) for x, y in zip(a, b)]
    want = [m["chorus_out"][0], m["chorus_out"][1], m["reverb_out"][0], m["reverb_out"][1]]
    for g, w in zip(got, want):
        assert g.size == n and np.array_equal(_bits(g), _bits(w)), name


@pytest.mark.parametrize("name", ["chorus_cc", "steal", "sr16k"])
def test_one_render_equals_three_uneven_renders(bank, rendered, name):
    events, n_blocks, poly, sr = FC.CASES[name]
    st = S.SynthState(bank, sr, poly, effects=True)
    parts = [st.render(events, nb) for nb in (1, 37, n_blocks - 38)]
    for c, key in enumerate(("left", "right")):
        assert np.array_equal(_bits(np.concatenate([p[c] for p in parts])), _bits(rendered[name][key])), name


@pytest.mark.parametrize("sr", [16000, 22050, 48000])
def test_reverb_impulse_returns_after_the_first_comb_and_four_empty_allpasses(sr):
    """A unit impulse at sample 0 of the reverb input: exactly 0 before L1 = round(sr / 44100 * 1116) on the left and exactly 1 at L1 —
    the first comb returns the impulse (filter_store 0.8, times feedback, goes back into the comb; the OUTPUT is the buffer value 1),
    the other combs are still empty, and four empty all-passes negate it four times.  The same on the right at round(sr / 44100 * 1139)."""
    fx = S.SynthEffects(sr)
    n_blocks = 1139 * sr // 44100 // 64 + 2
    x = np.zeros(n_blocks * 64, f32)
    x[0] = 1.0
    _, _, left, right = fx.process(np.zeros_like(x), np.zeros_like(x), x)
    for out, tuning in ((left, 1116), (right, 1139)):
        first = int(np.floor(sr / 44100.0 * tuning + 0.5))
        assert not out[:first].any() and out[first] == 1.0, (sr, tuning)


@pytest.mark.parametrize("sr", [16000, 22050, 192000])
def test_constant_chorus_input_comes_out_unchanged_once_the_ring_is_full(sr):
    fx = S.SynthEffects(sr)
    ring = FM.lengths(sr)[2]
    n = (ring // 64 + 3) * 64
    c = f32(0.37)
    left, right, _, _ = fx.process(np.full(n, c, f32), np.full(n, -c, f32), np.zeros(n, f32))
    assert np.all(left[ring:] == c) and np.all(right[ring:] == -c) and left[0] == 0.0


def test_host_only_batch_with_effects_checks_arguments_then_reports_no_device(bank):
    b = S.SynthBatch(bank, 2, 22050, device=None, effects=True)
    events = [FC.CASES["reverb_default"][0], None]
    with pytest.raises(ValueError, match="null left or right"):
        b.render(events, 4, [0, 16], [16, 16])
    with pytest.raises(ValueError, match="4-byte aligned"):
        b.render(events, 4, [18, 16], [16, 16])
    with pytest.raises(PvqError) as e:
        b.render(events, [4, 0], [16, 0], [16, 0])
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
