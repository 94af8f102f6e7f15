"""CPU checks of the synth stage's edge inputs (tests/synth_edge_cases.py), so that the device tests of tests/test_synth_edges_gpu.py
compare against a yardstick that has itself been checked: the conditions the inputs are made for (a whole chorus LFO cycle with
signal, blocks with nearly all and nearly no taps read from the block's own inputs, a ring index through all 65 residues, the
hard-left and hard-right skip values, samples that end inside a block, a filter that goes off and on), the host face against the
sample-by-sample NumPy model bit for bit, and split renders whose cuts isolate each wrap of the delay table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth_edge_cases as EC
import synth_fx_model as FM
from pitchvis_amd import synth as S

MODELLED = EC.LONG + ["pan_edges", "rate_44100", "rate_192000"]   # (the two-lap case: 10 s of model for a second lap the host walks like the first)
MODELLED_DRY = ["noloop_end", "exclusive", "sweep"]   # the other dry cases: device against host (the model takes 5 s per 650 blocks)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def bank():
    return S.SynthBank.from_arrays(**EC.bank_arrays())


@pytest.fixture(scope="module")
def rendered(bank):
    """every case on the host face with effects at polyphony 64, once: (group, name) -> dict(left, right, ptr, rec, sends)"""
    out = {}
    for group, cases in (("edge", EC.CASES), ("dry", EC.DRY)):
        for name, (events, n_blocks, sr) in cases.items():
            st = S.SynthState(bank, sr, EC.POLYPHONY, effects=True)
            left, right = st.render(events, n_blocks)
            ptr, rec = st.plan()
            sptr, sends = st.sends()
            assert np.array_equal(ptr, sptr) and sends.size == rec.size and ptr.size == n_blocks + 1
            for a in (left, right, ptr, rec, sends):
                a.setflags(write=False)
            out[group, name] = dict(left=left, right=right, ptr=ptr, rec=rec, sends=sends)
    return out


def test_the_case_tables_are_the_ones_the_device_tests_expect():
    assert list(EC.CASES) == EC.LONG + ["pan_edges"] + EC.HIGH_RATES + [EC.TWO_LAPS]
    _, n_blocks, sr = EC.CASES[EC.TWO_LAPS]   # the right channel's table index passes twice the table's length before the end
    assert sr == 16200 and FM.lengths(sr)[3] // 4 + (n_blocks - 16) * 64 > 2 * FM.lengths(sr)[3]
    assert len(EC.DRY) == 13 and all(c[2] == EC.SR for c in EC.DRY.values())
    assert [(EC.CASES[n][1], EC.CASES[n][2]) for n in EC.LONG] == [(640, 16000), (650, 16200)]
    assert [(EC.CASES[n][1], EC.CASES[n][2]) for n in EC.HIGH_RATES] == [(59, 44100), (129, 96000), (257, 192000)]
    for name in EC.HIGH_RATES:   # 2.3 wraps of the rate's longest comb, rounded up to whole blocks
        _, n_blocks, sr = EC.CASES[name]
        assert n_blocks == int(2.3 * FM.lengths(sr)[0].max() / 64) + 1, name
    assert sum(EC.SPLIT_16200) == 650


def test_tap_stats_restate_what_todays_cases_reach():
    """the helper on the rates and lengths of tests/synth_fx_cases.py: at 22 050 Hz over `mixed`'s 340 blocks at most 39 (left) and
    105 (right) of 128 taps are fresh and the table does not wrap; at 48 kHz no tap is fresh"""
    left, right = EC.chorus_tap_stats(22050, 340)
    assert (left["fresh_max"], right["fresh_max"], left["wraps"], right["wraps"]) == (39, 105, 0, 0)
    assert abs(left["delay_min"] - 44.1) < 1e-3 and 11.0 < right["delay_min"] < 11.1
    left, right = EC.chorus_tap_stats(48000, 40)
    assert left["fresh_max"] == right["fresh_max"] == 0
    assert EC.chorus_tap_stats(16000, 60)[0]["fresh_max"] <= 63


@pytest.mark.parametrize("name", EC.LONG)
def test_long_chorus_runs_a_whole_lfo_cycle_with_signal_in_the_ring(rendered, name):
    _, n_blocks, sr = EC.CASES[name]
    for c, stats in enumerate(EC.chorus_tap_stats(sr, n_blocks)):
        assert stats["wraps"] == 1, (c, stats)                                     # the table index returns to 0 exactly once
        assert stats["fresh_max"] >= 120 and stats["fresh_min"] <= 8, (c, stats)   # of 128: nearly all from the block's sums, nearly all from the ring
        assert stats["delay_min"] < 2.0, (c, stats)
        assert stats["fresh_max"] < 128                                            # (a delay is at least one sample: the first sample's taps are never fresh)
    h = rendered["edge", name]
    for b in range(1, n_blocks):   # the chorus send is audible in every block after the first, left and right
        s = h["sends"][h["ptr"][b]:h["ptr"][b + 1]]
        assert s.size and s["chorus"][:, 0:2].max() >= FM.NON_AUDIBLE and s["chorus"][:, 2:4].max() >= FM.NON_AUDIBLE, (name, b)
    assert h["left"][-64:].any() and h["right"][-64:].any()


def test_at_16200_hz_the_ring_index_takes_all_65_residues():
    _, n_blocks, sr = EC.CASES["long_chorus_16200"]
    ring = FM.lengths(sr)[2]
    assert ring == 65 and FM.lengths(16000)[2] == 64
    assert len({(64 * b) % ring for b in range(n_blocks)}) == 65
    assert all(FM.lengths(r)[2] == 65 for r in (16154, 16410)) and FM.lengths(16153)[2] == 64 and FM.lengths(16411)[2] == 66
    assert [FM.lengths(r)[2] for r in (44100, 96000, 192000)] == [173, 376, 750]
    assert int(FM.lengths(192000)[0].max()) == 7140


def test_pan_edges_reaches_hard_left_and_hard_right_with_the_chorus_on(rendered):
    h = rendered["edge", "pan_edges"]
    reached = set(EC.skip_values(h["rec"], h["sends"]).tolist())
    assert {5, 10, 21, 26} <= reached, sorted(reached)   # hard right, hard left; the same with the reverb off
    assert 0 in reached                                   # and, before the first pan change, every channel sounding


def test_dry_cases_carry_ending_samples_and_a_filter_that_goes_off_and_on(rendered):
    for name in ("noloop_end", "exclusive"):
        assert np.count_nonzero(rendered["dry", name]["rec"]["flags"] & S.F_ENDS) >= 2, name
    for name in ("sweep", "wobble"):
        h = rendered["dry", name]
        active = (h["rec"]["flags"] & S.F_FILTER) != 0
        assert active.any() and (~active).any(), name
        # a voice's inactive block followed by an active one: the filter memory the active block starts from is walk_end's copy
        last, off_to_on = {}, 0
        for k in range(h["rec"].size):
            v = int(h["rec"]["voice"][k])
            if h["rec"]["flags"][k] & S.F_START:
                last.pop(v, None)
            off_to_on += int(v in last and not last[v] and bool(active[k]))
            last[v] = bool(active[k])
        assert off_to_on > 0, name
    for name in EC.DRY:   # effects on: something but the dry sum reaches the rows of every case that sounds
        if name != "silence":
            h = rendered["dry", name]
            assert (EC.skip_values(h["rec"], h["sends"]) & 28 != 28).any(), name


@pytest.mark.parametrize("group,name", [("edge", n) for n in MODELLED] + [("dry", n) for n in MODELLED_DRY])
def test_model_equals_the_host_face_bit_for_bit(rendered, group, name):
    _, n_blocks, sr = (EC.CASES if group == "edge" else EC.DRY)[name]
    h = rendered[group, name]
    m = FM.render(EC.bank_arrays(), sr, h["ptr"], h["rec"], h["sends"], S.chorus_table(sr), n_blocks)
    assert np.array_equal(_bits(m["left"]), _bits(h["left"])), name
    assert np.array_equal(_bits(m["right"]), _bits(h["right"])), name
    assert m["reverb_out"].any() and h["left"].any()
    if group == "edge":
        assert m["chorus_out"][0].any() and m["chorus_out"][1].any()
    if name in EC.LONG:   # the chorus still sounds in the last block, after both table wraps
        assert m["chorus_out"][0][-64:].any() and m["chorus_out"][1][-64:].any()


def test_which_inputs_tell_a_wrong_block_chorus_from_the_right_one(bank):
    """The device computes the chorus a block at a time; EC.block_chorus restates that argument, and its variants are ways of
    getting it wrong.  Fed with a case's dry render as the chorus input (the case's chorus input is the same voice times a gain),
    the restatement equals the sample-by-sample host effects bit for bit, and each variant differs in the cases named here — so a
    device test on those cases fails for a kernel with that fault.  Two findings are kept as assertions:
    * `written <= lane` for `written < lane` changes NOTHING, at any admitted rate: a tap reads the slot its own sample writes only
      at a delay of exactly 1 sample, and the shortest delay is 0.0001 sr >= 1.6.  The off-by-one that matters is the other way
      (`stale_by_one`: the slot written by the sample just before), which only delays under 2 samples reach;
    * without the wrap of the per-block table index the first lap is still right (the per-lane wrap takes one table length off):
      only the second lap of `long_chorus_two_laps`, in one call, differs."""
    differs = {}
    for name in EC.LONG + [EC.TWO_LAPS]:
        events, n_blocks, sr = EC.CASES[name]
        dry = np.stack(S.SynthState(bank, sr, EC.POLYPHONY).render(events, n_blocks))
        assert dry[0][-64:].any() and dry[1][-64:].any()
        table = S.chorus_table(sr)
        want = np.stack(S.SynthEffects(sr).process(dry[0], dry[1], np.zeros_like(dry[0]))[:2])
        assert np.array_equal(_bits(EC.block_chorus(dry, sr, table)), _bits(want)), name
        differs[name] = {v for v in EC.VARIANTS if not np.array_equal(_bits(EC.block_chorus(dry, sr, table, v)), _bits(want))}
    assert differs["long_chorus_16000"] == {"stale_by_one"}                               # ring = one block: no ring wrap to get wrong
    assert differs["long_chorus_16200"] == {"stale_by_one", "masked", "lane_ring_wrap"}   # 65 slots: written == 64, every residue
    assert differs[EC.TWO_LAPS] == {"stale_by_one", "masked", "lane_ring_wrap", "block_table_wrap"}
    assert 1.0 < 0.0001 * 16000 and S.chorus_table(16000).min() > 1.5


def test_one_render_of_the_65_slot_case_equals_calls_that_isolate_each_table_wrap(bank, rendered):
    events, n_blocks, sr = EC.CASES["long_chorus_16200"]
    table = FM.lengths(sr)[3]
    starts = np.cumsum([0] + EC.SPLIT_16200)
    assert starts[1] * 64 <= table - table // 4 < (starts[1] + 1) * 64   # the right table index reaches 0 inside block 474
    assert starts[3] * 64 <= table < (starts[3] + 1) * 64                # and the left inside block 632
    st = S.SynthState(bank, sr, EC.POLYPHONY, effects=True)
    parts = [st.render(events, nb) for nb in EC.SPLIT_16200]
    for c, key in enumerate(("left", "right")):
        assert np.array_equal(_bits(np.concatenate([p[c] for p in parts])), _bits(rendered["edge", "long_chorus_16200"][key])), key
