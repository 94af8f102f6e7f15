"""Inputs of the synth stage's effect tests (reverb and chorus), kept small.  The bank is tests/synth_cases.py's with generators 15
(chorusEffectsSend) and 16 (reverbEffectsSend) set on two instrument regions: on the sine (region 0, preset 0) a reverb send of 0.8,
which clamps to 1 together with the channel's default CC 0x5B of 40 / 127, and a chorus send of 0.03; on the saw (region 1, preset 1)
a chorus send of 0.7 and a reverb send of 0.02.  Every other region has no send of its own."""
import numpy as np

import synth_cases as SC

ON, OFF, CC, PC = SC.ON, SC.OFF, SC.CC, SC.PC
SENDS = {0: dict(reverb=800, chorus=30), 1: dict(reverb=20, chorus=700)}   # instrument region -> generator values (0.1 % units)


def bank_arrays():
    a = SC.bank_arrays()
    gs = a["instrument_regions"][0].copy()
    for region, v in SENDS.items():
        gs[region, 16] = v["reverb"]
        gs[region, 15] = v["chorus"]
    a["instrument_regions"] = (gs, a["instrument_regions"][1])
    return a


def _loud(ch=0, patch=7):
    """the quiet sine (region 9: no sends of its own), as loud as the channel goes"""
    return [(0.0, ch, PC, patch, 0), (0.0, ch, CC, 0x07, 127)]


# name -> (events, n_blocks, maximum_polyphony, sample_rate)
CASES = {
    # one note and its tail at the default sends: several wraps of the longest comb (820 samples at 22 050 Hz)
    "reverb_default": (SC.ev(*_loud(), (0.0001, 0, ON, 57, 127), (0.1501, 0, OFF, 57, 0)), 120, 64, 22050),
    # chorus from the start; send steps large enough for the slope branch; CC 0x5B to 0: the reverb gain falls to 0 (slope, then skip)
    "chorus_cc": (SC.ev(*_loud(), (0.0, 0, CC, 0x5D, 127), (0.0001, 0, ON, 57, 127), (0.1001, 0, CC, 0x5D, 20), (0.2001, 0, CC, 0x5B, 0),
                        (0.2501, 0, CC, 0x5D, 90), (0.3001, 0, OFF, 57, 0)), 150, 64, 22050),
    # two presets of the modified bank on two channels; on channel 1 the CC and the instrument's 0.7 clamp to 1
    "instrument_sends": (SC.ev((0.0, 0, PC, 0, 0), (0.0, 1, PC, 1, 0), (0.0001, 0, ON, 57, 110), (0.0002, 1, ON, 60, 110), (0.0301, 1, CC, 0x5D, 60),
                               (0.1001, 0, OFF, 57, 0), (0.1201, 1, OFF, 60, 0)), 80, 64, 22050),
    # a short note, then silence until combs, filter stores and all-passes fall under 1e-6
    "flush": (SC.ev(*_loud(), (0.0001, 0, ON, 57, 60), (0.0301, 0, OFF, 57, 0)), 700, 64, 22050),
    "mixed": SC.CASES["mixed"] + (22050,),
    "steal": SC.CASES["steal"] + (22050,),
    # the chorus ring is exactly one block; the 82-sample all-pass reuses its slots in the very next block
    "sr16k": (SC.ev(*_loud(), (0.0, 0, CC, 0x5D, 127), (0.0001, 0, ON, 57, 127), (0.1501, 0, OFF, 57, 0)), 60, 64, 16000),
    "sr48k": (SC.ev(*_loud(), (0.0, 0, CC, 0x5D, 100), (0.0001, 0, ON, 64, 127), (0.0401, 0, OFF, 64, 0)), 40, 64, 48000),
    "silence": (SC.ev(), 40, 64, 22050),
}
AT_22050 = [n for n, c in CASES.items() if c[3] == 22050]
# the channel every instrument region sounds on, per case (a record names its region, not its channel): for the check of the sends
REGION_CHANNEL = {
    "reverb_default": {9: 0}, "chorus_cc": {9: 0}, "instrument_sends": {0: 0, 1: 1}, "flush": {9: 0}, "steal": {0: 0, 1: 1},
    "mixed": {0: 0, 1: 1, 2: 2, 3: 3, 6: 4, 7: 4, 4: 9, 5: 9}, "sr16k": {9: 0}, "sr48k": {9: 0}, "silence": {},
}


def channel_sends(events, n_blocks, sample_rate):
    """(reverb cc, chorus cc) int arrays [n_blocks][16]: the channels' CC 0x5B / 0x5D values when block b is processed
    (midifile_sequencer.rs:87-103: events with time <= current_time, current_time grown by the repeated f64 addition)"""
    t, ch, cmd, d1, d2 = events
    rev, cho = np.full(16, 40), np.zeros(16, np.int64)   # channel.rs:62-63
    out_r, out_c = np.zeros((n_blocks, 16), np.int64), np.zeros((n_blocks, 16), np.int64)
    now, i = 0.0, 0
    for b in range(n_blocks):
        while i < len(t) and t[i] <= now:
            if cmd[i] == CC and 0 <= ch[i] < 16:
                if d1[i] == 0x5B:
                    rev[ch[i]] = d2[i] & 0xFF
                elif d1[i] == 0x5D:
                    cho[ch[i]] = d2[i] & 0xFF
                elif d1[i] == 0x79:
                    pass   # reset_all_controllers leaves the sends (channel.rs:73-81)
            i += 1
        now += 64 / sample_rate
        out_r[b], out_c[b] = rev, cho
    return out_r, out_c
