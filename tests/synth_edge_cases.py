"""Inputs of the synth stage's edge tests (tests/test_synth_edges.py, tests/test_synth_edges_gpu.py), small and generated: a whole
cycle of the chorus LFO with signal in the ring, a ring of 65 slots whose index wraps at every residue, hard-left and hard-right
voices with the chorus on, the rates from 44 100 Hz up, and the dry cases of tests/synth_cases.py rendered with effects.  The bank is
tests/synth_fx_cases.py's.  `chorus_tap_stats` says, from the model's delay table alone, which taps of a block read a slot that the
same block has written, and how often the table wraps."""
import numpy as np

import synth_cases as SC
import synth_fx_cases as FC
import synth_fx_model as FM

ON, OFF, CC, PC = SC.ON, SC.OFF, SC.CC, SC.PC
SR = 22050
POLYPHONY = 64
bank_arrays = FC.bank_arrays

# the quiet sine (region 9 sustains: no note-off) with the chorus send at 1: the delay table has round(sr / 0.4) entries
_LONG = SC.ev(*FC._loud(), (0.0, 0, CC, 0x5D, 127), (0.0001, 0, ON, 57, 127))
# preset 5: the sine hard left (pan -500) layered with the saw at pan +250; CC 0x0A moves both to the clamps, CC 0x5B takes the reverb away
_PAN = SC.ev((0.0, 0, PC, 5, 0), (0.0, 0, CC, 0x07, 127), (0.0, 0, CC, 0x5D, 127), (0.0001, 0, ON, 57, 100), (0.0501, 0, CC, 0x0A, 127),
             (0.1001, 0, CC, 0x0A, 0), (0.1501, 0, CC, 0x5B, 0), (0.2001, 0, CC, 0x0A, 127), (0.2501, 0, OFF, 57, 0))
_NOTE = SC.ev(*FC._loud(), (0.0, 0, CC, 0x5D, 127), (0.0001, 0, ON, 57, 127), (0.1501, 0, OFF, 57, 0))   # FC.CASES["sr16k"]'s shape

# name -> (events, n_blocks, sample_rate), all at polyphony 64
CASES = {
    "long_chorus_16000": (_LONG, 640, 16000),   # 40 960 samples over a table of 40 000; the ring is exactly one block
    "long_chorus_16200": (_LONG, 650, 16200),   # 41 600 samples over a table of 40 500; a ring of 65 slots
    "pan_edges": (_PAN, 100, SR),
    "rate_44100": (_NOTE, 59, 44100),           # 2.3 wraps of each rate's longest comb (1 640, 3 570, 7 140 samples)
    "rate_96000": (_NOTE, 129, 96000),
    "rate_192000": (_NOTE, 257, 192000),
    # 72 960 samples in ONE call: the right channel's table index (it starts at table // 4) passes 2 x 40 500 inside block 1107.  A
    # kernel that forgot to wrap its per-block table index is still right in the first lap, because the per-lane wrap takes one
    # table length off; only a second lap within one call shows it (test_synth_edges.py: the block-at-a-time restatement)
    "long_chorus_two_laps": (_LONG, 1140, 16200),
}
LONG = ["long_chorus_16000", "long_chorus_16200"]
TWO_LAPS = "long_chorus_two_laps"
HIGH_RATES = ["rate_44100", "rate_96000", "rate_192000"]
SPLIT_16200 = [474, 1, 157, 1, 17]   # the right channel's table wraps inside block 474, the left's inside block 632: each alone in a call
# the thirteen dry cases with effects on, with their own block counts: name -> (events, n_blocks, sample_rate)
DRY = {name: (events, n_blocks, SR) for name, (events, n_blocks, _) in SC.CASES.items()}


def skip_values(rec, sends):
    """per record the five skip bits of write_block (synthesizer.rs:485: max(previous, current) < 1e-3), a set bit = not added:
    1 dry left, 2 dry right, 4 chorus left, 8 chorus right, 16 reverb"""
    pairs = [rec["gain"][:, 0:2], rec["gain"][:, 2:4], sends["chorus"][:, 0:2], sends["chorus"][:, 2:4], sends["reverb"][:, 0:2]]
    out = np.zeros(rec.size, np.int64)
    for c, p in enumerate(pairs):
        out |= (p.max(axis=1) < FM.NON_AUDIBLE).astype(np.int64) << c
    return out


VARIANTS = ("le", "stale_by_one", "masked", "lane_ring_wrap", "block_table_wrap")


def block_chorus(chorus_in, sr, table, variant=None):
    """The chorus a BLOCK at a time, lane = sample, as the device replay argues it (synth_fx_batch.hip, step 3): a tap whose slot an
    earlier sample of the same block writes (`written < lane`) takes that sample's input, any other the ring as it stood before the
    block; then the block's 64 inputs go to the ring; ring and table indices advance by 64 with one conditional subtraction.
    chorus_in float32 [2][n_blocks * 64] -> float32 [2][n_blocks * 64].  `variant` names one way of getting it wrong, so that a test
    can say which inputs tell the difference: "le" (`written <= lane`), "stale_by_one" (`written + 1 < lane`), "masked"
    (`(written & 63) < lane`), "lane_ring_wrap" (no `ri >= ring` wrap of a lane's ring index, in the tap and in the store),
    "block_table_wrap" (no wrap of the per-block table index).  The two rings lie side by side as on the device, so an index past a
    ring's end lands in the next one; the table is followed by zeros."""
    assert variant is None or variant in VARIANTS
    _, _, ring, table_len = FM.lengths(sr)
    assert table.size == table_len
    n_blocks = chorus_in.shape[1] // 64
    table = np.concatenate([table.astype(np.float64), np.zeros(n_blocks * 64 + 64)])
    rings = np.zeros(2 * ring + 192, np.float32)
    out = np.zeros((2, n_blocks * 64), np.float32)
    lane = np.arange(64, dtype=np.int64)
    ring_index, table_index = 0, [0, table_len // 4]
    for b in range(n_blocks):
        sums = chorus_in[:, b * 64:(b + 1) * 64]
        ri = ring_index + lane
        if variant != "lane_ring_wrap":
            ri = np.where(ri >= ring, ri - ring, ri)
        for c in range(2):
            ti = table_index[c] + lane
            ti = np.where(ti >= table_len, ti - table_len, ti)
            position = ri.astype(np.float64) - table[ti]
            position = np.where(position < 0.0, position + float(ring), position)
            index1 = position.astype(np.int64)
            index2 = np.where(index1 + 1 == ring, 0, index1 + 1)
            x = []
            for j in (index1, index2):
                written = np.where(j >= ring_index, j - ring_index, j + ring - ring_index)
                fresh = {None: written < lane, "le": written <= lane, "stale_by_one": written + 1 < lane, "masked": (written & 63) < lane}.get(
                    variant, written < lane)
                x.append(np.where(fresh, sums[c][written & 63], rings[c * ring + j]).astype(np.float64))
            out[c, b * 64:(b + 1) * 64] = (x[0] + (position - index1.astype(np.float64)) * (x[1] - x[0])).astype(np.float32)
        for c in range(2):   # every load of the block stands before its stores
            rings[c * ring + ri] = sums[c]
        ring_index += 64
        if ring_index >= ring:
            ring_index -= ring
        for c in range(2):
            table_index[c] += 64
            if table_index[c] >= table_len and variant != "block_table_wrap":
                table_index[c] -= table_len
    return out


def chorus_tap_stats(sr, n_blocks):
    """chorus.rs:59-117 restated for its indices alone, over the first `n_blocks` blocks of a stream: per channel (left, right) a dict
    of fresh_min / fresh_max (of a block's 64 x 2 taps, how many read a slot that an EARLIER sample of the same block has written),
    wraps (how often the table index returns to 0) and delay_min / delay_max (samples) over the table entries used."""
    _, _, ring, table_len = FM.lengths(sr)
    table = FM.delay_table(sr).astype(np.float64)
    n = np.arange(n_blocks * 64, dtype=np.int64)
    t = n % 64                          # the sample of its block
    ring_index = n % ring
    block_start = (n - t) % ring        # the ring index of the block's first sample
    out = []
    for c in range(2):
        table_index = (n + c * (table_len // 4)) % table_len
        delay = table[table_index]
        position = ring_index.astype(np.float64) - delay
        position = np.where(position < 0.0, position + float(ring), position)
        index1 = position.astype(np.int64)
        index2 = np.where(index1 + 1 == ring, 0, index1 + 1)
        fresh = np.zeros(n.size, np.int64)
        for index in (index1, index2):
            written = (index - block_start) % ring   # the sample of this block that writes the slot, if below 64
            fresh += written < t
        per_block = fresh.reshape(n_blocks, 64).sum(axis=1)
        out.append(dict(fresh_min=int(per_block.min()), fresh_max=int(per_block.max()), wraps=int(np.count_nonzero(table_index[1:] == 0)),
                        delay_min=float(delay.min()), delay_max=float(delay.max())))
    return tuple(out)
