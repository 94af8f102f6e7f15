#!/usr/bin/env python
"""What the synth stage's effects cost, in the manner of scripts/synth_rate.py: the replay kernel's device time with reverb and
chorus (synth_replay_fx) beside the dry replay (synth_replay) of the SAME build on the same events — the plans are equal, record for
record; effects add the sends — for 64 / 1 024 / 4 096 streams at a polyphony of about 8 and about 48, with the planner's host time
of both, a hipMemsetAsync over the output bytes, and the effect state a block touches.

usage: python scripts/synth_fx_rate.py [--out FILE] [--streams 64,1024,4096] [--seconds 0.75]
Needs a GPU; reads nothing outside the tree."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import synth_cases as SC  # noqa: E402
import synth_fx_cases as FC  # noqa: E402
import synth_fx_model as FM  # noqa: E402
from pitchvis_amd import synth as S  # noqa: E402
from synth_rate import CALL_BLOCKS, chords  # noqa: E402


def timed(bank, n, events, n_calls, d_l, d_r, effects):
    S.SynthBatch(bank, n, SC.SR, 64, effects=effects).render(events, CALL_BLOCKS, d_l, d_r)   # warm: the kernel's code, the allocator
    torch.cuda.synchronize()
    batch = S.SynthBatch(bank, n, SC.SR, 64, effects=effects)
    tot = dict(plan_ms=0.0, stage_ms=0.0, upload_ms=0.0, replay_ms=0.0, records=0)
    t0 = time.perf_counter()
    for _ in range(n_calls):
        batch.render(events, CALL_BLOCKS, d_l, d_r)
        for k, v in batch.last_times().items():
            tot[k] += v
    torch.cuda.synchronize()
    tot["wall_ms"] = (time.perf_counter() - t0) * 1e3
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", default="64,1024,4096")
    ap.add_argument("--seconds", type=float, default=0.75)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "synth_fx_rate.py needs a GPU"
    bank = S.SynthBank.from_arrays(**FC.bank_arrays())
    n_calls = max(1, int(args.seconds * SC.SR / 64 / CALL_BLOCKS))
    seconds = n_calls * CALL_BLOCKS * 64 / SC.SR
    comb, allpass, ring, table = FM.lengths(SC.SR)
    state = 4 * (int(comb.sum() + allpass.sum()) + 2 * ring + 16) + 8
    touched = 4 * 64 * (2 * 24 + 2 * 2 + 2)   # per block: 24 buffers read and written 64 values each, 2 rings written, <= 2 x 2 ring reads; 64 table reads x 2
    lines = [f"# synth stage with effects: n streams x {seconds:.3f} s at {SC.SR} Hz in {n_calls} calls of {CALL_BLOCKS} blocks; times in ms, summed over the calls",
             "# dry: synth_replay; fx: synth_replay_fx of the same build on the same events; planner: host, at most 16 threads; replay: HIP events; memset: the output bytes",
             f"# effect state of a stream: {state} bytes ({int(comb.sum() + allpass.sum())} reverb floats, 2 x {ring} ring floats, 16 filter stores, a count);"
             f" touched per block: about {touched} bytes (24 buffers x 64 values read and written, 2 ring rows written and up to 4 read, 128 table entries)",
             "# streams  voices  voice-blocks   dry_plan_ms  fx_plan_ms  dry_replay_ms  fx_replay_ms  fx/dry  fx_upload_ms  fx_call_wall_ms  stream-s/s (fx replay)  memset_ms"]
    for n in [int(x) for x in args.streams.split(",")]:
        for voices in (8, 48):
            events = chords(n, voices, seconds)   # (the saw's region has a chorus send of 0.7, every channel the default reverb send)
            d_l = [torch.empty(CALL_BLOCKS * 64, device="cuda") for _ in range(n)]
            d_r = [torch.empty(CALL_BLOCKS * 64, device="cuda") for _ in range(n)]
            dry = timed(bank, n, events, n_calls, d_l, d_r, False)
            fx = timed(bank, n, events, n_calls, d_l, d_r, True)
            assert dry["records"] == fx["records"]
            buf = torch.empty(2 * n * CALL_BLOCKS * 64, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            buf.zero_()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n_calls):
                buf.zero_()
            e1.record()
            torch.cuda.synchronize()
            lines.append(f"{n:9d}  {voices:6d}  {fx['records']:12d}  {dry['plan_ms']:12.2f}  {fx['plan_ms']:10.2f}  {dry['replay_ms']:13.2f}  {fx['replay_ms']:12.2f}"
                         f"  {fx['replay_ms'] / max(dry['replay_ms'], 1e-9):6.2f}  {fx['upload_ms']:12.2f}  {fx['wall_ms']:15.2f}"
                         f"  {n * seconds / max(fx['replay_ms'], 1e-9) * 1e3:22.1f}  {e0.elapsed_time(e1):9.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
