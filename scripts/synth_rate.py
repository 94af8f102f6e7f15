#!/usr/bin/env python
"""What the synth stage costs: stream-seconds of audio rendered per second for 64 / 1 024 / 4 096 streams at a polyphony of about 8
and about 48, with the planner's host time and the replay's device time reported separately (pvq_synth_batch_last_times), and beside
both the host face (pvq_synth_state_render, one state per stream on 16 threads) and a hipMemsetAsync over the output bytes, as the
other stages report.  A stream is rendered in calls of 32 blocks (93 ms at 22 050 Hz): the plan is 64 bytes per voice-block.

usage: python scripts/synth_rate.py [--out FILE] [--streams 64,1024,4096] [--seconds 0.75]
Needs a GPU; reads nothing outside the tree."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import synth_cases as SC  # noqa: E402
from pitchvis_amd import synth as S  # noqa: E402

CALL_BLOCKS, THREADS = 32, 16


def chords(n_streams, voices, seconds):
    """per stream: `voices` sustained notes struck over the first 50 ms (sine, saw and wobble presets by channel), one restruck every 100 ms"""
    out = []
    for s in range(n_streams):
        rows = [(0.0, c, SC.PC, (0, 1, 3)[c], 0) for c in range(3)]
        rows += [(0.0005 + 0.05 * i / voices, i % 3, SC.ON, 30 + (i * 7 + s) % 70, 60 + (i * 11 + s) % 60) for i in range(voices)]
        t = 0.1
        while t < seconds:
            i = int(t * 10) % voices
            rows += [(t, i % 3, SC.OFF, 30 + (i * 7 + s) % 70, 0), (t + 0.001, i % 3, SC.ON, 30 + (i * 7 + s) % 70, 90)]
            t += 0.1
        out.append(SC.ev(*rows))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", default="64,1024,4096")
    ap.add_argument("--seconds", type=float, default=0.75)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "synth_rate.py needs a GPU"
    bank = S.SynthBank.from_arrays(**SC.bank_arrays())
    n_calls = max(1, int(args.seconds * SC.SR / 64 / CALL_BLOCKS))
    seconds = n_calls * CALL_BLOCKS * 64 / SC.SR
    lines = [f"# synth stage: n streams x {seconds:.3f} s at {SC.SR} Hz in {n_calls} calls of {CALL_BLOCKS} blocks; times in ms, summed over the calls",
             f"# planner: host, at most 16 threads; upload and replay: HIP events; host face: pvq_synth_state_render on {THREADS} threads; memset: the output bytes",
             "# streams  voices  voice-blocks   planner_ms  layout_ms  upload_ms  replay_ms  call_wall_ms  stream-s/s (wall)  stream-s/s (replay)  host_face_ms  memset_ms"]
    for n in [int(x) for x in args.streams.split(",")]:
        for voices in (8, 48):
            events = chords(n, voices, seconds)
            d_l = [torch.empty(CALL_BLOCKS * 64, device="cuda") for _ in range(n)]
            d_r = [torch.empty(CALL_BLOCKS * 64, device="cuda") for _ in range(n)]
            S.SynthBatch(bank, n, SC.SR, 64).render(events, CALL_BLOCKS, d_l, d_r)   # warm: the kernel's code, the allocator
            torch.cuda.synchronize()
            batch = S.SynthBatch(bank, n, SC.SR, 64)
            tot = dict(plan_ms=0.0, stage_ms=0.0, upload_ms=0.0, replay_ms=0.0, records=0)
            t0 = time.perf_counter()
            for _ in range(n_calls):
                batch.render(events, CALL_BLOCKS, d_l, d_r)
                for k, v in batch.last_times().items():
                    tot[k] += v
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            # the host face: a state per stream, 16 threads (ctypes drops the GIL in the call); at most 256 streams, scaled
            m = min(n, 256)
            states = [S.SynthState(bank, SC.SR, 64) for _ in range(m)]
            with ThreadPoolExecutor(THREADS) as pool:
                t0 = time.perf_counter()
                list(pool.map(lambda s: [states[s].render(events[s], CALL_BLOCKS) for _ in range(n_calls)], range(m)))
                host = (time.perf_counter() - t0) * 1e3 * n / m
            buf = torch.empty(2 * n * CALL_BLOCKS * 64, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            buf.zero_()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n_calls):
                buf.zero_()
            e1.record()
            torch.cuda.synchronize()
            lines.append(f"{n:9d}  {voices:6d}  {tot['records']:12d}  {tot['plan_ms']:11.2f}  {tot['stage_ms']:9.2f}  {tot['upload_ms']:9.2f}  {tot['replay_ms']:9.2f}"
                         f"  {wall:12.2f}  {n * seconds / wall * 1e3:17.1f}  {n * seconds / max(tot['replay_ms'], 1e-9) * 1e3:19.1f}  {host:12.2f}"
                         f"{'*' if m < n else ' '} {e0.elapsed_time(e1):9.3f}")
    lines.append("# (* the host face was timed on 256 streams and scaled to the size)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
