#!/usr/bin/env python3
"""Rate of the pitch-ball scene stage (SceneBatch.frames_device) in stream-frames per second, beside the AnalysisBatch.preprocess_device
time for the same rows and the host SceneState on 16 threads, all from one run.  Settle phase, then the median of repeats; every timed
region is closed by a device synchronisation.  Writes the table to stdout (profiles/scene_batch_rate.txt keeps a run's output)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pitchvis_amd as P  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402

CASES = [(64, 7, 36, 64), (256, 7, 36, 64), (4096, 7, 36, 16), (256, 7, 84, 32)]   # streams, octaves, bpo, frames per call
MAX_PEAKS, DT = 64, 1.0 / 30.0


def db_frames(ns, nf, n, seed):
    """dB-like frames: a noise floor and a few held notes per stream, so that every frame has peaks to place"""
    rng = np.random.default_rng(seed)
    db = rng.random((ns, nf, n), dtype=np.float32) * 6.0
    for s in range(ns):
        for b in rng.integers(3, n - 3, 8):
            db[s, :, b] = rng.uniform(18.0, 50.0)
            db[s, :, b - 1] = np.maximum(db[s, :, b - 1], 12.0)
    return db


def timed(fn, settle, repeats):
    import torch
    for _ in range(settle):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def host_rate(rng, fields, n, nf, threads=16, streams=64):
    """the host SceneState over `streams` streams of the same inputs, on a pool of `threads` threads (the C call releases the GIL)"""
    L = _lib.load()
    h = {k: v[:streams].cpu().numpy() for k, v in fields.items()}
    fp = C.POINTER(C.c_float)

    def one(s):
        st = P.SceneState(rng)
        for f in range(nf):
            L.pvq_scene_state_update(st._h, h["center"][s, f].ctypes.data_as(fp), h["size"][s, f].ctypes.data_as(fp), int(h["peak_count"][s, f]),
                                     h["calmness"][s, f].ctypes.data_as(fp), h["pitch_accuracy"][s, f].ctypes.data_as(fp),
                                     h["pitch_deviation"][s, f].ctypes.data_as(fp), float(h["scene_calmness"][s, f]), int(round(DT * 1e9)))
    ts = []
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(one, range(streams)))
            ts.append(time.perf_counter() - t0)
    return streams * nf / statistics.median(ts)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}; settle {a.settle} calls, median of {a.repeats}; stream-frames per second")
    print("# streams x bins x frames/call | scene: median ms (min .. max), frames/s | AnalysisBatch.preprocess_device: median ms, frames/s | "
          "host SceneState, 16 threads: frames/s | mean peaks per frame")
    for ns, octaves, bpo, nf in CASES:
        n = octaves * bpo
        rng = P.VqtRange(55.0, octaves, bpo)
        d_db = torch.from_numpy(db_frames(ns, nf, n, ns + n)).to(dev)
        fields = {"center": torch.zeros((ns, nf, MAX_PEAKS), device=dev), "size": torch.zeros((ns, nf, MAX_PEAKS), device=dev),
                  "peak_count": torch.zeros((ns, nf), dtype=torch.int32, device=dev), "calmness": torch.zeros((ns, nf, n), device=dev),
                  "pitch_accuracy": torch.zeros((ns, nf, n), device=dev), "pitch_deviation": torch.zeros((ns, nf, n), device=dev),
                  "scene_calmness": torch.zeros((ns, nf), device=dev)}
        ab = P.AnalysisBatch(rng, ns)
        t_ab = timed(lambda: ab.preprocess_device(d_db, nf, DT, outputs=fields, max_peaks=MAX_PEAKS), a.settle, a.repeats)
        sb = P.SceneBatch(rng, ns)
        outs = {k: torch.empty(sb.output_shape(k, nf)[0], dtype=torch.int32 if sb.output_shape(k, nf)[1] == np.uint32 else torch.float32,
                               device=dev) for k in sb.OUTPUTS}
        t_sc = timed(lambda: sb.frames_device(fields, outs, frame_time=DT), a.settle, a.repeats)
        peaks = float(fields["peak_count"].float().mean())
        host = host_rate(rng, fields, n, nf, streams=min(ns, 64))
        rows = ns * nf
        print(f"{ns:5d} x {n} x {nf:3d} | {t_sc[0] * 1e3:8.3f} ms ({t_sc[1] * 1e3:.3f} .. {t_sc[2] * 1e3:.3f}), {rows / t_sc[0]:12.0f} /s | "
              f"{t_ab[0] * 1e3:8.3f} ms, {rows / t_ab[0]:12.0f} /s | {host:10.0f} /s | {peaks:.1f}", flush=True)


if __name__ == "__main__":
    main()
