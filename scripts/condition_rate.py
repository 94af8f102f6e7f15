#!/usr/bin/env python
"""What the many-streams conditioning (pvq_agc_batch_condition_device: cond_gate + cond_recurrence) costs beside the host's way of
doing the same job: pvq_train_condition_stream per stream on 16 host threads (one MonoAgc each, as rayon would have it) plus the upload
of the conditioned PCM.  64 / 256 / 1 024 / 4 096 stereo streams x 60 trainer chunks (train.rs:128-129: 1 984 samples at 22 050 Hz);
the device form timed with HIP events after a 300 ms settle load (as bench.py does), the host form with the host clock around work that
ends in a synchronise; median of 5 repetitions each.

usage: python scripts/condition_rate.py [--out FILE] [--streams 64,256,1024,4096] [--once]
       (--once: one untimed device call per size and nothing else, for a kernel trace)
Needs a GPU; reads nothing outside the tree."""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402

N_CHUNKS, THREADS, REPS, SETTLE_S = 60, 16, 5, 0.3
_fp = C.POINTER(C.c_float)


def stimuli(n, chunk):
    """n stereo streams: 64 seeded base streams (a tone, noise, a silent stretch in every fourth), scaled per stream"""
    m = N_CHUNKS * chunk
    rng = np.random.default_rng(1)
    t = np.arange(m) / 22050.0
    base = []
    for b in range(64):
        f = rng.uniform(100.0, 2000.0)
        left = (0.2 * np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(m)).astype(np.float32)
        right = (0.15 * np.sin(2 * np.pi * 1.5 * f * t) + 0.01 * rng.standard_normal(m)).astype(np.float32)
        if b % 4 == 0:
            left[20 * chunk:26 * chunk] = 0.0
            right[20 * chunk:26 * chunk] = 0.0
        base.append((left, right))
    left = np.empty((n, m), np.float32)
    right = np.empty((n, m), np.float32)
    for s in range(n):
        k = np.float32(0.5 + 0.01 * (s // 64))
        left[s] = base[s % 64][0] * k
        right[s] = base[s % 64][1] * k
    return left, right


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", default="64,256,1024,4096")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "condition_rate.py needs a GPU"
    L = _lib.load()
    q = 10.0   # train.rs:30-42
    vqt = P.Vqt.new(P.VqtParameters(sr=22050.0, n_fft=32768, range=P.VqtRange(55.0, 7, 36), sparsity_quantile=0.999, quality=q, gamma=5.3 * q), None)
    chunk = P.train_chunk_samples(vqt)
    sizes = [int(x) for x in args.streams.split(",")]
    lines = [f"# conditioning of n stereo streams x {N_CHUNKS} chunks of {chunk} samples, MonoAgc(0.07, 0.001); median of {REPS}, ms",
             f"# device: cond_gate + cond_recurrence (HIP events, after a {SETTLE_S * 1e3:.0f} ms settle load); host: pvq_train_condition_stream on {THREADS} threads"
             " + upload of the conditioned PCM (pinned source)",
             "# streams  device_ms  (min .. max)   host_condition_ms  host_upload_ms  host_total_ms  host/device  Msamples/s device"]
    crossover = None
    for n in sizes:
        left, right = stimuli(n, chunk)
        m = N_CHUNKS * chunk
        d_left, d_right = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        d_out = torch.empty_like(d_left)
        d_gain = torch.empty((n, N_CHUNKS), device="cuda")
        batch = P.AgcBatch(n, 0.07, 0.001)
        # the C call itself with tables built once: the events then see the call's own work, not Python filling 3 n pointers
        tab = lambda t: (C.c_void_p * n)(*[t[s].data_ptr() for s in range(n)])
        lefts, rights, outs, counts = tab(d_left), tab(d_right), tab(d_out), (C.c_size_t * n)(*[N_CHUNKS] * n)
        stream = torch.cuda.current_stream().cuda_stream

        def dev_call(b=batch):
            st = L.pvq_agc_batch_condition_device(b._h, lefts, rights, counts, chunk, outs, d_gain.data_ptr(), N_CHUNKS, stream)
            assert st == _lib.PVQ_OK, L.pvq_last_error()

        dev_call()
        torch.cuda.synchronize()
        if args.once:
            continue
        t_end = time.perf_counter() + SETTLE_S
        while time.perf_counter() < t_end:
            dev_call()
            torch.cuda.synchronize()
        dev = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dev_call()
            e1.record()
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1))
        # the parent's way: one MonoAgc and one pvq_train_condition_stream per stream on 16 threads (ctypes drops the GIL in the call),
        # then the conditioned PCM goes up
        pin = P.PinnedArray((n, m))
        mono = pin.array
        gains = np.empty((n, N_CHUNKS), np.float32)
        d_up = torch.empty((n, m), device="cuda")
        up_src = torch.from_numpy(mono)

        def host_stream(s):
            agc = P.MonoAgc(0.07, 0.001)
            st = L.pvq_train_condition_stream(agc._h, left[s].ctypes.data_as(_fp), right[s].ctypes.data_as(_fp), N_CHUNKS, chunk,
                                              mono[s].ctypes.data_as(_fp), gains[s].ctypes.data_as(_fp))
            assert st == _lib.PVQ_OK

        host_c, host_u = [], []
        with ThreadPoolExecutor(THREADS) as pool:
            list(pool.map(host_stream, range(n)))   # warm
            d_up.copy_(up_src)
            torch.cuda.synchronize()
            for _ in range(REPS):
                t0 = time.perf_counter()
                list(pool.map(host_stream, range(n)))
                t1 = time.perf_counter()
                d_up.copy_(up_src, non_blocking=True)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                host_c.append((t1 - t0) * 1e3)
                host_u.append((t2 - t1) * 1e3)
        # same job, same bits (fresh gains, like the host's fresh MonoAgc per stream)
        dev_call(P.AgcBatch(n, 0.07, 0.001))
        torch.cuda.synchronize()
        assert torch.equal(d_out.view(torch.int32), d_up.view(torch.int32)), "device and host conditioning differ"
        del up_src, mono, pin
        dm, hc, hu = float(np.median(dev)), float(np.median(host_c)), float(np.median(host_u))
        if crossover is None and dm < hc + hu:
            crossover = n
        lines.append(f"{n:9d}  {dm:9.3f}  ({min(dev):.3f} .. {max(dev):.3f})  {hc:17.3f}  {hu:14.3f}  {hc + hu:13.3f}  {(hc + hu) / dm:11.2f}"
                     f"  {n * m / dm * 1e-3:10.1f}")
    if not args.once:
        if crossover is None:
            lines.append("# the device form does not overtake the host form at any size measured")
        else:
            lines.append(f"# the device form is the faster one from {crossover} streams on (the smallest size measured where it is)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
