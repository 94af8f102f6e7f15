#!/usr/bin/env python
"""What the batched debug panels (pvq_panels_batch_rows_device, pvq_panels_batch_graph_device) cost: rows/s for all six row outputs
at 252 and 588 bins, 64 and 4 096 streams, and for the graph at capacity 300 with every frame emitted; beside each figure the time
of a plain hipMemsetAsync over the same number of output bytes in the same run — the yardstick of a stage bound by its stores (112
bytes written per segment against 4 to 8 read).  Device calls are timed with HIP events after a 300 ms settle load of the same call
(as bench.py does); median of 5.  No rate is fixed in advance.

usage: python scripts/panels_rate.py [--out FILE] [--streams 64,4096] [--frames 8] [--bins 252,588] [--once]
       (--once: one untimed call per configuration and nothing else, for a kernel trace)
Needs a GPU; reads nothing outside the tree."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402

REPS, SETTLE_S, MAX_PEAKS, CAPACITY, HBM_BPS = 5, 0.3, 32, 300, 8.0e12
GEOMS = {252: (55.0, 7, 36), 588: (55.0, 7, 84)}


def timed(call):
    call()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + SETTLE_S
    while time.perf_counter() < t_end:
        call()
        torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", default="64,4096")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--bins", default="252,588")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "panels_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    F = args.frames
    lines = [f"# batched debug panels, {F} frames per stream; median of {REPS} (min .. max), ms; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load",
             f"# memset: hipMemsetAsync over the same output bytes in the same run; of HBM: output bytes/s over {HBM_BPS / 1e12:.0f} TB/s",
             f"# rows: all six outputs, {MAX_PEAKS} peak slots per row; graph: capacity {CAPACITY}, every frame emitted"]

    def report(tag, rows, ms, set_ms, nbytes):
        return (f"{tag:34s}: {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e-3:8.3f} M rows/s  {nbytes / rows:7.0f} bytes/row"
                f"  {nbytes / (ms[0] * 1e-3) / HBM_BPS:.3f} of HBM | memset {set_ms[0]:8.3f} ms ({set_ms[1]:.3f} .. {set_ms[2]:.3f}): {ms[0] / set_ms[0]:.2f} x")

    for S in [int(s) for s in args.streams.split(",")]:
        rows = S * F
        stream = torch.cuda.current_stream().cuda_stream
        for n in [int(b) for b in args.bins.split(",")]:
            min_freq, octaves, bpo = GEOMS[n]
            g = torch.Generator(device="cuda").manual_seed(n + S)
            x = torch.rand((rows, n), device="cuda", generator=g) * 30.0
            calm = torch.rand((rows, n), device="cuda", generator=g)
            ctr = torch.rand((rows, MAX_PEAKS), device="cuda", generator=g) * (n - 0.01)
            sz = torch.rand((rows, MAX_PEAKS), device="cuda", generator=g) * 40.0
            cnt = torch.randint(0, MAX_PEAKS + 1, (rows,), device="cuda", generator=g, dtype=torch.int32)
            b = P.PanelsBatch(P.VqtRange(min_freq, octaves, bpo), S, graph_capacity=CAPACITY)
            outs = {name: torch.empty(b.output_shape(name, rows, MAX_PEAKS), device="cuda") for name in b.OUTPUTS}
            nbytes = sum(t.numel() * 4 for t in outs.values())
            call = lambda: b.rows_device(None, outs, x_vqt_smoothed=x, center=ctr, size=sz, peak_count=cnt, calmness=calm)

            def memset():
                for t in outs.values():
                    assert L.hipMemsetAsync(t.data_ptr(), 0, t.numel() * 4, stream) == 0
            if args.once:
                call()
                torch.cuda.synchronize()
            else:
                set_ms = timed(memset)
                ms = timed(call)
                lines.append(report(f"rows, {S} streams, {n} bins", rows, ms, set_ms, nbytes))
            del outs, x, calm, ctr, sz, cnt, b
            torch.cuda.empty_cache()
        b = P.PanelsBatch(P.VqtRange(*GEOMS[252]), S, graph_capacity=CAPACITY)
        vals = torch.rand((S, F), device="cuda")
        gouts = {name: torch.empty(b.output_shape(name, F), device="cuda") for name in b.GRAPH_OUTPUTS}
        nbytes = sum(t.numel() * 4 for t in gouts.values())
        call = lambda: b.graph_device(vals, gouts, first_emitted=0)

        def memset_g():
            for t in gouts.values():
                assert L.hipMemsetAsync(t.data_ptr(), 0, t.numel() * 4, stream) == 0
        if args.once:
            call()
            torch.cuda.synchronize()
        else:
            set_ms = timed(memset_g)
            ms = timed(call)
            lines.append(report(f"graph, {S} streams, capacity {CAPACITY}", rows, ms, set_ms, nbytes))
        del gouts, vals, b
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
