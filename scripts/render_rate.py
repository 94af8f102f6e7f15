#!/usr/bin/env python
"""What the batched render (pvq_render_batch_rows_device) costs: rows/s for all four outputs and for spectrogram_vqt alone at
4 096 streams x 512 frames, 252 and 588 bins, beside
  * the bytes per row the call must move, as a fraction of the HBM rate (8 TB/s nominal),
  * pvq_analysis_batch_preprocess_device's time for the same rows on the same box (every output written: the render reads what it wrote),
  * 16 host threads running pvq_spectrogram_row (both modes) + pvq_chroma_row + pvq_led_frame over rows downloaded from the same run
    (a sample of them: the host rate does not depend on how many).
Device calls are timed with HIP events after a 300 ms settle load of the same call (as bench.py does); median of 5.

The expectation this file confirms or refutes: the render moves well under half of preprocess's 8 KB per frame and carries no
recurrence, so it should cost less than preprocess does.

usage: python scripts/render_rate.py [--out FILE] [--streams 4096] [--frames 512] [--bins 252,588] [--once]
       (--once: one untimed render call per geometry and nothing else, for a kernel trace)
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
from pitchvis_amd import consumers as PC  # noqa: E402

THREADS, REPS, SETTLE_S, MAX_PEAKS, HOST_ROWS, HBM_BPS = 16, 5, 0.3, 32, 16384, 8.0e12
GEOMS = {252: (55.0, 7, 36), 588: (55.0, 7, 84)}
_fp, _bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


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
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--bins", default="252,588")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_rate.py needs a GPU"
    L = _lib.load()
    S, F = args.streams, args.frames
    rows = S * F
    lines = [f"# batched render of {S} streams x {F} frames = {rows} rows; median of {REPS} (min .. max), ms; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load",
             f"# bytes/row: what the call must read and write; of HBM: bytes/row x rows/s over {HBM_BPS / 1e12:.0f} TB/s",
             f"# host: {THREADS} threads, pvq_spectrogram_row x 2 + pvq_chroma_row + pvq_led_frame per row, measured on {HOST_ROWS} of the rows"]
    verdicts = []
    for n in [int(b) for b in args.bins.split(",")]:
        min_freq, octaves, bpo = GEOMS[n]
        rng = P.VqtRange(min_freq, octaves, bpo)
        g = torch.Generator(device="cuda").manual_seed(n)
        d_db = torch.rand((S, F, n), device="cuda", generator=g) * 6.0          # a noise floor ...
        tones = torch.zeros((S, 1, n), device="cuda")
        tones.scatter_(2, torch.randint(3, n - 3, (S, 1, 6), device="cuda", generator=g), 30.0)
        d_db += tones * (1.0 + 0.2 * torch.rand((S, F, 1), device="cuda", generator=g))   # ... and six held notes per stream
        del tones
        fields = {k: torch.zeros((S, F, n), device="cuda") for k in ("x_vqt_smoothed", "x_vqt_peakfiltered", "x_vqt_afterglow", "calmness",
                                                                     "pitch_accuracy", "pitch_deviation")}
        fields["peak_mask"] = torch.zeros((S, F, (n + 31) // 32), dtype=torch.int32, device="cuda")
        fields["peak_count"] = torch.zeros((S, F), dtype=torch.int32, device="cuda")
        fields["center"] = torch.zeros((S, F, MAX_PEAKS), device="cuda")
        fields["size"] = torch.zeros((S, F, MAX_PEAKS), device="cuda")
        fields["scene_calmness"] = torch.zeros((S, F), device="cuda")
        fields["tuning_grid_inaccuracy"] = torch.zeros((S, F), device="cuda")
        batch = P.AnalysisBatch(rng, S)
        pre = lambda: batch.preprocess_device(d_db, F, 256 / 48000.0, fields, max_peaks=MAX_PEAKS)
        r = P.RenderBatch(rng)
        outs = {name: torch.empty(r.output_shape(name, rows)[0], dtype=torch.uint8 if r.output_shape(name, rows)[1] == np.uint8 else torch.float32,
                                  device="cuda") for name in r.OUTPUTS}
        render_all = lambda: r.rows_device(fields, outs)
        render_vqt = lambda: r.rows_device(fields, {"spectrogram_vqt": outs["spectrogram_vqt"]})
        pre()
        torch.cuda.synchronize()
        if args.once:
            render_all()
            render_vqt()
            torch.cuda.synchronize()
            continue
        pre_ms = timed(pre)
        all_ms = timed(render_all)
        vqt_ms = timed(render_vqt)
        peaks_per_row = float(fields["peak_count"].float().mean())
        in_x, in_pk = 4 * n, 4 + 8 * peaks_per_row
        b_all = in_x + in_pk + 4 * n + 4 * n + 48 + 3 + 3 * n
        b_vqt = in_x + 4 * n
        b_pre = 4 * n + sum(t.element_size() * t.numel() for t in fields.values()) / rows
        # the host's way over the same rows
        m = min(HOST_ROWS, rows)
        x = fields["x_vqt_smoothed"].reshape(rows, n)[:m].cpu().numpy()
        cnt = fields["peak_count"].reshape(rows)[:m].cpu().numpy()
        ctr = fields["center"].reshape(rows, MAX_PEAKS)[:m].cpu().numpy()
        sz = fields["size"].reshape(rows, MAX_PEAKS)[:m].cpu().numpy()
        col = np.ascontiguousarray(PC.COLORS, np.float32)
        h_rgba = np.empty((2, m, n, 4), np.uint8)
        h_chroma = np.empty((m, 12), np.float32)
        h_led = np.empty((m, 3 + 3 * n), np.uint8)

        def host_rows(lo_hi):
            for i in range(*lo_hi):
                k = int(min(cnt[i], MAX_PEAKS))
                L.pvq_spectrogram_row(0, n, bpo, x[i].ctypes.data_as(_fp), None, None, 0, col.ctypes.data_as(_fp), PC.GRAY_LEVEL, PC.EASING_POW,
                                      h_rgba[0, i].ctypes.data_as(_bp))
                L.pvq_spectrogram_row(1, n, bpo, None, ctr[i].ctypes.data_as(_fp), sz[i].ctypes.data_as(_fp), k, col.ctypes.data_as(_fp),
                                      PC.GRAY_LEVEL, PC.EASING_POW, h_rgba[1, i].ctypes.data_as(_bp))
                L.pvq_chroma_row(min_freq, n, bpo, x[i].ctypes.data_as(_fp), h_chroma[i].ctypes.data_as(_fp))
                L.pvq_led_frame(n, bpo, ctr[i].ctypes.data_as(_fp), sz[i].ctypes.data_as(_fp), k, col.ctypes.data_as(_fp), PC.GRAY_LEVEL,
                                PC.EASING_POW, h_led[i].ctypes.data_as(_bp))

        step = (m + THREADS - 1) // THREADS
        parts = [(lo, min(m, lo + step)) for lo in range(0, m, step)]
        with ThreadPoolExecutor(THREADS) as pool:
            t0 = time.perf_counter()
            list(pool.map(host_rows, parts))
            host_s = time.perf_counter() - t0
        d = np.abs(outs["led"][:m].cpu().numpy().astype(int) - h_led.astype(int))
        assert d.max() <= 1, "device and host LED frames differ by more than a level"
        lines += [f"## {n} bins ({peaks_per_row:.1f} peaks per row)",
                  f"render, all four outputs : {all_ms[0]:8.3f} ms ({all_ms[1]:.3f} .. {all_ms[2]:.3f})  {rows / all_ms[0] * 1e-3:8.1f} M rows/s  {b_all:7.0f} bytes/row"
                  f"  {b_all * rows / (all_ms[0] * 1e-3) / HBM_BPS:.3f} of HBM",
                  f"render, spectrogram_vqt  : {vqt_ms[0]:8.3f} ms ({vqt_ms[1]:.3f} .. {vqt_ms[2]:.3f})  {rows / vqt_ms[0] * 1e-3:8.1f} M rows/s  {b_vqt:7.0f} bytes/row"
                  f"  {b_vqt * rows / (vqt_ms[0] * 1e-3) / HBM_BPS:.3f} of HBM",
                  f"preprocess, every output : {pre_ms[0]:8.3f} ms ({pre_ms[1]:.3f} .. {pre_ms[2]:.3f})  {rows / pre_ms[0] * 1e-3:8.1f} M rows/s  {b_pre:7.0f} bytes/row"
                  f"  {b_pre * rows / (pre_ms[0] * 1e-3) / HBM_BPS:.3f} of HBM",
                  f"host, {THREADS} threads         : {host_s * 1e3:8.1f} ms for {m} rows  {m / host_s * 1e-6:8.3f} M rows/s"
                  f"  (device, all outputs: {rows / all_ms[0] * 1e-3 / (m / host_s * 1e-6):.0f} x)"]
        verdicts.append((n, all_ms[0], pre_ms[0]))
        del fields, outs, d_db, batch, r
        torch.cuda.empty_cache()
    for n, a, p in verdicts:
        lines.append(f"# {n} bins: the render of all four outputs takes {a / p:.2f} of preprocess's time: the expectation (less than preprocess) is "
                     + ("CONFIRMED" if a < p else "REFUTED — see the kernel trace for where the time goes"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
