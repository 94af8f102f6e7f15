#!/usr/bin/env python
"""What the note model costs on the 16-bit matrix instructions (NoteModel(precision="bf16" / "f16")) beside the f32 path: the trainer's
model (252 bins, mlp 1024, 2 hidden layers) at T = 5 and T = 3, 4 096 and 65 536 rows.  The three paths run alternating in one
process: a round is one timed call of each (HIP events), after a 300 ms settle load of each (as scripts/note_model_rate.py); REPS
rounds.  Reported per path: the median time (min .. max), rows/s, and the share of the 16-bit matrix peak (16 x the f32 matrix
peak of 157.3 TFLOP/s: eight times the multiply-adds in half the cycles) with F = 2 (n_features mlp + layers mlp^2 + 128 mlp) flop
per row; per 16-bit path the ratio to the f32 path's time, median and spread of the per-round ratios.

Before anything is timed the 16-bit logits are held against the f32 path's on the same inputs under bar (a) of
tests/test_note_model_half_gpu.py: over the first rows of stream 0, max |16-bit - f32 path| <= 1.5 max |Q64 - L64|, Q64 and L64 the
float64 model with and without the rule's rounding points (include/pvq.h), computed here on the device in float64.

The gate this file confirms or refutes: at 65 536 rows each 16-bit path is faster than the f32 path by more than the spread (every
round's ratio above 1).

usage: python scripts/note_model_half_rate.py [--out FILE] [--rows 4096,65536] [--once]
       (--once: one untimed call per configuration and path and nothing else, for a kernel trace)
Needs a GPU; reads nothing outside the tree."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import pitchvis_amd as P  # noqa: E402

REPS, SETTLE_S, PEAK16_FLOPS = 7, 0.3, 16 * 157.3e12
N_BINS, MLP, LAYERS, FRAMES_PER_STREAM, CHECK_ROWS = 252, 1024, 2, 512, 256
PATHS = ("f32", "bf16", "f16")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def make_weights(T, seed):
    rng = np.random.default_rng(seed)
    n_feat = P.NoteModelParams(N_BINS, T, MLP, LAYERS).sizes()[3]

    def u(shape, fan_in):
        return ((2.0 * rng.random(shape) - 1.0) / np.sqrt(fan_in)).astype(np.float32)
    w = {"conv1.weight": u((16, 1, 5), 5), "conv1.bias": u((16,), 5), "fc1.weight": u((MLP, n_feat), n_feat), "fc1.bias": u((MLP,), n_feat)}
    for i in range(LAYERS):
        w[f"layers.{i}.weight"] = u((MLP, MLP), MLP)
        w[f"layers.{i}.bias"] = u((MLP,), MLP)
    w["output.weight"] = u((128, MLP), MLP)
    w["output.bias"] = u((128,), MLP)
    return w


def logits64(d, windows, dt):
    """float64 logits of windows [rows][L]; dt: the type every feature, dense weight and hidden activation is cast to once, or None"""
    q = (lambda x: x.to(dt).double()) if dt is not None else (lambda x: x.double())
    h = F.conv1d(windows.double().unsqueeze(1), d["conv1.weight"].double(), d["conv1.bias"].double(), stride=2)
    h = q(F.max_pool1d(F.relu(h), 2).flatten(1))
    h = q(F.relu(F.linear(h, q(d["fc1.weight"]), d["fc1.bias"].double())))
    for i in range(LAYERS):
        h = q(F.relu(F.linear(h, q(d[f"layers.{i}.weight"]), d[f"layers.{i}.bias"].double())))
    return F.linear(h, q(d["output.weight"]), d["output.bias"].double())


def settle(call):
    call()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + SETTLE_S
    while time.perf_counter() < t_end:
        call()
        torch.cuda.synchronize()


def once_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_model_half_rate.py needs a GPU"
    lines = [f"# note model, {N_BINS} bins, mlp {MLP}, {LAYERS} hidden layers; streams of {FRAMES_PER_STREAM} + T - 1 frames; f32, bf16, f16 alternating in one process,",
             f"# {REPS} rounds of one timed call each (HIP events) after a {SETTLE_S * 1e3:.0f} ms settle load of each; median (min .. max), ms",
             f"# of peak: F = 2 (n_features mlp + layers mlp^2 + 128 mlp) flop per row over {PEAK16_FLOPS / 1e12:.1f} TFLOP/s (the 16-bit matrix peak; the f32 path's own peak is 1/16 of it)",
             "# vs f32: the f32 path's time over this path's, per round; median (min .. max)"]
    gate = []
    for T in (5, 3):
        for rows in [int(r) for r in args.rows.split(",")]:
            S = max(1, rows // FRAMES_PER_STREAM)
            per = rows // S
            Fr = per + T - 1
            w = make_weights(T, 7)
            n_feat = P.NoteModelParams(N_BINS, T, MLP, LAYERS).sizes()[3]
            flop = 2.0 * (n_feat * MLP + LAYERS * MLP * MLP + 128 * MLP)
            g = torch.Generator(device="cuda").manual_seed(T)
            d_db = 60.0 * torch.rand((S, Fr, N_BINS), device="cuda", generator=g) ** 4
            models = {p: P.NoteModel(P.NoteModelParams(N_BINS, T, MLP, LAYERS), w, precision=p) for p in PATHS}
            outs = {p: {n: torch.empty(models[p].output_shape(n, S, Fr)[0], dtype=torch.float32 if n != "d_mask" else torch.int32, device="cuda")
                        for n in models[p].OUTPUTS} for p in PATHS}
            calls = {p: (lambda p=p: models[p].rows_device(d_db, None, Fr, outs[p])) for p in PATHS}
            for p in PATHS:
                calls[p]()
            torch.cuda.synchronize()
            if args.once:
                continue
            # bar (a) against the f32 path, on the first rows of stream 0, before any is timed
            n_chk = min(CHECK_ROWS, per)
            d = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
            win = d_db[0].reshape(-1).unfold(0, T * N_BINS, N_BINS)[:n_chk]
            l64 = logits64(d, win, None)
            f32_lg = outs["f32"]["d_logits"][0, T - 1:T - 1 + n_chk].double()
            checks = []
            for p in PATHS[1:]:
                quant = float((logits64(d, win, DTYPES[p]) - l64).abs().max())
                dev = float((outs[p]["d_logits"][0, T - 1:T - 1 + n_chk].double() - f32_lg).abs().max())
                assert dev <= 1.5 * quant, f"{p} and the f32 path disagree: {dev} against 1.5 x {quant}"
                checks.append(f"{p} {dev / quant:.3f}")
            del d, win, l64
            for p in PATHS:
                settle(calls[p])
            ms = {p: [] for p in PATHS}
            for _ in range(REPS):
                for p in PATHS:
                    ms[p].append(once_ms(calls[p]))
            n = S * per
            lines.append(f"## T = {T}, {S} streams x {per} rows = {n} rows, {n_feat} features, {flop / 1e6:.2f} MFLOP per row; max |16-bit - f32 path| over max |Q64 - L64|, {n_chk} rows: "
                         + ", ".join(checks) + " (bar 1.5)")
            for p in PATHS:
                med = float(np.median(ms[p]))
                line = f"{p:4s}: {med:8.3f} ms ({min(ms[p]):.3f} .. {max(ms[p]):.3f})  {n / med * 1e-3:8.3f} M rows/s  {flop * n / (med * 1e-3) / PEAK16_FLOPS:.3f} of peak"
                if p != "f32":
                    ratio = [a / b for a, b in zip(ms["f32"], ms[p])]
                    line += f"  vs f32 {float(np.median(ratio)):.2f} ({min(ratio):.2f} .. {max(ratio):.2f})"
                    if rows >= 65536:
                        gate.append((T, n, p, float(np.median(ratio)), min(ratio)))
                lines.append(line)
            del models, outs, calls, d_db
            torch.cuda.empty_cache()
    for T, n, p, med, lo in gate:
        lines.append(f"# T = {T}, {n} rows, {p}: {med:.2f} x the f32 path (least round {lo:.2f}): the gate (faster than f32 by more than the spread) is "
                     + ("MET" if lo > 1.0 else "MISSED"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
