#!/usr/bin/env python
"""What one optimisation step of the note trainer costs with its dense products in bf16 (NoteTrainer(precision="bf16")) beside the f32
step, for the trainer's model (252 bins, T = 5, mlp 1024, 2 hidden layers) at batches of 100, 300, 1024 and 4096.  The two handles run
alternating in one process: a round is STEPS consecutive steps of each, timed with HIP events, after a 300 ms settle load of each (as
scripts/note_model_half_rate.py); REPS rounds.  Reported per path: the median ms per step (min .. max) and the matrix work's rate;
for bf16 the f32 time over its own, median and spread of the per-round ratios; and per batch the per-kernel split of the bf16 step from
one `rocprofv3 --kernel-trace --stats` run of this script with --once (a child process; the program goes directly after `--`), with
nth_gemm's share of the 16-bit matrix peak (16 x the f32 matrix peak of 157.3 TFLOP/s) over its own kernel time.

Before anything is timed the two handles' EVAL losses on the batch are held together: they differ by the type's rounding only.

The gate this file confirms or refutes: at batches 300 and 1024 the bf16 step is faster than the f32 step of the same process by more
than the spread of the rounds (every round's ratio above 1).  No factor is promised: nt_conv_reduce, nt_bias_grad's row walk (nth_bias_grad
keeps it) and nt_adam are the f32 step's and bound what the step can gain.

usage: python scripts/note_trainer_half_rate.py [--out FILE] [--batches 100,300,1024,4096] [--no-trace]
       python scripts/note_trainer_half_rate.py --once --batches 300     (a few untimed bf16 steps and nothing else, for a kernel trace)
Needs a GPU; reads nothing outside the tree."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402

REPS, STEPS, SETTLE_S, ONCE_STEPS, PEAK16_FLOPS = 7, 20, 0.3, 10, 16 * 157.3e12
N_BINS, T, MLP, LAYERS, N_ROWS = 252, 5, 1024, 2, 20000
PATHS = ("f32", "bf16")


def make_weights(seed):
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


def settle(call):
    call()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + SETTLE_S
    while time.perf_counter() < t_end:
        call()
        torch.cuda.synchronize()


def round_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


def kernel_split(batch):
    """rocprofv3 --kernel-trace --stats over a child that runs a few bf16 steps -> [(kernel, calls per step, mean us, share)] of the nt_ / nth_ kernels"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--once", "--batches", str(batch)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, f"rocprofv3 exit {r.returncode}, {len(files)} stats files; last output: {r.stdout[-400:]!r}"
        rows = []
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                for prefix in ("nth_", "nt_"):
                    if prefix in name:
                        rows.append((name[name.index(prefix):].split("(")[0], int(row["Calls"]), float(row["TotalDurationNs"])))
                        break
        total = sum(r_[2] for r_ in rows) or 1.0
        return [(n, c / ONCE_STEPS, ns / c / 1e3, ns / total) for n, c, ns in sorted(rows, key=lambda r_: -r_[2])], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="100,300,1024,4096")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_trainer_half_rate.py needs a GPU"
    batches = [int(b) for b in args.batches.split(",")]
    w = make_weights(7)
    g = torch.Generator(device="cuda").manual_seed(3)
    d_db = 60.0 * torch.rand((N_ROWS, N_BINS), device="cuda", generator=g) ** 4
    d_tg = torch.rand((N_ROWS, 128), device="cuda", generator=g)
    rng = np.random.default_rng(5)
    params = P.NoteModelParams(N_BINS, T, MLP, LAYERS)
    lines = [f"# note trainer, {N_BINS} bins, T = {T}, mlp {MLP}, {LAYERS} hidden layers; dataset of {N_ROWS} rows on the device; f32 and bf16 handles alternating in one process,",
             f"# {REPS} rounds of {STEPS} consecutive PVQ_TRAIN_STEP each (HIP events) after a {SETTLE_S * 1e3:.0f} ms settle load of each; ms per step, median (min .. max)",
             "# vs f32: the f32 step's time over the bf16 step's, per round; median (min .. max)"]
    gate = []
    for batch in batches:
        idx = rng.integers(T - 1, N_ROWS, size=batch).astype(np.uint32)
        if args.once:
            tr = P.NoteTrainer(params, w, P.NoteTrainerHyper(seed=1), batch, precision="bf16")
            for _ in range(ONCE_STEPS):
                tr.step(d_db, d_tg, idx)
            torch.cuda.synchronize()
            continue
        trs = {p: P.NoteTrainer(params, w, P.NoteTrainerHyper(seed=1), batch, precision=p) for p in PATHS}
        calls = {p: (lambda p=p: trs[p].step(d_db, d_tg, idx)) for p in PATHS}
        d_loss = torch.zeros(1, device="cuda")
        loss = {}
        for p in PATHS:
            trs[p].step(d_db, d_tg, idx, "eval", d_loss=d_loss)
            loss[p] = float(d_loss)
        assert abs(loss["f32"] - loss["bf16"]) < 2e-3, f"the two handles disagree on the loss: {loss}"
        for p in PATHS:
            settle(calls[p])
        ms = {p: [] for p in PATHS}
        for _ in range(REPS):
            for p in PATHS:
                ms[p].append(round_ms(calls[p]))
        n_feat = trs["f32"].n_features
        flop = 6.0 * batch * (n_feat * MLP + LAYERS * MLP * MLP + 128 * MLP)
        lines.append(f"## batch {batch}: EVAL loss f32 {loss['f32']:.6f}, bf16 {loss['bf16']:.6f}; {flop / 1e9:.2f} GFLOP of matrix work per step (three products per layer)")
        for p in PATHS:
            med = float(np.median(ms[p]))
            line = f"{p:4s}: {med:8.3f} ms ({min(ms[p]):.3f} .. {max(ms[p]):.3f})  {flop / (med * 1e-3) / 1e12:7.2f} TFLOP/s  {batch / med * 1e-3:7.3f} M rows/s"
            if p == "bf16":
                ratio = [a / b for a, b in zip(ms["f32"], ms["bf16"])]
                line += f"  vs f32 {float(np.median(ratio)):.2f} ({min(ratio):.2f} .. {max(ratio):.2f})"
                gate.append((batch, float(np.median(ratio)), min(ratio)))
            lines.append(line)
        del trs, calls
        torch.cuda.empty_cache()
        if not args.no_trace:
            split, err = kernel_split(batch)
            if split is None:
                lines.append(f"  per-kernel split: not collected ({err})")
            else:
                lines.append("  per-kernel split of the bf16 step (rocprofv3 --kernel-trace --stats, one child run): kernel, launches per step, mean us, share of the step's kernel time")
                lines += [f"    {n:<24s} {c:5.1f}  {us:9.1f} us  {share * 100:5.1f} %" for n, c, us, share in split]
                gemm_us = sum(c * us for n, c, us, _ in split if n == "nth_gemm")
                if gemm_us > 0:
                    lines.append(f"  nth_gemm: {gemm_us:.1f} us per step for {flop / 1e9:.2f} GFLOP = {flop / (gemm_us * 1e-6) / 1e12:.1f} TFLOP/s = "
                                 f"{flop / (gemm_us * 1e-6) / PEAK16_FLOPS * 100:.1f} % of the 16-bit matrix peak ({PEAK16_FLOPS / 1e12:.1f} TFLOP/s)")
    if args.once:
        return
    for batch, med, lo in gate:
        if batch in (300, 1024):
            lines.append(f"# batch {batch}: the bf16 step is {med:.2f} x the f32 step's rate (least round {lo:.2f}): the gate (faster than f32 by more than the spread) is "
                         + ("MET" if lo > 1.0 else "MISSED"))
        else:
            lines.append(f"# batch {batch}: the bf16 step is {med:.2f} x the f32 step's rate (least round {lo:.2f}); " + ("it gains" if lo > 1.0 else "it does not gain"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
