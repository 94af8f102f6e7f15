#!/usr/bin/env python
"""What the note model on the device (pvq_note_model_rows_device) costs: rows/s for the trainer's model (252 bins, T = 5 and T = 3,
mlp 1024, 2 hidden layers) at 4 096 and 65 536 rows, beside
  * the fraction of the f32 matrix peak (157.3 TFLOP/s) with F = 2 (n_features mlp + layers mlp^2 + 128 mlp) flop per row,
  * the time of each of its kernels (HIP events around calls of models cut short: conv + fc1 alone is a model whose hidden layers
    are left out, and so on; differences of medians),
  * the same model's eager torch f32 forward on the same device and rows (unfold of the same dB buffer -> conv1d -> relu ->
    max_pool1d -> linear ...), which writes the pooled activations to memory.
Device calls are timed with HIP events after a 300 ms settle load of the same call (as bench.py does); median of 5.

The aim this file confirms or refutes: at least level with eager torch, the margin being the spread of repeated runs.

usage: python scripts/note_model_rate.py [--out FILE] [--rows 4096,65536] [--once]
       (--once: one untimed call per configuration and nothing else, for a kernel trace)
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

REPS, SETTLE_S, PEAK_FLOPS = 5, 0.3, 157.3e12
N_BINS, MLP, LAYERS, FRAMES_PER_STREAM = 252, 1024, 2, 512


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


def make_weights(T, layers, seed):
    rng = np.random.default_rng(seed)
    n_feat = P.NoteModelParams(N_BINS, T, MLP, layers).sizes()[3]

    def u(shape, fan_in):
        return ((2.0 * rng.random(shape) - 1.0) / np.sqrt(fan_in)).astype(np.float32)
    w = {"conv1.weight": u((16, 1, 5), 5), "conv1.bias": u((16,), 5), "fc1.weight": u((MLP, n_feat), n_feat), "fc1.bias": u((MLP,), n_feat)}
    for i in range(layers):
        w[f"layers.{i}.weight"] = u((MLP, MLP), MLP)
        w[f"layers.{i}.bias"] = u((MLP,), MLP)
    w["output.weight"] = u((128, MLP), MLP)
    w["output.bias"] = u((128,), MLP)
    return w


def torch_forward(d, d_db, T):
    """eager f32: every window of every stream, as rows"""
    S, Fr, nb = d_db.shape
    x = d_db.reshape(S, Fr * nb).unfold(1, T * nb, nb).reshape(-1, 1, T * nb)   # [S * (Fr - T + 1)][1][L]
    h = F.max_pool1d(F.relu(F.conv1d(x, d["conv1.weight"], d["conv1.bias"], stride=2)), 2).flatten(1)
    h = F.relu(F.linear(h, d["fc1.weight"], d["fc1.bias"]))
    i = 0
    while f"layers.{i}.weight" in d:
        h = F.relu(F.linear(h, d[f"layers.{i}.weight"], d[f"layers.{i}.bias"]))
        i += 1
    return torch.sigmoid(F.linear(h, d["output.weight"], d["output.bias"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_model_rate.py needs a GPU"
    lines = [f"# note model, {N_BINS} bins, mlp {MLP}, {LAYERS} hidden layers; streams of {FRAMES_PER_STREAM} + T - 1 frames; median of {REPS} (min .. max), ms;"
             f" HIP events after a {SETTLE_S * 1e3:.0f} ms settle load",
             f"# of peak: F = 2 (n_features mlp + layers mlp^2 + 128 mlp) flop per row over {PEAK_FLOPS / 1e12:.1f} TFLOP/s (f32 matrix peak)",
             "# per kernel: differences of the medians of models cut short (fc1 only / + hidden layers / whole); the output layer's launch is in every one"]
    verdicts = []
    for T in (5, 3):
        for rows in [int(r) for r in args.rows.split(",")]:
            S = max(1, rows // FRAMES_PER_STREAM)
            per = rows // S
            Fr = per + T - 1
            w = make_weights(T, LAYERS, 7)
            n_feat = P.NoteModelParams(N_BINS, T, MLP, LAYERS).sizes()[3]
            flop = 2.0 * (n_feat * MLP + LAYERS * MLP * MLP + 128 * MLP)
            g = torch.Generator(device="cuda").manual_seed(T)
            d_db = 60.0 * torch.rand((S, Fr, N_BINS), device="cuda", generator=g) ** 4
            full = P.NoteModel(P.NoteModelParams(N_BINS, T, MLP, LAYERS), w)
            outs = {n: torch.empty(full.output_shape(n, S, Fr)[0], dtype=torch.float32 if n != "d_mask" else torch.int32, device="cuda")
                    for n in full.OUTPUTS}
            run = lambda: full.rows_device(d_db, None, Fr, outs)
            d = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
            ref = lambda: torch_forward(d, d_db, T)
            run()
            torch.cuda.synchronize()
            if args.once:
                continue
            # the same numbers from both, before any is timed
            want = ref().reshape(S, per, 128)
            got = outs["d_prob"][:, T - 1:]
            diff = float((want - got).abs().max())
            assert diff < 1e-5, f"device and eager torch disagree: {diff}"
            ms = timed(run)
            t_ms = timed(ref)
            w0 = {k: v for k, v in w.items() if not k.startswith("layers.")}
            cut0 = P.NoteModel(P.NoteModelParams(N_BINS, T, MLP, 0), w0)
            cut0_ms = timed(lambda: cut0.rows_device(d_db, None, Fr, outs))
            w1 = dict(w0, **{k: v for k, v in w.items() if k.startswith("layers.0.")})
            cut1 = P.NoteModel(P.NoteModelParams(N_BINS, T, MLP, 1), w1)
            cut1_ms = timed(lambda: cut1.rows_device(d_db, None, Fr, outs))
            out_flop, fc1_flop, hid_flop = 2.0 * 128 * MLP, 2.0 * n_feat * MLP, 2.0 * MLP * MLP
            hidden_ms = cut1_ms[0] - cut0_ms[0]
            lines += [f"## T = {T}, {S} streams x {per} rows = {S * per} rows, {n_feat} features, {flop / 1e6:.2f} MFLOP per row; max |p - p_torch| = {diff:.1e}",
                      f"pvq_note_model_rows_device : {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {S * per / ms[0] * 1e-3:7.3f} M rows/s  {flop * S * per / (ms[0] * 1e-3) / PEAK_FLOPS:.3f} of peak",
                      f"eager torch f32            : {t_ms[0]:8.3f} ms ({t_ms[1]:.3f} .. {t_ms[2]:.3f})  {S * per / t_ms[0] * 1e-3:7.3f} M rows/s  {flop * S * per / (t_ms[0] * 1e-3) / PEAK_FLOPS:.3f} of peak",
                      f"  nm_conv_fc1 + output layer + zero fill : {cut0_ms[0]:8.3f} ms  ({(fc1_flop + out_flop) * S * per / (cut0_ms[0] * 1e-3) / PEAK_FLOPS:.3f} of peak)",
                      f"  nm_dense<hidden>, each                 : {hidden_ms:8.3f} ms  ({hid_flop * S * per / (max(hidden_ms, 1e-6) * 1e-3) / PEAK_FLOPS:.3f} of peak)"]
            verdicts.append((T, S * per, ms, t_ms))
            del full, cut0, cut1, d, outs, d_db
            torch.cuda.empty_cache()
    for T, rows, ms, t_ms in verdicts:
        level = ms[0] <= t_ms[0] or ms[1] <= t_ms[2]   # inside the spread of repeated runs
        lines.append(f"# T = {T}, {rows} rows: {ms[0] / t_ms[0]:.2f} of eager torch's time: the aim (at least level with eager torch) is "
                     + ("MET" if level else "MISSED — see the per-kernel split above"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
