#!/usr/bin/env python
"""What one optimisation step of the note trainer (pvq_note_trainer_step, PVQ_TRAIN_STEP) costs for the trainer's model (252 bins,
T = 5, mlp 1024, 2 hidden layers: 7.3 M parameters) at batches of 300 (train.py's), 100 and 1024, beside
  * the same model's eager torch f32 step on the same device (train.py:153-158 on device tensors: gather the windows, forward in
    training mode, BCELoss, backward, optim.Adam with weight decay),
  * the per-kernel split of the step at each batch, from one `rocprofv3 --kernel-trace --stats` run of this script with --once
    (a child process; the program goes directly after `--`).
Steps are timed with HIP events around a run of STEPS consecutive steps after a 300 ms settle load of the same call; median of 5 runs.
No ratio is fixed in advance: the file records what was measured, and where the step is slower than torch's it names the kernel
with the largest share.

usage: python scripts/note_trainer_rate.py [--out FILE] [--batches 300,100,1024] [--no-trace]
       python scripts/note_trainer_rate.py --once --batches 300     (a few untimed steps and nothing else, for a kernel trace)
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
import torch.nn.functional as F  # noqa: E402

import pitchvis_amd as P  # noqa: E402

REPS, STEPS, SETTLE_S = 5, 20, 0.3
N_BINS, T, MLP, LAYERS, N_ROWS = 252, 5, 1024, 2, 20000


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


def timed(call):
    """ms per call: HIP events around STEPS calls, after a settle load; (median, min, max) of REPS"""
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
        for _ in range(STEPS):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / STEPS)
    return float(np.median(ms)), min(ms), max(ms)


class TorchTrainer:
    """train.py:67-99,141-158 on device tensors"""

    def __init__(self, w, d_db, d_tg):
        self.p = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in w.items()}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=1e-5, eps=float(np.finfo(np.float32).eps), weight_decay=5e-4)
        self.windows = d_db.reshape(-1).unfold(0, T * N_BINS, N_BINS)     # window j ends at row j + T - 1 (a view)
        self.d_tg = d_tg
        self.loss = torch.nn.BCELoss()

    def step(self, d_idx):
        p = self.p
        x = self.windows[d_idx - (T - 1)]
        y = self.d_tg[d_idx]
        self.opt.zero_grad()
        h = F.max_pool1d(F.relu(F.conv1d(x.unsqueeze(1), p["conv1.weight"], p["conv1.bias"], stride=2)), 2).flatten(1)
        h = F.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
        for i in range(LAYERS):
            h = F.dropout(F.relu(F.linear(h, p[f"layers.{i}.weight"], p[f"layers.{i}.bias"])), 0.1, True)
        loss = self.loss(torch.sigmoid(F.linear(h, p["output.weight"], p["output.bias"])), y)
        loss.backward()
        self.opt.step()
        return loss


def kernel_split(batch):
    """rocprofv3 --kernel-trace --stats over a child that runs a few steps -> [(kernel, calls per step, mean us, share)] of the nt_ kernels"""
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
                if "nt_" in name:
                    short = name[name.index("nt_"):].split("(")[0]
                    rows.append((short, int(row["Calls"]), float(row["TotalDurationNs"])))
        total = sum(r_[2] for r_ in rows) or 1.0
        return [(n, c / ONCE_STEPS, ns / c / 1e3, ns / total) for n, c, ns in sorted(rows, key=lambda r_: -r_[2])], None


ONCE_STEPS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="300,100,1024")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_trainer_rate.py needs a GPU"
    batches = [int(b) for b in args.batches.split(",")]
    w = make_weights(7)
    g = torch.Generator(device="cuda").manual_seed(3)
    d_db = 60.0 * torch.rand((N_ROWS, N_BINS), device="cuda", generator=g) ** 4
    d_tg = torch.rand((N_ROWS, 128), device="cuda", generator=g)
    rng = np.random.default_rng(5)
    n_params = sum(v.size for v in w.values())
    lines = [f"# note trainer, {N_BINS} bins, T = {T}, mlp {MLP}, {LAYERS} hidden layers, {n_params} parameters; dataset of {N_ROWS} rows on the device;",
             f"# ms per PVQ_TRAIN_STEP: HIP events around {STEPS} consecutive steps after a {SETTLE_S * 1e3:.0f} ms settle load; median of {REPS} (min .. max)",
             "# eager torch f32: gather, forward (training mode), BCELoss, backward, optim.Adam(weight_decay) on the same device"]
    for batch in batches:
        idx = rng.integers(T - 1, N_ROWS, size=batch).astype(np.uint32)
        tr = P.NoteTrainer(P.NoteModelParams(N_BINS, T, MLP, LAYERS), w, P.NoteTrainerHyper(seed=1), batch)
        run = lambda: tr.step(d_db, d_tg, idx)
        if args.once:
            for _ in range(ONCE_STEPS):
                run()
            torch.cuda.synchronize()
            continue
        # the same loss from both before either is timed (EVAL: no dropout; torch in eval form)
        d_loss = torch.zeros(1, device="cuda")
        tr.step(d_db, d_tg, idx, "eval", d_loss=d_loss)
        tt = TorchTrainer(w, d_db, d_tg)
        d_idx = torch.from_numpy(idx.astype(np.int64)).cuda()
        with torch.no_grad():
            p = tt.p
            x = tt.windows[d_idx - (T - 1)]
            h = F.max_pool1d(F.relu(F.conv1d(x.unsqueeze(1), p["conv1.weight"], p["conv1.bias"], stride=2)), 2).flatten(1)
            h = F.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
            for i in range(LAYERS):
                h = F.relu(F.linear(h, p[f"layers.{i}.weight"], p[f"layers.{i}.bias"]))
            want = float(tt.loss(torch.sigmoid(F.linear(h, p["output.weight"], p["output.bias"])), d_tg[d_idx]))
        got = float(d_loss)
        assert abs(got - want) < 1e-5, f"device and eager torch disagree on the loss: {got} vs {want}"
        ms = timed(run)
        t_ms = timed(lambda: tt.step(d_idx))
        flop = 6.0 * batch * (tr.n_features * MLP + LAYERS * MLP * MLP + 128 * MLP)
        lines += [f"## batch {batch}: EVAL loss {got:.6f} (torch {want:.6f}); {flop / 1e9:.2f} GFLOP of matrix work per step (three products per layer)",
                  f"pvq_note_trainer_step : {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {flop / (ms[0] * 1e-3) / 1e12:6.2f} TFLOP/s  {batch / ms[0] * 1e-3:7.3f} M rows/s",
                  f"eager torch f32       : {t_ms[0]:8.3f} ms ({t_ms[1]:.3f} .. {t_ms[2]:.3f})  {flop / (t_ms[0] * 1e-3) / 1e12:6.2f} TFLOP/s  {batch / t_ms[0] * 1e-3:7.3f} M rows/s",
                  f"ratio                 : {ms[0] / t_ms[0]:.2f} of eager torch's time"]
        del tr, tt
        torch.cuda.empty_cache()
        if not args.no_trace:
            split, err = kernel_split(batch)
            if split is None:
                lines.append(f"  per-kernel split: not collected ({err})")
            else:
                lines.append("  per-kernel split (rocprofv3 --kernel-trace --stats, one child run): kernel, launches per step, mean us, share of the step's kernel time")
                lines += [f"    {n:<24s} {c:5.1f}  {us:9.1f} us  {share * 100:5.1f} %" for n, c, us, share in split]
                if ms[0] > t_ms[0]:
                    lines.append(f"  slower than eager torch at this batch; the largest share is {split[0][0]}")
    if args.once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
