#!/usr/bin/env python
"""What the test pass of the note trainer (pvq_note_trainer_test; train.py:164-198) costs for the trainer's model (252 bins, T = 5, mlp
1024, 2 hidden layers) over 69 322 test indices in batches of 100, on handles of max_batch 300 and 4096, beside
  (a) a loop of step(mode="eval", d_logits=...) per batch of 100 with the logits read back and counted on the host: what the library
      offered before the pass existed,
  (b) eager torch f32 in eval form on the same device, per batch of 100, with the counting done in torch (no sklearn, one read-back at
      the end),
and the per-kernel split of the pass, from one `rocprofv3 --kernel-trace --stats` run of this script with --once per max_batch (a
child process; the program goes directly after `--`).
A pass is synchronous, so it is timed with the host clock around PASSES consecutive passes after a settle load of the same call; median
of REPS.  No figure is fixed in advance.  The aim: the pass at max_batch 4096 is faster than (a) and no slower than (b); the file says
whether it was met.

usage: python scripts/note_test_rate.py [--out FILE] [--no-trace]
       python scripts/note_test_rate.py --once --max-batch 4096     (a few untimed passes and nothing else, for a kernel trace)
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

REPS, PASSES, SETTLE_S, ONCE_PASSES = 5, 2, 0.3, 3
N_BINS, T, MLP, LAYERS = 252, 5, 1024, 2
N_TEST, BATCH = 69322, 100
N_ROWS = 5 * N_TEST + T       # train.py's split: a fifth of the samples is the test set


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
    """ms per call of a synchronous call: the host clock around PASSES calls, after a settle load; (median, min, max) of REPS"""
    call()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + SETTLE_S
    while time.perf_counter() < t_end:
        call()
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(PASSES):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / PASSES)
    return float(np.median(ms)), min(ms), max(ms)


def f1_of(tp, fp, fn):
    den = 2.0 * tp + fp + fn
    return 2.0 * tp / den if den > 0 else 0.0


def step_loop(tr, d_db, d_tg, tg_host, idx):
    """(a): step(mode="eval") per batch, the logits over PCIe, the counting on the host -> (mean F1, accuracy)"""
    d_logits = torch.empty((BATCH, 128), device="cuda")
    f1s, correct, total = [], 0, 0
    for b in P.epoch(idx, BATCH):
        tr.step(d_db, d_tg, b, "eval", d_logits=d_logits)
        z = d_logits[:b.size].cpu().numpy()
        pred, lab = z > 0, tg_host[b.astype(np.int64)] > 0.5
        tp, fp, fn = int((pred & lab).sum()), int((pred & ~lab).sum()), int((~pred & lab).sum())
        f1s.append(f1_of(tp, fp, fn))
        correct += int((pred == lab).sum())
        total += pred.size
    return float(np.mean(f1s)), correct / total


class TorchModel:
    """train.py:67-99 in eval form on device tensors, and train.py:171-198 with the counting in torch"""

    def __init__(self, w, d_db, d_tg):
        self.p = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
        self.windows = d_db.reshape(-1).unfold(0, T * N_BINS, N_BINS)     # window j ends at row j + T - 1 (a view)
        self.d_tg = d_tg

    @torch.no_grad()
    def test(self, d_idx):
        p = self.p
        f1_sum = torch.zeros((), device="cuda", dtype=torch.float64)
        correct = torch.zeros((), device="cuda", dtype=torch.int64)
        n_batches = 0
        for at in range(0, d_idx.numel(), BATCH):
            ix = d_idx[at:at + BATCH]
            x, y = self.windows[ix - (T - 1)], self.d_tg[ix]
            h = F.max_pool1d(F.relu(F.conv1d(x.unsqueeze(1), p["conv1.weight"], p["conv1.bias"], stride=2)), 2).flatten(1)
            h = F.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
            for i in range(LAYERS):
                h = F.relu(F.linear(h, p[f"layers.{i}.weight"], p[f"layers.{i}.bias"]))
            pred = torch.sigmoid(F.linear(h, p["output.weight"], p["output.bias"])) > 0.5
            lab = y > 0.5
            tp = (pred & lab).sum()
            den = pred.sum() + lab.sum()          # 2 tp + fp + fn
            f1_sum += 2.0 * tp.double() / den.clamp(min=1).double()      # (0 when den is 0: tp is 0 then)
            correct += (pred == lab).sum()
            n_batches += 1
        return float(f1_sum) / n_batches, int(correct) / (128.0 * d_idx.numel())


def kernel_split(max_batch):
    """rocprofv3 --kernel-trace --stats over a child that runs a few passes -> [(kernel, launches per pass, mean us, share)] of the nt_ kernels"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--once", "--max-batch", str(max_batch)]
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
        return [(n, c / ONCE_PASSES, ns / c / 1e3, ns / total, ns / ONCE_PASSES / 1e6) for n, c, ns in sorted(rows, key=lambda r_: -r_[2])], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--max-batch", type=int, default=4096)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_test_rate.py needs a GPU"
    w = make_weights(7)
    g = torch.Generator(device="cuda").manual_seed(3)
    d_db = 60.0 * torch.rand((N_ROWS, N_BINS), device="cuda", generator=g) ** 4
    d_tg = torch.rand((N_ROWS, 128), device="cuda", generator=g)
    idx = P.random_split(N_ROWS, T, 0.8, seed=5)[1][:N_TEST]
    assert idx.size == N_TEST
    params = P.NoteModelParams(N_BINS, T, MLP, LAYERS)
    if args.once:
        tr = P.NoteTrainer(params, w, P.NoteTrainerHyper(seed=1), args.max_batch)
        for _ in range(ONCE_PASSES):
            tr.test(d_db, d_tg, idx, BATCH)
        return
    tg_host = d_tg.cpu().numpy()
    d_idx = torch.from_numpy(idx.astype(np.int64)).cuda()
    tm = TorchModel(w, d_db, d_tg)
    f1_t, acc_t = tm.test(d_idx)
    t_ms = timed(lambda: tm.test(d_idx))
    lines = [f"# note trainer test pass, {N_BINS} bins, T = {T}, mlp {MLP}, {LAYERS} hidden layers; {N_TEST} test indices of a dataset of {N_ROWS} rows on the device,",
             f"# metric batch {BATCH} ({-(-N_TEST // BATCH)} batches); ms per pass: host clock around {PASSES} consecutive synchronous passes after a "
             f"{SETTLE_S * 1e3:.0f} ms settle load; median of {REPS} (min .. max)",
             f"(b) eager torch f32, eval, counting in torch   : {t_ms[0]:9.3f} ms ({t_ms[1]:.3f} .. {t_ms[2]:.3f})   mean F1 {f1_t:.6f}  accuracy {acc_t:.6f}"]
    results = {}
    for max_batch in (300, 4096):
        tr = P.NoteTrainer(params, w, P.NoteTrainerHyper(seed=1), max_batch)
        res = tr.test(d_db, d_tg, idx, BATCH)
        ms = timed(lambda: tr.test(d_db, d_tg, idx, BATCH))
        results[max_batch] = ms
        lines.append(f"pvq_note_trainer_test, max_batch {max_batch:4d}          : {ms[0]:9.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})   mean F1 {res.mean_f1:.6f}  accuracy "
                     f"{res.accuracy:.6f}  mean loss {res.mean_loss:.6f}  {N_TEST / ms[0] * 1e-3:.2f} M rows/s")
        if max_batch == 300:
            f1_a, acc_a = step_loop(tr, d_db, d_tg, tg_host, idx)
            a_ms = timed(lambda: step_loop(tr, d_db, d_tg, tg_host, idx))
            lines.append(f"(a) step(eval) per batch of {BATCH}, host counting   : {a_ms[0]:9.3f} ms ({a_ms[1]:.3f} .. {a_ms[2]:.3f})   mean F1 {f1_a:.6f}  accuracy {acc_a:.6f}")
        # the three count the same thing: decisions may differ only where an f32 logit is within rounding of 0
        assert abs(res.accuracy - acc_t) < 1e-4 and abs(res.mean_f1 - f1_t) < 1e-4, (res.accuracy, acc_t, res.mean_f1, f1_t)
        del tr
        torch.cuda.empty_cache()
    ms = results[4096][0]
    met = ms < a_ms[0] and ms <= t_ms[0]
    lines.append(f"the pass at max_batch 4096 takes {ms / a_ms[0]:.3f} of (a)'s time and {ms / t_ms[0]:.3f} of (b)'s: the aim (faster than (a), no slower than (b)) is "
                 f"{'met' if met else 'MISSED'}")
    if not args.no_trace:
        for max_batch in (300, 4096):
            split, err = kernel_split(max_batch)
            if split is None:
                lines.append(f"per-kernel split at max_batch {max_batch}: not collected ({err})")
            else:
                lines.append(f"per-kernel split at max_batch {max_batch} (rocprofv3 --kernel-trace --stats, one child run): kernel, launches per pass, mean us, "
                             "share of the pass's kernel time, ms per pass")
                lines += [f"    {n:<24s} {c:7.1f}  {us:9.1f} us  {share * 100:5.1f} %  {tot:8.3f} ms" for n, c, us, share, tot in split]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
