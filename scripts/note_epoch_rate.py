#!/usr/bin/env python
"""What one epoch of the note trainer (pvq_note_trainer_epoch; train.py:147-162) costs for the trainer's model (252 bins, T = 5, mlp
1024, 2 hidden layers) over 20 000 train indices at batches of 100 and 300, in f32 and bf16, on a handle of max_batch 300, beside the
Python loop of `step` over idx[epoch_order(...)] on the same commit, which is what the caller wrote before the epoch existed:
  (a) with the loss read after every step (train.py:157, running_loss += loss.item()),
  (b) with every loss left in a slot of a device array and one read at the end.
An epoch and both loops end synchronised, so they are timed with the host clock around PASSES consecutive epochs after a settle load of
the same call; median of REPS.  Every timed epoch trains on: the weights move, the work per step does not.  No figure is fixed in
advance.  The expectation: the epoch is no slower than either loop; the file says whether it was met.  The script also checks that
the three give the same losses, bit for bit, from equal handles.

usage: python scripts/note_epoch_rate.py [--out FILE]
Needs a GPU; reads nothing outside the tree."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402

REPS, PASSES, SETTLE_S = 5, 2, 0.3
N_BINS, T, MLP, LAYERS = 252, 5, 1024, 2
N_TRAIN, MAX_BATCH = 20000, 300
N_ROWS = N_TRAIN * 5 // 4 + T


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


def loop_item(tr, d_db, d_tg, idx, batch, epoch, d_loss):
    """(a)"""
    seq = idx[P.epoch_order(0, epoch, idx.size).astype(np.int64)]
    losses = []
    for b in P.epoch(seq, batch):
        tr.step(d_db, d_tg, b, d_loss=d_loss)
        losses.append(d_loss.item())
    return np.array(losses, np.float32)


def loop_slots(tr, d_db, d_tg, idx, batch, epoch, d_losses):
    """(b)"""
    seq = idx[P.epoch_order(0, epoch, idx.size).astype(np.int64)]
    for k, b in enumerate(P.epoch(seq, batch)):
        tr.step(d_db, d_tg, b, d_loss=d_losses[k:k + 1])
    return d_losses[:-(-idx.size // batch)].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_epoch_rate.py needs a GPU"
    w = make_weights(7)
    g = torch.Generator(device="cuda").manual_seed(3)
    d_db = 60.0 * torch.rand((N_ROWS, N_BINS), device="cuda", generator=g) ** 4
    d_tg = torch.rand((N_ROWS, 128), device="cuda", generator=g)
    idx = P.random_split(N_ROWS, T, 0.8, seed=5)[0][:N_TRAIN]
    assert idx.size == N_TRAIN
    params = P.NoteModelParams(N_BINS, T, MLP, LAYERS)
    d_loss = torch.zeros(1, device="cuda")
    d_losses = torch.zeros(N_TRAIN, device="cuda")
    lines = [f"# note trainer epoch, {N_BINS} bins, T = {T}, mlp {MLP}, {LAYERS} hidden layers; {N_TRAIN} train indices of a dataset of {N_ROWS} rows on the device,",
             f"# max_batch {MAX_BATCH}; ms per epoch: host clock around {PASSES} consecutive synchronous epochs after a {SETTLE_S * 1e3:.0f} ms settle load; "
             f"median of {REPS} (min .. max)"]
    met = True
    for precision in ("f32", "bf16"):
        for batch in (100, 300):
            n_batches = -(-N_TRAIN // batch)
            trs = [P.NoteTrainer(params, w, P.NoteTrainerHyper(seed=1), MAX_BATCH, precision=precision) for _ in range(3)]
            first = [trs[0].epoch(d_db, d_tg, idx, batch, 0, 0)[0], loop_item(trs[1], d_db, d_tg, idx, batch, 0, d_loss),
                     loop_slots(trs[2], d_db, d_tg, idx, batch, 0, d_losses)]
            assert all(np.array_equal(first[0].view(np.uint32), f.view(np.uint32)) for f in first[1:]), "the epoch and the loops disagree"
            e_ms = timed(lambda: trs[0].epoch(d_db, d_tg, idx, batch, 0, 1))
            a_ms = timed(lambda: loop_item(trs[1], d_db, d_tg, idx, batch, 1, d_loss))
            b_ms = timed(lambda: loop_slots(trs[2], d_db, d_tg, idx, batch, 1, d_losses))
            met = met and e_ms[0] <= min(a_ms[0], b_ms[0])
            lines += [f"{precision:>4s}, batch {batch} ({n_batches} steps): pvq_note_trainer_epoch          : {e_ms[0]:9.3f} ms ({e_ms[1]:.3f} .. {e_ms[2]:.3f})   "
                      f"{e_ms[0] / n_batches * 1e3:7.1f} us per step",
                      f"{'':>4s}  {'':{len(str(batch)) + len(str(n_batches)) + 15}s} (a) step loop, loss.item() per step : {a_ms[0]:9.3f} ms ({a_ms[1]:.3f} .. {a_ms[2]:.3f})   "
                      f"{a_ms[0] / n_batches * 1e3:7.1f} us per step   epoch / (a) {e_ms[0] / a_ms[0]:.3f}",
                      f"{'':>4s}  {'':{len(str(batch)) + len(str(n_batches)) + 15}s} (b) step loop, one read at the end  : {b_ms[0]:9.3f} ms ({b_ms[1]:.3f} .. {b_ms[2]:.3f})   "
                      f"{b_ms[0] / n_batches * 1e3:7.1f} us per step   epoch / (b) {e_ms[0] / b_ms[0]:.3f}"]
            del trs
            torch.cuda.empty_cache()
    lines.append(f"the expectation (the epoch no slower than either loop, at every batch and precision) is {'met' if met else 'MISSED'}; "
                 "the epoch and both loops gave the same losses bit for bit")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
