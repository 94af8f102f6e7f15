#!/usr/bin/env python
"""What a carried call of the note model costs (pvq_note_model_rows_carry_device: windows that continue across calls, the rows of
all streams packed into shared 128-row tiles) for {64, 4 096} streams x {1, 4, 64} new frames per call at T = 3 and T = 5, 252 bins,
mlp 1024, 2 hidden layers, in f32 and bf16 — and one stream x 65 536 frames.  Beside each, pvq_note_model_rows_device on the same
d_db: the path that existed before, which restarts at every call, so it yields FEWER model rows (frames - T + 1 per stream, none at
one frame per call) and spends a tile per stream; the tile count of each is given.  Device calls are timed with HIP events after a
300 ms settle load of the same call (scripts/note_model_rate.py's `timed`); median of 5 with the spread.

Then scripts/note_model_rate.py is run again, twice each and alternating: with lib/libpvq_parent.so when it is there (a build of the
parent commit's sources kept beside the library, PVQ_DEV_LIB=parent; never committed) and with the library as it is — rows_device
before and after its kernels took the nullable row-table argument.

usage: python scripts/note_carry_rate.py [--out FILE] [--quick]     (--quick: 64 streams only, no rerun)
Needs a GPU; reads nothing outside the tree."""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
from note_model_rate import LAYERS, MLP, N_BINS, REPS, SETTLE_S, make_weights, timed  # noqa: E402


def measure(T, precision, S, frames, lines):
    w = make_weights(T, LAYERS, 7)
    m = P.NoteModel(P.NoteModelParams(N_BINS, T, MLP, LAYERS), w, precision=precision)
    carry = P.NoteCarry(m, S)
    g = torch.Generator(device="cuda").manual_seed(T)
    d_db = 60.0 * torch.rand((S, frames, N_BINS), device="cuda", generator=g) ** 4
    outs = {n: torch.empty(m.output_shape(n, S, frames)[0], dtype=torch.float32 if n != "d_mask" else torch.int32, device="cuda") for n in m.OUTPUTS}
    if T > 1:      # every stream has seen T - 1 frames: each frame of a call is a model row from here on
        m.rows_device(60.0 * torch.rand((S, T - 1, N_BINS), device="cuda", generator=g) ** 4, None, T - 1, {}, carry=carry)
    c_ms = timed(lambda: m.rows_device(d_db, None, frames, outs, carry=carry))
    r_ms = timed(lambda: m.rows_device(d_db, None, frames, outs))
    c_rows, r_rows = S * frames, S * max(0, frames - T + 1)
    c_tiles, r_tiles = -(-c_rows // 128), S * -(-max(0, frames - T + 1) // 128)
    lines.append(f"T {T} {precision:4s} {S:5d} streams x {frames:5d} frames | carry {c_ms[0]:9.3f} ms ({c_ms[1]:.3f} .. {c_ms[2]:.3f}) {c_rows:7d} rows {c_tiles:5d} tiles"
                 f" | rows_device {r_ms[0]:9.3f} ms ({r_ms[1]:.3f} .. {r_ms[2]:.3f}) {r_rows:7d} rows {r_tiles:5d} tiles")
    print(lines[-1], flush=True)
    del m, carry, d_db, outs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "note_carry_rate.py needs a GPU"
    lines = [f"# carried calls of the note model, {N_BINS} bins, mlp {MLP}, {LAYERS} hidden layers; median of {REPS} (min .. max), ms; HIP events after a"
             f" {SETTLE_S * 1e3:.0f} ms settle load",
             "# carry: pvq_note_model_rows_carry_device in its steady state (every frame of the call is a model row; tiles = ceil(rows / 128))",
             "# rows_device: pvq_note_model_rows_device on the same d_db (rows = streams x (frames - T + 1); a tile per stream and 128 of them)"]
    for T in (3, 5):
        for precision in ("f32", "bf16"):
            for S in ((64,) if args.quick else (64, 4096)):
                for frames in (1, 4, 64):
                    measure(T, precision, S, frames, lines)
            measure(T, precision, 1, 4096 if args.quick else 65536, lines)
    if not args.quick:
        parent = os.path.join(ROOT, "pitchvis_amd", "lib", "libpvq_parent.so")
        runs = ([("before (the parent commit's sources)", {"PVQ_DEV_LIB": "parent"})] if os.path.exists(parent) else []) + [("after (this tree)", {})]
        if len(runs) == 1:
            lines.append("# lib/libpvq_parent.so is not there: scripts/note_model_rate.py with this tree's library only")
        for rnd in (1, 2):
            for tag, env in runs:
                r = subprocess.run([sys.executable, os.path.join(HERE, "note_model_rate.py")], env=dict(os.environ, **env), capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-2000:]
                lines.append(f"# ---- scripts/note_model_rate.py, {tag}, round {rnd} ----")
                lines += [ln for ln in r.stdout.splitlines() if "rows_device" in ln or ln.startswith("## ")]
                print("\n".join(lines[-9:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
