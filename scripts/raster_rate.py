#!/usr/bin/env python
"""What drawing the pitch balls (pvq_raster_batch_frames_device) costs: rows/s and covered-pixel x balls per second at 252 bins for
256 x 256 and 1280 x 720 images, on a lit scene — synthetic polyphony (tests/synth.py) through Vqt, AnalysisBatch and SceneBatch on
the device, the last frames of it drawn.  Beside each figure the time of a plain hipMemsetAsync over the same output bytes in the
same run: the parent has no such path, so the memset is the yardstick (a stage that only stored its pixels would cost that).
The per-pixel sin, cos and atan2 go through double precision for bit parity with the host face; the figures include that price.
Device calls are timed with HIP events after a 300 ms settle load of the same call (as bench.py does); median of 5.
No rate is fixed in advance.

usage: python scripts/raster_rate.py [--out FILE] [--streams 4] [--frames 8] [--sizes 256x256,1280x720] [--once]
       (--once: one untimed call per configuration and nothing else, for a kernel trace)
Needs a GPU; reads nothing outside the tree."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402
from synth import piano_roll  # noqa: E402

REPS, SETTLE_S, MAX_PEAKS, HOP, SR, WARM = 5, 0.3, 32, 1024, 48000.0, 56


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


def lit_scene(S, F):
    """S streams of polyphony -> the scene's ball records and the peak arrays of the last F of WARM + F frames (device tensors)"""
    rng = P.VqtRange(55.0, 7, 36)
    v = P.Vqt(P.VqtParameters(sr=SR, range=rng), device=0)
    nf, n = WARM + F, 252
    pcms = [torch.from_numpy(piano_roll(SR, nf * HOP / SR + 0.5, 40 + s)[0][:nf * HOP].copy()).cuda() for s in range(S)]
    fields = {"center": torch.zeros((S, nf, MAX_PEAKS), device="cuda"), "size": torch.zeros((S, nf, MAX_PEAKS), device="cuda"),
              "peak_count": torch.zeros((S, nf), dtype=torch.int32, device="cuda"), "calmness": torch.zeros((S, nf, n), device="cuda"),
              "pitch_accuracy": torch.zeros((S, nf, n), device="cuda"), "pitch_deviation": torch.zeros((S, nf, n), device="cuda"),
              "scene_calmness": torch.zeros((S, nf), device="cuda")}
    P.AnalysisBatch(rng, S).preprocess_pcm(v, pcms, nf, HOP, outputs=fields, max_peaks=MAX_PEAKS)
    balls = P.SceneBatch(rng, S).frames_device(fields, frame_time=HOP / SR)
    torch.cuda.synchronize()
    last = lambda d, keys: {k: d[k][:, WARM:].contiguous() for k in keys}
    return rng, last(balls, ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible")), last(fields, ("center", "peak_count"))


def covered(balls, W, H, vh):
    """(drawable balls, pixels x balls with length(p) < 1) over all rows, counted with torch in f32 (boundary pixels may differ by a few)"""
    xyzs = balls["ball_xyzs"].reshape(-1, 252, 4)
    vis = balls["ball_visible"].reshape(-1, 8)
    bit = (vis[:, torch.arange(252, device="cuda") // 32] >> (torch.arange(252, device="cuda") % 32)) & 1
    ok = (bit != 0) & (xyzs[..., 3] > 0) & torch.isfinite(xyzs).all(-1)
    s = vh / H
    wx = ((torch.arange(W, device="cuda") + 0.5 - 0.5 * W) * s)[None, None, :]
    wy = ((0.5 * H - (torch.arange(H, device="cuda") + 0.5)) * s)[None, :, None]
    pairs = 0
    for r in range(xyzs.shape[0]):
        b = xyzs[r][ok[r]]
        for chunk in b.split(8):
            d2 = (wx - chunk[:, 0, None, None]) ** 2 + (wy - chunk[:, 1, None, None]) ** 2
            pairs += int((d2 < (10.0 * chunk[:, 3, None, None]) ** 2).sum())
    return int(ok.sum()), pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="256x256,1280x720")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raster_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    S, F = args.streams, args.frames
    rows = S * F
    rng, balls, peaks = lit_scene(S, F)
    elapsed = (WARM + np.arange(F)) * (HOP / SR)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# {torch.cuda.get_device_name(0)}: the pitch balls drawn, 252 bins, {S} streams x {F} frames = {rows} rows of a lit scene "
             f"(polyphony, frames {WARM} .. {WARM + F - 1})",
             f"# median of {REPS} (min .. max), ms; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load; memset: hipMemsetAsync over the same output bytes"]
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        b = P.RasterBatch(rng, S, W, H)
        image = torch.empty((S, F, H, W, 4), device="cuda")
        call = lambda: b.frames_device(balls, peaks, elapsed=elapsed, image=image)
        if args.once:
            call()
            torch.cuda.synchronize()
            continue
        n_balls, pairs = covered(balls, W, H, P.raster.VIEWPORT_HEIGHT)
        set_ms = timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream))
        ms = timed(call)
        lines.append(f"{W:5d} x {H:4d}: {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e3:9.0f} rows/s  "
                     f"{pairs / ms[0] * 1e-6:8.3f} G covered-pixel x balls/s  ({n_balls / rows:.1f} balls drawn and {pairs / rows / (W * H):.2f} "
                     f"layers per pixel a row)  {image.numel() * 4 / 1e6:.0f} MB | memset {set_ms[0]:8.3f} ms ({set_ms[1]:.3f} .. {set_ms[2]:.3f}): "
                     f"{ms[0] / set_ms[0]:.1f} x")
        del image, b
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
