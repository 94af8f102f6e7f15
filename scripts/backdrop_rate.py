#!/usr/bin/env python
"""What the picture behind the pitch balls costs (pvq_backdrop_batch_frames_device, pvq_backdrop_balls_over_device): rows/s at 252
bins for 256 x 256 and 1280 x 720 images on the lit scene of scripts/raster_rate.py — synthetic polyphony through Vqt,
AnalysisBatch, SceneBatch and PanelsBatch on the device, the last frames of it drawn with the viewer's view and the reference's
panel transforms.  Per size: the backdrop alone without panels (net and lit bass segments) and with all three panels, the
backdrop followed by the balls drawn over it, the balls alone over the clear colour (RasterBatch.frames_device, the parent's
picture), and a plain hipMemsetAsync over the same output bytes.  The ratio of the full picture to the balls alone is the figure a
later fusion of the layers into the ball kernel would be judged against.
The method is raster_rate.py's: HIP events after a 300 ms settle load of the same call, median of 5.  No rate is fixed in advance.

usage: python scripts/backdrop_rate.py [--out FILE] [--streams 4] [--frames 8] [--sizes 256x256,1280x720]
Needs a GPU; reads nothing outside the tree."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402
from raster_rate import HOP, MAX_PEAKS, REPS, SETTLE_S, SR, WARM, timed  # noqa: E402
from synth import piano_roll  # noqa: E402

CAPACITY = 300


def lit_scene(S, F):
    """the last F of WARM + F frames of S streams of polyphony: ball records, bass state, peak arrays and panel meshes (device)"""
    rng = P.VqtRange(55.0, 7, 36)
    v = P.Vqt(P.VqtParameters(sr=SR, range=rng), device=0)
    nf, n = WARM + F, 252
    pcms = [torch.from_numpy(piano_roll(SR, nf * HOP / SR + 0.5, 40 + s)[0][:nf * HOP].copy()).cuda() for s in range(S)]
    fields = {"center": torch.zeros((S, nf, MAX_PEAKS), device="cuda"), "size": torch.zeros((S, nf, MAX_PEAKS), device="cuda"),
              "peak_count": torch.zeros((S, nf), dtype=torch.int32, device="cuda"), "scene_calmness": torch.zeros((S, nf), device="cuda")}
    fields.update({k: torch.zeros((S, nf, n), device="cuda") for k in ("x_vqt_smoothed", "calmness", "pitch_accuracy", "pitch_deviation")})
    P.AnalysisBatch(rng, S).preprocess_pcm(v, pcms, nf, HOP, outputs=fields, max_peaks=MAX_PEAKS)
    scene = P.SceneBatch(rng, S).frames_device(fields, frame_time=HOP / SR)
    last = lambda d, keys: {k: d[k][:, WARM:].contiguous() for k in keys}
    tail = last(fields, ("x_vqt_smoothed", "center", "size", "peak_count", "calmness"))
    pb = P.PanelsBatch(rng, S, graph_capacity=CAPACITY)
    panels = pb.rows_device(tail)
    graph = pb.graph_device(fields["scene_calmness"], first_emitted=WARM)
    torch.cuda.synchronize()
    return (rng, last(scene, ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible")), last(scene, ("bass_lit", "bass_rgba")),
            {k: tail[k] for k in ("center", "peak_count")}, panels, graph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="256x256,1280x720")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "backdrop_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    S, F = args.streams, args.frames
    rows = S * F
    rng, balls, bass, peaks, panels, graph = lit_scene(S, F)
    elapsed = (WARM + np.arange(F)) * (HOP / SR)
    stream = torch.cuda.current_stream().cuda_stream
    lit = bass["bass_lit"].float().mean().item()
    lines = [f"# {torch.cuda.get_device_name(0)}: the backdrop and the balls over it, 252 bins, {S} streams x {F} frames = {rows} rows of a lit "
             f"scene (polyphony, frames {WARM} .. {WARM + F - 1}; {lit:.1f} lit bass segments and {peaks['peak_count'].float().mean().item():.1f} "
             f"peak discs a row, graph of {CAPACITY})",
             f"# median of {REPS} (min .. max), ms, and rows/s; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load; the viewer's view and "
             "panel transforms"]
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        t = P.panel_transforms(252, W, H)
        tr = dict(spectrum_transform=t[0], histogram_transform=t[1], graph_transform=t[2])
        bd, rb = P.BackdropBatch(rng, S, W, H), P.RasterBatch(rng, S, W, H)
        image = torch.empty((S, F, H, W, 4), device="cuda")
        bare = lambda: bd.frames(F, bass, image=image)
        full = lambda: bd.frames(F, bass, panels, graph, peak_count=peaks["peak_count"], image=image, **tr)

        def picture():
            full()
            rb.frames_over(image, balls, peaks, elapsed=elapsed)
        res = [("memset", timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream))),
               ("balls alone (frames_device)", timed(lambda: rb.frames_device(balls, peaks, elapsed=elapsed, image=image))),
               ("backdrop, no panels", timed(bare)), ("backdrop, three panels", timed(full)), ("backdrop + balls over it", timed(picture))]
        lines.append(f"{W} x {H} ({image.numel() * 4 / 1e6:.0f} MB):")
        for name, ms in res:
            lines.append(f"  {name:30s} {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e3:9.0f} rows/s")
        lines.append(f"  full picture / balls alone: {res[4][1][0] / res[1][1][0]:.2f} x")
        del image, bd, rb
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
