#!/usr/bin/env python
"""What the overlay in front of the pitch balls costs (pvq_overlay_batch_frames_device): rows/s at 252 bins for 256 x 256 and
1280 x 720 images with the reference's quad and view, a ring of 200 rows that is full, on the lit scene of scripts/backdrop_rate.py —
synthetic polyphony through Vqt, AnalysisBatch, SceneBatch, PanelsBatch and RenderBatch on the device, the last frames of it drawn.
Per size: the overlay alone (quad and boxes, the quad alone, the boxes alone), a plain hipMemsetAsync over the image bytes, the
backdrop with its three panels followed by the balls (BackdropBatch.frames + RasterBatch.frames_over) from the same run, and the
three together: the whole debug picture.  Beside the overlay the share of the image its tiles and its quad cover, so the draw can be
held against a memset over the covered pixels alone.
The method is raster_rate.py's: HIP events after a 300 ms settle load of the same call, median of 5.  No rate is fixed in advance.

usage: python scripts/overlay_rate.py [--out FILE] [--streams 4] [--frames 8] [--sizes 256x256,1280x720]
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

CAPACITY, HISTORY = 300, 200


def lit_scene(S, F):
    """backdrop_rate.lit_scene plus the rendered rows: the last F of WARM + F frames of S streams of polyphony (device tensors)"""
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
    rendered = P.RenderBatch(rng).rows_device(tail, outputs=("spectrogram_vqt", "chroma"))
    torch.cuda.synchronize()
    return (rng, last(scene, ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible")), last(scene, ("bass_lit", "bass_rgba")),
            {k: tail[k] for k in ("center", "peak_count")}, panels, graph, rendered)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="256x256,1280x720")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "overlay_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    S, F = args.streams, args.frames
    rows = S * F
    rng, balls, bass, peaks, panels, graph, rendered = lit_scene(S, F)
    texels = rendered["spectrogram_vqt"].reshape(S, F, 252, 4)
    elapsed = (WARM + np.arange(F)) * (HOP / SR)
    stream = torch.cuda.current_stream().cuda_stream
    lit = (texels[..., 3] != 0).float().mean().item()
    lines = [f"# {torch.cuda.get_device_name(0)}: the spectrogram quad and the chroma boxes over the finished picture, 252 bins, {S} streams x {F} "
             f"frames = {rows} rows of a lit scene (polyphony, frames {WARM} .. {WARM + F - 1}; {100 * lit:.0f} % of the texels have alpha), "
             f"ring of {HISTORY} rows, full",
             f"# median of {REPS} (min .. max), ms, and rows/s; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load; the viewer's view, quad "
             "and panel transforms"]
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        t = P.panel_transforms(252, W, H)
        tr = dict(spectrum_transform=t[0], histogram_transform=t[1], graph_transform=t[2])
        bd, rb, ov = P.BackdropBatch(rng, S, W, H), P.RasterBatch(rng, S, W, H), P.OverlayBatch(rng, S, W, H, history_rows=HISTORY)
        image = torch.empty((S, F, H, W, 4), device="cuda")
        L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream)
        for _ in range(HISTORY // F + 1):                                       # fill the rings
            ov.frames(F, image, rendered)
        torch.cuda.synchronize()
        L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream)
        ov.frames(F, image, rendered)
        torch.cuda.synchronize()
        drawn = (image != 0).any(-1).float().mean().item()                       # pixels of a cleared image that one call draws on

        def behind():
            bd.frames(F, bass, panels, graph, peak_count=peaks["peak_count"], image=image, **tr)
            rb.frames_over(image, balls, peaks, elapsed=elapsed)

        def picture():
            behind()
            ov.frames(F, image, rendered)
        res = [("memset", timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream))),
               ("overlay: quad and boxes", timed(lambda: ov.frames(F, image, rendered))),
               ("overlay: quad alone", timed(lambda: ov.frames(F, image, texels))),
               ("overlay: boxes alone", timed(lambda: ov.frames(F, image, None, rendered["chroma"]))),
               ("backdrop + balls over it", timed(behind)), ("backdrop + balls + overlay", timed(picture))]
        lines.append(f"{W} x {H} ({image.numel() * 4 / 1e6:.0f} MB; the overlay draws on {100 * drawn:.1f} % of the pixels):")
        for name, ms in res:
            lines.append(f"  {name:30s} {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e3:9.0f} rows/s")
        lines.append(f"  overlay / memset over the drawn pixels alone: {res[1][1][0] / max(res[0][1][0] * drawn, 1e-9):.1f} x;  "
                     f"whole debug picture / picture without the overlay: {res[5][1][0] / res[4][1][0]:.3f} x")
        del image, bd, rb, ov
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
