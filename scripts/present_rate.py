#!/usr/bin/env python
"""What the present stage costs (pvq_present_batch_rows_device: bloom, display transform, sRGB bytes): rows/s for 256 x 256 and
1280 x 720 pictures at the reference's settings and intensity 1 in every row, on the finished debug picture of
scripts/overlay_rate.py's lit scene.  Per size: the stage, the stage with the linear picture written too, the stage without bloom
(display transform and encode alone: d_intensity NULL), a plain hipMemsetAsync over the bytes the stage must move (the picture read,
16 bytes a pixel, and the bytes written, 4 a pixel), and the whole picture (BackdropBatch.frames + RasterBatch.frames_over +
OverlayBatch.frames) from the same run.
The method is raster_rate.py's — HIP events after a 300 ms settle load of the same call, median of 5 — with the runs of the
variants alternated, so a drift of the clock falls on all of them alike.  No rate is fixed in advance.

The split of a call by kernel (first pass, pyramid, last pass) needs the kernels' own durations: run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o present -- python scripts/present_rate.py --once --sizes 1280x720
and pass the kernel statistics it leaves (DIR/**/present_kernel_stats.csv) with --kernel-stats; the file is then quoted per size.

usage: python scripts/present_rate.py [--out FILE] [--streams 4] [--frames 8] [--sizes 256x256,1280x720] [--kernel-stats CSV ...] [--once]
Needs a GPU; reads nothing outside the tree."""
import argparse
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402
from overlay_rate import HISTORY, lit_scene  # noqa: E402
from raster_rate import HOP, REPS, SETTLE_S, SR, WARM  # noqa: E402


def alternated(calls):
    """every call settled once (SETTLE_S of itself), then REPS rounds over all of them in turn -> [(median, min, max)] in ms"""
    for call in calls:
        call()
        torch.cuda.synchronize()
        t_end = time.perf_counter() + SETTLE_S
        while time.perf_counter() < t_end:
            call()
            torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for _ in range(REPS):
        for k, call in enumerate(calls):
            call()                                            # the variant's own warm run, then the timed one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def kernel_split(path):
    """a rocprofv3 kernel statistics file -> {first pass, pyramid, last pass: (calls, mean us)}"""
    parts = {"first pass": [0, 0.0], "pyramid": [0, 0.0], "last pass": [0, 0.0]}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            row = {k.lower(): v for k, v in row.items()}
            name = row.get("name", "")
            if "present_down<true" in name or "present_downILb1" in name:
                part = "first pass"
            elif "present_up<true" in name or "present_upILb1" in name:
                part = "last pass"
            elif "present_down" in name or "present_up" in name:
                part = "pyramid"
            else:
                continue
            parts[part][0] += int(row["calls"])
            parts[part][1] += float(row["totaldurationns"])
    return {k: (c, t / 1e3) for k, (c, t) in parts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="256x256,1280x720")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="SIZE=CSV: rocprofv3 kernel statistics of a --once run at that size")
    ap.add_argument("--once", action="store_true", help="20 calls of the stage per size and nothing else: for a kernel trace")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "present_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    S, F = args.streams, args.frames
    rows = S * F
    stats = dict(item.split("=", 1) for item in args.kernel_stats)
    stream = torch.cuda.current_stream().cuda_stream
    if not args.once:
        rng, balls, bass, peaks, panels, graph, rendered = lit_scene(S, F)
        elapsed = (WARM + np.arange(F)) * (HOP / SR)
    lines = [f"# {torch.cuda.get_device_name(0)}: bloom, display transform and sRGB bytes of the finished picture, {S} streams x {F} frames = {rows} "
             "rows, the reference's settings (max_mip_dimension 512: 8 mips), intensity 1 in every row",
             f"# median of {REPS} (min .. max), ms, and rows/s; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load of each variant, the "
             "variants' runs alternated"]
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        image = torch.rand((S, F, H, W, 4), device="cuda")
        out = torch.empty((S, F, H, W, 4), dtype=torch.uint8, device="cuda")
        hdr = torch.empty_like(image)
        intensity = torch.ones((S, F), device="cuda")
        pb = P.PresentBatch(W, H)
        if args.once:
            for _ in range(20):
                pb.rows_device(image, intensity, out=out)
            torch.cuda.synchronize()
            continue
        t = P.panel_transforms(252, W, H)
        tr = dict(spectrum_transform=t[0], histogram_transform=t[1], graph_transform=t[2])
        bd, rb, ov = P.BackdropBatch(rng, S, W, H), P.RasterBatch(rng, S, W, H), P.OverlayBatch(rng, S, W, H, history_rows=HISTORY)
        for _ in range(HISTORY // F + 1):                                       # fill the overlay's rings
            ov.frames(F, image, rendered)

        def picture():
            bd.frames(F, bass, panels, graph, peak_count=peaks["peak_count"], image=image, **tr)
            rb.frames_over(image, balls, peaks, elapsed=elapsed)
            ov.frames(F, image, rendered)
        picture()                                                               # the stage is timed on the picture it is meant for
        torch.cuda.synchronize()
        moved = image.numel() * 4 + out.numel()
        sink = torch.empty(moved, dtype=torch.uint8, device="cuda")
        names = ["memset over the bytes moved", "present", "present, linear picture written too", "present without bloom", "the whole picture"]
        res = alternated([lambda: L.hipMemsetAsync(sink.data_ptr(), 0, moved, stream), lambda: pb.rows_device(image, intensity, out=out),
                          lambda: pb.rows_device(image, intensity, out=out, hdr=hdr), lambda: pb.rows_device(image, None, out=out), picture])
        mips = P.present_mips(W, H)
        chain = 16 * sum(w * h for w, h in mips)
        lines.append(f"{W} x {H} ({image.numel() * 4 / 1e6:.0f} MB read + {out.numel() / 1e6:.0f} MB written; mip 0 {mips[0][0]} x {mips[0][1]}, "
                     f"{chain * rows / 1e6:.0f} MB of mip chains):")
        for name, ms in zip(names, res):
            lines.append(f"  {name:38s} {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e3:9.0f} rows/s")
        lines.append(f"  present / memset: {res[1][0] / res[0][0]:.1f} x;  present without bloom / memset: {res[3][0] / res[0][0]:.1f} x;  "
                     f"present / the whole picture: {res[1][0] / res[4][0]:.2f} x")
        if size in stats:
            split = kernel_split(stats[size])
            calls = max(split["first pass"][0], 1)
            lines.append("  a call by kernel (kernel trace of 20 calls, mean us a call): " +
                         ", ".join(f"{k} {us / calls:.1f} us in {c // calls} launch{'es' if c // calls != 1 else ''}" for k, (c, us) in split.items()))
        del image, out, hdr, sink, bd, rb, ov, pb
        torch.cuda.empty_cache()
    if args.once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
