#!/usr/bin/env python
"""What the pitch-name labels cost on the device (pvq_text_batch_rows_device): rows/s for 32 rows of the reference's twelve labels
(7 octaves, the viewer's view, the DejaVuSans outlines of tests/golden/dejavu_pitch_glyphs.npz) at 256 x 256 and 1280 x 720.  Per
size: the blend, a plain hipMemsetAsync over the whole image and one over as many bytes as the covered pixels hold, the one-off
time of a handle's create (layout on the host, uploads and the text_coverage kernel; wall clock, median of 5), and, where
profiles/overlay_rate.txt has the size, the overlay's figures from there for comparison.
The method is raster_rate.py's: HIP events after a 300 ms settle load of the same call, median of 5.  No rate is fixed in advance.

usage: python scripts/text_rate.py [--out FILE] [--rows 32] [--sizes 256x256,1280x720]
Needs a GPU; reads nothing outside the tree."""
import argparse
import ctypes as C
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
import text_cases as TC  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402
from raster_rate import REPS, SETTLE_S, timed  # noqa: E402


def overlay_figures(size):
    """the lines of profiles/overlay_rate.txt for `size`: {name: ms}"""
    path, out, on = os.path.join(ROOT, "profiles", "overlay_rate.txt"), {}, False
    if not os.path.exists(path):
        return out
    for line in open(path):
        if re.match(r"\d+ x \d+", line):
            on = line.startswith(size)
        m = re.match(r"\s+(memset|overlay: quad and boxes)\s+([\d.]+) ms", line)
        if on and m:
            out[m.group(1)] = float(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--sizes", default="256x256,1280x720")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "text_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    rows = args.rows
    font, labels = TC.font_of(TC.fixture()), P.pitch_name_labels(7)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# {torch.cuda.get_device_name(0)}: the twelve pitch-name labels (7 octaves, DejaVuSans outlines, the viewer's view) over {rows} rows",
             f"# median of {REPS} (min .. max), ms, and rows/s; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load; create: wall clock"]
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        lay = P.text_layout(font, labels, W, H)
        create = []
        for _ in range(REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tb = P.TextBatch(font, labels, W, H)
            create.append((time.perf_counter() - t0) * 1e3)
        create = create[1:]
        covered = float((tb.coverage() > 0).mean())
        image = torch.empty((rows, H, W, 4), device="cuda")
        L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream)
        torch.cuda.synchronize()
        part = max(16, int(image.numel() * 4 * covered) // 16 * 16)
        res = [("memset, whole image", timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream))),
               ("memset, covered pixels' bytes", timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, part, stream))),
               ("text blend", timed(lambda: tb.rows(rows, image)))]
        lines.append(f"{W} x {H} ({image.numel() * 4 / 1e6:.0f} MB; the labels cover {100 * covered:.2f} % of the pixels, "
                     f"{sum(d['n_tiles'] for d in lay)} (tile, label) entries, {sum(d['n_segments'] for d in lay)} segments):")
        for name, ms in res:
            lines.append(f"  {name:30s} {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e3:9.0f} rows/s")
        lines.append(f"  {'create (once per handle)':30s} {float(np.median(create)):8.3f} ms ({min(create):.3f} .. {max(create):.3f})")
        ov = overlay_figures(f"{W} x {H}")
        if ov:
            lines.append("  profiles/overlay_rate.txt at this size: " + ", ".join(f"{k} {v:.3f} ms" for k, v in ov.items()))
        lines.append(f"  text blend / memset over the covered pixels' bytes: {res[2][1][0] / res[1][1][0]:.1f} x;  / memset over the image: "
                     f"{res[2][1][0] / res[0][1][0]:.2f} x" + (f";  / overlay draw: {res[2][1][0] / ov['overlay: quad and boxes']:.2f} x"
                                                               if "overlay: quad and boxes" in ov else ""))
        del image, tb
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
