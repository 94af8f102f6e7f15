#!/usr/bin/env python
"""What the tuning-drift readout costs on the device (pvq_readout_batch_rows_device): rows/s for 32 rows, each its own value (-40 ..
40, so every colour branch and strings of three characters), at 256 x 256 and 1280 x 720, ui_scale 1.  The font is the curved one of
tests/readout_cases.py: the nine DejaVuSans outlines of tests/golden/dejavu_pitch_glyphs.npz given to the readout's 24 codepoints.
Per size: the readout, TextBatch.rows over the reference's twelve pitch-name labels on the same pictures, a plain hipMemsetAsync
over the whole image and one over as many bytes as the drawn pixels hold, and the one-off time of a handle's create (layout and
flattening on the host, uploads and the readout_atlas kernel; wall clock, median of 5).
The method is raster_rate.py's: HIP events after a 300 ms settle load of the same call, median of 5.  No rate is fixed in advance.

usage: python scripts/readout_rate.py [--out FILE] [--rows 32] [--sizes 256x256,1280x720]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import pitchvis_amd as P  # noqa: E402
import readout_cases as RC  # noqa: E402
import text_cases as TC  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402
from raster_rate import REPS, SETTLE_S, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--sizes", default="256x256,1280x720")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "readout_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    rows = args.rows
    font, label_font, labels = RC.lib_font("curved"), TC.font_of(TC.fixture()), P.pitch_name_labels(7)
    stream = torch.cuda.current_stream().cuda_stream
    values = torch.linspace(-40.0, 40.0, rows, device="cuda")
    lines = [f"# {torch.cuda.get_device_name(0)}: the tuning-drift readout (ui_scale 1, DejaVuSans outlines) over {rows} rows, values -40 .. 40",
             f"# median of {REPS} (min .. max), ms, and rows/s; HIP events after a {SETTLE_S * 1e3:.0f} ms settle load; create: wall clock"]
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        create = []
        for _ in range(REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rb = P.ReadoutBatch(font, W, H)
            create.append((time.perf_counter() - t0) * 1e3)
        create = create[1:]
        tb = P.TextBatch(label_font, labels, W, H)
        drawn = float((P.readout_frame(font, -40.0, np.zeros((H, W, 4), np.float32))[..., 3] > 0).mean())
        image = torch.empty((rows, H, W, 4), device="cuda")
        L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream)
        torch.cuda.synchronize()
        part = max(16, int(image.numel() * 4 * drawn) // 16 * 16)
        res = [("memset, whole image", timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream))),
               ("memset, drawn pixels' bytes", timed(lambda: L.hipMemsetAsync(image.data_ptr(), 0, part, stream))),
               ("text blend, twelve labels", timed(lambda: tb.rows(rows, image))),
               ("readout", timed(lambda: rb.rows(values, image)))]
        lines.append(f"{W} x {H} ({image.numel() * 4 / 1e6:.0f} MB; the readout of -40 draws on {100 * drawn:.2f} % of the pixels):")
        for name, ms in res:
            lines.append(f"  {name:30s} {ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {rows / ms[0] * 1e3:9.0f} rows/s")
        lines.append(f"  {'create (once per handle)':30s} {float(np.median(create)):8.3f} ms ({min(create):.3f} .. {max(create):.3f})")
        lines.append(f"  readout / memset over the drawn pixels' bytes: {res[3][1][0] / res[1][1][0]:.1f} x;  / memset over the image: "
                     f"{res[3][1][0] / res[0][1][0]:.2f} x;  / text blend: {res[3][1][0] / res[2][1][0]:.2f} x")
        del image, tb, rb
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
