#!/usr/bin/env python
"""What four samples a pixel cost the backdrop (BackdropBatch(samples=4): backdrop_tiles_msaa in backdrop_tiles' place): rows/s at
252 bins for 256 x 256 and 1280 x 720 images on the lit scene of scripts/backdrop_rate.py, with the viewer's view and the
reference's panel transforms.  Per size: a plain hipMemsetAsync over the output bytes, and the backdrop without panels and with all
three, each at samples = 1 and samples = 4 of this build.  No ratio is fixed in advance.

With --parent-lib FILE (a libpvq.so built from the parent commit's sources, kept outside the tree's history) the one-sample draw of
that library is timed in the same process on the same inputs, its handle made and called through ctypes.  The one-sample kernel of
this build comes from a template the four-sample kernel shares; the condition is that it is not slower than the parent's by more
than the spread among the parent's own five runs.

The method: a run is scripts/raster_rate.py's `timed` — HIP events around one call, after a 300 ms settle load of the same call, the
median of 5 — and every call gets five runs, the calls taking turns within a round so that none has the quiet minute to itself.
Reported: the median of the five runs and their spread (min .. max).

usage: python scripts/backdrop_msaa_rate.py [--out FILE] [--parent-lib FILE] [--streams 4] [--frames 8] [--sizes 256x256,1280x720]
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
from backdrop_rate import CAPACITY, lit_scene  # noqa: E402
from pitchvis_amd import _lib  # noqa: E402
from raster_rate import HOP, REPS, SETTLE_S, SR, WARM, timed  # noqa: E402

RUNS = 5


def parent_batch(path, rng, S, W, H):
    """a one-sample BackdropBatch whose handle and calls are those of the library at `path`"""
    L = _lib.load()
    Lp = C.CDLL(path)
    for name in ("pvq_backdrop_batch_create", "pvq_backdrop_batch_destroy", "pvq_backdrop_batch_frames_device", "pvq_last_error"):
        getattr(Lp, name).argtypes, getattr(Lp, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
    b = P.BackdropBatch(rng, S, W, H)
    L.pvq_backdrop_batch_destroy(b._h)
    b._h = C.c_void_p()
    st = Lp.pvq_backdrop_batch_create(0, rng.octaves, rng.buckets_per_octave, 0, 0.0, S, W, H, C.byref(b._h))
    assert st == _lib.PVQ_OK and b._h.value, st
    b._L = Lp
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="256x256,1280x720")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "backdrop_msaa_rate.py needs a GPU"
    L = _lib.load()
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]   # the HIP runtime libpvq is linked against
    L.hipMemsetAsync.restype = C.c_int
    S, F = args.streams, args.frames
    rows = S * F
    rng, _, bass, peaks, panels, graph = lit_scene(S, F)
    stream = torch.cuda.current_stream().cuda_stream
    lit = bass["bass_lit"].float().mean().item()
    lines = [f"# {torch.cuda.get_device_name(0)}: the backdrop at one and at four samples a pixel, 252 bins, {S} streams x {F} frames = {rows} rows of "
             f"a lit scene (polyphony, frames {WARM} .. {WARM + F - 1}; {lit:.1f} lit bass segments and {peaks['peak_count'].float().mean().item():.1f} "
             f"peak discs a row, graph of {CAPACITY})",
             f"# a run: the median of {REPS} calls timed with HIP events after a {SETTLE_S * 1e3:.0f} ms settle load of the same call; {RUNS} runs a "
             "call, the calls taking turns; median of the runs (min .. max), ms, and rows/s; the viewer's view and panel transforms"]
    verdicts = []
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        t = P.panel_transforms(252, W, H)
        tr = dict(spectrum_transform=t[0], histogram_transform=t[1], graph_transform=t[2])
        image = torch.empty((S, F, H, W, 4), device="cuda")
        full = lambda b: (lambda: b.frames(F, bass, panels, graph, peak_count=peaks["peak_count"], image=image, **tr))
        bare = lambda b: (lambda: b.frames(F, bass, image=image))
        b1, b4 = P.BackdropBatch(rng, S, W, H), P.BackdropBatch(rng, S, W, H, samples=4)
        calls = [("memset", lambda: L.hipMemsetAsync(image.data_ptr(), 0, image.numel() * 4, stream)),
                 ("no panels, 1 sample", bare(b1)), ("no panels, 4 samples", bare(b4)),
                 ("three panels, 1 sample", full(b1)), ("three panels, 4 samples", full(b4))]
        if args.parent_lib:
            bp = parent_batch(os.path.abspath(args.parent_lib), rng, S, W, H)
            calls.append(("three panels, 1 sample, parent", full(bp)))
            full(b1)()
            mine = image.clone()
            full(bp)()
            torch.cuda.synchronize()
            differ = int((image.view(torch.int32) != mine.view(torch.int32)).sum())
        runs = {name: [] for name, _ in calls}
        for r in range(RUNS):
            order = calls if r % 2 == 0 else calls[::-1]
            for name, call in order:
                runs[name].append(timed(call)[0])
        lines.append(f"{W} x {H} ({image.numel() * 4 / 1e6:.0f} MB):")
        med = {}
        for name, _ in calls:
            v = sorted(runs[name])
            med[name] = float(np.median(v))
            lines.append(f"  {name:32s} {med[name]:8.3f} ms ({v[0]:.3f} .. {v[-1]:.3f})  {rows / med[name] * 1e3:9.0f} rows/s")
        lines.append(f"  4 samples / 1 sample: {med['no panels, 4 samples'] / med['no panels, 1 sample']:.2f} x without panels, "
                     f"{med['three panels, 4 samples'] / med['three panels, 1 sample']:.2f} x with three panels")
        if args.parent_lib:
            p = sorted(runs["three panels, 1 sample, parent"])
            spread = p[-1] - p[0]
            ok = med["three panels, 1 sample"] <= med["three panels, 1 sample, parent"] + spread
            verdicts.append(ok)
            lines.append(f"  one sample, this build against the parent: {med['three panels, 1 sample']:.3f} ms against {med['three panels, 1 sample, parent']:.3f} ms, "
                         f"the parent's five runs spread over {spread:.3f} ms: {'not slower' if ok else 'SLOWER'} beyond that spread; "
                         f"{differ} 32-bit words of the two pictures differ")
        del image, b1, b4
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    if verdicts and not all(verdicts):
        sys.exit(1)


if __name__ == "__main__":
    main()
