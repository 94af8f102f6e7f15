"""Writes tests/golden/dejavu_pitch_glyphs.npz: the outlines and metrics of the nine glyphs the pitch names need (C D E F G A B,
U+266F, U+266D), read with fontTools from the viewer's assets/fonts/DejaVuSans.ttf (version 2.37).  Only outlines and metrics go
in: the font file itself holds hinting bytecode and stays out of the repository.

    python tests/golden/make_text_golden.py path/to/DejaVuSans.ttf
"""
import os
import sys

import numpy as np
from fontTools.ttLib import TTFont

GLYPHS = "CDEFGAB♯♭"


def main(path):
    font = TTFont(path)
    cmap, glyf, hmtx = font.getBestCmap(), font["glyf"], font["hmtx"]
    out = {"codepoints": np.asarray([ord(c) for c in GLYPHS], np.uint32), "units_per_em": np.uint32(font["head"].unitsPerEm),
           "ascent": np.int32(font["hhea"].ascent), "descent": np.int32(font["hhea"].descent)}
    advances, n_contours, n_points, ends, points, on = [], [], [], [], [], []
    for c in GLYPHS:
        name = cmap[ord(c)]
        g = glyf[name]
        assert g.numberOfContours > 0, (c, "not a simple glyph")
        coords, end_pts, flags = g.getCoordinates(glyf)
        advances.append(hmtx[name][0])
        n_contours.append(len(end_pts))
        n_points.append(len(coords))
        ends.extend(end_pts)
        points.extend(coords)
        on.extend(f & 1 for f in flags)
    out.update(advances=np.asarray(advances, np.float32), n_contours=np.asarray(n_contours, np.uint32), n_points=np.asarray(n_points, np.uint32),
               contour_ends=np.asarray(ends, np.uint32), points=np.asarray(points, np.float32).reshape(-1, 2), on_curve=np.asarray(on, np.uint8))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dejavu_pitch_glyphs.npz")
    np.savez_compressed(dst, **out)
    print(dst, "glyphs", len(GLYPHS), "points", len(on), "bytes", os.path.getsize(dst))


if __name__ == "__main__":
    main(sys.argv[1])
