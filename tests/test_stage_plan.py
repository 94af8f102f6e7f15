"""The batch stages' shared host planner (pitchvis_amd/csrc/stage_plan.cpp): image, visuals-mode and frame-count checks with their
texts, and the cut of a call into workspace pieces.  tests/sanitize/stage_plan_main.cpp is built with -fsanitize=address,undefined
(note_plan_tool's flags) and run once with every question below.  No GPU."""
import pytest

import note_plan_tool

WHOS = ("raster batch", "backdrop frame")
SIZE = "{}: width and height are 1 .. 4096"
VH = "{}: viewport_height is 0 (the viewer's) or positive and finite"

# (question, answer)
IMAGE = [(("image", who, w, h, vh), want.format(who)) for who in WHOS for w, h, vh, want in [
    (0, 16, 0, "refused " + SIZE), (16, 0, 0, "refused " + SIZE), (4097, 16, 0, "refused " + SIZE), (16, 4097, 0, "refused " + SIZE),
    (1, 1, 0, "ok"), (4096, 4096, 0, "ok"), (1, 4096, 2.5, "ok"), (16, 16, "-0.0", "ok"),
    (16, 16, -1, "refused " + VH), (16, 16, "nan", "refused " + VH), (16, 16, "inf", "refused " + VH),
    (0, 16, "nan", "refused " + SIZE),   # the size is checked first
]]
MODE = [(("mode", who, m), want.format(who)) for who in WHOS for m, want in [
    (-1, "refused {}: unknown visuals mode"), (0, "ok"), (3, "ok"), (4, "refused {}: unknown visuals mode")]]
MANY = "refused {}: too many frames in one call"
FRAMES = [(("frames", who, n, s), want.format(who)) for who in WHOS for n, s, want in [
    (2**31 - 1, 1, "ok"), (0x3FFFFFFF, 2, "ok"), (0, 7, "ok"), (2**31, 1, MANY), (2**30, 2, MANY), (2**63, 2, MANY)]]
PIECE = [(("piece", n, s, per_row, limit), str(want)) for n, s, per_row, limit, want in [
    (7, 2, 1000, 4096, 2),                  # pieces of 2, 2, 2, 1 frames: the shape of the GPU piece tests
    (7, 2, 1000, 999, 1), (7, 2, 1000, 1, 1),   # a limit below one row: one frame a piece all the same
    (7, 2, 1000, 1 << 40, 7),               # far above the whole call
    (9, 4, 1000, 1000 * 4 * 3, 3),          # an exact fit of three frames
    (9, 4, 1000, 1000 * 4 * 3 - 1, 2), (1, 1, 1, 1, 1),
]]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = note_plan_tool.build(tmp_path_factory.mktemp("stage_plan"), "stage_plan_main.cpp", ["stage_plan.cpp"])
    asked = IMAGE + MODE + FRAMES + PIECE
    out = note_plan_tool.run(exe, *[a for q, _ in asked for a in q]).splitlines()
    assert len(out) == len(asked), out
    return {q: line for (q, _), line in zip(asked, out)}


@pytest.mark.parametrize("cases", [IMAGE, MODE, FRAMES, PIECE], ids=["image", "mode", "frames", "piece"])
def test_stage_plan(answers, cases):
    for q, want in cases:
        print(q, "->", answers[q])
    assert [answers[q] for q, _ in cases] == [want for _, want in cases]
