"""What the tests of the note model's carried windows share (tests/test_note_carry.py, tests/test_note_carry_gpu.py): the schedules —
per stream the frames it is given call by call — and the rule that says which frames become model rows."""


def schedules(T):
    """five streams x six calls: a frame per call (the viewer's cadence); empty calls between short ones, with a call of T - 2 that
    merges old and new frames in the tail; calls of exactly T - 1 and T, one over a tile, then one frame; a long first call and
    nothing after; a stream that never gets a frame"""
    per_stream = [(1, 1, 1, 1, 1, 1), (0, 2, 0, 1, max(T - 2, 0), 3), (T - 1, T, 130, 1, 0, 0), (257, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)]
    return [[per_stream[s][c] for s in range(5)] for c in range(6)]   # [call][stream]


def model_rows(T, seen, n):
    """frames f of a call of n that are model rows for a stream that has seen `seen` frames: seen + f >= T - 1"""
    return list(range(min(max(T - 1 - seen, 0), n), n))
