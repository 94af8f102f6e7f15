"""The note model's carried windows without a GPU (pvq_note_carry_*, pvq_note_model_rows_carry_device): the symbols, the argument
checks on host-only handles (every one returns before PVQ_ERR_NO_DEVICE), the host counters, and the host planner of a call
(note_model_plan.cpp: note_carry_plan, note_carry_row) through tests/sanitize/note_carry_plan_main.cpp, a stand-alone program built
with -fsanitize=address,undefined."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import note_carry_cases as K
import note_model_ref as R
import note_plan_tool
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd.note_model import _c_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pvq_note_carry_create", "pvq_note_carry_destroy", "pvq_note_carry_reset", "pvq_note_carry_frames_seen", "pvq_note_model_rows_carry_device")


def test_symbols_are_exported_and_declared():
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "pvq.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.pvq_abi_version() == 4 and re.search(r"#define PVQ_ABI_VERSION 4\b", hdr)


def _host_model(name, precision=0):
    n_bins, T, mlp, layers, _ = R.shape(name)
    L = _lib.load()
    par = _lib.CNoteModelParams(n_bins, T, mlp, layers)
    cw, keep = _c_weights(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name))
    h = C.c_void_p()
    assert L.pvq_note_model_create_precision(-1, C.byref(par), C.byref(cw), precision, C.byref(h)) == _lib.PVQ_OK and h.value
    del keep
    return h


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_argument_checks_come_before_no_device(precision):
    L = _lib.load()
    OK, INV, NODEV = _lib.PVQ_OK, _lib.PVQ_ERR_INVALID_ARG, _lib.PVQ_ERR_NO_DEVICE
    m, other = _host_model("G", precision), _host_model("D", precision)   # 3 bins x T 3; 180 bins x T 3
    c, c_other = C.c_void_p(), C.c_void_p()
    assert L.pvq_note_carry_create(None, 2, C.byref(c)) == INV and not c.value
    assert L.pvq_note_carry_create(m, 2, None) == INV
    assert L.pvq_note_carry_create(m, 0, C.byref(c)) == INV and not c.value
    assert L.pvq_note_carry_create(m, 2, C.byref(c)) == OK and c.value
    assert L.pvq_note_carry_create(other, 2, C.byref(c_other)) == OK and c_other.value
    try:
        db = np.zeros((2, 4, 3), np.float32)
        buf = np.zeros(2 * 4 * 128 + 8, np.float32)
        o = _lib.CNoteModelOutputs()
        o.d_prob = buf.ctypes.data
        call = L.pvq_note_model_rows_carry_device
        nf = (C.c_size_t * 2)(4, 1)
        assert call(None, c, db.ctypes.data, nf, 2, 4, C.byref(o), None) == INV              # null handles
        assert call(m, None, db.ctypes.data, nf, 2, 4, C.byref(o), None) == INV
        assert call(m, c, None, nf, 2, 4, C.byref(o), None) == INV                           # null d_db
        assert call(m, c, db.ctypes.data, nf, 3, 4, C.byref(o), None) == INV                 # n_streams is not the carry's
        assert call(m, c, db.ctypes.data, nf, 1, 4, C.byref(o), None) == INV
        assert call(m, c_other, db.ctypes.data, nf, 2, 4, C.byref(o), None) == INV           # a carry of a model of other sizes
        assert call(other, c, db.ctypes.data, nf, 2, 4, C.byref(o), None) == INV
        assert call(m, c, db.ctypes.data, (C.c_size_t * 2)(4, 5), 2, 4, C.byref(o), None) == INV   # n_frames[1] > stride_frames
        bad = _lib.CNoteModelOutputs()
        bad.d_mask = buf.ctypes.data + 2                                                     # d_mask is 4-byte aligned at every precision
        assert call(m, c, db.ctypes.data, nf, 2, 4, C.byref(bad), None) == INV
        mis = _lib.CNoteModelOutputs()
        mis.d_logits = buf.ctypes.data + 4                                                   # a 16-bit handle stores four values at a time
        assert buf.ctypes.data % 16 == 0
        assert call(m, c, db.ctypes.data, nf, 2, 4, C.byref(mis), None) == (INV if precision else NODEV)
        # everything in order: the host-only handles have no device
        assert call(m, c, db.ctypes.data, nf, 2, 4, C.byref(o), None) == NODEV
        assert call(m, c, db.ctypes.data, None, 2, 4, None, None) == NODEV
        assert b"GPU" in L.pvq_last_error()
        # the counters of a host-only carry: nothing was taken in
        seen = C.c_uint64(7)
        assert L.pvq_note_carry_frames_seen(c, 0, C.byref(seen)) == OK and seen.value == 0
        assert L.pvq_note_carry_frames_seen(c, 1, C.byref(seen)) == OK and seen.value == 0
        assert L.pvq_note_carry_frames_seen(c, 2, C.byref(seen)) == INV
        assert L.pvq_note_carry_frames_seen(c, 0, None) == INV
        assert L.pvq_note_carry_frames_seen(None, 0, C.byref(seen)) == INV
        assert L.pvq_note_carry_reset(c, -1, None) == OK and L.pvq_note_carry_reset(c, 1, None) == OK
        assert L.pvq_note_carry_reset(c, 2, None) == INV and L.pvq_note_carry_reset(None, 0, None) == INV
    finally:
        L.pvq_note_carry_destroy(c)
        L.pvq_note_carry_destroy(c_other)
        L.pvq_note_carry_destroy(None)
        L.pvq_note_model_destroy(m)
        L.pvq_note_model_destroy(other)


def test_python_face_on_host_only_handles():
    n_bins, T, mlp, layers, _ = R.shape("G")
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights("G"), device=None)
    c = P.NoteCarry(m, 3)
    assert [c.frames_seen(s) for s in range(3)] == [0, 0, 0]
    c.reset()
    c.reset(2)
    with pytest.raises(ValueError):
        c.reset(3)
    with pytest.raises(ValueError):
        c.frames_seen(3)
    with pytest.raises(ValueError):
        P.NoteCarry(m, 0)
    db = np.zeros((3, 2, n_bins), np.float32)
    with pytest.raises(RuntimeError):      # no CPU fallback: the call needs a device
        m.rows_device(db.ctypes.data, [1, 1, 1], 2, {}, n_streams=3, carry=c)
    with pytest.raises(ValueError):        # another n_streams
        m.rows_device(db.ctypes.data, [1, 1], 2, {}, n_streams=2, carry=c)


# ---- the planner ----
@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    return note_plan_tool.build(tmp_path_factory.mktemp("note_carry_plan"), main="note_carry_plan_main.cpp", units=("note_model_plan.cpp",))


def _plan(tool, n_bins, T, calls, strides):
    """[call] -> dict(rows, tiles, streams=[dict], table=[dict]); one program run per call sequence with a fixed stride is not enough
    (the stride differs per call), so the sequence is replayed up to each call and the last one kept"""
    out = []
    for c in range(len(calls)):
        text = note_plan_tool.run(tool, "plan", n_bins, T, strides[c], len(calls[0]), c + 1, *[n for call in calls[:c + 1] for n in call])
        blocks = text.split("call ")[1:]
        assert len(blocks) == c + 1
        lines = blocks[-1].splitlines()
        head = lines[0].split()
        assert int(head[0]) == c
        rec = dict(zip(head[1::2], map(int, head[2::2])), streams=[], table=[])
        for ln in lines[1:]:
            w = ln.split()
            d = dict(zip(w[0::2], map(int, w[1::2])))
            (rec["streams"] if w[0] == "stream" else rec["table"]).append(d)
        out.append(rec)
    return out


@pytest.mark.parametrize("T", [1, 3, 5, 8])
def test_plan_of_the_schedules(plan_tool, T):
    n_bins = 7
    calls = K.schedules(T)
    strides = [max(call) + 3 for call in calls]
    plans = _plan(plan_tool, n_bins, T, calls, strides)
    seen = [0] * 5
    some_head = some_body = False
    for c, (call, plan) in enumerate(zip(calls, plans)):
        stride = strides[c]
        want_rows = sum(max(0, n - max(0, T - 1 - seen[s])) for s, n in enumerate(call))
        assert plan["rows"] == want_rows and plan["tiles"] == -(-want_rows // 128)
        assert plan["max_n"] == max(call)
        first = 0
        for s, st in enumerate(plan["streams"]):
            fs = K.model_rows(T, seen[s], call[s])
            assert st["stream"] == s and st["seen"] == seen[s] and st["n"] == call[s]
            assert st["first_row"] == first and st["rows"] == len(fs) and (not fs or st["f_first"] == fs[0])
            assert st["head"] == sum(f < T - 1 for f in fs)
            first += len(fs)
        # every model row exactly once, in the order of the row list
        want = [(s, f) for s in range(5) for f in K.model_rows(T, seen[s], call[s])]
        assert [(r["stream"], r["f"]) for r in plan["table"]] == want and [r["row"] for r in plan["table"]] == list(range(len(want)))
        L = T * n_bins
        for r in plan["table"]:
            s, f = r["stream"], r["f"]
            assert r["out_row"] == s * stride + f and f < call[s]
            assert r["in_stitch"] == (1 if f < T - 1 else 0)
            if r["in_stitch"]:      # entirely inside the stream's 2 (T - 1) stitched frames, ending at the call's frame f
                assert 0 <= r["at"] and r["at"] + L <= 2 * (T - 1) * n_bins and r["at"] + L == (T - 1 + f + 1) * n_bins
                # and the frames it begins in were given: the tail holds min(T - 1, seen) of them
                assert r["at"] >= (T - 1 - min(T - 1, seen[s])) * n_bins
                some_head = True
            else:                   # entirely inside the stream's n frames of d_db
                assert r["at"] == (s * stride + f - (T - 1)) * n_bins and r["at"] + L <= (s * stride + call[s]) * n_bins
                some_body = True
        seen = [a + n for a, n in zip(seen, call)]
    assert some_body and (some_head or T == 1)


def test_300_streams_of_one_frame_plan_to_3_tiles(plan_tool):
    T = 3
    plans = _plan(plan_tool, 5, T, [[1] * 300] * 4, [1] * 4)
    assert [p["rows"] for p in plans] == [0, 0, 300, 300] and [p["tiles"] for p in plans] == [0, 0, 3, 3]
    assert [r["stream"] for r in plans[2]["table"]] == list(range(300)) and all(r["in_stitch"] and r["at"] == 0 for r in plans[2]["table"])
    assert plans[3]["max_rows"] == 1
