"""The note model's carried windows on the GPU (NoteModel.rows_device(..., carry=NoteCarry), pvq_note_model_rows_carry_device).

The one bar: a row's logits, probability and mask carry the bits pvq_note_model_rows_device gives the same window.  So every test
feeds a stream's frames call by call through a carry, concatenates the outputs of the calls per stream, and compares them bit for
bit with ONE rows_device call over the stream's concatenated frames (whose rows f < T - 1 are zeros, as the carried rows before a
stream has seen T - 1 frames are).  Rows of a call beyond a stream's count must be zero, and 1024 guard elements behind each output
untouched.  In every call the d_db rows beyond a stream's count hold NaN, and the whole d_db is overwritten with NaN on the same
stream right after the call: a frame read late, or read where none was given, shows as NaN or as other bits.

Shapes of tests/note_model_ref.py: G (3 bins, T 3, mlp 16), B (the viewer's), A (T 5), H (T 1, eight layers), J (T 8, 1024 bins).
The schedules (tests/note_carry_cases.py) run as five streams in one carry, stride_frames = the call's largest count + 3."""
import functools

import numpy as np
import pytest

import note_carry_cases as K
import note_model_ref as R
import pitchvis_amd as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 1024
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _model(name, precision="f32"):
    n_bins, T, mlp, layers, _ = R.shape(name)
    return P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), device=0, precision=precision)


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _whole(m, seqs):
    """one rows_device call over every stream's whole sequence: dict name -> host array [S][max frames][...]"""
    n_bins = m.params.n_bins
    stride = max(max(len(q) for q in seqs), 1)
    db = np.full((len(seqs), stride, n_bins), np.nan, np.float32)
    for s, q in enumerate(seqs):
        db[s, :len(q)] = q
    o = m.rows_device(torch.from_numpy(db).cuda(), [len(q) for q in seqs], stride)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _carry_call(m, carry, seqs, pos, counts, stride, wait=True):
    """one carried call giving stream s the frames seqs[s][pos[s] : pos[s] + counts[s]]; returns the host outputs [S][stride][...]
    (wait=False: the device tensors and their guards, nothing synchronised)"""
    S, n_bins = len(seqs), m.params.n_bins
    db = np.full((S, stride, n_bins), np.nan, np.float32)
    for s in range(S):
        db[s, :counts[s]] = seqs[s][pos[s]:pos[s] + counts[s]]
    d_db = torch.from_numpy(db).cuda()
    prob, prob_all = _guarded((S, stride, 128), torch.float32, 7.0)
    logits, logits_all = _guarded((S, stride, 128), torch.float32, 7.0)
    mask, mask_all = _guarded((S, stride, 4), torch.int32, -1)
    m.rows_device(d_db, counts, stride, {"d_prob": prob, "d_logits": logits, "d_mask": mask}, carry=carry)
    d_db.fill_(NAN)                     # enqueued on the same stream right after the call
    if not wait:
        return {"d_prob": (prob, prob_all), "d_logits": (logits, logits_all), "d_mask": (mask, mask_all)}
    torch.cuda.synchronize()
    assert (prob_all[-GUARD:] == 7.0).all() and (logits_all[-GUARD:] == 7.0).all() and (mask_all[-GUARD:] == -1).all()
    return {"d_prob": prob.cpu().numpy(), "d_logits": logits.cpu().numpy(), "d_mask": mask.cpu().numpy()}


def _run_schedule(m, calls, seed, carry=None, seqs=None, check_zero_rows=True):
    """the calls [call][stream] through one carry; returns (per-stream concatenated outputs, the sequences, the carry)"""
    S, n_bins, T = len(calls[0]), m.params.n_bins, m.params.t_frames
    totals = [sum(call[s] for call in calls) for s in range(S)]
    if seqs is None:
        seqs = [R.db_like((totals[s], n_bins), seed + s) for s in range(S)]
    carry = carry or P.NoteCarry(m, S)
    seen0 = [carry.frames_seen(s) for s in range(S)]
    pos = [0] * S
    got = {k: [[] for _ in range(S)] for k in m.OUTPUTS}
    for call in calls:
        stride = max(call) + 3
        out = _carry_call(m, carry, seqs, pos, call, stride)
        for s in range(S):
            for k in got:
                got[k][s].append(out[k][s, :call[s]])
                if check_zero_rows:
                    assert not out[k][s, call[s]:].any(), (k, s, call)      # rows outside are zero (NaN would be "any")
            pos[s] += call[s]
        assert [carry.frames_seen(s) for s in range(S)] == [a + p for a, p in zip(seen0, pos)]
    return {k: [np.concatenate(v) for v in got[k]] for k in got}, seqs, carry


def _assert_equals_whole(m, got, seqs):
    T = m.params.t_frames
    whole = _whole(m, seqs)
    rows = 0
    for s, q in enumerate(seqs):
        for k in m.OUTPUTS:
            assert np.array_equal(_bits(got[k][s]), _bits(whole[k][s, :len(q)])), (k, s)
        assert not got["d_prob"][s][:T - 1].any()
        if len(q) >= T:
            assert (got["d_prob"][s][T - 1:] > 0).all()           # every model row was written (sigmoid > 0)
            rows += len(q) - (T - 1)
    return rows


CASES = [(name, "f32") for name in "GBAHJ"] + [(name, prec) for name in "GBJ" for prec in ("bf16", "f16")]


@pytest.mark.parametrize("name,precision", CASES)
def test_schedules_equal_one_whole_call(name, precision):
    m = _model(name, precision)
    T = m.params.t_frames
    got, seqs, _ = _run_schedule(m, K.schedules(T), 7000 + ord(name))
    rows = _assert_equals_whole(m, got, seqs)
    assert [len(q) for q in seqs] == [6, 6 + max(T - 2, 0), 2 * T + 130, 257, 0] and rows > 380


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_workspace_limit_of_one_tile(precision):
    """shape B under a limit below one tile: every call runs tile by tile (the third has T + 130 + ... rows, the first 257), same bits"""
    n_bins, T, mlp, layers, _ = R.shape("B")
    m = P.NoteModel(P.NoteModelParams(n_bins, T, mlp, layers), R.weights("B"), device=0, precision=precision)
    m.set_workspace_limit(1)
    got, seqs, _ = _run_schedule(m, K.schedules(T), 7100)
    ref = _model("B", precision)
    _assert_equals_whole(ref, got, seqs)


@pytest.mark.parametrize("rows", [32, 33, 97, 129, 257])
def test_row_totals_of_one_frame_streams(rows):
    """`rows` streams of one frame each in one call: 32 and 33 rows sit at the wave-activity edge, 97 reaches the fourth wave, 129 and
    257 leave a one-row last tile"""
    for name, precision in (("G", "f32"), ("G", "bf16"), ("C", "f32"), ("C", "f16")):
        m = _model(name, precision)
        T = m.params.t_frames
        got, seqs, _ = _run_schedule(m, [[T - 1] * rows, [1] * rows], 7200 + rows)
        assert _assert_equals_whole(m, got, seqs) == rows


def test_calls_queued_back_to_back():
    """twelve calls (the schedules twice over: more than the ring of descriptor slots) queued without a host wait between them, every
    call's plan overwriting the one before it on the host; compared after one synchronisation at the end"""
    m = _model("B", "bf16")
    T, n_bins = m.params.t_frames, m.params.n_bins
    calls = K.schedules(T) + K.schedules(T)
    totals = [sum(call[s] for call in calls) for s in range(5)]
    seqs = [R.db_like((totals[s], n_bins), 7600 + s) for s in range(5)]
    carry, pos, queued = P.NoteCarry(m, 5), [0] * 5, []
    for call in calls:
        queued.append((call, _carry_call(m, carry, seqs, pos, call, max(call) + 3, wait=False)))
        pos = [p + n for p, n in zip(pos, call)]
    torch.cuda.synchronize()
    got = {k: [np.concatenate([out[k][0][s, :call[s]].cpu().numpy() for call, out in queued]) for s in range(5)] for k in m.OUTPUTS}
    for call, out in queued:
        for k, (view, whole) in out.items():
            assert (whole[-GUARD:] == (-1 if k == "d_mask" else 7.0)).all()
            for s in range(5):
                assert not view[s, call[s]:].any()
    _assert_equals_whole(m, got, seqs)


def test_reset_of_one_stream_only():
    m = _model("A")
    T = m.params.t_frames
    seqs = [R.db_like((2 * (T + 2), m.params.n_bins), 7300 + s) for s in range(3)]
    first = [[T + 2] * 3]
    got1, _, carry = _run_schedule(m, first, 0, seqs=[q[:T + 2] for q in seqs])
    carry.reset(1)
    assert [carry.frames_seen(s) for s in range(3)] == [T + 2, 0, T + 2]
    got2, _, _ = _run_schedule(m, first, 0, carry=carry, seqs=[q[T + 2:] for q in seqs])
    whole = _whole(m, [seqs[0], seqs[1][T + 2:], seqs[2]])
    for k in m.OUTPUTS:
        for s in (0, 2):      # continue across the reset of their neighbour
            assert np.array_equal(_bits(np.concatenate([got1[k][s], got2[k][s]])), _bits(whole[k][s]))
        assert np.array_equal(_bits(got2[k][1]), _bits(whole[k][1, :T + 2]))     # stream 1 starts afresh: T - 1 zero rows again
    assert not got2["d_prob"][1][:T - 1].any() and got2["d_prob"][0][:T - 1].all()
    carry.reset()
    assert [carry.frames_seen(s) for s in range(3)] == [0, 0, 0]
    got3, _, _ = _run_schedule(m, first, 0, carry=carry, seqs=[q[:T + 2] for q in seqs])
    for k in m.OUTPUTS:
        for s in range(3):
            assert np.array_equal(_bits(got3[k][s]), _bits(got1[k][s]))


def test_300_streams_a_frame_per_call():
    """the viewer's cadence for 300 streams: six calls of one frame each against one whole call of six frames per stream"""
    m = _model("B")
    got, seqs, _ = _run_schedule(m, [[1] * 300] * 6, 7400)
    assert _assert_equals_whole(m, got, seqs) == 300 * 4


def test_single_outputs_and_no_outputs_still_take_the_frames_in():
    m = _model("G")
    T, n_bins = m.params.t_frames, m.params.n_bins
    seq = R.db_like((2, T + 3, n_bins), 7500)
    carry = P.NoteCarry(m, 2)
    d0 = torch.from_numpy(np.ascontiguousarray(seq[:, :T - 1])).cuda()
    assert m.rows_device(d0, outputs={}, carry=carry) == {}               # nothing to write, yet the frames count
    d0.fill_(NAN)
    assert [carry.frames_seen(s) for s in range(2)] == [T - 1, T - 1]
    only = m.rows_device(torch.from_numpy(np.ascontiguousarray(seq[:, T - 1:])).cuda(), outputs=("d_mask",), carry=carry)
    torch.cuda.synchronize()
    whole = _whole(m, [seq[0], seq[1]])
    assert list(only) == ["d_mask"]
    assert np.array_equal(_bits(only["d_mask"].cpu().numpy()), _bits(whole["d_mask"][:, T - 1:]))
    other = _model("B")
    with pytest.raises(ValueError):                                        # a model of other sizes
        other.rows_device(torch.zeros((2, 4, other.params.n_bins), device="cuda"), carry=carry)
