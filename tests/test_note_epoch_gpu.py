"""Whole epochs and restored checkpoints of the note trainer on the GPU (pvq_note_trainer_epoch, pvq_note_trainer_write,
pvq_note_trainer_set_steps; pitchvis_train/train.py:147-162).  The reference of an epoch is the same library's ``step`` in a Python loop
over ``idx[epoch_order(...)]``; the reference of a restored handle is the handle the checkpoint was read from.  Every comparison is of
bits, so there is no tolerance anywhere.  Shape D of note_model_ref.SHAPES (180 bins, T = 3, mlp 48, no hidden layer) at max_batch 64
with note_trainer_ref.dataset (400 rows); D has no dropout layer, so one case runs shape C (three hidden layers), where a batch at the
wrong counter or in the wrong row order meets other dropout keys.  Every test prints what it observes before it asserts."""
import functools

import numpy as np
import pytest

import note_model_ref as R
import note_trainer_ref as TR
import pitchvis_amd as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ARRAYS = ("weights", "grads", "adam_m", "adam_v")
MAX_BATCH = 64
GUARD = 1024
SEED = 11
SHUFFLE = 5


def _trainer(precision, name="D", weights=None):
    n_bins, T, mlp, layers, _ = R.shape(name)
    h = P.NoteTrainerHyper(seed=SEED, dropout=0.1, lr=1e-3)
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), weights or R.weights(name), h, MAX_BATCH, device=0, precision=precision)


@functools.lru_cache(maxsize=None)
def _device_data(name):
    db, tg = TR.dataset(name)
    return torch.from_numpy(db.copy()).cuda(), torch.from_numpy(tg.copy()).cuda()


def _split(name, n, seed=0):
    """a train split of n entries that is not sorted, reaches both ends of the admissible range and holds duplicates"""
    T = R.shape(name)[1]
    idx = np.random.default_rng(40 + seed + n).integers(T - 1, TR.N_ROWS, size=n).astype(np.uint32)
    idx[0] = TR.N_ROWS - 1
    if n > 2:
        idx[1], idx[-1] = T - 1, idx[2]
        assert len(set(idx.tolist())) < n and (np.diff(idx.astype(np.int64)) < 0).any()
    return idx


def _state(t):
    s = {k: t.read_flat(k).view(np.uint32) for k in ARRAYS}
    s["steps"] = t.steps
    return s


def _same(tag, a, b):
    differ = {k: int((a[k] != b[k]).sum()) for k in ARRAYS}
    print(f"{tag}: words that differ {differ}; steps {a['steps']} and {b['steps']}")
    return not any(differ.values()) and a["steps"] == b["steps"]


def _loop(t, name, idx, batch, epoch):
    """the epoch as the caller wrote it before: one step per slice of the permuted split, the loss read after each"""
    d_db, d_tg = _device_data(name)
    seq = idx[P.epoch_order(SHUFFLE, epoch, idx.size).astype(np.int64)]
    d_loss = torch.zeros(1, device="cuda")
    losses = []
    for b in P.epoch(seq, batch):
        t.step(d_db, d_tg, b, d_loss=d_loss)
        losses.append(d_loss.cpu().numpy()[0])
    return np.array(losses, np.float32)


def _check_epoch(tag, got, want_losses):
    losses, mean = got
    s = 0.0
    for v in want_losses:
        s += float(v)
    print(f"{tag}: {losses.size} batches, losses {losses.tolist()[:6]}, mean {mean!r}, the loop's {want_losses.tolist()[:6]}, mean {s / want_losses.size!r}")
    assert losses.dtype == np.float32 and np.array_equal(losses.view(np.uint32), want_losses.view(np.uint32))
    assert mean == s / want_losses.size and np.isfinite(losses).all() and (losses > 0).all()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("name,n_idx,batch", [("D", 1, 64), ("D", 64, 64), ("D", 65, 64), ("D", 150, 37), ("D", 5, 1), ("C", 150, 37)])
def test_epoch_equals_loop(name, n_idx, batch, precision):
    d_db, d_tg = _device_data(name)
    idx = _split(name, n_idx)
    a, b = _trainer(precision, name), _trainer(precision, name)
    w0 = a.read_flat("weights")
    got = a.epoch(d_db, d_tg, idx, batch, SHUFFLE, 3)
    want = _loop(b, name, idx, batch, 3)
    n_batches = -(-n_idx // batch)
    assert want.size == n_batches and a.steps == n_batches
    _check_epoch(f"{name} {precision} {n_idx}/{batch}", got, want)
    assert _same(f"{name} {precision} {n_idx}/{batch}", _state(a), _state(b))
    assert (a.read_flat("weights") != w0).any() and a.read_flat("adam_v").any()      # the epoch did train


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_epochs_in_a_row(precision):
    """epochs 0, 1 and 2 on one handle: the order buffer grows (65 -> 150 entries), is then reused, and the counter carries over"""
    name = "D"
    d_db, d_tg = _device_data(name)
    a, b = _trainer(precision), _trainer(precision)
    steps = 0
    for e, (n_idx, batch) in enumerate([(65, 64), (150, 37), (150, 37)]):
        idx = _split(name, n_idx, seed=e)
        got = a.epoch(d_db, d_tg, idx, batch, SHUFFLE, e)
        want = _loop(b, name, idx, batch, e)
        steps += want.size
        _check_epoch(f"{precision} epoch {e}", got, want)
        assert _same(f"{precision} epoch {e}", _state(a), _state(b)) and a.steps == steps
    assert steps == 2 + 5 + 5
    # the two passes over 150 entries met them in different orders
    assert not np.array_equal(P.epoch_order(SHUFFLE, 1, 150), P.epoch_order(SHUFFLE, 2, 150))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_checkpoint_restores_the_run(precision):
    name = "D"
    d_db, d_tg = _device_data(name)
    batches = [TR.batch_idx(name, 37, seed=k) for k in range(5)]
    a = _trainer(precision)
    for ix in batches[:3]:
        a.step(d_db, d_tg, ix)
    ck = a.checkpoint()
    assert ck["steps"] == 3 and ck["precision"] == precision and ck["hyper"]["lr"] == 1e-3 and all(ck[k].any() for k in ("weights", "adam_m", "adam_v"))
    for ix in batches[3:]:
        a.step(d_db, d_tg, ix)
    A = _state(a)

    other = R.weights(name, seed=77)
    b = _trainer(precision, weights=other)
    assert not np.array_equal(b.read_flat("weights"), ck["weights"])
    b.load_checkpoint(ck)
    assert b.steps == 3
    for k in ("weights", "adam_m", "adam_v"):
        assert np.array_equal(b.read_flat(k).view(np.uint32), ck[k].view(np.uint32)), k      # write, then read: the same bits
    for ix in batches[3:]:
        b.step(d_db, d_tg, ix)
    assert _same(f"{precision} restored", A, _state(b)) and A["steps"] == 5

    # the arrays without the counter: Adam's bias correction runs at t = 1, 2 instead of 4, 5
    c = _trainer(precision, weights=other)
    for k in ("weights", "adam_m", "adam_v"):
        c.write_flat(k, ck[k])
    assert c.steps == 0
    for ix in batches[3:]:
        c.step(d_db, d_tg, ix)
    Cs = _state(c)
    print(f"{precision} without set_steps: {int((Cs['weights'] != A['weights']).sum())} of {A['weights'].size} weight words differ")
    assert Cs["steps"] == 2 and (Cs["weights"] != A["weights"]).any()

    # "grads" is written like the others, and nothing but the array named moves
    g = np.arange(c.n_params, dtype=np.float32)
    before = _state(c)
    c.write_flat("grads", g)
    after = _state(c)
    assert np.array_equal(after["grads"], g.view(np.uint32)) and all(np.array_equal(before[k], after[k]) for k in ("weights", "adam_m", "adam_v"))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_stops_and_resumes(precision):
    """train.py:147-162 as trainer.fit: three epochs in one run, and one epoch, a checkpoint, a fresh handle and the other two"""
    name = "D"
    d_db, d_tg = _device_data(name)
    idx = _split(name, 100)
    a = _trainer(precision)
    whole = a.fit(d_db, d_tg, idx, 3, 48, SHUFFLE)
    b = _trainer(precision)
    first = b.fit(d_db, d_tg, idx, 1, 48, SHUFFLE)
    ck = b.checkpoint()
    c = _trainer(precision, weights=R.weights(name, seed=77))
    c.load_checkpoint(ck)
    rest = c.fit(d_db, d_tg, idx, 2, 48, SHUFFLE, start_epoch=1)
    print(f"{precision}: mean losses of one run {whole.tolist()}, of the resumed one {first.tolist() + rest.tolist()}")
    assert whole.dtype == np.float64 and whole.shape == (3,) and np.array_equal(whole, np.concatenate([first, rest]))
    assert _same(f"{precision} resumed", _state(a), _state(c)) and a.steps == 9


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_a_refused_epoch_leaves_the_handle(precision):
    name = "D"
    d_db, d_tg = _device_data(name)
    a, b = _trainer(precision), _trainer(precision)
    for t in (a, b):
        t.step(d_db, d_tg, TR.batch_idx(name, 37))
    before = _state(a)
    bad = np.concatenate([_split(name, 149), [TR.N_ROWS]]).astype(np.uint32)      # the one bad index is the last
    with pytest.raises(ValueError, match=r"idx\[149\] = 400"):
        a.epoch(d_db, d_tg, bad, 37, SHUFFLE, 0)
    with pytest.raises(ValueError, match="max_batch"):
        a.epoch(d_db, d_tg, bad[:-1], MAX_BATCH + 1, SHUFFLE, 0)
    assert _same(f"{precision} refused", before, _state(a)) and a.steps == 1
    # and goes on as a handle that was never asked
    idx = _split(name, 65)
    ga, gb = a.epoch(d_db, d_tg, idx, 64, SHUFFLE, 0), b.epoch(d_db, d_tg, idx, 64, SHUFFLE, 0)
    assert np.array_equal(ga[0].view(np.uint32), gb[0].view(np.uint32)) and ga[1] == gb[1] and _same(f"{precision} after", _state(a), _state(b))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_nothing_outside_the_handle_is_written(precision):
    name = "D"
    n_bins = R.shape(name)[0]
    db, tg = TR.dataset(name)
    n = TR.N_ROWS
    buf_db = torch.full((n * n_bins + 2 * GUARD,), 7.0, device="cuda")
    buf_tg = torch.full((n * 128 + 2 * GUARD,), 7.0, device="cuda")
    d_db, d_tg = buf_db[GUARD:GUARD + n * n_bins].view(n, n_bins), buf_tg[GUARD:GUARD + n * 128].view(n, 128)
    d_db.copy_(torch.from_numpy(db.copy()))
    d_tg.copy_(torch.from_numpy(tg.copy()))
    t = _trainer(precision)
    idx = _split(name, 150)
    losses, mean = t.epoch(d_db, d_tg, idx, 37, SHUFFLE, 0)
    torch.cuda.synchronize()
    changed = [int((b[:GUARD] != 7.0).sum()) + int((b[-GUARD:] != 7.0).sum()) for b in (buf_db, buf_tg)]
    print(f"{precision}: guard words changed {changed}; mean loss {mean}")
    assert changed == [0, 0]
    assert np.array_equal(d_db.cpu().numpy(), db) and np.array_equal(d_tg.cpu().numpy(), tg)
    # the same epoch on the plain tensors: the placement of the dataset does not reach the bits
    t2 = _trainer(precision)
    l2, m2 = t2.epoch(*_device_data(name), idx, 37, SHUFFLE, 0)
    assert np.array_equal(losses.view(np.uint32), l2.view(np.uint32)) and mean == m2 and _same(f"{precision} placement", _state(t), _state(t2))
    # outputs a caller does not want
    L = t._L
    import ctypes as C
    st = L.pvq_note_trainer_epoch(t._h, d_db.data_ptr(), d_tg.data_ptr(), n, idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size, 37, SHUFFLE, 1, None, None, None)
    assert st == 0 and t.steps == 10
