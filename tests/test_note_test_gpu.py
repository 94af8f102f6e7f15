"""The note trainer's test pass on the GPU (pvq_note_trainer_test; pitchvis_train/train.py:164-198) against tests/note_test_ref.py, the
float64 restatement.  All inputs are note_trainer_ref.dataset (400 rows, soft targets uniform in [0, 1]: half the labels are positive)
with note_model_ref.weights; shapes C, D and F of note_model_ref.SHAPES (odd O_conv, an mlp that is no multiple of 64, zero, one and
three hidden layers, T = 1).

Bars:
  * logits within LOGIT_REL = 1e-5 of the largest |float64 logit|, the bar tests/test_note_trainer_gpu.py asserts for EVAL logits.
  * a decision z > 0 is left open where |z64| <= 1e-4 * max|z64| (ten times the logit bar): a count of a batch (of a pitch) may differ
    from the float64 count by at most the number of that batch's (that pitch's) elements inside the band.  The band may hold at most
    5e-3 of the elements (NoteModel's cap); the float64 model puts 3.3e-4 (C), 3.7e-4 (D) and 2.0e-4 (F) there.
  * the loss of a batch within 1e-5 * max|logit of the batch| + 1e-6 * loss of float64 BCE, the bar of the existing EVAL-loss test.
  * counts against the logits the call itself wrote: exact.  mean_f1, accuracy and mean_loss against the formulas on the returned
    records: 1e-15.
Every test prints the figures it observes before it asserts.  Not yet observed on a device: no GPU could be obtained while these
tests were written; the float64 figures above come from the reference alone."""
import functools

import numpy as np
import pytest

import note_model_ref as R
import note_test_ref as NR
import note_trainer_ref as TR
import pitchvis_amd as P
from pitchvis_amd.note_trainer import random_split

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGIT_REL = 1e-5
GUARD = 1024
SEED = 11


def _trainer(name, max_batch=300, weights=None, **hyper):
    n_bins, T, mlp, layers, _ = R.shape(name)
    h = P.NoteTrainerHyper(**dict(dict(seed=SEED, dropout=0.5), **hyper))      # (the pass must not apply the dropout)
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), weights or R.weights(name), h, max_batch, device=0)


@functools.lru_cache(maxsize=None)
def _device_data(name):
    db, tg = TR.dataset(name)
    return torch.from_numpy(db.copy()).cuda(), torch.from_numpy(tg.copy()).cuda()


def _run(t, name, idx, batch, d_tg=None):
    d_db, d_tg0 = _device_data(name)
    d_logits = torch.full((idx.size, 128), 7.0, device="cuda")
    res = t.test(d_db, d_tg0 if d_tg is None else d_tg, idx, batch, d_logits=d_logits)
    return res, d_logits.cpu().numpy()


def _check_exact(tag, res, z, y, batch):
    """test 2's rules: the returned counts are the counts of the logits the call wrote; the scalars are the formulas on the records"""
    own = NR.counts(z, y, batch)
    assert res.records.size == own["rows"].size == -(-z.shape[0] // batch)
    for k in ("rows", "tp", "fp", "fn", "correct"):
        assert np.array_equal(getattr(res, k).astype(np.int64), own[k]), (tag, k)
    assert np.array_equal(res.pitch_counts.astype(np.int64), own["pitch"]), tag
    assert int(res.tp.sum()) == int(own["pitch"][:, 0].sum()) and (res.records["_pad"] == 0).all()
    want = NR.scalars(res.rows, res.tp, res.fp, res.fn, res.correct, res.loss)
    got = (res.mean_f1, res.accuracy, res.mean_loss)
    print(f"{tag}: mean F1 {got[0]:.6f}, accuracy {got[1]:.6f}, mean loss {got[2]:.6f}; formulas off by {[abs(g - w) for g, w in zip(got, want)]}")
    assert all(abs(g - w) <= 1e-15 for g, w in zip(got, want))
    assert np.array_equal(res.f1, NR.f1(res.tp, res.fp, res.fn)) and np.array_equal(res.pitch_f1, NR.f1(*res.pitch_counts.T))


def _check_f64(tag, res, z, z64, y, batch):
    """test 1's rules"""
    top = float(np.abs(z64).max())
    err = float(np.abs(z - z64).max())
    open_ = NR.band(z64)
    share = float(open_.mean())
    pred_share, lab_share = float((z64 > 0).mean()), float((y > 0.5).mean())
    print(f"{tag}: {z.shape[0]} rows in {res.records.size} batches of {batch}; max|z64| {top:.4f}; logits off by {err:.2e} (bar {LOGIT_REL * top:.2e}); "
          f"{int(open_.sum())} of {open_.size} elements in the band ({share:.2e}, cap {NR.BAND_CAP:.0e}); {pred_share:.3f} predicted, {lab_share:.3f} labelled")
    want = NR.counts(z64, y, batch, open_)
    loss64 = NR.batch_losses64(z64, y, batch)
    sl = NR.slices(z.shape[0], batch)
    bars = np.array([1e-5 * float(np.abs(z64[s]).max()) + 1e-6 * l for s, l in zip(sl, loss64)])
    for k in ("tp", "fp", "fn", "correct"):
        diff = np.abs(getattr(res, k).astype(np.int64) - want[k])
        print(f"  {k}: device {getattr(res, k).tolist()}, f64 {want[k].tolist()}, |difference| {diff.tolist()}, elements in the band {want['open'].tolist()}")
    pdiff = np.abs(res.pitch_counts.astype(np.int64) - want["pitch"]).max(axis=1)
    print(f"  per pitch: worst |difference| {int(pdiff.max())}, pitches that differ {int((pdiff > 0).sum())}, in the band per pitch at most {int(want['pitch_open'].max())}")
    print(f"  loss per batch: device {res.loss.tolist()}, |difference| {np.abs(res.loss - loss64).tolist()}, bars {bars.tolist()}")
    assert err <= LOGIT_REL * top
    assert share <= NR.BAND_CAP
    assert np.array_equal(res.rows.astype(np.int64), want["rows"])
    for k in ("tp", "fp", "fn", "correct"):
        assert (np.abs(getattr(res, k).astype(np.int64) - want[k]) <= want["open"]).all(), k
    assert (np.abs(res.pitch_counts.astype(np.int64) - want["pitch"]) <= want["pitch_open"][:, None]).all()
    assert (np.abs(res.loss - loss64) <= bars).all()


@pytest.mark.parametrize("name", ["C", "D", "F"])
def test_against_f64_and_exact_integers(name):
    """tests 1 and 2 of the issue: max_batch 300, every admissible row shuffled (two chunks), batches of 100 (the last one short)"""
    T = R.shape(name)[1]
    idx = NR.shuffled(name)
    assert idx.size == TR.N_ROWS - (T - 1) > 300 and np.array_equal(np.sort(idx), np.arange(T - 1, TR.N_ROWS))
    t = _trainer(name, 300)
    res, z = _run(t, name, idx, 100)
    y = TR.dataset(name)[1][idx.astype(np.int64)]
    _check_f64(f"{name}/300", res, z, NR.all_logits64(name)[idx.astype(np.int64)], y, 100)
    _check_exact(f"{name}/300", res, z, y, 100)
    assert int(res.tp.min()) > 1000 and int(res.fn.min()) > 1000 and 0.3 < res.mean_f1 < 0.7     # every count is in the thousands
    assert t.steps == 0


def test_the_metric_batch_does_not_reach_the_arithmetic():
    """test 3: shape C, one idx at batches 100, 37, 1 and 1000: equal logit bits, equal sums, equal pitch counts; at 37 batch 8 is
    rows 296 .. 332 and straddles the chunk edge at 300"""
    name = "C"
    idx = NR.shuffled(name, seed=3)
    y = TR.dataset(name)[1][idx.astype(np.int64)]
    t = _trainer(name, 300)
    runs = {b: _run(t, name, idx, b) for b in (100, 37, 1, 1000)}
    z0 = runs[100][1]
    assert (z0 != 7.0).all()
    for b, (res, z) in runs.items():
        sums = [int(getattr(res, k).astype(np.int64).sum()) for k in ("rows", "tp", "fp", "fn", "correct")]
        print(f"batch {b}: {res.records.size} records, sums rows / tp / fp / fn / correct {sums}, mean F1 {res.mean_f1:.6f}, accuracy {res.accuracy:.6f}, "
              f"{int((z.view(np.uint32) != z0.view(np.uint32)).sum())} logit words differ from batch 100")
        assert res.records.size == -(-idx.size // b)
        assert np.array_equal(z.view(np.uint32), z0.view(np.uint32))
        assert sums == [int(getattr(runs[100][0], k).astype(np.int64).sum()) for k in ("rows", "tp", "fp", "fn", "correct")]
        assert np.array_equal(res.pitch_counts, runs[100][0].pitch_counts)
        assert res.accuracy == runs[100][0].accuracy
        _check_exact(f"C/batch {b}", res, z, y, b)
    assert (runs[1][0].rows == 1).all() and runs[1000][0].rows.tolist() == [idx.size] and runs[37][0].rows[-1] == idx.size % 37
    assert 37 * 8 < 300 < 37 * 9


@pytest.mark.parametrize("n_idx", [1, 64, 65, 397])
def test_chunk_edges(n_idx):
    """test 4: shape D at max_batch 64 (397 rows: six chunks of 64 and one of 13); idx holds T - 1, n_rows - 1 and a duplicate"""
    name = "D"
    T = R.shape(name)[1]
    idx = TR.batch_idx(name, n_idx)
    assert idx.size == n_idx and idx[0] == T - 1 and (n_idx == 1 or (idx[1] == TR.N_ROWS - 1 and len(set(idx.tolist())) < n_idx))
    t = _trainer(name, 64)
    res, z = _run(t, name, idx, 100)
    y = TR.dataset(name)[1][idx.astype(np.int64)]
    _check_f64(f"D/64/{n_idx}", res, z, NR.all_logits64(name)[idx.astype(np.int64)], y, 100)
    _check_exact(f"D/64/{n_idx}", res, z, y, 100)


def test_known_answers():
    """test 5: shape D with output.weight = 0, so every logit is output.bias: exact counts without a band"""
    name = "D"
    idx = NR.shuffled(name, seed=5)
    tg = TR.dataset(name)[1]
    lab = tg[idx.astype(np.int64)] > 0.5
    sl = NR.slices(idx.size, 100)
    for bias in (-1.0, 1.0):
        w = dict(R.weights(name))
        w["output.weight"] = np.zeros_like(w["output.weight"])
        w["output.bias"] = np.full_like(w["output.bias"], bias)
        t = _trainer(name, 300, weights=w)
        res, z = _run(t, name, idx, 100)
        print(f"bias {bias}: tp {res.tp.tolist()} fp {res.fp.tolist()} fn {res.fn.tolist()} correct {res.correct.tolist()} F1 {res.f1.tolist()}")
        assert (z == np.float32(bias)).all()
        pos, neg = np.array([int(lab[s].sum()) for s in sl]), np.array([int((~lab[s]).sum()) for s in sl])
        zero = np.zeros(len(sl), np.int64)
        if bias < 0:        # every prediction negative
            want = (zero, zero, pos, neg)
            assert (res.f1 == 0.0).all() and res.mean_f1 == 0.0
        else:               # every prediction positive
            want = (pos, neg, zero, pos)
        for k, wv in zip(("tp", "fp", "fn", "correct"), want):
            assert np.array_equal(getattr(res, k).astype(np.int64), wv), (bias, k)
        assert np.array_equal(res.pitch_counts[:, 0 if bias > 0 else 2].astype(np.int64), lab.sum(0)) and (res.pitch_counts[:, 1 if bias < 0 else 2] == 0).all()
        # BCE of a constant logit: softplus(bias) - bias * y
        want_loss = np.array([(np.log1p(np.exp(bias)) - bias * tg[idx.astype(np.int64)][s].astype(np.float64)).mean() for s in sl])
        assert (np.abs(res.loss - want_loss) <= 1e-5 + 1e-6 * want_loss).all()
        if bias < 0:
            # the targets of batch 1's rows set to 0: nothing predicted, nothing labelled
            tg2 = tg.copy()
            tg2[idx[100:200].astype(np.int64)] = 0.0
            res2, _ = _run(t, name, idx, 100, d_tg=torch.from_numpy(tg2).cuda())
            print(f"  batch 1 without labels: tp {res2.tp[1]} fp {res2.fp[1]} fn {res2.fn[1]} correct {res2.correct[1]} F1 {res2.f1[1]}")
            assert (res2.tp[1], res2.fp[1], res2.fn[1], res2.correct[1], res2.f1[1]) == (0, 0, 0, 100 * 128, 0.0)
            assert np.array_equal(res2.fn[[0, 2, 3]], res.fn[[0, 2, 3]]) and res2.mean_f1 == 0.0


def test_nothing_else_moves():
    """test 6"""
    name = "C"
    d_db0, d_tg0 = _device_data(name)
    d_db, d_tg = d_db0.clone(), d_tg0.clone()
    idx = NR.shuffled(name, seed=6)
    n = idx.size
    t = _trainer(name, 300, dropout=0.1)
    t.step(d_db, d_tg, TR.batch_idx(name, 37))           # so that gradients, moments and the counter are not zero
    before = {k: t.read_flat(k) for k in ("weights", "grads", "adam_m", "adam_v")}
    assert t.steps == 1 and all(v.any() for v in before.values())
    buf = torch.full((n * 128 + 2 * GUARD,), 7.0, device="cuda")
    res = t.test(d_db, d_tg, idx, 100, d_logits=buf[GUARD:GUARD + n * 128])
    torch.cuda.synchronize()
    z = buf[GUARD:GUARD + n * 128].cpu().numpy().reshape(n, 128)
    print(f"guards: {int((buf[:GUARD] != 7.0).sum())} + {int((buf[GUARD + n * 128:] != 7.0).sum())} words changed; {int((z == 7.0).sum())} logits unwritten")
    assert (buf[:GUARD] == 7.0).all() and (buf[GUARD + n * 128:] == 7.0).all() and (z != 7.0).all()
    assert torch.equal(d_db, d_db0) and torch.equal(d_tg, d_tg0)
    assert t.steps == 1
    for k, v in before.items():
        assert np.array_equal(t.read_flat(k).view(np.uint32), v.view(np.uint32)), k
    # a second handle in the same state: equal logit bits, equal records
    t2 = _trainer(name, 300, dropout=0.1)
    t2.step(d_db, d_tg, TR.batch_idx(name, 37))
    res2, z2 = _run(t2, name, idx, 100)
    assert np.array_equal(z.view(np.uint32), z2.view(np.uint32)) and res.records.tobytes() == res2.records.tobytes()
    assert np.array_equal(res.pitch_counts, res2.pitch_counts)
    # a gradient step after a pass (t) and without one (t3, fresh but for the same first step): equal gradients
    t3 = _trainer(name, 300, dropout=0.1)
    t3.step(d_db, d_tg, TR.batch_idx(name, 37))
    gi = TR.batch_idx(name, 130, seed=2)
    t.step(d_db, d_tg, gi, "grad")
    t3.step(d_db, d_tg, gi, "grad")
    a, b = t.read_flat("grads").view(np.uint32), t3.read_flat("grads").view(np.uint32)
    print(f"gradients after a pass against none: {int((a != b).sum())} of {a.size} words differ")
    assert np.array_equal(a, b) and t.steps == 1
    # a pass without pitch counts and without logits, and a refused one
    res3 = t2.test(d_db, d_tg, idx, 100, pitches=False)
    assert res3.pitch_counts is None and res3.records.tobytes() == res2.records.tobytes()
    with pytest.raises(ValueError):
        t2.test(d_db, d_tg, np.array([TR.N_ROWS], np.uint32))


def test_a_trained_handles_verdict_is_the_shipped_models():
    """test 7: after three steps on shape C the pass decides as NoteModel.from_state_dict(trainer.state_dict()) does, outside the band"""
    name = "C"
    n_bins, T, mlp, layers, _ = R.shape(name)
    d_db, d_tg = _device_data(name)
    train_idx, test_idx = random_split(TR.N_ROWS, T, 0.25, seed=4)
    t = _trainer(name, 300, dropout=0.1, lr=1e-3)
    for b in P.epoch(train_idx[:99], 33):
        t.step(d_db, d_tg, b)
    assert t.steps == 3
    res, z = _run(t, name, test_idx, 100)
    sd = t.state_dict()
    m = P.NoteModel.from_state_dict(sd, n_bins, T, device=0)
    o = m.rows_device(d_db.view(1, TR.N_ROWS, n_bins), [TR.N_ROWS], TR.N_ROWS, outputs=("d_mask",))
    shipped = R.mask_bits(o["d_mask"][0].cpu().numpy())[test_idx.astype(np.int64)]
    z64 = NR.logits64(sd, TR.dataset(name)[0], test_idx, T)
    open_ = NR.band(z64)
    differ = (z > 0) != shipped
    print(f"{test_idx.size} rows: {int(differ.sum())} decisions differ from NoteModel's mask, {int((differ & ~open_).sum())} of them outside the band "
          f"({int(open_.sum())} elements, {open_.mean():.2e}); mean F1 {res.mean_f1:.4f}, accuracy {res.accuracy:.4f}")
    assert open_.mean() <= NR.BAND_CAP and not (differ & ~open_).any()
    assert not ((z > 0) != (z64 > 0))[~open_].any()
    _check_exact("C trained", res, z, TR.dataset(name)[1][test_idx.astype(np.int64)], 100)
