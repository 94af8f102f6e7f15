"""The trainer's test pass in float64, restated from its description (include/pvq.h: "The test pass of the trainer";
pitchvis_train/train.py:164-198), not from the library's code: float64 logits through note_model_ref.logits64 over
note_trainer_ref.windows, the decisions (z > 0, y > 0.5), the counts per test batch and per output, the float64 BCE per batch, and the
three scalars train.py prints.  Shared, cached and read-only."""
import functools

import numpy as np

import note_model_ref as R
import note_trainer_ref as TR

BAND_REL = 1e-4     # a decision is left open where |z64| <= BAND_REL * max|z64|
BAND_CAP = 5e-3     # and at most this share of the elements may lie there (NoteModel's cap)


@functools.lru_cache(maxsize=None)
def all_logits64(name):
    """float64 logits of note_model_ref.weights(name) for every admissible row of note_trainer_ref.dataset(name): [N_ROWS][128], rows
    below T - 1 zero"""
    T = R.shape(name)[1]
    db, _ = TR.dataset(name)
    z = np.zeros((TR.N_ROWS, 128))
    rows = np.arange(T - 1, TR.N_ROWS)
    z[rows] = R.logits64(R.weights(name), TR.windows(db, rows, T))
    z.setflags(write=False)
    return z


def logits64(w, db, idx, T):
    return R.logits64(w, TR.windows(db, idx, T))


def shuffled(name, seed=0):
    """every admissible row of the shape's dataset, shuffled"""
    T = R.shape(name)[1]
    return (np.random.default_rng(1000 + seed).permutation(TR.N_ROWS - (T - 1)) + (T - 1)).astype(np.uint32)


def f1(tp, fp, fn):
    """2 tp / (2 tp + fp + fn), 0 where the denominator is 0 (sklearn's zero-division value)"""
    tp, fp, fn = (np.asarray(a, np.float64) for a in (tp, fp, fn))
    den = 2.0 * tp + fp + fn
    return np.where(den > 0, 2.0 * tp / np.where(den > 0, den, 1.0), 0.0)


def bce64(z, y):
    """per element, float64: max(z, 0) - z y + log1p(exp(-|z|)) = -(y log s + (1 - y) log(1 - s)) with s = sigmoid(z)"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    return np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))


def slices(n, batch):
    return [slice(at, min(at + batch, n)) for at in range(0, n, batch)]


def counts(z, y, batch, open_=None):
    """z, y [n][128] (rows in idx order) -> dict of per-batch int64 arrays rows, tp, fp, fn, correct, the per-batch number of elements
    of `open_` (a bool array, or None), pitch [128][3] tp / fp / fn over all rows and pitch_open [128]"""
    pred, lab = np.asarray(z) > 0, np.asarray(y) > 0.5
    tp, fp, fn, ok = pred & lab, pred & ~lab, ~pred & lab, pred == lab
    sl = slices(pred.shape[0], batch)
    out = {"rows": np.array([s.stop - s.start for s in sl], np.int64)}
    for k, a in (("tp", tp), ("fp", fp), ("fn", fn), ("correct", ok)):
        out[k] = np.array([int(a[s].sum()) for s in sl], np.int64)
    out["pitch"] = np.stack([tp.sum(0), fp.sum(0), fn.sum(0)], axis=1).astype(np.int64)
    if open_ is not None:
        out["open"] = np.array([int(open_[s].sum()) for s in sl], np.int64)
        out["pitch_open"] = open_.sum(0).astype(np.int64)
    return out


def batch_losses64(z, y, batch):
    l = bce64(z, y)
    return np.array([l[s].mean() for s in slices(l.shape[0], batch)])


def scalars(rows, tp, fp, fn, correct, loss):
    """(mean_f1, accuracy, mean_loss): the plain mean of the batch F1 scores, sum(correct) / (128 sum(rows)), the plain mean of the
    batch losses (train.py:193, 198, 162)"""
    rows, correct = np.asarray(rows, np.int64), np.asarray(correct, np.int64)
    return float(np.mean(f1(tp, fp, fn))), float(int(correct.sum()) / (128.0 * int(rows.sum()))), float(np.mean(np.asarray(loss, np.float64)))


def band(z64):
    """bool array: the elements whose float64 logit is too close to 0 for an f32 forward to decide"""
    return np.abs(z64) <= BAND_REL * np.abs(z64).max()
