"""The trainer's optimisation step (pitchvis_train/train.py:108-162) on the GPU: pvq_note_trainer_* of include/pvq.h.  ``NoteTrainer``
owns the parameters, their gradients and Adam's moments on the device and runs forward (training mode), BCE loss, backward and Adam on
a batch of rows gathered by index from a dataset in device memory: the ``[n_rows][n_bins]`` dB rows and ``[n_rows][128]`` targets
``train_dataset_streams`` leaves there.  ``state_dict()`` is what ``NoteModel.from_state_dict`` takes.  ``NoteTrainer.test`` is the test
pass that follows the last epoch (train.py:164-198): micro-F1 per batch, accuracy and loss, counted on the device.  ``NoteTrainer.epoch``
and ``fit`` are the epoch loop (train.py:147-162) with its shuffle made on the device (``epoch_order`` is that order on the host);
``checkpoint`` and ``load_checkpoint`` stop a run and continue it with the same bits."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .note_model import N_OUT, NoteModelParams, _c_weights

_fp = C.POINTER(C.c_float)
STEP, GRAD, EVAL = _lib.TRAIN_STEP, _lib.TRAIN_GRAD, _lib.TRAIN_EVAL
_MODES = {"step": STEP, "grad": GRAD, "eval": EVAL}
_ARRAYS = {"weights": _lib.TRAIN_WEIGHTS, "grads": _lib.TRAIN_GRADS, "adam_m": _lib.TRAIN_ADAM_M, "adam_v": _lib.TRAIN_ADAM_V}


@dataclass
class NoteTrainerHyper:
    """train.py:111,131-144: lr, torch.optim.Adam's betas, eps = finfo(float32).eps, L2 weight decay, dropout; the mask's seed"""
    lr: float = 1e-5
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1.1920928955078125e-7
    weight_decay: float = 5e-4
    dropout: float = 0.1
    seed: int = 0

    @staticmethod
    def default() -> "NoteTrainerHyper":
        h = _lib.CNoteTrainerHyper()
        _lib.load().pvq_note_trainer_hyper_default(C.byref(h))
        return NoteTrainerHyper(h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.dropout, int(h.seed))

    def _c(self) -> _lib.CNoteTrainerHyper:
        return _lib.CNoteTrainerHyper(self.lr, self.beta1, self.beta2, self.eps, self.weight_decay, self.dropout, int(self.seed) & (2 ** 64 - 1))


def dropout_keep(seed: int, step: int, layer: int, row: int, col0: int, n: int, dropout: float) -> np.ndarray:
    """the dropout mask of include/pvq.h on the host: bool [n], True where element (row, col0 + j) of hidden layer ``layer`` is kept"""
    from . import _check
    out = np.empty(max(int(n), 1), np.uint8)
    _check(_lib.load().pvq_note_trainer_dropout_keep(int(seed), int(step), int(layer), int(row), int(col0), int(n), float(dropout),
                                                     out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out[:int(n)].astype(bool)


def epoch(indices, batch: int):
    """the batches of one epoch: consecutive slices of ``indices``, a permutation the caller seeded (the last one may be short)"""
    idx = np.ascontiguousarray(indices, np.uint32)
    for at in range(0, idx.size, int(batch)):
        yield idx[at:at + int(batch)]


def epoch_order(seed: int, epoch: int, n: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
    """``order(first) .. order(first + count - 1)`` (uint32) of the permutation of ``[0, n)`` in which ``NoteTrainer.epoch`` visits ``n``
    samples at ``(seed, epoch)``: the counter-based rule of include/pvq.h, on the host by ``pvq_note_epoch_order``.  ``count`` defaults
    to the rest of the order."""
    n, first = int(n), int(first)
    count = max(n - first, 0) if count is None else int(count)
    if min(n, first, count) < 0:
        raise ValueError("note epoch order: n, first and count must not be negative")
    out = np.empty(max(count, 1), np.uint32)
    m = 2 ** 64 - 1
    st = _lib.load().pvq_note_epoch_order(int(seed) & m, int(epoch) & m, n, first, count, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((_lib.load().pvq_last_error() or b"").decode())
    from . import _check
    _check(st)
    return out[:count]


def random_split(n_rows: int, t_frames: int, train_fraction: float = 0.8, seed: int = 0):
    """``(train_idx, test_idx)``: a seeded permutation of the admissible sample indices ``t_frames - 1 .. n_rows - 1``, cut at
    ``int(total * train_fraction)`` (train.py:56-61).  Stands for ``random_split`` and the loaders' shuffle, as ``epoch`` stands for the
    ``DataLoader``.  Host only."""
    first = int(t_frames) - 1
    total = int(n_rows) - first
    if first < 0 or total < 1:
        raise ValueError("random_split: n_rows must exceed t_frames - 1 >= 0")
    if not 0.0 <= train_fraction <= 1.0:
        raise ValueError("random_split: train_fraction must lie in [0, 1]")
    perm = (np.random.default_rng(seed).permutation(total) + first).astype(np.uint32)
    cut = int(total * train_fraction)
    return perm[:cut], perm[cut:]


_RECORD = np.dtype([(n, np.uint32) for n in ("rows", "tp", "fp", "fn", "correct", "_pad")] + [("loss", np.float64)])   # pvq_note_test_batch
assert _RECORD.itemsize == C.sizeof(_lib.CNoteTestBatch) == 32


def _f1(tp, fp, fn) -> np.ndarray:
    """2 tp / (2 tp + fp + fn) per entry, 0 where that denominator is 0"""
    num = 2.0 * np.asarray(tp, np.float64)
    den = num + np.asarray(fp, np.float64) + np.asarray(fn, np.float64)
    return np.divide(num, den, out=np.zeros_like(den), where=den > 0)


def note_test_metrics(records: np.ndarray):
    """``(mean_f1, accuracy, mean_loss)`` of an array of batch records (``NoteTestResult.records``): what train.py:193-198 prints, by
    ``pvq_note_test_metrics``"""
    from . import _check
    rec = np.ascontiguousarray(records, _RECORD).reshape(-1)
    f1, acc, loss = C.c_double(), C.c_double(), C.c_double()
    st = _lib.load().pvq_note_test_metrics(rec.ctypes.data_as(C.POINTER(_lib.CNoteTestBatch)), rec.size, C.byref(f1), C.byref(acc), C.byref(loss))
    if st == _lib.PVQ_ERR_INVALID_ARG:
        raise ValueError((_lib.load().pvq_last_error() or b"").decode())
    _check(st)
    return f1.value, acc.value, loss.value


@dataclass
class NoteTestResult:
    """One test pass (train.py:164-198).  Per batch: ``rows``, ``tp``, ``fp``, ``fn``, ``correct`` (uint32), ``loss`` (the batch's mean
    BCE) and ``f1``, views of ``records`` (the ``pvq_note_test_batch`` array) but for ``f1``; ``mean_f1``, ``accuracy`` and
    ``mean_loss`` as train.py prints them; ``pitch_counts`` ``[128][3]`` tp / fp / fn per output over the whole pass and ``pitch_f1``
    ``[128]`` (both None when the pass was run without them)."""
    records: np.ndarray
    rows: np.ndarray
    tp: np.ndarray
    fp: np.ndarray
    fn: np.ndarray
    correct: np.ndarray
    loss: np.ndarray
    f1: np.ndarray
    mean_f1: float
    accuracy: float
    mean_loss: float
    pitch_counts: Optional[np.ndarray]
    pitch_f1: Optional[np.ndarray]

    @staticmethod
    def from_records(records: np.ndarray, pitch_counts: Optional[np.ndarray] = None) -> "NoteTestResult":
        r = records
        mean_f1, accuracy, mean_loss = note_test_metrics(r)
        c = pitch_counts
        return NoteTestResult(r, r["rows"], r["tp"], r["fp"], r["fn"], r["correct"], r["loss"], _f1(r["tp"], r["fp"], r["fn"]), mean_f1, accuracy,
                              mean_loss, c, None if c is None else _f1(c[:, 0], c[:, 1], c[:, 2]))


class NoteTrainer:
    """``weights``: the initial ``state_dict`` (names as for ``NoteModel``).  ``device=None``: a host-only handle (argument checks
    work; ``step`` raises: no CPU fallback).  ``max_batch`` sizes the workspace once."""

    def __init__(self, params: NoteModelParams, weights, hyper: Optional[NoteTrainerHyper] = None, max_batch: int = 300, device: Optional[int] = 0,
                 precision: str = "f32"):
        """``precision``: "f32" (the default, pvq_note_trainer_create) or "bf16": mixed-precision training under the rule of
        include/pvq.h (pvq_note_trainer_create_precision): bf16 operands, f32 sums, f32 master weights, gradients and moments.
        "f16" is refused: the gradients underflow it without loss scaling."""
        from . import _check
        from .note_model import _precision
        self._L = _lib.load()
        self.precision = str(precision)
        code = _precision(self.precision)
        self.params = params
        self.hyper = hyper or NoteTrainerHyper()
        self.max_batch = int(max_batch)
        self.device = device
        self._h = C.c_void_p()
        cw, keep = _c_weights(params, weights)   # (keep: alive until the library has copied them)
        cp = _lib.CNoteModelParams(params.n_bins, params.t_frames, params.mlp_size, params.mlp_layers)
        ch = self.hyper._c()
        dev = -1 if device is None else int(device)
        if self.precision == "f32":
            st = self._L.pvq_note_trainer_create(dev, C.byref(cp), C.byref(cw), C.byref(ch), self.max_batch, C.byref(self._h))
        else:
            st = self._L.pvq_note_trainer_create_precision(dev, C.byref(cp), C.byref(cw), C.byref(ch), self.max_batch, code, C.byref(self._h))
        del keep
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        self.n_params = int(self._L.pvq_note_trainer_param_count(self._h))
        self.window_len, _, _, self.n_features = params.sizes()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pvq_note_trainer_destroy(h)
            self._h = None

    @property
    def steps(self) -> int:
        """completed ``step`` calls in mode "step": Adam's t - 1 and the step the dropout mask is keyed by"""
        return int(self._L.pvq_note_trainer_steps(self._h))

    def _dataset_rows(self, d_db, d_targets, n_rows: Optional[int]) -> int:
        """the layout checks of a dataset given as tensors -> n_rows"""
        if hasattr(d_db, "shape"):
            if d_db.dim() != 2 or d_db.shape[1] != self.params.n_bins or not d_db.is_contiguous() or d_db.element_size() != 4:
                raise ValueError("d_db must be a contiguous f32 tensor [n_rows][n_bins]")
            if n_rows is None:
                n_rows = int(d_db.shape[0])
            if n_rows > d_db.shape[0]:
                raise ValueError("d_db holds fewer than n_rows rows")
        if n_rows is None:
            raise ValueError("n_rows is needed with a raw pointer")
        if hasattr(d_targets, "shape"):
            if d_targets.dim() != 2 or d_targets.shape[1] != N_OUT or not d_targets.is_contiguous() or d_targets.element_size() != 4:
                raise ValueError("d_targets must be a contiguous f32 tensor [n_rows][128]")
            if n_rows > d_targets.shape[0]:
                raise ValueError("d_targets holds fewer than n_rows rows")
        return int(n_rows)

    def step(self, d_db, d_targets, idx, mode="step", d_loss=None, d_logits=None, *, n_rows: Optional[int] = None, stream=None) -> None:
        """One step on the batch ``idx`` (host sequence of sample indices, T - 1 <= i < n_rows).  ``d_db`` ``[n_rows][n_bins]`` and
        ``d_targets`` ``[n_rows][128]``: contiguous f32 device tensors (or raw pointers, with ``n_rows``).  ``mode``: "step" (dropout,
        backward, Adam), "grad" (the same without Adam and without advancing the counter) or "eval" (no dropout, forward and loss only).
        ``d_loss`` (one float) and ``d_logits`` (``[len(idx)][128]``): optional device tensors to fill.  Asynchronous on ``stream``."""
        from . import _check, _ptr, _stream_handle
        n_rows = self._dataset_rows(d_db, d_targets, n_rows)
        ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        if hasattr(d_logits, "numel") and (d_logits.numel() < ix.size * N_OUT or not d_logits.is_contiguous() or d_logits.element_size() != 4):
            raise ValueError("d_logits must be a contiguous f32 tensor [len(idx)][128]")
        if hasattr(d_loss, "numel") and (d_loss.numel() < 1 or d_loss.element_size() != 4):
            raise ValueError("d_loss must be an f32 tensor of one element")
        st = self._L.pvq_note_trainer_step(self._h, _MODES[mode] if isinstance(mode, str) else int(mode), _ptr(d_db), _ptr(d_targets), int(n_rows),
                                           ix.ctypes.data_as(C.POINTER(C.c_uint32)), ix.size, _ptr(d_loss), _ptr(d_logits), _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def test(self, d_db, d_targets, idx, batch: int = 100, d_logits=None, pitches: bool = True, *, n_rows: Optional[int] = None,
             stream=None) -> NoteTestResult:
        """The test pass (train.py:164-198) over ``idx`` (host sequence of sample indices; the caller's permutation is the shuffle) in
        batches of ``batch`` (the last may be short; not bounded by ``max_batch``: it shapes only the metric).  Dropout is off; the
        prediction is logit > 0, the label target > 0.5.  ``d_logits`` (``[len(idx)][128]``): optional device tensor to fill.
        Synchronous: waits on ``stream`` once.  Leaves ``steps``, the weights, the gradients and the moments as they are."""
        from . import _check, _ptr, _stream_handle
        n_rows = self._dataset_rows(d_db, d_targets, n_rows)
        ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        if hasattr(d_logits, "numel") and (d_logits.numel() < ix.size * N_OUT or not d_logits.is_contiguous() or d_logits.element_size() != 4):
            raise ValueError("d_logits must be a contiguous f32 tensor [len(idx)][128]")
        batch = int(batch)
        if not 0 <= batch < 2 ** 32:
            raise ValueError("note trainer: the test batch must lie in 1 .. 2^32 - 1")
        rec = np.zeros(-(-ix.size // batch) if batch > 0 and ix.size else 1, _RECORD)
        counts = np.zeros((N_OUT, 3), np.uint32) if pitches else None
        st = self._L.pvq_note_trainer_test(self._h, _ptr(d_db), _ptr(d_targets), n_rows, ix.ctypes.data_as(C.POINTER(C.c_uint32)), ix.size, batch,
                                           rec.ctypes.data_as(C.POINTER(_lib.CNoteTestBatch)),
                                           counts.ctypes.data_as(C.POINTER(C.c_uint32)) if pitches else None, _ptr(d_logits), _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        return NoteTestResult.from_records(rec, counts)

    def epoch(self, d_db, d_targets, idx, batch: int, shuffle_seed: int = 0, epoch: int = 0, *, n_rows: Optional[int] = None, stream=None):
        """One epoch (train.py:147-162) over the train split ``idx`` (host sequence of sample indices): batch ``k`` is
        ``idx[epoch_order(shuffle_seed, epoch, len(idx))[k * batch:(k + 1) * batch]]`` (the last may be short and still counts), each
        batch one ``step`` in mode "step" with that call's bits.  ``idx`` goes to the device once; the order is made and every batch
        gathered there.  Returns ``(losses, mean_loss)``: the f32 loss of every batch, and their sum in double over their number, what
        train.py:162 prints.  Synchronous: waits on ``stream`` once.  ``steps`` advances by ``len(losses)``."""
        from . import _check, _ptr, _stream_handle
        n_rows = self._dataset_rows(d_db, d_targets, n_rows)
        ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        batch = int(batch)
        if not 0 <= batch < 2 ** 32:
            raise ValueError("note trainer: batch must lie in 1 .. max_batch")
        losses = np.zeros(-(-ix.size // batch) if batch > 0 and ix.size else 1, np.float32)
        mean = C.c_double()
        m = 2 ** 64 - 1
        st = self._L.pvq_note_trainer_epoch(self._h, _ptr(d_db), _ptr(d_targets), n_rows, ix.ctypes.data_as(C.POINTER(C.c_uint32)), ix.size, batch,
                                            int(shuffle_seed) & m, int(epoch) & m, losses.ctypes.data_as(_fp), C.byref(mean), _stream_handle(stream))
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)
        return losses, mean.value

    def fit(self, d_db, d_targets, train_idx, epochs: int, batch: int, shuffle_seed: int = 0, start_epoch: int = 0, *, n_rows: Optional[int] = None,
            stream=None) -> np.ndarray:
        """train.py:147-162: ``epochs`` epochs ``start_epoch ..`` over ``train_idx``, each in its own order.  Returns the mean loss of
        every epoch (f64).  A run stopped after epoch ``e`` continues from ``checkpoint()`` with ``start_epoch=e + 1``."""
        ix = np.ascontiguousarray(train_idx, np.uint32).reshape(-1)
        return np.array([self.epoch(d_db, d_targets, ix, batch, shuffle_seed, e, n_rows=n_rows, stream=stream)[1]
                         for e in range(int(start_epoch), int(start_epoch) + int(epochs))], np.float64)

    def write_flat(self, what: str, flat) -> None:
        """the inverse of ``read_flat``: one f32 array of ``n_params`` values in state_dict order becomes "weights", "grads", "adam_m" or
        "adam_v" (``pvq_note_trainer_write``; a bf16 handle's 16-bit shadow follows its weights).  Synchronises."""
        from . import _check
        a = np.ascontiguousarray(flat, np.float32).reshape(-1)
        st = self._L.pvq_note_trainer_write(self._h, _ARRAYS[what], a.ctypes.data_as(_fp), a.size)
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def set_steps(self, steps: int) -> None:
        """sets ``steps``: Adam's t - 1 and the step the dropout mask is keyed by"""
        from . import _check
        steps = int(steps)
        if not 0 <= steps < 2 ** 64:
            raise ValueError("note trainer: steps must lie below 2^53")
        st = self._L.pvq_note_trainer_set_steps(self._h, steps)
        if st == _lib.PVQ_ERR_INVALID_ARG:
            raise ValueError((self._L.pvq_last_error() or b"").decode())
        _check(st)

    def checkpoint(self) -> dict:
        """What continues this run with the same bits: "weights", "adam_m", "adam_v" (flat f32 arrays in state_dict order), "steps",
        "hyper" (the ``NoteTrainerHyper`` fields), "precision" and "params" (n_bins, t_frames, mlp_size, mlp_layers).  The gradients are
        left out: every step writes them anew.  Arrays, ints, floats, strings and two flat dicts of them: ``pickle`` stores it."""
        from dataclasses import asdict
        p = self.params
        return {"weights": self.read_flat("weights"), "adam_m": self.read_flat("adam_m"), "adam_v": self.read_flat("adam_v"), "steps": self.steps,
                "hyper": asdict(self.hyper), "precision": self.precision,
                "params": {"n_bins": p.n_bins, "t_frames": p.t_frames, "mlp_size": p.mlp_size, "mlp_layers": p.mlp_layers}}

    def load_checkpoint(self, ck: dict) -> None:
        """Puts a ``checkpoint()`` back: weights, both moments and ``steps``.  The handle must have been made with the checkpoint's
        model sizes, hyper-parameters and precision (ValueError otherwise): they are fixed when a handle is made, and a run
        continues with the same bits only under the same ones.  Checked in full before anything is written."""
        from dataclasses import asdict
        p = self.params
        mine = {"n_bins": p.n_bins, "t_frames": p.t_frames, "mlp_size": p.mlp_size, "mlp_layers": p.mlp_layers}
        if "params" in ck and {k: int(v) for k, v in dict(ck["params"]).items()} != mine:
            raise ValueError(f"note trainer: the checkpoint is of a model {dict(ck['params'])}, the handle of {mine}")
        if str(ck["precision"]) != self.precision:
            raise ValueError(f"note trainer: the checkpoint is of precision {ck['precision']}, the handle of {self.precision}")
        if dict(ck["hyper"]) != asdict(self.hyper):
            raise ValueError(f"note trainer: the checkpoint's hyper-parameters {dict(ck['hyper'])} are not the handle's {asdict(self.hyper)}")
        arrays = {k: np.ascontiguousarray(ck[k], np.float32).reshape(-1) for k in ("weights", "adam_m", "adam_v")}
        for k, a in arrays.items():
            if a.size != self.n_params:
                raise ValueError(f"note trainer: the checkpoint's {k} holds {a.size} values, the handle {self.n_params} parameters")
        steps = int(ck["steps"])
        if not 0 <= steps < 2 ** 53:
            raise ValueError("note trainer: steps must lie below 2^53")
        for k, a in arrays.items():
            self.write_flat(k, a)
        self.set_steps(steps)

    def read_flat(self, what: str = "weights", out: Optional[np.ndarray] = None) -> np.ndarray:
        """"weights", "grads", "adam_m" or "adam_v" as one f32 array in state_dict order.  Synchronises."""
        from . import _check
        if out is None:
            out = np.empty(self.n_params, np.float32)
        _check(self._L.pvq_note_trainer_read(self._h, _ARRAYS[what], out.ctypes.data_as(_fp), out.size))
        return out

    def split(self, flat: np.ndarray) -> dict:
        """a flat array in state_dict order -> state_dict names -> arrays in PyTorch's shapes (views)"""
        p = self.params
        shapes = [("conv1.weight", (16, 1, 5)), ("conv1.bias", (16,)), ("fc1.weight", (p.mlp_size, self.n_features)), ("fc1.bias", (p.mlp_size,))]
        for i in range(p.mlp_layers):
            shapes += [(f"layers.{i}.weight", (p.mlp_size, p.mlp_size)), (f"layers.{i}.bias", (p.mlp_size,))]
        shapes += [("output.weight", (N_OUT, p.mlp_size)), ("output.bias", (N_OUT,))]
        out, at = {}, 0
        for name, shape in shapes:
            n = int(np.prod(shape))
            out[name] = flat[at:at + n].reshape(shape)
            at += n
        assert at == flat.size
        return out

    def read(self, what: str = "weights") -> dict:
        return self.split(self.read_flat(what))

    def state_dict(self) -> dict:
        """the parameters, exactly what ``NoteModel.from_state_dict`` takes"""
        return self.read("weights")
