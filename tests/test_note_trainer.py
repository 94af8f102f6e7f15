"""The note trainer's host side (pvq_note_trainer_* of include/pvq.h): exported symbols, the defaults, every argument check, the
host-only handle, and the dropout mask against tests/note_trainer_ref.py, the restatement of the header's text.  No GPU."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import note_model_ref as R
import note_plan_tool
import note_trainer_ref as TR
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import note_trainer as NT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pvq_note_trainer_hyper_default", "pvq_note_trainer_create", "pvq_note_trainer_destroy", "pvq_note_trainer_step",
           "pvq_note_trainer_steps", "pvq_note_trainer_param_count", "pvq_note_trainer_read", "pvq_note_trainer_dropout_keep")


ALL_SHAPES = sorted(R.SHAPES) + sorted(R.EDGE_SHAPES)


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    return note_plan_tool.build(tmp_path_factory.mktemp("note_plan"))


def _params(name="D"):
    n_bins, T, mlp, layers, _ = R.shape(name)
    return P.NoteModelParams(n_bins, T, mlp, layers)


def _host(name="D", hyper=None, max_batch=8):
    return P.NoteTrainer(_params(name), R.weights(name), hyper, max_batch, device=None)


def test_symbols_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("pvq_note_trainer_hyper", "pvq_train_mode", "pvq_train_array"):
        assert re.search(r"\}\s*%s;" % name, hdr), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.NoteTrainer is NT.NoteTrainer and P.NoteTrainerHyper is NT.NoteTrainerHyper and P.epoch is NT.epoch
    assert (NT.STEP, NT.GRAD, NT.EVAL) == (0, 1, 2)


def test_hyper_default_is_train_py():
    h = P.NoteTrainerHyper.default()
    print(h)
    # train.py:111 lr, :141-144 Adam(eps=finfo(float32).eps, weight_decay=5e-4) with torch's betas, :131-138 dropout
    assert (h.lr, h.beta1, h.beta2, h.weight_decay, h.dropout, h.seed) == (1e-5, 0.9, 0.999, 5e-4, 0.1, 0)
    assert h.eps == float(np.finfo(np.float32).eps) == 2.0 ** -23
    assert h == P.NoteTrainerHyper()


@pytest.mark.parametrize("field,value", [("lr", 0.0), ("lr", -1e-3), ("lr", float("nan")), ("lr", float("inf")), ("beta1", -0.1), ("beta1", 1.0),
                                         ("beta2", 1.0), ("beta2", float("nan")), ("eps", 0.0), ("eps", -1e-8), ("weight_decay", -1e-4),
                                         ("weight_decay", float("nan")), ("dropout", -0.1), ("dropout", 1.0), ("dropout", float("nan"))])
@pytest.mark.parametrize("device", [None, 0])
def test_create_refuses_hyper_parameters_before_any_device(field, value, device):
    """device 0 too: the checks run before a device is touched, so they answer on a machine without one"""
    h = P.NoteTrainerHyper()
    setattr(h, field, value)
    with pytest.raises(ValueError) as e:
        P.NoteTrainer(_params(), R.weights("D"), h, 8, device=device)
    print(field, value, "->", e.value)
    assert field.rstrip("12") in str(e.value)


@pytest.mark.parametrize("max_batch", [0, 4097])
def test_create_refuses_max_batch(max_batch):
    with pytest.raises(ValueError, match="max_batch"):
        P.NoteTrainer(_params(), R.weights("D"), None, max_batch, device=0)


def test_create_takes_the_edges():
    h = P.NoteTrainerHyper(lr=1e-12, beta1=0.0, beta2=0.0, eps=1e-30, weight_decay=0.0, dropout=0.0)
    for mb in (1, 4096):
        t = _host(hyper=h, max_batch=mb)
        assert t.steps == 0
    n_bins, T, mlp, layers, (_, _, n_feat) = R.SHAPES["C"]
    t = _host("C")
    assert t.n_params == 96 + mlp * (n_feat + 1) + layers * mlp * (mlp + 1) + 128 * (mlp + 1)


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_layout_and_arena_are_the_state_dict_in_its_order(name, plan_tool, tmp_path):
    """note_trainer_layout: the tensors in state_dict order, back to back, every offset a multiple of 4 floats (nt_adam and the GEMMs
    read 16 bytes at a time); note_trainer_arena: every tensor's elements at its offset.  Shape H has 22 tensors, K 16.9 M parameters."""
    n_bins, T, mlp, layers, (_, _, n_feat) = R.shape(name)
    path = str(tmp_path / "arena.f32")
    lines = [line.split() for line in note_plan_tool.run(plan_tool, "layout", n_bins, T, mlp, layers, path).splitlines()]
    want = [("conv1.weight", 80), ("conv1.bias", 16), ("fc1.weight", mlp * n_feat), ("fc1.bias", mlp)]
    for i in range(layers):
        want += [(f"layers.{i}.weight", mlp * mlp), (f"layers.{i}.bias", mlp)]
    want += [("output.weight", 128 * mlp), ("output.bias", 128)]
    assert [k for k, _ in want] == list(R.weights(name)) and [n for _, n in want] == [v.size for v in R.weights(name).values()]
    arena = np.fromfile(path, np.float32)
    os.remove(path)
    at = 0
    for j, ((k, n), line) in enumerate(zip(want, lines)):
        assert (line[0], int(line[1]), int(line[2])) == (k, at, n) and at % 4 == 0, (k, line, at)
        assert np.array_equal(arena[at:at + n], note_plan_tool.fill(1000003 * j + np.arange(n, dtype=np.int64))), k
        at += n
    assert lines[len(want)] == ["n_params", str(at)] and arena.size == at and len(lines) == len(want) + 1
    assert _host(name).n_params == at
    print(f"shape {name}: {len(want)} tensors, {at} parameters")


def _splits(m, n, k):
    """nt_splits restated from note_trainer_plan.hpp: enough workgroups for a fixed 512, at least 8 K stages of 32 per split, at most 8
    splits, splits * m * n within 4 Mi floats"""
    tiles, stages = -(-m // 64) * -(-n // 64), -(-k // 32)
    s = min(512 // tiles, stages // 8, 8)
    while s > 1 and s * m * n > 4 << 20:
        s -= 1
    return max(s, 1)


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_splits_of_every_product_of_a_step(name, plan_tool):
    """the nine kinds of product of NoteTrainer::step at batches 1, 37, 130, 300 and 4096"""
    n_bins, T, mlp, layers, (_, _, F) = R.shape(name)
    products = []
    for b in (1, 37, 130, 300, 4096):
        products += [(b, mlp, F), (b, mlp, mlp), (b, 128, mlp),            # forward: fc1, a hidden layer, the output layer
                     (128, mlp, b), (b, mlp, 128), (mlp, mlp, b), (b, mlp, mlp), (mlp, F, b), (b, F, mlp)]     # backward
    got = [int(x) for x in note_plan_tool.run(plan_tool, "splits", *[v for p in products for v in p]).split()]
    assert got == [_splits(*p) for p in products]
    for (m, n, k), s in zip(products, got):
        assert 1 <= s <= 8 and (s == 1 or (s * m * n <= 4 << 20 and -(-k // 32) >= 8 * s))
    print(f"shape {name}: splits at batch 37: {got[9:18]}")
    pinned = {"G": [1] * 9, "J": [8, 1, 1, 1, 1, 1, 1, 1, 1], "K": [1, 8, 8, 1, 1, 1, 8, 1, 8], "H": [2, 1, 1, 1, 1, 1, 1, 1, 1]}
    if name in pinned:      # worked out by hand from the rule: J's fc1 has 1024 stages in one tile, K's products over mlp 128 stages in at most 64 tiles
        assert got[9:18] == pinned[name]


def test_create_keeps_the_note_model_size_checks():
    L = _lib.load()
    w = R.weights("D")
    with pytest.raises(ValueError, match="multiple of 16"):
        P.NoteTrainer(P.NoteModelParams(180, 3, 40, 0), w, device=None)
    with pytest.raises(P.PvqError) as e:
        P.NoteTrainer(P.NoteModelParams(2000, 3, 48, 0), w, device=None)
    assert e.value.status == _lib.PVQ_ERR_UNSUPPORTED
    h = C.c_void_p()
    ch = P.NoteTrainerHyper()._c()
    assert L.pvq_note_trainer_create(-1, None, None, C.byref(ch), 8, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h
    cp = _lib.CNoteModelParams(180, 3, 48, 0)
    cw = _lib.CNoteModelWeights()
    assert L.pvq_note_trainer_create(-1, C.byref(cp), C.byref(cw), C.byref(ch), 8, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG   # null weight pointers
    assert b"null" in L.pvq_last_error()
    from pitchvis_amd.note_model import _c_weights
    cw, keep = _c_weights(_params(), w)
    assert L.pvq_note_trainer_create(-1, C.byref(cp), C.byref(cw), None, 8, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG             # null hyper
    assert b"hyper" in L.pvq_last_error()


def test_step_checks_then_no_device():
    """a host-only handle: every argument check answers PVQ_ERR_INVALID_ARG with a message; a call that passes them PVQ_ERR_NO_DEVICE"""
    L = _lib.load()
    t = _host("D", max_batch=8)     # T = 3
    T, n_rows = 3, 50
    fake = 4096                     # stands for a device pointer: no check reads it
    good = np.array([T - 1, n_rows - 1, 7, 7], np.uint32)

    def call(mode=NT.STEP, db=fake, tg=fake, rows=n_rows, idx=good, batch=None):
        p = idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx is not None else None
        st = L.pvq_note_trainer_step(t._h, mode, db, tg, rows, p, (idx.size if idx is not None else 1) if batch is None else batch, None, None, None)
        return st, L.pvq_last_error().decode()

    refused = {
        "mode": call(mode=3), "db": call(db=None), "targets": call(tg=None), "idx": call(idx=None),
        "batch 0": call(batch=0), "batch > max": call(idx=np.full(9, T - 1, np.uint32)),
        "index < T - 1": call(idx=np.array([T - 1, T - 2], np.uint32)), "index >= n_rows": call(idx=np.array([T - 1, n_rows], np.uint32)),
    }
    for what, (st, msg) in refused.items():
        print(f"{what}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_INVALID_ARG and msg.startswith("note trainer:"), what
    assert "idx[1] = 1" in refused["index < T - 1"][1] and "idx[1] = 50" in refused["index >= n_rows"][1]
    st, msg = call()
    print(f"valid call: status {st}: {msg}")
    assert st == _lib.PVQ_ERR_NO_DEVICE and "GPU" in msg
    for mode in (NT.GRAD, NT.EVAL):
        assert call(mode=mode)[0] == _lib.PVQ_ERR_NO_DEVICE
    assert t.steps == 0
    with pytest.raises(ValueError, match="outside"):
        t.step(fake, fake, [0], n_rows=n_rows)
    buf = np.empty(t.n_params, np.float32)
    assert L.pvq_note_trainer_read(t._h, 7, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_note_trainer_read(t._h, 0, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size - 1) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_note_trainer_read(t._h, 0, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size) == _lib.PVQ_ERR_NO_DEVICE


@pytest.mark.parametrize("seed,step,layer,row,col0,n,p", [
    (0, 0, 0, 0, 0, 300, 0.1), (11, 3, 2, 129, 65, 200, 0.5), (2 ** 64 - 1, 2 ** 40 + 5, 7, 4095, 4000, 96, 0.1),
    (0x123456789ABCDEF, 1, 1, 36, 1, 1023, 0.25), (5, 0, 0, 299, 63, 66, 0.999),
])
def test_dropout_keep_equals_the_restatement(seed, step, layer, row, col0, n, p):
    got = P.dropout_keep(seed, step, layer, row, col0, n, p)
    want = TR.dropout_keep(seed, step, layer, [row], np.arange(col0, col0 + n), p)[0]
    print(f"seed {seed:#x} step {step} layer {layer} row {row} cols {col0}..{col0 + n}: kept {int(got.sum())} of {n}, restatement {int(want.sum())}")
    assert got.shape == (n,) and np.array_equal(got, want)


def test_dropout_keep_refuses():
    L = _lib.load()
    out = np.empty(4, np.uint8)
    bp = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.pvq_note_trainer_dropout_keep(0, 0, 0, 0, 0, 4, 0.1, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_note_trainer_dropout_keep(0, 0, 0, 0, 0, 4, 1.0, bp) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_note_trainer_dropout_keep(0, 0, 0, 0, 0, 4, 0.0, bp) == _lib.PVQ_OK and out.all()   # p = 0 keeps everything


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_share(p):
    """10^6 draws (1000 rows x 1000 columns): the kept share within 5 standard deviations of 1 - p"""
    n = 1000
    kept = sum(int(P.dropout_keep(77, 2, 1, row, 0, n, p).sum()) for row in range(n))
    share, bar = kept / n ** 2, 5.0 * np.sqrt(p * (1.0 - p) / n ** 2)
    print(f"p = {p}: kept share {share:.6f}, 1 - p = {1 - p}, |difference| {abs(share - (1 - p)):.2e} (bar {bar:.2e})")
    assert abs(share - (1.0 - p)) <= bar


def test_mask_changes_with_step_layer_seed_and_row():
    base = P.dropout_keep(9, 4, 1, 20, 0, 4096, 0.5)
    for what, args in (("step", (9, 5, 1, 20)), ("layer", (9, 4, 2, 20)), ("seed", (10, 4, 1, 20)), ("row", (9, 4, 1, 21))):
        other = P.dropout_keep(*args, 0, 4096, 0.5)
        same = float((other == base).mean())
        print(f"another {what}: {same:.3f} of the decisions agree")
        assert 0.45 < same < 0.55, what     # independent fair coins agree on half (4096 draws: sd 0.008)
    assert np.array_equal(base, P.dropout_keep(9, 4, 1, 20, 0, 4096, 0.5))


def test_epoch_slices_the_permutation():
    perm = np.random.default_rng(3).permutation(np.arange(4, 1004))
    batches = list(P.epoch(perm, 300))
    assert [b.size for b in batches] == [300, 300, 300, 100] and all(b.dtype == np.uint32 for b in batches)
    assert np.array_equal(np.concatenate(batches), perm)
