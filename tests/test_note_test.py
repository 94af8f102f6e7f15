"""The host side of the note trainer's test pass (pvq_note_trainer_test, pvq_note_test_metrics of include/pvq.h;
pitchvis_train/train.py:164-198): exported symbols, pvq_note_test_metrics against tests/note_test_ref.py on hand-made records, the
chunk plan, every argument check on a host-only handle, random_split, and the new kernels' resources.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import note_model_ref as R
import note_plan_tool
import note_test_ref as NR
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import note_trainer as NT
from pitchvis_amd.note_trainer import random_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _host(name="D", max_batch=8):
    n_bins, T, mlp, layers, _ = R.shape(name)
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), None, max_batch, device=None)


def _records(rows):
    """[(rows, tp, fp, fn, correct, loss)] -> the record array"""
    rec = np.zeros(len(rows), NT._RECORD)
    for k, r in enumerate(rows):
        rec[k] = (*r[:5], 0, r[5])
    return rec


def test_symbols_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in ("pvq_note_trainer_test", "pvq_note_test_metrics"):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"\}\s*pvq_note_test_batch;", hdr) and "train.py:164-198" in hdr
    assert C.sizeof(_lib.CNoteTestBatch) == 32 and _lib.CNoteTestBatch.loss.offset == 24 and NT._RECORD.itemsize == 32
    assert L.pvq_abi_version() == 4   # additive
    assert P.random_split is random_split and P.NoteTestResult is NT.NoteTestResult


def test_metrics_on_hand_made_records():
    """a full batch, a batch without a single positive (tp = fp = fn = 0: F1 0), and a short last batch, which weighs as one batch in
    mean_f1 and mean_loss and by its rows in accuracy"""
    rows = [(100, 3000, 500, 700, 11600, 0.70), (100, 0, 0, 0, 12800, 0.01), (7, 100, 0, 50, 846, 0.35)]
    rec = _records(rows)
    got = P.note_test_metrics(rec)
    want = NR.scalars(*(rec[k] for k in ("rows", "tp", "fp", "fn", "correct", "loss")))
    f1 = NR.f1(rec["tp"], rec["fp"], rec["fn"])
    print(f"F1 per batch {f1}, got {got}, want {want}")
    assert f1[1] == 0.0 and f1[0] == 6000 / 7200 and f1[2] == 200 / 250
    assert want[0] == (6000 / 7200 + 0.0 + 0.8) / 3 and want[1] == (11600 + 12800 + 846) / (128 * 207)
    assert all(abs(g - w) <= 1e-15 for g, w in zip(got, want))
    # the short batch alone, and the dataclass's own columns
    res = P.NoteTestResult.from_records(rec)
    assert np.array_equal(res.f1, f1) and (res.mean_f1, res.accuracy, res.mean_loss) == got and res.pitch_f1 is None
    assert abs(P.note_test_metrics(rec[2:])[1] - 846 / (128 * 7)) <= 1e-15
    assert P.note_test_metrics(rec[1:2]) == (0.0, 1.0, 0.01)


def test_metrics_refuses():
    L = _lib.load()
    d = C.c_double()
    assert L.pvq_note_test_metrics(None, 1, C.byref(d), None, None) == _lib.PVQ_ERR_INVALID_ARG
    rec = _records([(5, 1, 1, 1, 600, 0.5)])
    p = rec.ctypes.data_as(C.POINTER(_lib.CNoteTestBatch))
    assert L.pvq_note_test_metrics(p, 0, C.byref(d), None, None) == _lib.PVQ_ERR_INVALID_ARG and L.pvq_last_error()
    assert L.pvq_note_test_metrics(p, 1, None, None, C.byref(d)) == _lib.PVQ_OK and d.value == 0.5      # every output may be null
    with pytest.raises(ValueError):
        P.note_test_metrics(_records([(0, 0, 0, 0, 0, 0.0)]))


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    return note_plan_tool.build(tmp_path_factory.mktemp("note_test_plan"), "note_test_plan_main.cpp")


def _plan(exe, n_idx, max_batch, batch):
    lines = [line.split() for line in note_plan_tool.run(exe, "plan", n_idx, max_batch, batch).splitlines()]
    chunks = [(int(a), int(b)) for tag, a, b in (x for x in lines if x[0] == "chunk")]
    rest = {x[0]: int(x[1]) for x in lines if x[0] != "chunk"}
    return chunks, rest


@pytest.mark.parametrize("n_idx,max_batch,want", [(1, 300, [(0, 1)]), (299, 300, [(0, 299)]), (300, 300, [(0, 300)]), (301, 300, [(0, 300), (300, 1)]),
                                                  (397, 300, [(0, 300), (300, 97)]), (13, 64, [(0, 13)]),
                                                  (397, 64, [(64 * i, 64) for i in range(6)] + [(384, 13)])])
def test_plan(plan_tool, n_idx, max_batch, want):
    """chunks of at most max_batch consecutive entries, back to back; they depend on n_idx and max_batch, never on the metric batch"""
    for batch in (100, 37, 1, 1000):
        chunks, rest = _plan(plan_tool, n_idx, max_batch, batch)
        print(f"n_idx {n_idx} max_batch {max_batch} batch {batch}: {chunks} {rest}")
        assert chunks == want
        assert rest == {"n_batches": -(-n_idx // batch), "rows_bytes": 56 * n_idx, "out_bytes": 32 * -(-n_idx // batch) + 1536}


def test_plan_tool_metrics_under_the_sanitizers(plan_tool):
    out = note_plan_tool.run(plan_tool, "metrics", 100, 3000, 500, 700, 11600, 0.70, 100, 0, 0, 0, 12800, 0.01, 7, 100, 0, 50, 846, 0.35).split()
    want = NR.scalars([100, 100, 7], [3000, 0, 100], [500, 0, 0], [700, 0, 50], [11600, 12800, 846], [0.70, 0.01, 0.35])
    assert all(abs(float(g) - w) <= 1e-15 for g, w in zip(out, want)), (out, want)
    assert note_plan_tool.run(plan_tool, "metrics").startswith("refused 4")


def test_argument_checks_then_no_device():
    """a host-only handle: every argument check answers PVQ_ERR_INVALID_ARG with a message; a call that passes them PVQ_ERR_NO_DEVICE"""
    L = _lib.load()
    t = _host("D", max_batch=8)     # T = 3
    T, n_rows = 3, 50
    fake = 4096                     # stands for a device pointer: no check reads it
    good = np.array([T - 1, n_rows - 1, 7, 7] * 5, np.uint32)      # 20 entries: more than max_batch, and batch 100 more than both
    rec = np.zeros(32, NT._RECORD)

    def call(db=fake, tg=fake, rows=n_rows, idx=good, n_idx=None, batch=100, out=rec):
        p = idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx is not None else None
        o = out.ctypes.data_as(C.POINTER(_lib.CNoteTestBatch)) if out is not None else None
        st = L.pvq_note_trainer_test(t._h, db, tg, rows, p, (idx.size if idx is not None else 1) if n_idx is None else n_idx, batch, o, None, None, None)
        return st, L.pvq_last_error().decode()

    refused = {
        "db": call(db=None), "targets": call(tg=None), "idx": call(idx=None), "out_batches": call(out=None), "batch 0": call(batch=0),
        "n_idx 0": call(n_idx=0), "index < T - 1": call(idx=np.array([T - 1, T - 2], np.uint32)),
        "index >= n_rows": call(idx=np.array([T - 1, n_rows], np.uint32)),
    }
    for what, (st, msg) in refused.items():
        print(f"{what}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_INVALID_ARG and msg.startswith("note trainer:"), what
    assert "idx[1] = 1" in refused["index < T - 1"][1] and "idx[1] = 50" in refused["index >= n_rows"][1]
    assert "out_batches" in refused["out_batches"][1] and "batch" in refused["batch 0"][1] and "n_idx" in refused["n_idx 0"][1]
    for batch in (100, 1, 2 ** 32 - 1):
        st, msg = call(batch=batch)
        print(f"valid call, batch {batch}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_NO_DEVICE and "GPU" in msg
    assert t.steps == 0 and not rec.view(np.uint8).any()
    with pytest.raises(ValueError, match="outside"):
        t.test(fake, fake, [0], n_rows=n_rows)
    with pytest.raises(ValueError, match="batch"):
        t.test(fake, fake, good, batch=0, n_rows=n_rows)
    with pytest.raises(P.PvqError) as e:
        t.test(fake, fake, good, n_rows=n_rows)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    assert L.pvq_note_trainer_test(None, fake, fake, n_rows, None, 0, 0, None, None, None, None) != _lib.PVQ_OK     # a null handle


@pytest.mark.parametrize("n_rows,T", [(400, 3), (400, 1), (69322 * 5 + 4, 5), (6, 5)])
def test_random_split(n_rows, T):
    total = n_rows - (T - 1)
    tr, te = random_split(n_rows, T)
    print(f"n_rows {n_rows}, T {T}: {total} admissible, {tr.size} train, {te.size} test")
    assert tr.dtype == te.dtype == np.uint32
    assert tr.size == int(0.8 * total) and te.size == total - tr.size        # train.py:56-58
    both = np.concatenate([tr, te])
    assert np.array_equal(np.sort(both), np.arange(T - 1, n_rows))           # disjoint, and together every admissible index
    again = random_split(n_rows, T, 0.8, 0)
    assert np.array_equal(again[0], tr) and np.array_equal(again[1], te)
    other = random_split(n_rows, T, seed=1)
    assert total < 8 or not np.array_equal(np.concatenate(other), both)
    assert total < 8 or not np.array_equal(both, np.arange(T - 1, n_rows))   # a permutation, not the identity
    half = random_split(n_rows, T, 0.5, 0)
    assert half[0].size == int(total * 0.5) and np.array_equal(np.concatenate(half), both)     # the fraction moves the cut alone


def test_random_split_refuses():
    for args in ((3, 5), (400, 0), (400, 3, 1.5)):
        with pytest.raises(ValueError):
            random_split(*args)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """in the manner of test_note_model.py::test_kernel_resources: the three kernels of the test pass use no scratch, and stay within
    64 VGPRs: at 64 a SIMD's 512 registers per lane hold the full 8 waves, which is where the trainer's other small kernels (under 56)
    sit.  Resource figures only."""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "note_trainer.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "x.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    kern = {k: u for k, u in usage.items() if "nt_test_" in k}
    assert all(sum(n in k for k in kern) == 1 for n in ("nt_test_rows", "nt_test_batches", "nt_test_pitches")) and len(kern) == 3, list(usage)
    for k, u in sorted(kern.items()):
        print(f"{k}: {u}")
        assert u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64, (k, u)
        assert u["LDS"] <= 2048, (k, u)      # nt_test_rows: 128 doubles and 8 counts; the other two none
