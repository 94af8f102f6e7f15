"""The host side of the note trainer's epochs and checkpoints (pvq_note_trainer_epoch, pvq_note_epoch_order, pvq_note_trainer_write,
pvq_note_trainer_set_steps of include/pvq.h; pitchvis_train/train.py:147-162): exported symbols, the epoch order as a permutation and
against a pure-Python restatement of the header's rule, the epoch plan, every argument check on host-only handles of both
precisions, and the new kernel's resources.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import note_model_ref as R
import note_plan_tool
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd.note_trainer import epoch_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NEW =("pvq_note_trainer_epoch", "pvq_note_epoch_order", "pvq_note_trainer_write", "pvq_note_trainer_set_steps")
SIZES = (1, 2, 3, 5, 64, 65, 300, 1000, 4097, 65537)
EPOCHS = (0, 1, 7)
M64 = 2 ** 64 - 1


def _host(precision, name="D", max_batch=8):
    n_bins, T, mlp, layers, _ = R.shape(name)
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), None, max_batch, device=None, precision=precision)


# the rule of include/pvq.h, restated
def _mix(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def _order(seed, epoch, n):
    """[order(0), .., order(n - 1)] and the longest walk"""
    if n == 1:
        return [0], 0
    b = max(2, (n - 1).bit_length())
    b += b & 1
    h = b // 2
    mask = (1 << h) - 1
    base = _mix(_mix((seed + 0x9E3779B97F4A7C15 * (epoch + 1)) & M64) ^ 0x45504F4348)
    keys = [_mix(base ^ i) for i in range(4)]

    def one_pass(x):
        l, r = x >> h, x & mask
        for k in keys:
            l, r = r, l ^ (_mix(k ^ r) & mask)
        return (l << h) | r

    out, longest = [], 0
    for j in range(n):
        x, walk = one_pass(j), 1
        while x >= n:
            x, walk = one_pass(x), walk + 1
        out.append(x)
        longest = max(longest, walk)
    return out, longest


def test_symbols_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert "train.py:147-162" in hdr and "0x45504F4348" in hdr
    assert L.pvq_abi_version() == 4   # additive
    assert P.epoch_order is epoch_order
    for name in ("epoch", "fit", "checkpoint", "load_checkpoint", "write_flat", "set_steps"):
        assert callable(getattr(P.NoteTrainer, name)), name


@pytest.mark.parametrize("n", SIZES)
def test_epoch_order_is_a_permutation(n):
    seen = []
    for e in EPOCHS:
        o = epoch_order(5, e, n)
        assert o.dtype == np.uint32 and o.size == n
        assert np.array_equal(np.sort(o), np.arange(n, dtype=np.uint32)), (n, e)
        seen.append(o)
    if n >= 64:
        moved = [float((o != np.arange(n)).mean()) for o in seen]
        print(f"n {n}: share of elements that moved at epochs {EPOCHS}: {moved}")
        assert min(moved) > 0.9          # a shuffle, not nearly the identity: a random permutation moves all but about one element


@pytest.mark.parametrize("n", SIZES)
def test_epoch_order_is_the_headers_rule(n):
    """the pure-Python restatement; n = 65537 (the longest walks) at one epoch only, to stay quick"""
    for seed, e in ((0, 0), (5, 1), (M64, 7), (1234567890123456789, M64)) if n <= 4097 else ((5, 7),):
        want, longest = _order(seed, e, n)
        got = epoch_order(seed, e, n)
        print(f"n {n}, seed {seed}, epoch {e}: longest walk {longest} passes")
        assert got.tolist() == want, (n, seed, e)
        assert longest <= 200            # 2^b <= 4 n: a pass lands below n with probability >= 1 / 4


@pytest.mark.parametrize("n", [2, 5, 65, 1000])
def test_epoch_order_slices_agree_with_the_whole(n):
    whole = epoch_order(9, 3, n)
    for first, count in ((0, n), (0, 1), (n - 1, 1), (n // 2, n - n // 2), (1, n - 2), (n, 0), (0, 0)):
        part = epoch_order(9, 3, n, first, count)
        assert part.size == count and np.array_equal(part, whole[first:first + count]), (n, first, count)
    assert np.array_equal(epoch_order(9, 3, n, n // 2), whole[n // 2:])        # count defaults to the rest


@pytest.mark.parametrize("n", [64, 65, 300, 4097])
def test_epoch_order_depends_on_seed_and_epoch(n):
    a = epoch_order(0, 0, n)
    assert np.array_equal(a, epoch_order(0, 0, n))
    for seed, e in ((1, 0), (0, 1), (0, 2), (2 ** 63, 0)):
        b = epoch_order(seed, e, n)
        same = float((a == b).mean())
        print(f"n {n}: seed {seed} epoch {e} agrees with (0, 0) in {same:.4f} of the positions")
        assert same < 0.25, (n, seed, e)     # two independent permutations agree in about 1 / n of them


def test_epoch_order_refuses():
    L = _lib.load()
    out = np.zeros(8, np.uint32)
    p = out.ctypes.data_as(C.POINTER(C.c_uint32))
    bad = {"n 0": (0, 0, 0, p), "n above 2^32": (2 ** 32 + 1, 0, 1, p), "first + count > n": (8, 4, 5, p), "first > n": (8, 9, 0, p),
           "count wraps": (8, 1, M64, p), "null out": (8, 0, 8, None)}
    for what, (n, first, count, o) in bad.items():
        st = L.pvq_note_epoch_order(0, 0, n, first, count, o)
        msg = L.pvq_last_error().decode()
        print(f"{what}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_INVALID_ARG and msg.startswith("note epoch order:"), what
    assert not out.any()
    assert L.pvq_note_epoch_order(0, 0, 8, 0, 8, p) == _lib.PVQ_OK and sorted(out.tolist()) == list(range(8))
    assert L.pvq_note_epoch_order(0, 0, 2 ** 32, 2 ** 32 - 3, 3, p) == _lib.PVQ_OK      # the largest n: b = 32
    for args in ((0, 0, 0), (0, 0, 8, 4, 5), (0, 0, 8, -1, 2)):
        with pytest.raises(ValueError):
            epoch_order(*args)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_argument_checks_then_no_device(precision):
    """a host-only handle: every argument check answers PVQ_ERR_INVALID_ARG with a message; a call that passes them PVQ_ERR_NO_DEVICE,
    and the counter stays"""
    L = _lib.load()
    t = _host(precision, "D", max_batch=8)     # T = 3
    T, n_rows = 3, 50
    fake = 4096                                # stands for a device pointer: no check reads it
    good = np.array([T - 1, n_rows - 1, 7, 7] * 5, np.uint32)      # 20 entries: three batches of 8
    losses = np.zeros(32, np.float32)
    mean = C.c_double(-1.0)

    def call(db=fake, tg=fake, rows=n_rows, idx=good, n_idx=None, batch=8, out=losses):
        p = idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx is not None else None
        o = out.ctypes.data_as(C.POINTER(C.c_float)) if out is not None else None
        st = L.pvq_note_trainer_epoch(t._h, db, tg, rows, p, (idx.size if idx is not None else 1) if n_idx is None else n_idx, batch, 3, 1, o,
                                      C.byref(mean), None)
        return st, L.pvq_last_error().decode()

    refused = {
        "db": call(db=None), "targets": call(tg=None), "idx": call(idx=None), "batch 0": call(batch=0), "batch above max_batch": call(batch=9),
        "n_idx 0": call(n_idx=0), "n_idx above 2^25": call(n_idx=2 ** 25 + 1), "index < T - 1": call(idx=np.array([T - 1, T - 2], np.uint32)),
        "index >= n_rows": call(idx=np.array([T - 1, n_rows], np.uint32)),
        "the last index": call(idx=np.concatenate([good, [n_rows]]).astype(np.uint32)),
    }
    for what, (st, msg) in refused.items():
        print(f"{what}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_INVALID_ARG and msg.startswith("note trainer:"), what
    assert "idx[1] = 1" in refused["index < T - 1"][1] and "idx[1] = 50" in refused["index >= n_rows"][1] and "idx[20] = 50" in refused["the last index"][1]
    assert "max_batch (8)" in refused["batch 0"][1] and "max_batch (8)" in refused["batch above max_batch"][1] and "n_idx" in refused["n_idx 0"][1]
    for kw in (dict(), dict(batch=1), dict(out=None), dict(idx=good[:1])):
        st, msg = call(**kw)
        print(f"valid call {kw and list(kw)}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_NO_DEVICE and "GPU" in msg
    assert t.steps == 0 and not losses.any() and mean.value == -1.0

    # pvq_note_trainer_write
    n = t.n_params
    w = np.zeros(n + 1, np.float32)
    fp = w.ctypes.data_as(C.POINTER(C.c_float))
    wrong = {"null host": (_lib.TRAIN_WEIGHTS, None, n), "count below": (_lib.TRAIN_WEIGHTS, fp, n - 1), "count above": (_lib.TRAIN_ADAM_V, fp, n + 1),
             "count 0": (_lib.TRAIN_ADAM_M, fp, 0), "array 4": (4, fp, n), "array -1": (-1, fp, n)}
    for what, (arr, host, count) in wrong.items():
        st = L.pvq_note_trainer_write(t._h, arr, host, count)
        msg = L.pvq_last_error().decode()
        print(f"write, {what}: status {st}: {msg}")
        assert st == _lib.PVQ_ERR_INVALID_ARG and msg.startswith("note trainer:"), what
    for arr in (_lib.TRAIN_WEIGHTS, _lib.TRAIN_GRADS, _lib.TRAIN_ADAM_M, _lib.TRAIN_ADAM_V):
        assert L.pvq_note_trainer_write(t._h, arr, fp, n) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
    assert L.pvq_note_trainer_write(None, 0, fp, n) not in (_lib.PVQ_OK, _lib.PVQ_ERR_NO_DEVICE)      # a null handle
    with pytest.raises(ValueError, match="count"):
        t.write_flat("adam_m", w)
    with pytest.raises(P.PvqError) as e:
        t.write_flat("adam_m", w[:n])
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE

    # pvq_note_trainer_set_steps: the counter is the handle's own, a host-only handle keeps one too
    assert L.pvq_note_trainer_set_steps(None, 1) != _lib.PVQ_OK
    for steps in (2 ** 53, M64):
        assert L.pvq_note_trainer_set_steps(t._h, steps) == _lib.PVQ_ERR_INVALID_ARG and "2^53" in L.pvq_last_error().decode()
    assert t.steps == 0
    t.set_steps(2 ** 53 - 1)
    assert t.steps == 2 ** 53 - 1
    t.set_steps(41)
    assert t.steps == 41
    assert call()[0] == _lib.PVQ_ERR_NO_DEVICE and call(batch=0)[0] == _lib.PVQ_ERR_INVALID_ARG and t.steps == 41
    for bad in (-1, 2 ** 64, 2 ** 53):
        with pytest.raises(ValueError):
            t.set_steps(bad)

    # the Python face
    with pytest.raises(ValueError, match="outside"):
        t.epoch(fake, fake, [0], 4, n_rows=n_rows)
    with pytest.raises(ValueError, match="batch"):
        t.epoch(fake, fake, good, 0, n_rows=n_rows)
    with pytest.raises(ValueError, match="n_idx"):
        t.epoch(fake, fake, [], 4, n_rows=n_rows)
    with pytest.raises(P.PvqError) as e:
        t.fit(fake, fake, good, 2, 8, n_rows=n_rows)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE and t.steps == 41


def test_load_checkpoint_checks_before_it_writes():
    """a checkpoint of another precision, other hyper-parameters, another model or a wrong length is refused with a ValueError before
    any array is written (a host-only handle would answer a write with PVQ_ERR_NO_DEVICE)"""
    t = _host("f32")
    n = t.n_params
    from dataclasses import asdict
    z = np.zeros(n, np.float32)
    ck = {"weights": z, "adam_m": z, "adam_v": z, "steps": 3, "hyper": asdict(t.hyper), "precision": "f32",
          "params": {"n_bins": 180, "t_frames": 3, "mlp_size": 48, "mlp_layers": 0}}
    for what, change in {"precision": {"precision": "bf16"}, "hyper": {"hyper": dict(asdict(t.hyper), lr=1e-3)}, "length": {"adam_v": z[:-1]},
                         "model": {"params": dict(ck["params"], mlp_size=64)}, "steps": {"steps": 2 ** 53}}.items():
        with pytest.raises(ValueError) as e:
            t.load_checkpoint(dict(ck, **change))
        print(f"{what}: {e.value}")
    with pytest.raises(P.PvqError) as e:
        t.load_checkpoint(ck)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE and t.steps == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """in the manner of test_note_test.py::test_kernel_resources: the epoch's unit holds one kernel, which uses no scratch and no LDS
    and stays within 64 VGPRs (the full 8 waves of a SIMD).  Resource figures only."""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "note_epoch.hip")
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
    print(usage)
    assert len(usage) == 1 and "ne_gather" in next(iter(usage)), list(usage)
    u = next(iter(usage.values()))
    assert u["ScratchSize"] == 0 and u["LDS"] == 0 and u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy"] == 8, u


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    return note_plan_tool.build(tmp_path_factory.mktemp("note_epoch_plan"), "note_epoch_plan_main.cpp")


@pytest.mark.parametrize("n_idx,batch,want", [(1, 64, (1, 1)), (64, 64, (1, 64)), (65, 64, (2, 1)), (150, 37, (5, 2)), (5, 1, (5, 1)), (20000, 300, (67, 200)),
                                              (2 ** 25, 4096, (8192, 4096))])
def test_plan_under_the_sanitizers(plan_tool, n_idx, batch, want):
    got = {k: int(v) for k, v in (line.split() for line in note_plan_tool.run(plan_tool, "plan", n_idx, batch).splitlines())}
    print(f"n_idx {n_idx}, batch {batch}: {got}")
    nb, last = want
    assert (got["n_batches"], got["last_rows"]) == (nb, last) == (-(-n_idx // batch), n_idx - (nb - 1) * batch)
    # the three device arrays and the two host arrays lie back to back, in words, and fill their buffers
    assert (got["idx_at"], got["order_at"], got["loss_at"], got["device_bytes"]) == (0, n_idx, 2 * n_idx, 4 * (2 * n_idx + nb))
    assert (got["h_idx_at"], got["h_loss_at"], got["host_bytes"]) == (0, n_idx, 4 * (n_idx + nb))


def test_order_and_mean_under_the_sanitizers(plan_tool):
    for n in (1, 2, 65, 4097):
        out = note_plan_tool.run(plan_tool, "order", 5, 7, n, 0, n).split()
        assert [int(v) for v in out] == epoch_order(5, 7, n).tolist()
    assert note_plan_tool.run(plan_tool, "order", 5, 7, 8, 4, 5).startswith("refused 4")
    vals = [0.7, 0.25, 1e-8, 3.5]
    f = np.array(vals, np.float32)
    want = float(((np.float64(f[0]) + np.float64(f[1])) + np.float64(f[2]) + np.float64(f[3])) / 4)
    assert float(note_plan_tool.run(plan_tool, "mean", *vals)) == want
