"""The note trainer's bf16 step (pvq_note_trainer_create_precision, PVQ_NOTE_BF16) as far as it goes without a GPU: the new entry
points and what they refuse, nth_splits and the 16-bit layout through a stand-alone program under ASan and UBSan against a restatement,
the float32 reference's own share of the bars on every case of tests/test_note_trainer_half_gpu.py, and what the compiler made of the
kernels.

Q32's figures (tests/note_trainer_half_ref.py states the bars and how they are read), the worst of each case's tensors and logits as (a) / (b):
    C/1 (row 3) 1.000 / 0.000    C/37 1.000 / 0.000    C/130 1.001 / 0.031    D/1 1.000 / 0.000    D/37 1.000 / 0.000    D/130 1.002 / 0.009
    F/1 1.000 / 0.000    F/37 1.000 / 0.000    F/130 1.000 / 0.001    A/300 1.016 / 0.075    D/481 1.000 / 0.060    G/37, I/37, H/37 (p = 0.5, the
    masks of steps 0 and 1) 1.000 / 0.000
and C/1 on row T - 1 = 2, which was replaced: 1.55 / 0.56.  (b) = 0.000 means that no f32 sum of the case rounds to another bf16 value
than the float64 sum does; the larger cases have a few hundred such values among a million.  Every test prints before it asserts."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import note_model_ref as R
import note_plan_tool
import note_trainer_half_ref as HR
import pitchvis_amd as P
from pitchvis_amd import _lib

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_note_trainer_create_precision", "pvq_note_trainer_precision")
ALL_SHAPES = sorted(R.SHAPES) + sorted(R.EDGE_SHAPES)
BATCHES = (1, 37, 300, 481, 4096)
Q32_ROOM = 0.5       # Q32 alone may use half of the room a factor leaves above an implementation that equals Q64


def _create(L, name, precision, dev=-1, max_batch=300, hyper=None, params=None):
    n_bins, T, mlp, layers, _ = R.shape(name)
    from pitchvis_amd.note_model import _c_weights
    par = _lib.CNoteModelParams(*(params or (n_bins, T, mlp, layers)))
    cw, keep = _c_weights(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name))
    ch = (hyper or P.NoteTrainerHyper())._c()
    h = C.c_void_p()
    st = L.pvq_note_trainer_create_precision(dev, C.byref(par), C.byref(cw), C.byref(ch), max_batch, precision, C.byref(h))
    del keep
    return st, h


def test_symbols_and_handles():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.pvq_abi_version() == 4   # additive
    assert L.pvq_note_trainer_precision(None) == 0
    for value, text in ((0, "f32"), (1, "bf16")):
        st, h = _create(L, "D", value)
        assert st == _lib.PVQ_OK and h.value
        try:
            assert L.pvq_note_trainer_precision(h) == value
            assert L.pvq_note_trainer_param_count(h) == 96 + 48 * (2144 + 1) + 128 * (48 + 1) and L.pvq_note_trainer_steps(h) == 0
            # a host-only handle of either precision: the argument checks, then PVQ_ERR_NO_DEVICE
            idx = np.array([5], np.uint32)
            up = idx.ctypes.data_as(C.POINTER(C.c_uint32))
            assert L.pvq_note_trainer_step(h, 1, None, None, 400, up, 1, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
            assert L.pvq_note_trainer_step(h, 1, idx.ctypes.data, idx.ctypes.data, 400, up, 1, None, None, None) == _lib.PVQ_ERR_NO_DEVICE
            buf = np.zeros(8, np.float32)
            assert L.pvq_note_trainer_read(h, 0, buf.ctypes.data_as(C.POINTER(C.c_float)), 8) == _lib.PVQ_ERR_INVALID_ARG
        finally:
            L.pvq_note_trainer_destroy(h)
    # refused before a device is touched, with the reason
    for dev in (-1, 0):
        st, h = _create(L, "D", 2, dev)
        msg = L.pvq_last_error().decode()
        print(f"f16 on device {dev}: status {st}, \"{msg}\"")
        assert st == _lib.PVQ_ERR_INVALID_ARG and not h.value and "f16" in msg and "loss scaling" in msg
        for bad in (3, -1, 77):
            st, h = _create(L, "D", bad, dev)
            assert st == _lib.PVQ_ERR_INVALID_ARG and not h.value and "precision" in L.pvq_last_error().decode()
    # the size corners of the f32 trainer, for both precisions
    for value in (0, 1):
        for kw in (dict(max_batch=0), dict(max_batch=4097), dict(hyper=P.NoteTrainerHyper(lr=0.0)), dict(hyper=P.NoteTrainerHyper(dropout=1.0)),
                   dict(params=(180, 3, 40, 0)), dict(params=(180, 3, 0, 0))):
            st, h = _create(L, "D", value, **kw)
            assert st == _lib.PVQ_ERR_INVALID_ARG and not h.value and L.pvq_last_error(), (value, kw)
        for kw in (dict(params=(180, 3, 4112, 0)), dict(params=(180, 3, 48, 9)), dict(params=(2000, 3, 48, 0))):
            st, h = _create(L, "D", value, **kw)
            assert st == _lib.PVQ_ERR_UNSUPPORTED and not h.value, (value, kw)
        st, h = _create(L, "D", value, max_batch=4096)
        assert st == _lib.PVQ_OK
        L.pvq_note_trainer_destroy(h)
    par = _lib.CNoteModelParams(180, 3, 48, 0)
    assert L.pvq_note_trainer_create_precision(-1, C.byref(par), None, None, 300, 1, None) == _lib.PVQ_ERR_INVALID_ARG
    # the Python face
    pd = P.NoteModelParams(*R.shape("D")[:4])
    assert P.NoteTrainer(pd, R.weights("D"), device=None).precision == "f32"
    t = P.NoteTrainer(pd, R.weights("D"), device=None, precision="bf16")
    assert t.precision == "bf16" and L.pvq_note_trainer_precision(t._h) == 1
    with pytest.raises(ValueError, match="loss scaling"):
        P.NoteTrainer(pd, R.weights("D"), device=None, precision="f16")
    with pytest.raises(ValueError):
        P.NoteTrainer(pd, R.weights("D"), device=None, precision="half")


# ---- nth_splits and the 16-bit layout, through the stand-alone program ----
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    return note_plan_tool.build(tmp_path_factory.mktemp("note_trainer_half_plan"), main="note_trainer_half_plan_main.cpp",
                                units=("note_model_plan.cpp", "note_trainer_plan.cpp"))


def _pad32(n):
    return -(-n // 32) * 32


def _r64(n):
    return -(-n // 64) * 64


def _splits(m, n, k):
    """include/pvq.h's determinism rests on it: 512 workgroups of 64 x 64, at least 4 stages of 64 k per split, at most 8 splits, the
    partial sums within 4 Mi floats"""
    blocks = -(-m // 64) * -(-n // 64)
    s = min(512 // blocks, -(-k // 64) // 4, 8)
    while s > 1 and s * m * n > 4 << 20:
        s -= 1
    return max(s, 1)


def _products(name, batch):
    """(m, n, k) of every product of a step, k padded"""
    _, _, mlp, layers, (_, _, F) = R.shape(name)
    Fp, Mp, Bp = _pad32(F), _pad32(mlp), _pad32(batch)
    out = [(batch, mlp, Fp), (batch, 128, Mp), (128, mlp, Bp), (batch, mlp, 128), (mlp, F, Bp), (batch, F, Mp)]
    if layers:
        out += [(batch, mlp, Mp), (mlp, mlp, Bp)]
    return out


def test_splits_match_the_restatement(tool):
    triples = sorted({p for name in ALL_SHAPES for b in BATCHES for p in _products(name, b)})
    got = list(map(int, note_plan_tool.run(tool, "splits", *[x for t in triples for x in t]).split()))
    want = [_splits(*t) for t in triples]
    print(f"{len(triples)} products, splits 1 .. {max(want)}: {sum(w > 1 for w in want)} split")
    assert got == want
    # the cases the GPU tests name: A at 300 splits its hidden products and no weight gradient; D's weight gradients split first at 481
    assert _splits(300, 1024, 1024) == 4 and _splits(1024, 1024, 320) == 1 and _splits(128, 1024, 320) == 1
    assert _splits(128, 48, _pad32(481)) == 2 and _splits(48, 2144, _pad32(481)) == 2 and _splits(128, 48, _pad32(300)) == 1
    assert _pad32(481) - 481 == 31      # row 480 alone in the last chunk of 32


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_layout_matches_the_restatement(name, tool):
    n_bins, T, mlp, layers, (_, _, F) = R.shape(name)
    for B in BATCHES:
        lines = note_plan_tool.run(tool, "plan", n_bins, T, mlp, layers, B).splitlines()
        got = {l.split()[0]: int(l.split()[1]) for l in lines if not l.startswith("shadow ")}
        shadow = [tuple(map(int, l.split()[1:])) for l in lines if l.startswith("shadow ")]
        Fp, Mp, Bp = _pad32(F), _pad32(mlp), _pad32(B)
        # the shadow weights: fc1, the hidden layers, the output layer, each [n][pad32(k)] then [k][pad32(n)]
        want_shadow, at, src = [], 0, 96
        for n, k in [(mlp, F)] + [(mlp, mlp)] * layers + [(128, mlp)]:
            w_at, wt_at = at, at + _r64(n * _pad32(k))
            at = wt_at + _r64(k * _pad32(n))
            want_shadow.append((src, n, k, w_at, wt_at))
            src += n * k + n
        assert shadow == want_shadow and got["shadow_total"] == at and got["n_params"] == src
        want, at = {}, 0
        hs, hts = _r64(B * Mp), _r64(mlp * Bp)
        for key, size in (("feat_at", B * Fp), ("featt_at", F * Bp), ("h_at", (layers + 1) * hs), ("ht_at", (layers + 1) * hts), ("dz_at", B * 128),
                          ("dzt_at", 128 * Bp), ("da_at", 2 * hs), ("dat_at", 2 * hts)):
            want[key] = at
            at += _r64(size)
        want.update(ws_total=at, h_stride=hs, ht_stride=hts, f_pad=Fp, mlp_pad=Mp, b_pad=Bp)
        for key, v in want.items():
            assert got[key] == v, (name, B, key, got[key], v)
        assert all(v % 64 == 0 for k, v in got.items() if k.endswith("_at") or k.endswith("_stride"))
    print(f"shape {name}: f_pad {Fp}, mlp_pad {Mp}; at batch {B}: {got['ws_total'] * 2 >> 10} KiB of 16-bit workspace, {got['shadow_total'] * 2 >> 10} KiB of shadow weights")


def test_precision_check_through_the_program(tool):
    for value, ok in ((0, True), (1, True), (2, False), (3, False), (-1, False)):
        st, _, text = note_plan_tool.run(tool, "precision", value).partition(" ")
        assert (int(st) == 0) == ok and (ok or "precision" in text), (value, st, text)


# ---- Q32's own share of the bars ----
@pytest.mark.parametrize("case", HR.GRAD_CASES, ids=HR.case_id)
def test_q32_leaves_half_of_the_room(case):
    (_, lz, lg), (_, qz, qg) = HR.refs(case)
    _, sz, sg = HR.q32(case)
    bar_a, bar_b = 1.0 + Q32_ROOM * (HR.FACTOR_A - 1.0), Q32_ROOM * HR.FACTOR_B
    for k in list(lg) + ["logits"]:
        a, b, quant = HR.ratios(sz, qz, lz) if k == "logits" else HR.ratios(sg[k], qg[k], lg[k])
        print(f"{HR.case_id(case)} {k}: max |Q64 - L64| {quant:.2e}; Q32 (a) {a:.3f} (bar {bar_a}), (b) {b:.3f} (bar {bar_b})")
        assert quant > 0.0
        assert a <= bar_a and b <= bar_b, k


def test_the_replaced_case_is_what_the_docstring_says():
    """shape C at batch 1 on row T - 1: Q32 alone passes neither half bar, which is why the case sits on row 3"""
    import note_trainer_ref as TR
    db, tg = TR.dataset("C")
    w, idx = R.weights("C"), np.array([2], np.uint32)
    l, q, s = TR.step(w, db, tg, idx, 3), HR.step_q(w, db, tg, idx, 3), HR.step_q(w, db, tg, idx, 3, dtype=torch.float32)
    worst = [max(HR.ratios(s[2][k], q[2][k], l[2][k])[i] for k in l[2]) for i in (0, 1)]
    print(f"C/1 on row 2: Q32 worst (a) {worst[0]:.3f}, worst (b) {worst[1]:.3f}")
    assert worst[0] > 1.25 and worst[1] > 0.25 and HR.BATCH_OF_ONE == {"C": 3}


# ---- the kernels ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """what DESIGN.md section 6b states of the bf16 step's kernels: none uses scratch; nth_gemm 32 KiB of LDS and at least two waves per
    SIMD (VGPRs + AGPRs <= 256)"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "note_trainer_half.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage",
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
    for kernel in ("nth_gemm", "nth_gemm_finish", "nth_features", "nth_relayout", "nth_bias_grad"):
        hits = {k: u for k, u in usage.items() if re.search(r"\d%s[A-Z]" % kernel, k)}
        assert len(hits) == 1, (kernel, list(usage))
        (k, u), = hits.items()
        print(f"{kernel}: {u}")
        assert u["ScratchSize"] == 0, (k, u)
        if kernel == "nth_gemm":
            assert u["LDS"] == 32 * 1024 and u["VGPRs"] + u.get("AGPRs", 0) <= 256 and u["Occupancy"] >= 2, (k, u)
