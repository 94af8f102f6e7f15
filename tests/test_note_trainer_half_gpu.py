"""The note trainer's bf16 step on the GPU (pvq_note_trainer_create_precision, PVQ_NOTE_BF16) against tests/note_trainer_half_ref.py:
L64 the unrounded float64 step, Q64 the float64 step with the rule's rounding points.  Bars per tensor, that module's:
  (a) max |dev - L64| <= 1.5 * max |Q64 - L64|      (b) rms(dev - Q64) <= 0.5 * rms(Q64 - L64)
tests/test_note_trainer_half.py holds Q32, the same step with float32 sums, to half of the room these leave on every case below.

Gradients (PVQ_TRAIN_GRAD): shapes C, D, F of note_model_ref.SHAPES at batches 1, 37 and 130 (C at batch 1 on row 3: that module's
docstring); A at 300, whose hidden products (300 x 1024 over 1024) split 4 ways forward and backward, so nth_gemm_finish rounds and
stores both copies; D at 481, the first case whose weight gradients split (K = pad32(481) = 512: 8 stages, 2 splits) and whose last
chunk of 32 holds row 480 alone; G (fc1 with K = 16 -> one half chunk, N = 16); I (mlp 112 -> 128, n_features 752 -> 768: both an odd
number of chunks); H (eight hidden layers) at p = 0.5 at step counters 0 and 1, the second on the weights the handle has after one step.
EVAL: logits under (a) and (b); against NoteModel(precision="bf16").rows_device on the same rows as max |dev - model| <= 1.5 * max |Q64 -
L64| and rms(dev - model) <= 0.5 * rms(Q64 - L64) (the two sum in different orders and pack K differently, so a hidden activation may
round to its neighbour: no bit equality); the loss within 5e-8 of the float64 BCE of the device's own logits.
Adam on the f32 master weights by tests/test_note_trainer_gpu.py's bar, from the device's own gradients; the shadow by bit equality of
the EVAL logits of a stepped handle and of a fresh one made from its state_dict().  Every test prints its figures before it asserts;
DESIGN.md section 6b records them."""
import ctypes as C
import functools

import numpy as np
import pytest

import note_model_ref as R
import note_test_ref as NR
import note_trainer_half_ref as HR
import note_trainer_ref as TR
import pitchvis_amd as P
from pitchvis_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 1024
SEED = HR.SEED
EVAL_CASES = [c for c in HR.GRAD_CASES if (c[0], c[1]) in (("C", 130), ("D", 37), ("F", 1), ("A", 300), ("G", 37), ("I", 37))]


def _trainer(name, max_batch=300, precision="bf16", weights=None, **hyper):
    n_bins, T, mlp, layers, _ = R.shape(name)
    h = P.NoteTrainerHyper(**dict(dict(seed=SEED), **hyper))
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), weights or R.weights(name), h, max_batch, device=0, precision=precision)


@functools.lru_cache(maxsize=None)
def _device_data(name):
    db, tg = TR.dataset(name)
    return torch.from_numpy(db.copy()).cuda(), torch.from_numpy(tg.copy()).cuda()


def _under_the_bars(tag, got, q64, l64):
    a, b, quant = HR.ratios(got, q64, l64)
    print(f"{tag}: max |L64| {float(np.abs(l64).max()):.3e}, max |Q64 - L64| {quant:.2e}; (a) {a:.3f} (bar {HR.FACTOR_A}); (b) {b:.3f} (bar {HR.FACTOR_B})")
    return a <= HR.FACTOR_A and b <= HR.FACTOR_B


@pytest.mark.parametrize("case", HR.GRAD_CASES, ids=HR.case_id)
def test_gradients_under_the_bars(case):
    name, batch, p, step = case
    d_db, d_tg = _device_data(name)
    idx = HR.batch_idx(name, batch)
    t = _trainer(name, max(batch, 300), dropout=p, lr=1e-3)
    assert t.precision == "bf16"
    if step:
        t.step(d_db, d_tg, TR.batch_idx(name, batch, seed=5))
        (_, _, want), (_, _, q) = HR.refs_at(case, t.state_dict())
    else:
        (_, _, want), (_, _, q) = HR.refs(case)
    assert t.steps == step
    d_loss = torch.zeros(1, device="cuda")
    t.step(d_db, d_tg, idx, "grad", d_loss=d_loss)
    got = t.read("grads")
    print(f"{HR.case_id(case)}: loss {float(d_loss):.7f}")
    ok = [_under_the_bars(f"{HR.case_id(case)} {k}", got[k], q[k], want[k]) for k in want]
    assert all(got[k].shape == want[k].shape for k in want)
    assert all(ok), [k for k, o in zip(want, ok) if not o]
    assert t.steps == step


@pytest.mark.parametrize("case", EVAL_CASES, ids=HR.case_id)
def test_eval_logits_and_loss(case):
    name, batch, _, _ = case
    n_bins, T, mlp, layers, _ = R.shape(name)
    d_db, d_tg = _device_data(name)
    idx = HR.batch_idx(name, batch)
    t = _trainer(name, dropout=0.5)          # (EVAL must not apply it)
    d_loss = torch.zeros(1, device="cuda")
    d_logits = torch.zeros((batch, 128), device="cuda")
    t.step(d_db, d_tg, idx, "eval", d_loss=d_loss, d_logits=d_logits)
    (_, l64, _), (_, q64, _) = HR.refs(case)
    z = d_logits.cpu().numpy()
    ok = _under_the_bars(f"{HR.case_id(case)} EVAL logits", z, q64, l64)
    m = P.NoteModel.from_state_dict(t.state_dict(), n_bins, T, device=0, precision="bf16")
    o = m.rows_device(d_db.view(1, TR.N_ROWS, n_bins), [TR.N_ROWS], TR.N_ROWS, outputs=("d_logits",))
    ref = o["d_logits"][0].cpu().numpy()[idx.astype(np.int64)].astype(np.float64)
    quant, quant_rms = float(np.abs(q64 - l64).max()), float(np.sqrt(np.mean((q64 - l64) ** 2)))
    am, bm = float(np.abs(z - ref).max()) / quant, float(np.sqrt(np.mean((z - ref) ** 2))) / quant_rms
    print(f"  against NoteModel bf16 rows_device: max difference {am:.3f} of max |Q64 - L64| (bar {HR.FACTOR_A}), rms {bm:.3f} of its rms (bar {HR.FACTOR_B}); "
          f"{int((z != ref).sum())} of {z.size} logits differ")
    y = TR.dataset(name)[1][idx.astype(np.int64)]
    own = float(NR.bce64(z, y).mean())
    print(f"  EVAL loss {float(d_loss):.9f}, float64 BCE of the device's logits {own:.9f}, difference {abs(float(d_loss) - own):.2e} (bar 5e-08)")
    assert ok
    assert am <= HR.FACTOR_A and bm <= HR.FACTOR_B
    assert abs(float(d_loss) - own) <= 5e-8
    assert t.steps == 0 and not any(g.any() for g in t.read("grads").values())     # EVAL: no backward


def _ulp32(x64):
    a = np.maximum(np.abs(x64), np.finfo(np.float32).tiny)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def _eval_logits(t, d_db, d_tg, idx):
    d_logits = torch.zeros((idx.size, 128), device="cuda")
    t.step(d_db, d_tg, idx, "eval", d_logits=d_logits)
    return d_logits.cpu().numpy()


@pytest.mark.parametrize("name", ["C", "I"])
def test_adam_on_the_master_weights_and_the_shadow(name):
    """one STEP: the f32 master weights against float64 Adam fed the device's own gradients (tests/test_note_trainer_gpu.py's bar:
    |w_dev - w_64| <= 1/2 ulp(w) + 1e-6 |dw_64|, m and v within 4 * 2^-24), then the shadow: the stepped handle's EVAL logits are those
    of a fresh handle made from its state_dict(), bit for bit, and no longer those of the initial weights.  Shape I has mlp 112 and 752
    features: both copies of every shadow matrix carry padding."""
    d_db, d_tg = _device_data(name)
    idx, held = TR.batch_idx(name, 37), TR.batch_idx(name, 130, seed=3)
    t = _trainer(name, lr=1e-3, weight_decay=5e-4, dropout=0.1)
    h = t.hyper
    z0 = _eval_logits(t, d_db, d_tg, held)
    w0, m0, v0 = t.read_flat("weights"), t.read_flat("adam_m"), t.read_flat("adam_v")
    t.step(d_db, d_tg, idx, "grad")
    g = t.read_flat("grads")
    t.step(d_db, d_tg, idx, "step")
    assert t.steps == 1 and np.array_equal(t.read_flat("grads").view(np.uint32), g.view(np.uint32))     # the same mask, the same bits
    w1, m1, v1 = t.read_flat("weights"), t.read_flat("adam_m"), t.read_flat("adam_v")
    w64, m64, v64 = TR.adam(w0, g, m0, v0, 1, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay)
    dw = np.abs(w64 - w0.astype(np.float64))
    excess = np.abs(w1 - w64) - (0.5 * _ulp32(w64) + 1e-6 * dw)
    em = float((np.abs(m1 - m64) / np.maximum(np.abs(m64), 1e-300)).max())
    ev = float((np.abs(v1 - v64) / np.maximum(np.abs(v64), 1e-300)).max())
    print(f"{name}: median |dw| {np.median(dw):.2e} = {np.median(dw / _ulp32(w64)):.0f} ulp of f32, {np.median(dw / (2.0 ** 16 * _ulp32(w64))):.3f} ulp of bf16; "
          f"worst |w_dev - w_64| - bar {excess.max():.2e}; m within {em * 2 ** 24:.2f} x 2^-24, v within {ev * 2 ** 24:.2f} x 2^-24")
    z1 = _eval_logits(t, d_db, d_tg, held)
    fresh = _trainer(name, weights=t.state_dict(), lr=1e-3, weight_decay=5e-4, dropout=0.1)
    z2 = _eval_logits(fresh, d_db, d_tg, held)
    print(f"  EVAL logits: {int((z1 != z0).sum())} of {z1.size} moved with the step; {int((z1.view(np.uint32) != z2.view(np.uint32)).sum())} differ from a fresh "
          f"handle made from the stepped state_dict")
    assert np.median(dw / _ulp32(w64)) > 100
    assert excess.max() <= 0.0
    assert em <= 4 * 2.0 ** -24 and ev <= 4 * 2.0 ** -24
    assert (z1 != z0).mean() > 0.9
    assert np.array_equal(z1.view(np.uint32), z2.view(np.uint32))


def test_determinism_and_seed():
    name = "C"
    d_db, d_tg = _device_data(name)

    def run(seed):
        t = _trainer(name, seed=seed, lr=1e-3)       # p = 0.1, the default
        for step in range(3):
            t.step(d_db, d_tg, TR.batch_idx(name, 130 - step, seed=step))
        return t.read_flat("weights"), t.read_flat("adam_v")
    (w_a, v_a), (w_b, v_b), (w_c, _) = run(SEED), run(SEED), run(SEED + 1)
    print(f"same seed: {int((w_a.view(np.uint32) != w_b.view(np.uint32)).sum())} of {w_a.size} weights differ; another seed: "
          f"{int((w_a != w_c).sum())} differ")
    assert np.array_equal(w_a.view(np.uint32), w_b.view(np.uint32)) and np.array_equal(v_a.view(np.uint32), v_b.view(np.uint32))
    assert (w_a != w_c).mean() > 0.1


def test_the_new_constructor_with_f32_is_the_old_one():
    """pvq_note_trainer_create_precision(PVQ_NOTE_F32) against pvq_note_trainer_create over two steps: equal bits; a bf16 handle differs"""
    name = "C"
    d_db, d_tg = _device_data(name)
    n_bins, T, mlp, layers, _ = R.shape(name)
    old = _trainer(name, precision="f32", lr=1e-3)
    new = _trainer(name, precision="f32", lr=1e-3)
    L = _lib.load()
    from pitchvis_amd.note_model import _c_weights
    cw, keep = _c_weights(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name))
    cp, ch, h = _lib.CNoteModelParams(n_bins, T, mlp, layers), new.hyper._c(), C.c_void_p()
    assert L.pvq_note_trainer_create_precision(0, C.byref(cp), C.byref(cw), C.byref(ch), 300, 0, C.byref(h)) == _lib.PVQ_OK
    del keep
    L.pvq_note_trainer_destroy(new._h)
    new._h = h                                       # `new` now drives (and frees) the handle of the new entry point
    assert L.pvq_note_trainer_precision(new._h) == 0 and L.pvq_note_trainer_precision(old._h) == 0
    half = _trainer(name, lr=1e-3)
    for t in (old, new, half):
        for step in range(2):
            t.step(d_db, d_tg, TR.batch_idx(name, 130 - step, seed=step))
    a, b, c = (t.read_flat("weights").view(np.uint32) for t in (old, new, half))
    ga, gb = (t.read_flat("grads").view(np.uint32) for t in (old, new))
    print(f"f32 by the old and the new entry: {int((a != b).sum())} of {a.size} weights and {int((ga != gb).sum())} gradients differ; bf16: {int((a != c).sum())} weights differ")
    assert np.array_equal(a, b) and np.array_equal(ga, gb)
    assert (a != c).mean() > 0.1


def test_values_do_not_depend_on_max_batch():
    """shape C at batch 130 on handles of max_batch 300 and 481 (other strides of the workspace, other offsets behind them), p = 0.1"""
    name, batch = "C", 130
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)

    def run(max_batch):
        t = _trainer(name, max_batch, lr=1e-3)
        t.step(d_db, d_tg, idx, "grad")
        g = t.read_flat("grads").view(np.uint32)
        t.step(d_db, d_tg, idx)
        return g, t.read_flat("weights").view(np.uint32)
    (ga, wa), (gb, wb) = run(300), run(481)
    print(f"C/130: {int((ga != gb).sum())} of {ga.size} gradient words and {int((wa != wb).sum())} weights differ between max_batch 300 and 481; "
          f"{int((ga.view(np.float32) != 0).sum())} gradients are not zero")
    assert (ga.view(np.float32) != 0).mean() > 0.5
    assert np.array_equal(ga, gb) and np.array_equal(wa, wb)


@pytest.mark.parametrize("name", ["C", "G"])
def test_nothing_else_is_written_and_a_refused_call_launches_nothing(name):
    batch = 37
    d_db0, d_tg0 = _device_data(name)
    d_db, d_tg = d_db0.clone(), d_tg0.clone()
    idx = TR.batch_idx(name, batch)
    t = _trainer(name)
    loss_all = torch.full((1 + GUARD,), 7.0, device="cuda")
    logits_all = torch.full((batch * 128 + GUARD,), 7.0, device="cuda")
    for mode in ("eval", "grad", "step"):
        t.step(d_db, d_tg, idx, mode, d_loss=loss_all[:1], d_logits=logits_all[:batch * 128])
    torch.cuda.synchronize()
    print(f"{name}/{batch}: guards changed behind d_loss {int((loss_all[1:] != 7.0).sum())}, behind d_logits {int((logits_all[batch * 128:] != 7.0).sum())}")
    assert (loss_all[1:] == 7.0).all() and (logits_all[batch * 128:] == 7.0).all() and loss_all[0] != 7.0 and (logits_all[:batch * 128] != 7.0).all()
    assert torch.equal(d_db, d_db0) and torch.equal(d_tg, d_tg0)
    for what in ("weights", "grads", "adam_m", "adam_v"):
        buf = np.full(t.n_params + GUARD, 7.0, np.float32)
        t.read_flat(what, buf[:t.n_params])
        assert (buf[t.n_params:] == 7.0).all() and np.isfinite(buf).all(), what
    # refused calls: the counter, the weights and the outputs stay
    w = t.read_flat("weights")
    loss_all.fill_(7.0)
    T = R.shape(name)[1]
    for bad in (np.array([T - 2], np.uint32), np.array([TR.N_ROWS], np.uint32), np.full(301, T - 1, np.uint32)):
        with pytest.raises(ValueError):
            t.step(d_db, d_tg, bad, "step", d_loss=loss_all[:1])
    torch.cuda.synchronize()
    assert t.steps == 1 and np.array_equal(t.read_flat("weights").view(np.uint32), w.view(np.uint32)) and (loss_all == 7.0).all()


def test_the_test_pass_counts_its_own_logits():
    """NoteTrainer.test on a bf16 handle of max_batch 300 over every admissible row of shape C (two chunks), batches of 100: the counts
    are those of the logits it returns; a batch's loss is the float64 BCE of those logits within 1e-6 of itself (the terms are f32:
    a few 2^-24 each; their sum is double)"""
    name = "C"
    d_db, d_tg = _device_data(name)
    idx = NR.shuffled(name)
    t = _trainer(name, dropout=0.5)
    d_logits = torch.full((idx.size, 128), 7.0, device="cuda")
    res = t.test(d_db, d_tg, idx, 100, d_logits=d_logits)
    z = d_logits.cpu().numpy()
    y = TR.dataset(name)[1][idx.astype(np.int64)]
    own = NR.counts(z, y, 100)
    loss = NR.batch_losses64(z, y, 100)
    print(f"C: {idx.size} rows in {res.records.size} batches; tp {res.tp.tolist()}, own {own['tp'].tolist()}; loss off by at most "
          f"{float(np.abs(res.loss - loss).max()):.2e} (bar {1e-6 * float(loss.min()):.2e})")
    for k in ("rows", "tp", "fp", "fn", "correct"):
        assert np.array_equal(getattr(res, k).astype(np.int64), own[k]), k
    assert np.array_equal(res.pitch_counts.astype(np.int64), own["pitch"])
    assert (np.abs(res.loss - loss) <= 1e-6 * loss).all()
    assert t.steps == 0 and (z != 7.0).all()


def test_it_learns_as_the_f32_handle_does():
    """the toy set of tests/test_note_trainer_gpu.py, 30 steps at lr 1e-3 with f32 and bf16 handles on the same data, seed and masks: the
    bf16 held-out EVAL loss falls, and ends within twice the gap that Q32 shows against torch's f32 on the same set-up on the CPU (one
    share for the type, one for the summation order)"""
    db, tg, train, held = HR.toy()
    d_db, d_tg = torch.from_numpy(db).cuda(), torch.from_numpy(tg).cuda()
    d_loss = torch.zeros(1, device="cuda")
    out = {}
    for precision in ("f32", "bf16"):
        t = _trainer("F", precision=precision, lr=1e-3)
        t.step(d_db, d_tg, held, "eval", d_loss=d_loss)
        before = float(d_loss)
        for ep in range(10):
            for b in P.epoch(train, 100):
                t.step(d_db, d_tg, b)
        t.step(d_db, d_tg, held, "eval", d_loss=d_loss)
        out[precision] = (before, float(d_loss))
        assert t.steps == 30
    hyper = P.NoteTrainerHyper(seed=SEED, lr=1e-3)
    cpu32, cpuq = HR.toy_cpu(False, hyper), HR.toy_cpu(True, hyper)
    gap = abs(cpuq[1] - cpu32[1])
    print(f"held-out EVAL loss, before -> after 30 steps: device f32 {out['f32'][0]:.5f} -> {out['f32'][1]:.5f}, device bf16 {out['bf16'][0]:.5f} -> {out['bf16'][1]:.5f}; "
          f"CPU f32 {cpu32[0]:.5f} -> {cpu32[1]:.5f}, CPU Q32 {cpuq[0]:.5f} -> {cpuq[1]:.5f}")
    print(f"  |bf16 - f32| on the device {abs(out['bf16'][1] - out['f32'][1]):.2e}; |Q32 - f32| on the CPU {gap:.2e} (bar: twice that, {2 * gap:.2e})")
    assert out["bf16"][1] < out["bf16"][0]
    assert abs(out["bf16"][1] - out["f32"][1]) <= 2 * gap
