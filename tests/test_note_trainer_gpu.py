"""The note trainer on the GPU (pvq_note_trainer_step) against tests/note_trainer_ref.py, the float64 restatement of
pitchvis_train/train.py:108-162.  Shapes C, D and F of note_model_ref.SHAPES (odd O_conv, an mlp that is no multiple of 64, zero and
three hidden layers, T = 1) at batches of 1, 37 (no multiple of 4 or 16: the K tail of the weight gradient) and 130 (one past two
64-row tiles and past the inference kernels' 128), and shape A once at the trainer's batch of 300.  The dataset is 400 dB-like rows
with soft targets; every batch holds index T - 1, index n_rows - 1 and one duplicate (a batch of 1 is index T - 1 alone).

Bars:
  * gradients: per parameter tensor within 1e-5 * max|g64| of float64 autograd, the project's magnitude bar.  torch's own f32 CPU
    autograd on the same inputs (all 13 cases below, dropout 0 and 0.5) was measured first, as a share of max|g64| per tensor: conv1.weight
    at most 5.5e-7, conv1.bias 5.6e-7, the dense weights 8.4e-7 (fc1.weight of shape A at batch 300), the dense biases 4.4e-7.  Every
    one sits inside 1e-5 with more than 4x room (2.5e-6), so the bar stands for every tensor, the conv gradients included.
  * EVAL loss within 1e-5 * max|logit| + 1e-6 * loss of nn.BCELoss in float64: the logit bar through a 1-Lipschitz function, and the
    mean's roundings.  EVAL logits within the LOGIT_REL bar (1e-5 * max|logit|) of NoteModel.rows_device on the same rows.
  * Adam: |w_dev - w_64| <= 1/2 ulp(w) + 1e-6 |dw_64| (the final rounding; the dozen roundings of the formula); m and v within
    4 * 2^-24 relative.  w_64, m_64, v_64 come from the device's own f32 gradients (PVQ_TRAIN_GRAD on the same batch: the counter
    does not move, so the mask is the same) and the previous device state.
Every test prints the figures it observes before it asserts; DESIGN.md section 6b records them."""
import functools

import numpy as np
import pytest

import note_model_ref as R
import note_trainer_ref as TR
import pitchvis_amd as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GRAD_REL, LOGIT_REL = 1e-5, 1e-5
GUARD = 1024
SEED = 11
CASES = [(n, b) for n in "CDF" for b in (1, 37, 130)] + [("A", 300)]


def _trainer(name, max_batch=300, **hyper):
    n_bins, T, mlp, layers, _ = R.SHAPES[name]
    h = P.NoteTrainerHyper(**dict(dict(seed=SEED), **hyper))
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), h, max_batch, device=0)


@functools.lru_cache(maxsize=None)
def _device_data(name):
    db, tg = TR.dataset(name)
    return torch.from_numpy(db.copy()).cuda(), torch.from_numpy(tg.copy()).cuda()


def _compare_grads(tag, got, want):
    worst = 0.0
    for k, g64 in want.items():
        top = float(np.abs(g64).max())
        err = float(np.abs(got[k].astype(np.float64) - g64).max())
        worst = max(worst, err / top)
        print(f"{tag} {k}: max|g64| {top:.3e}, max error {err:.2e} = {err / top:.2e} of it (bar {GRAD_REL:.0e})")
        assert got[k].shape == g64.shape
        assert err <= GRAD_REL * top, k
    return worst


@pytest.mark.parametrize("name,batch", CASES)
def test_gradients_match_f64_autograd(name, batch):
    T = R.SHAPES[name][1]
    db, tg = TR.dataset(name)
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)
    assert idx[0] == T - 1 and (batch == 1 or (idx[1] == TR.N_ROWS - 1 and len(set(idx.tolist())) < batch))
    t = _trainer(name, dropout=0.0)
    d_loss = torch.zeros(1, device="cuda")
    t.step(d_db, d_tg, idx, "grad", d_loss=d_loss)
    got = t.read("grads")
    loss64, _, want = TR.step(R.weights(name), db, tg, idx, T)
    print(f"shape {name} batch {batch}: loss {float(d_loss):.7f}, f64 {loss64:.7f}")
    _compare_grads(f"{name}/{batch}", got, want)
    assert t.steps == 0


@pytest.mark.parametrize("batch", [37, 130])
def test_gradients_with_dropout(batch):
    """shape C (three hidden layers), p = 0.5, at step counter 0 and, after one optimisation step, at 1: the f64 model gets the mask of
    the restatement.  A wrong mask, scale, layer index or step shows as an O(1) error."""
    name, p = "C", 0.5
    n_bins, T, mlp, layers, _ = R.SHAPES[name]
    db, tg = TR.dataset(name)
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)
    t = _trainer(name, dropout=p, lr=1e-3)
    for step in (0, 1):
        w = t.state_dict()
        t.step(d_db, d_tg, idx, "grad")
        got = t.read("grads")
        keep = TR.masks(SEED, step, layers, batch, mlp, p)
        print(f"step {step}: kept shares {[round(float(k.mean()), 3) for k in keep]}")
        _, _, want = TR.step(w, db, tg, idx, T, keep, p)
        _compare_grads(f"C/{batch}/step {step}", got, want)
        _, _, plain = TR.step(w, db, tg, idx, T)
        far = max(float(np.abs(plain[k] - want[k]).max() / np.abs(want[k]).max()) for k in want)
        print(f"  (the gradients without the mask differ by {far:.2f} of the maximum)")
        assert far > 0.05
        if step == 0:
            t.step(d_db, d_tg, TR.batch_idx(name, batch, seed=5))
            assert t.steps == 1


@pytest.mark.parametrize("name,batch", [("C", 130), ("D", 37), ("F", 1), ("A", 300)])
def test_eval_loss_and_logits(name, batch):
    n_bins, T, mlp, layers, _ = R.SHAPES[name]
    db, tg = TR.dataset(name)
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)
    t = _trainer(name, dropout=0.5)          # (EVAL must not apply it)
    d_loss = torch.zeros(1, device="cuda")
    d_logits = torch.zeros((batch, 128), device="cuda")
    t.step(d_db, d_tg, idx, "eval", d_loss=d_loss, d_logits=d_logits)
    loss64, z64, _ = TR.step(R.weights(name), db, tg, idx, T)
    top = float(np.abs(z64).max())
    got, z = float(d_loss), d_logits.cpu().numpy()
    bar = 1e-5 * top + 1e-6 * loss64
    print(f"shape {name} batch {batch}: EVAL loss {got:.8f}, BCELoss f64 {loss64:.8f}, difference {abs(got - loss64):.2e} (bar {bar:.2e}); max|logit| {top:.3f}")
    assert abs(got - loss64) <= bar
    m = P.NoteModel.from_state_dict(t.state_dict(), n_bins, T, device=0)
    o = m.rows_device(d_db.view(1, TR.N_ROWS, n_bins), [TR.N_ROWS], TR.N_ROWS, outputs=("d_logits",))
    ref = o["d_logits"][0].cpu().numpy()[idx.astype(np.int64)]
    err, e64 = float(np.abs(z - ref).max()), float(np.abs(z - z64).max())
    print(f"  logits vs NoteModel.rows_device {err:.2e}, vs f64 {e64:.2e} (bar {LOGIT_REL * top:.2e})")
    assert err <= LOGIT_REL * top and e64 <= LOGIT_REL * top
    assert t.steps == 0 and not any(g.any() for g in t.read("grads").values())     # EVAL: no backward


def _ulp32(x64):
    """the f32 spacing of the binade x lies in"""
    a = np.maximum(np.abs(x64), np.finfo(np.float32).tiny)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


@pytest.mark.parametrize("wd", [5e-4, 0.0])
def test_adam_in_isolation(wd):
    name = "C"
    d_db, d_tg = _device_data(name)
    hy = dict(lr=1e-3, weight_decay=wd, dropout=0.1)
    t = _trainer(name, **hy)
    h = t.hyper
    for step in range(3):
        idx = TR.batch_idx(name, 37 + step, seed=step)
        w0, m0, v0 = t.read_flat("weights"), t.read_flat("adam_m"), t.read_flat("adam_v")
        t.step(d_db, d_tg, idx, "grad")
        g = t.read_flat("grads")
        assert t.steps == step
        t.step(d_db, d_tg, idx, "step")
        assert np.array_equal(t.read_flat("grads").view(np.uint32), g.view(np.uint32))     # the same mask, the same bits; no decay term stored
        w1, m1, v1 = t.read_flat("weights"), t.read_flat("adam_m"), t.read_flat("adam_v")
        w64, m64, v64 = TR.adam(w0, g, m0, v0, step + 1, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay)
        dw = np.abs(w64 - w0.astype(np.float64))
        excess = np.abs(w1 - w64) - (0.5 * _ulp32(w64) + 1e-6 * dw)
        em = float((np.abs(m1 - m64) / np.maximum(np.abs(m64), 1e-300)).max())
        ev = float((np.abs(v1 - v64) / np.maximum(np.abs(v64), 1e-300)).max())
        print(f"wd {wd} step {step + 1}: median |dw| {np.median(dw):.2e} = {np.median(dw / _ulp32(w64)):.0f} ulp; worst |w_dev - w_64| - bar {excess.max():.2e}; "
              f"m within {em * 2 ** 24:.2f} x 2^-24, v within {ev * 2 ** 24:.2f} x 2^-24")
        assert np.median(dw / _ulp32(w64)) > 100      # the updates are well above an ulp
        assert excess.max() <= 0.0
        assert em <= 4 * 2.0 ** -24 and ev <= 4 * 2.0 ** -24
    assert t.steps == 3
    if wd == 0.0:
        other = _trainer(name, **dict(hy, weight_decay=5e-4))
        other.step(d_db, d_tg, TR.batch_idx(name, 37, seed=0))
        again = _trainer(name, **hy)
        again.step(d_db, d_tg, TR.batch_idx(name, 37, seed=0))
        a, b = other.read_flat("adam_m"), again.read_flat("adam_m")
        w = np.concatenate([v.reshape(-1) for v in R.weights(name).values()])
        rel = float(np.abs((a - b) - 0.1 * 5e-4 * w).max() / np.abs(0.1 * 5e-4 * w).max())
        print(f"first step: m with decay - m without = 0.1 * 5e-4 * w within {rel:.1e} of its maximum")
        assert not np.array_equal(a, b) and rel < 1e-3


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


def _toy():
    """shape F (T = 1): output k is 1 when bin 30 (k % 8) of the row is above 4 dB (the median of 60 u^4 is 3.75)"""
    n_bins = R.SHAPES["F"][0]
    db = R.db_like((TR.N_ROWS, n_bins), seed=4242)
    tg = np.ascontiguousarray(db[:, 30 * (np.arange(128) % 8)] > 4.0, np.float32)
    perm = np.random.default_rng(1).permutation(TR.N_ROWS)
    return db, tg, perm[:300].astype(np.uint32), perm[300:].astype(np.uint32)


def test_it_learns():
    """30 steps at lr 1e-3 on the toy set; the EVAL loss on the 100 held-out rows must fall.  torch f32 on the CPU, same set-up
    (Adam, weight decay 5e-4, no dropout there, batches of 100 in the same order), goes from 0.824 to 0.694."""
    db, tg, train, held = _toy()
    d_db, d_tg = torch.from_numpy(db).cuda(), torch.from_numpy(tg).cuda()
    t = _trainer("F", lr=1e-3)
    d_loss = torch.zeros(1, device="cuda")
    t.step(d_db, d_tg, held, "eval", d_loss=d_loss)
    before = float(d_loss)
    for ep in range(10):
        for b in P.epoch(train, 100):
            t.step(d_db, d_tg, b)
    t.step(d_db, d_tg, held, "eval", d_loss=d_loss)
    after = float(d_loss)
    print(f"held-out EVAL loss: {before:.4f} before, {after:.4f} after {t.steps} steps")
    assert t.steps == 30 and after < before


def test_nothing_else_is_written_and_a_refused_call_launches_nothing():
    name, batch = "C", 37
    d_db0, d_tg0 = _device_data(name)
    d_db, d_tg = d_db0.clone(), d_tg0.clone()
    idx = TR.batch_idx(name, batch)
    t = _trainer(name)
    loss_all = torch.full((1 + GUARD,), 7.0, device="cuda")
    logits_all = torch.full((batch * 128 + GUARD,), 7.0, device="cuda")
    for mode in ("eval", "grad", "step"):
        t.step(d_db, d_tg, idx, mode, d_loss=loss_all[:1], d_logits=logits_all[:batch * 128])
    torch.cuda.synchronize()
    assert (loss_all[1:] == 7.0).all() and (logits_all[batch * 128:] == 7.0).all() and loss_all[0] != 7.0 and (logits_all[:batch * 128] != 7.0).all()
    assert torch.equal(d_db, d_db0) and torch.equal(d_tg, d_tg0)
    for what in ("weights", "grads", "adam_m", "adam_v"):
        buf = np.full(t.n_params + GUARD, 7.0, np.float32)
        t.read_flat(what, buf[:t.n_params])
        assert (buf[t.n_params:] == 7.0).all() and np.isfinite(buf).all(), what
    # refused calls: the counter, the weights and the outputs stay
    w = t.read_flat("weights")
    loss_all.fill_(7.0)
    T = R.SHAPES[name][1]
    for bad in (np.array([T - 2], np.uint32), np.array([TR.N_ROWS], np.uint32), np.full(301, T - 1, np.uint32)):
        with pytest.raises(ValueError):
            t.step(d_db, d_tg, bad, "step", d_loss=loss_all[:1])
    torch.cuda.synchronize()
    assert t.steps == 1 and np.array_equal(t.read_flat("weights").view(np.uint32), w.view(np.uint32)) and (loss_all == 7.0).all()
