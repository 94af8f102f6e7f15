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
Every test prints the figures it observes before it asserts; DESIGN.md section 6b records them.

Batches above 300 (trainers with max_batch = 4096, the most the API admits; the dataset keeps its 400 rows, so indices repeat).  A
product M x N over K is split along K by nt_splits: want = min(512 / tiles, stages / 8, 8) with stages = ceil(K / 32) and 64 x 64 tiles,
then stages_per_split = ceil(stages / want) and splits = ceil(stages / stages_per_split); a split product leaves partial sums that
nt_gemm_finish adds and passes through the epilogue.  In the weight gradients (TN) K is the batch: 10 stages at 300, so none of the
cases above splits one; the first that does is 481 (16 stages).  The smallest case of each path, splits as "n x stages (last)":
  * D/481:  output.weight (128 x 48) and fc1.weight (48 x 2144, 34 tiles) 2 x 8 (8); stage 15 holds row 480 alone.
  * D/2049: 65 stages; both weight gradients 8 x 9 (2), stage 64 holds row 2048 alone; 33 row tiles forward.
  * C/2049: three hidden layers.  output.weight and layers.*.weight (2 x 2 tiles) 8 x 9 (2); fc1.weight (80 x 2496, 78 tiles: 512 / 78 = 6)
    6 x 11 (10); the forward fc1 (2049 x 80 over 2496: 66 tiles, 78 stages) 7 x 12 (6).
  * C/4096: 128 stages, exactly 64 row tiles, every reduction over the batch 4096 terms long.  output.weight and layers.*.weight
    8 x 16 (16); fc1.weight 6 x 22 (18); the forward fc1 (128 tiles) 4 x 20 (18).
  * F/2049: T = 1, mlp 64: one column tile in every hidden product.  All three weight gradients 8 x 9 (2); layers.0.weight is one tile.
  * E/513:  mlp 256, 17 stages.  output.weight and layers.0.weight (256 x 256, 16 tiles) 2 x 9 (8); fc1.weight (256 x 7040, 440 tiles)
    unsplit over its 17 stages.
  * A/1025: mlp 1024, 33 stages, one past 16 row tiles.  layers.*.weight (256 tiles) 2 x 17 (16); output.weight (32 tiles) 4 x 9 (6);
    fc1.weight (1264 tiles) unsplit.
  * A/300 with p = 0.5: the hidden products (300 x 1024 over 1024: 80 tiles, 32 stages) are 4 x 8 (8) forward (NT, E_HIDDEN) and
    backward (NN, E_GATE), so the mask and the gate are applied by nt_gemm_finish; no weight gradient splits.
  * C/2049 with p = 0.5: the splits of C/2049; the mask's row numbers run to 2048 (applied inside nt_gemm: K = 80 does not split).
The bars are the ones above.  torch's f32 CPU autograd against float64 on these inputs, worst share of max|g64| as conv1.weight /
conv1.bias / dense weights / dense biases, measured before the bar was trusted:
    D/481  5.6e-7 / 3.8e-7 / 5.2e-7 / 1.1e-7        D/2049 1.8e-6 / 1.1e-6 / 4.7e-7 / 1.2e-7
    C/2049 2.4e-6 / 2.2e-6 / 5.1e-7 / 1.1e-7        C/4096 3.5e-6 / 3.7e-6 / 4.4e-7 / 1.2e-7
    F/2049 1.8e-6 / 1.0e-6 / 4.0e-7 / 1.3e-7        E/513  1.6e-6 / 8.4e-7 / 5.5e-7 / 1.3e-7
    A/1025 3.6e-6 / 2.0e-6 / 5.4e-7 / 1.3e-7
    A/300, p = 0.5 (step 0)  8.8e-7 / 6.3e-7 / 8.3e-7 / 1.9e-7        C/2049, p = 0.5 (step 0)  1.5e-6 / 1.5e-6 / 3.0e-7 / 1.0e-7
The f32 losses differ from float64 by at most 1.9e-7, the f32 logits by at most 7.6e-7 of max|logit|.  The worst, conv1.bias of C/4096
at 3.7e-6, leaves 2.7 x room under 1e-5; no case exceeds 5e-6 (2 x room), so none was replaced by a smaller batch and GRAD_REL
stands at 1e-5 for every tensor.

The edges of the admitted sizes: shapes G - K of note_model_ref.EDGE_SHAPES (trainers of max_batch 300), all at batch 37, G and K at 1, G
and J at 130.  What they reach: G: L = 9 < 256 threads in nt_features and nt_conv_grad, O_pool = 1 (one of a channel's 16 threads
has a term), fc1 with K = 16 (the second chunk of its only stage is zero fill) and N = 16 (fetch_cols' x < X bound), no hidden layer.
H: eight hidden layers, 22 tensors in the arena, dropout layer keys 0 .. 7.  I: mlp 112 (a column tile of three strips), O_pool 47.
J: L = 8192 (32 KiB of dynamic LDS), fc1 forward 8 x 128 stages over K = 32752 in one tile, fc1.weight 16 x 32752 (512 column tiles).
K: mlp 4096: the hidden products 8 x 16 stages forward and backward, layers.0.weight 4096 x 4096 (4096 tiles, unsplit), dfeat 37 x 32 over
4096 split 8 ways, 16.9 M parameters under nt_adam.  torch's f32 CPU autograd against float64 on these inputs, as above:
    G/37   8.4e-8 / 8.8e-8 / 2.3e-7 / 1.3e-7        H/37   3.5e-7 / 2.7e-7 / 4.5e-7 / 4.5e-7
    I/37   1.3e-7 / 1.2e-7 / 2.2e-7 / 1.5e-7        J/37   6.7e-7 / 4.4e-7 / 2.8e-7 / 1.5e-7
    K/37   8.3e-8 / 7.9e-8 / 2.2e-7 / 1.4e-7        G/1    1.0e-7 / 8.4e-8 / 1.9e-7 / 1.6e-7
    G/130  6.2e-8 / 6.2e-8 / 3.6e-7 / 1.0e-7        J/130  1.8e-6 / 1.3e-6 / 4.8e-7 / 1.1e-7
    K/1 (row 1)  6.4e-7 / 6.2e-7 / 1.4e-6 / 1.4e-6
    H/37, p = 0.5  step 0: 5.2e-7 / 4.1e-7 / 7.3e-7 / 3.7e-7;  the mask of step 1 on the initial weights: 4.7e-7 / 7.2e-7 / 6.1e-7 / 6.5e-7
The f32 losses differ from float64 by at most 1.5e-7, the f32 logits by at most 4.5e-7 of max|logit|.  The worst is conv1.weight of J/130
at 1.8e-6 (5.5 x room); none exceeds 5e-6 but one: K at batch 1 on row T - 1 = 0, the batch batch_idx() gives, measured 9.6e-3 / 6.1e-3 /
2.0e-1 / 2.0e-1.  That is no rounding figure: unit 3083 of layers.0 has a float64 pre-activation of +1.5e-7 on that row, a 4096-term sum
whose f32 value (torch's: -5.1e-7) has the other sign, so its ReLU gate, and with it a fifth of the largest layers.0.bias gradient, is
not decidable in f32.  The standing rule replaces such a case by a smaller batch; below 1 there is none, so K at batch 1 takes row 1
instead (BATCH_OF_ONE; smallest float64 |pre-activation| 2.5e-4, smallest pool difference 6.6e-2).  Row 0 is in every larger batch too:
in K/37 torch's f32 GEMM keeps the sign (2.2e-7 above), so by the rule the case stands as it is, but the device's k order may not; the
other new cases' smallest float64 margins (pre-activations, conv outputs, pool differences) are at least 4.6e-6 (a pool pair of J)."""
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
# shapes G - K of note_model_ref.EDGE_SHAPES (the module docstring)
EDGE_CASES = [(n, 37) for n in "GHIJK"] + [("G", 1), ("K", 1), ("G", 130), ("J", 130)]
# K at batch 1 takes row 1, not row T - 1 = 0: a ReLU of row 0 is undecidable in f32 (the module docstring)
BATCH_OF_ONE = {"K": 1}
SPLIT_CASES = [("D", 481), ("D", 2049), ("C", 2049), ("C", 4096), ("F", 2049), ("E", 513), ("A", 1025)]      # (the module docstring)
MAX_BATCH = 4096


def _batch_idx(name, batch, seed=0):
    if batch == 1 and name in BATCH_OF_ONE:
        return np.array([BATCH_OF_ONE[name]], np.uint32)
    return TR.batch_idx(name, batch, seed)


def _trainer(name, max_batch=300, **hyper):
    n_bins, T, mlp, layers, _ = R.shape(name)
    h = P.NoteTrainerHyper(**dict(dict(seed=SEED), **hyper))
    return P.NoteTrainer(P.NoteModelParams(n_bins, T, mlp, layers), R.weights(name), h, max_batch, device=0)


@functools.lru_cache(maxsize=None)
def _device_data(name):
    db, tg = TR.dataset(name)
    return torch.from_numpy(db.copy()).cuda(), torch.from_numpy(tg.copy()).cuda()


def _max_batch(batch):
    """the trainers of the cases up to 300 keep their max_batch of 300; above, the most the API admits"""
    return 300 if batch <= 300 else MAX_BATCH


@functools.lru_cache(maxsize=None)
def _ref64(name, batch):
    """TR.step on the initial weights without dropout, once per case: (loss, logits, gradients), read-only"""
    db, tg = TR.dataset(name)
    loss, z, g = TR.step(R.weights(name), db, tg, _batch_idx(name, batch), R.shape(name)[1])
    for a in (z, *g.values()):
        a.setflags(write=False)
    return loss, z, g


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


@pytest.mark.parametrize("name,batch", CASES + SPLIT_CASES + EDGE_CASES)
def test_gradients_match_f64_autograd(name, batch):
    T = R.shape(name)[1]
    d_db, d_tg = _device_data(name)
    idx = _batch_idx(name, batch)
    assert idx[0] == (BATCH_OF_ONE.get(name, T - 1) if batch == 1 else T - 1)
    assert batch == 1 or (idx[1] == TR.N_ROWS - 1 and len(set(idx.tolist())) < batch)
    t = _trainer(name, _max_batch(batch), dropout=0.0)
    d_loss = torch.zeros(1, device="cuda")
    t.step(d_db, d_tg, idx, "grad", d_loss=d_loss)
    got = t.read("grads")
    loss64, _, want = _ref64(name, batch)
    print(f"shape {name} batch {batch}: loss {float(d_loss):.7f}, f64 {loss64:.7f}")
    _compare_grads(f"{name}/{batch}", got, want)
    assert t.steps == 0


# (the first two keep the ids they had when shape C was the only one)
@pytest.mark.parametrize("name,batch,max_batch", [pytest.param("C", 37, 300, id="37"), pytest.param("C", 130, 300, id="130"),
                                                  pytest.param("A", 300, MAX_BATCH, id="A-300"), pytest.param("C", 2049, MAX_BATCH, id="C-2049"),
                                                  pytest.param("H", 37, 300, id="H-37")])
def test_gradients_with_dropout(name, batch, max_batch):
    """p = 0.5, at step counter 0 and, after one optimisation step, at 1: the f64 model gets the mask of the restatement.  A wrong
    mask, scale, layer index, row number or step shows as an O(1) error.  Shape C (three hidden layers) applies the mask inside nt_gemm,
    at 2049 with row numbers up to 2048; shape A at 300 splits its hidden products, so nt_gemm_finish applies mask and gate.  Shape H
    has eight hidden layers, every one masked: layer keys 0 .. 7."""
    p = 0.5
    n_bins, T, mlp, layers, _ = R.shape(name)
    db, tg = TR.dataset(name)
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)
    t = _trainer(name, max_batch, dropout=p, lr=1e-3)
    for step in (0, 1):
        w = t.state_dict()
        t.step(d_db, d_tg, idx, "grad")
        got = t.read("grads")
        keep = TR.masks(SEED, step, layers, batch, mlp, p)
        print(f"step {step}: kept shares {[round(float(k.mean()), 3) for k in keep]}")
        _, _, want = TR.step(w, db, tg, idx, T, keep, p)
        _compare_grads(f"{name}/{batch}/step {step}", got, want)
        _, _, plain = TR.step(w, db, tg, idx, T)
        far = max(float(np.abs(plain[k] - want[k]).max() / np.abs(want[k]).max()) for k in want)
        print(f"  (the gradients without the mask differ by {far:.2f} of the maximum)")
        assert far > 0.05
        if step == 0:
            t.step(d_db, d_tg, TR.batch_idx(name, batch, seed=5))
            assert t.steps == 1


@pytest.mark.parametrize("name,batch", [("C", 130), ("D", 37), ("F", 1), ("A", 300), ("C", 4096), ("D", 2049), ("G", 130), ("J", 130)])
def test_eval_loss_and_logits(name, batch):
    n_bins, T, mlp, layers, _ = R.shape(name)
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)
    t = _trainer(name, _max_batch(batch), dropout=0.5)          # (EVAL must not apply it)
    d_loss = torch.zeros(1, device="cuda")
    d_logits = torch.zeros((batch, 128), device="cuda")
    t.step(d_db, d_tg, idx, "eval", d_loss=d_loss, d_logits=d_logits)
    loss64, z64, _ = _ref64(name, batch)
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


def _check_adam_step(t, d_db, d_tg, idx, step, tag):
    """step `step` (0-based) of trainer t on batch idx, against TR.adam on the device's own gradients and previous state"""
    h = t.hyper
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
    print(f"{tag} step {step + 1}: median |dw| {np.median(dw):.2e} = {np.median(dw / _ulp32(w64)):.0f} ulp; worst |w_dev - w_64| - bar {excess.max():.2e}; "
          f"m within {em * 2 ** 24:.2f} x 2^-24, v within {ev * 2 ** 24:.2f} x 2^-24")
    assert np.median(dw / _ulp32(w64)) > 100      # the updates are well above an ulp
    assert excess.max() <= 0.0
    assert em <= 4 * 2.0 ** -24 and ev <= 4 * 2.0 ** -24


@pytest.mark.parametrize("name", ["H", "K"])
def test_adam_steps_an_arena_at_the_edges(name):
    """one step through the bars of test_adam_in_isolation: H has eight hidden layers (22 tensors in the arena), K 16.9 M parameters;
    the stepped H trainer's state_dict builds a NoteModel"""
    n_bins, T, mlp, layers, _ = R.shape(name)
    d_db, d_tg = _device_data(name)
    t = _trainer(name, lr=1e-3, weight_decay=5e-4, dropout=0.1)
    assert t.n_params == 96 + mlp * (R.sizes(n_bins, T)[3] + 1) + layers * mlp * (mlp + 1) + 128 * (mlp + 1)
    _check_adam_step(t, d_db, d_tg, TR.batch_idx(name, 37), 0, name)
    assert t.steps == 1
    if name == "H":
        sd = t.state_dict()
        m = P.NoteModel.from_state_dict(sd, n_bins, T, device=0)
        assert (m.params.mlp_size, m.params.mlp_layers) == (mlp, layers) and len(sd) == 6 + 2 * layers
        assert all(np.array_equal(sd[k], v) for k, v in t.split(t.read_flat("weights")).items())


@pytest.mark.parametrize("wd", [5e-4, 0.0])
def test_adam_in_isolation(wd):
    name = "C"
    d_db, d_tg = _device_data(name)
    hy = dict(lr=1e-3, weight_decay=wd, dropout=0.1)
    t = _trainer(name, **hy)
    for step in range(3):
        _check_adam_step(t, d_db, d_tg, TR.batch_idx(name, 37 + step, seed=step), step, f"wd {wd}")
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


def test_gradients_depend_on_neither_the_handle_nor_the_workspace():
    """shape C at 2049 (every weight gradient and the forward fc1 split, p = 0.1): two fresh handles give equal bits, and so does a
    handle whose workspace was sized for 2049 rows and not 4096 (another h_stride, other offsets of everything behind it)."""
    name, batch = "C", 2049
    d_db, d_tg = _device_data(name)
    idx = TR.batch_idx(name, batch)

    def run(max_batch):
        t = _trainer(name, max_batch)
        t.step(d_db, d_tg, idx, "grad")
        return t.read_flat("grads").view(np.uint32)
    a, b, c = run(MAX_BATCH), run(MAX_BATCH), run(batch)
    print(f"C/2049 grad: {int((a != b).sum())} of {a.size} gradient words differ between two handles of max_batch {MAX_BATCH}, "
          f"{int((a != c).sum())} against a handle of max_batch {batch}; {int((a.view(np.float32) != 0).sum())} are not zero")
    assert (a.view(np.float32) != 0).mean() > 0.5
    assert np.array_equal(a, b) and np.array_equal(a, c)


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
    _check_nothing_else_is_written("C", 37)


def test_nothing_else_is_written_around_the_smallest_buffers():
    """shape G: 16 features, mlp 16, no hidden layer: a stray store lands outside soonest"""
    _check_nothing_else_is_written("G", 37)


def _check_nothing_else_is_written(name, batch):
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
    T = R.shape(name)[1]
    for bad in (np.array([T - 2], np.uint32), np.array([TR.N_ROWS], np.uint32), np.full(301, T - 1, np.uint32)):
        with pytest.raises(ValueError):
            t.step(d_db, d_tg, bad, "step", d_loss=loss_all[:1])
    torch.cuda.synchronize()
    assert t.steps == 1 and np.array_equal(t.read_flat("weights").view(np.uint32), w.view(np.uint32)) and (loss_all == 7.0).all()



def test_nothing_else_is_written_at_the_largest_batch():
    """shape C at 4096 rows of a handle of max_batch 4096, the top of the range: the outputs are written in full and nothing
    behind them; one row more is refused with nothing launched."""
    name, batch = "C", MAX_BATCH
    d_db0, d_tg0 = _device_data(name)
    d_db, d_tg = d_db0.clone(), d_tg0.clone()
    idx = TR.batch_idx(name, batch)
    t = _trainer(name, MAX_BATCH)
    loss_all = torch.full((1 + GUARD,), 7.0, device="cuda")
    logits_all = torch.full((batch * 128 + GUARD,), 7.0, device="cuda")
    for mode in ("eval", "grad", "step"):
        loss_all.fill_(7.0)
        logits_all.fill_(7.0)
        t.step(d_db, d_tg, idx, mode, d_loss=loss_all[:1], d_logits=logits_all[:batch * 128])
        torch.cuda.synchronize()
        unwritten = int((logits_all[:batch * 128] == 7.0).sum())
        print(f"C/{batch} {mode}: loss {float(loss_all[0]):.6f}, {unwritten} of {batch * 128} logits unwritten, guards "
              f"{int((loss_all[1:] != 7.0).sum())} + {int((logits_all[batch * 128:] != 7.0).sum())} words changed")
        assert (loss_all[1:] == 7.0).all() and (logits_all[batch * 128:] == 7.0).all()
        assert loss_all[0] != 7.0 and torch.isfinite(loss_all[0]) and unwritten == 0 and torch.isfinite(logits_all).all()
    assert t.steps == 1
    assert torch.equal(d_db, d_db0) and torch.equal(d_tg, d_tg0)
    for what in ("weights", "grads", "adam_m", "adam_v"):
        buf = np.full(t.n_params + GUARD, 7.0, np.float32)
        t.read_flat(what, buf[:t.n_params])
        assert (buf[t.n_params:] == 7.0).all() and np.isfinite(buf).all(), what
    # one row more than max_batch: the counter, the weights and the outputs stay
    w = t.read_flat("weights")
    loss_all.fill_(7.0)
    logits_all.fill_(7.0)
    T = R.SHAPES[name][1]
    with pytest.raises(ValueError):
        t.step(d_db, d_tg, np.full(batch + 1, T - 1, np.uint32), "step", d_loss=loss_all[:1], d_logits=logits_all)
    torch.cuda.synchronize()
    assert t.steps == 1 and np.array_equal(t.read_flat("weights").view(np.uint32), w.view(np.uint32))
    assert (loss_all == 7.0).all() and (logits_all == 7.0).all()
