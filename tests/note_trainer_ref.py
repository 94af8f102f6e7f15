"""The trainer's optimisation step in float64, restated from its description (include/pvq.h: "The trainer's optimisation step";
pitchvis_train/train.py:108-162), not from the library's code: forward in training mode with the dropout mask passed in, nn.BCELoss,
torch.double autograd, and torch.optim.Adam's formula with L2 weight decay.  Also the NumPy restatement of the dropout mask hash and
the datasets and batches the tests share."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import note_model_ref as R

M64 = (1 << 64) - 1
N_ROWS = 400


def _mix_int(z):
    """splitmix64's finaliser on a Python int"""
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def _mix_array(z):
    """the same on a uint64 array (NumPy's unsigned arithmetic wraps modulo 2^64)"""
    z = z.astype(np.uint64)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return z


def dropout_keep(seed, step, layer, rows, cols, p):
    """bool [len(rows)][len(cols)]: element (row, col) of hidden layer `layer` is kept at `step`
       key = mix(mix(seed + 0x9E3779B97F4A7C15 (step + 1)) ^ layer);  u = mix(key ^ (row 2^32 + col)) >> 40;  keep = u >= floor(p 2^24)"""
    key = _mix_int(_mix_int((seed + 0x9E3779B97F4A7C15 * (step + 1)) & M64) ^ layer)
    rows = np.asarray(rows, np.uint64)[:, None]
    cols = np.asarray(cols, np.uint64)[None, :]
    u = _mix_array(np.uint64(key) ^ ((rows << np.uint64(32)) | cols)) >> np.uint64(40)
    return u >= np.uint64(int(np.floor(float(p) * 16777216.0)))


def masks(seed, step, n_layers, batch, mlp, p):
    """the masks of one step: [n_layers][batch][mlp] bool"""
    return [dropout_keep(seed, step, i, np.arange(batch), np.arange(mlp), p) for i in range(n_layers)]


def forward(d, x, keep=None, p=0.0):
    """train.py:87-99 over a dict of tensors (any dtype); keep: one [batch][mlp] bool array per hidden layer (training mode) or None"""
    h = F.conv1d(x.unsqueeze(1), d["conv1.weight"], d["conv1.bias"], stride=2)
    h = F.max_pool1d(F.relu(h), 2).flatten(1)
    h = F.relu(F.linear(h, d["fc1.weight"], d["fc1.bias"]))
    i = 0
    while f"layers.{i}.weight" in d:
        h = F.relu(F.linear(h, d[f"layers.{i}.weight"], d[f"layers.{i}.bias"]))
        if keep is not None:
            h = h * torch.from_numpy(keep[i]).to(h.dtype) * (1.0 / (1.0 - p))
        i += 1
    return F.linear(h, d["output.weight"], d["output.bias"])


def windows(db, idx, T):
    """db [n_rows][n_bins], sample indices -> [batch][T n_bins]: rows i - T + 1 .. i, flat"""
    nb = db.shape[1]
    flat = db.reshape(-1)
    return np.stack([flat[(int(i) - T + 1) * nb:(int(i) + 1) * nb] for i in idx])


def step(w, db, targets, idx, T, keep=None, p=0.0, dtype=torch.double):
    """one forward + BCELoss + backward -> (loss, logits [batch][128], gradients by state_dict name), NumPy arrays of `dtype`"""
    d = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in w.items()}
    x = torch.from_numpy(windows(db, idx, T)).to(dtype)
    y = torch.from_numpy(np.ascontiguousarray(targets[np.asarray(idx, np.int64)])).to(dtype)
    z = forward(d, x, keep, p)
    loss = torch.nn.BCELoss()(torch.sigmoid(z), y)
    loss.backward()
    return float(loss.detach()), z.detach().numpy(), {k: v.grad.numpy() for k, v in d.items()}


def adam(w, g, m, v, t, lr, beta1, beta2, eps, wd):
    """torch.optim.Adam, weight decay added to the gradient, step t (1-based), in float64 -> (w, m, v)"""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    g = g + wd * w
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    w = w - (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return w, m, v


@functools.lru_cache(maxsize=None)
def dataset(name):
    """400 dB-like rows and soft targets in [0, 1] for a shape of note_model_ref.SHAPES or EDGE_SHAPES (read-only)"""
    n_bins = R.shape(name)[0]
    db = R.db_like((N_ROWS, n_bins), seed=700 + ord(name))
    tg = np.random.default_rng(800 + ord(name)).random((N_ROWS, 128)).astype(np.float32)
    db.setflags(write=False)
    tg.setflags(write=False)
    return db, tg


def batch_idx(name, batch, seed=0):
    """a batch that holds index T - 1, index n_rows - 1 and one duplicate (batch 1: index T - 1 alone)"""
    T = R.shape(name)[1]
    if batch == 1:
        return np.array([T - 1], np.uint32)
    rng = np.random.default_rng(900 + seed + batch)
    rest = rng.integers(T - 1, N_ROWS, size=batch - 2)
    if batch > 2:
        rest[-1] = rest[0] if batch > 3 else T - 1     # the duplicate
    return np.concatenate([[T - 1, N_ROWS - 1], rest]).astype(np.uint32)
