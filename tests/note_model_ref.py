"""The note model in float64, restated from its description (include/pvq.h; pitchvis_train/train.py:67-99): a window of T dB frames,
flattened -> conv1d(1 -> 16, kernel 5, stride 2) -> ReLU -> max_pool1d(2) -> flatten (channel-major) -> linear -> ReLU ->
layers x (linear -> ReLU) -> linear(., 128) -> sigmoid, as torch.nn.functional calls over a dict of tensors.  Also the seeded
weights (uniform +-1/sqrt(fan_in), what nn.Linear and nn.Conv1d default to) and dB-like inputs (60 u^4) the tests share."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# name: (n_bins, T, mlp_size, mlp_layers, (O_conv, O_pool, n_features))
SHAPES = {
    "A": (252, 5, 1024, 2, (628, 314, 5024)),   # the trainer's model; 314 pooled positions are no multiple of a K stage
    "B": (252, 3, 1024, 2, (376, 188, 3008)),   # the viewer's T
    "C": (210, 3, 80, 3, (313, 156, 2496)),     # odd O_conv: the pool drops a position; mlp no multiple of 64
    "D": (180, 3, 48, 0, (268, 134, 2144)),     # no hidden layer, narrow mlp
    "E": (588, 3, 256, 1, (880, 440, 7040)),    # wide window (1764 values per row)
    "F": (252, 1, 64, 1, (124, 62, 992)),       # no history rows
}
# the edges of the sizes note_model_check admits (3 .. 1024 bins, T 1 .. 8 with L >= 8, mlp 16 .. 4096, 0 .. 8 hidden layers); a table
# of its own, so that every parametrisation over SHAPES keeps its cases
EDGE_SHAPES = {
    "G": (3, 3, 16, 0, (3, 1, 16)),             # the smallest of everything: L = 9, one pooled position, K = 16 in fc1, N = 16
    "H": (183, 1, 32, 8, (90, 45, 720)),        # O_pool mod 4 = 1; eight hidden layers (dropout layer keys 0 .. 7)
    "I": (191, 1, 112, 1, (94, 47, 752)),       # O_pool mod 4 = 3; mlp = 64 + 48: a column tile of three strips, 7 K chunks
    "J": (1024, 8, 16, 1, (4094, 2047, 32752)),  # the widest window, L = 8192: 512 K stages, 3 chunks in the last
    "K": (12, 1, 4096, 1, (4, 2, 32)),          # the widest mlp: 64 column tiles, 256 K chunks; O_pool = 2 < 4, L = 12 < 19
}


def shape(name):
    """the tuple of a name of SHAPES or EDGE_SHAPES"""
    return SHAPES[name] if name in SHAPES else EDGE_SHAPES[name]


def sizes(n_bins, t_frames):
    L = t_frames * n_bins
    o_conv = (L - 5) // 2 + 1
    return L, o_conv, o_conv // 2, 16 * (o_conv // 2)


@functools.lru_cache(maxsize=None)
def weights(name, seed=1234):
    """state_dict-named f32 arrays, uniform +-1/sqrt(fan_in)"""
    n_bins, T, mlp, layers, _ = shape(name)
    n_feat = sizes(n_bins, T)[3]
    rng = np.random.default_rng(seed + sum(map(ord, name)))

    def u(shape, fan_in):
        return ((2.0 * rng.random(shape) - 1.0) / np.sqrt(fan_in)).astype(np.float32)
    w = {"conv1.weight": u((16, 1, 5), 5), "conv1.bias": u((16,), 5), "fc1.weight": u((mlp, n_feat), n_feat), "fc1.bias": u((mlp,), n_feat)}
    for i in range(layers):
        w[f"layers.{i}.weight"] = u((mlp, mlp), mlp)
        w[f"layers.{i}.bias"] = u((mlp,), mlp)
    w["output.weight"] = u((128, mlp), mlp)
    w["output.bias"] = u((128,), mlp)
    return w


def db_like(shape, seed):
    """60 u^4: mostly near 0 dB with a few loud bins, like a VQT frame"""
    return (60.0 * np.random.default_rng(seed).random(shape) ** 4).astype(np.float32)


def logits64(w, windows):
    """windows [rows][L] -> float64 logits [rows][128]"""
    d = {k: torch.from_numpy(np.asarray(v)).double() for k, v in w.items()}
    x = torch.from_numpy(np.ascontiguousarray(windows)).double()
    h = F.conv1d(x.unsqueeze(1), d["conv1.weight"], d["conv1.bias"], stride=2)
    h = F.max_pool1d(F.relu(h), 2).flatten(1)
    h = F.relu(F.linear(h, d["fc1.weight"], d["fc1.bias"]))
    i = 0
    while f"layers.{i}.weight" in d:
        h = F.relu(F.linear(h, d[f"layers.{i}.weight"], d[f"layers.{i}.bias"]))
        i += 1
    return F.linear(h, d["output.weight"], d["output.bias"]).numpy()


def rows64(w, db, n_frames, t_frames):
    """db [streams][stride][n_bins] -> float64 logits [streams][stride][128] and the bool array of model rows: row (s, f) is the
    model on frames f - T + 1 .. f for T - 1 <= f < n_frames[s]; every other row stays zero"""
    S, stride, nb = db.shape
    out = np.zeros((S, stride, 128))
    valid = np.zeros((S, stride), bool)
    for s in range(S):
        fs = np.arange(t_frames - 1, n_frames[s])
        if fs.size:
            flat = db[s].reshape(-1)
            win = np.stack([flat[(f - t_frames + 1) * nb:(f + 1) * nb] for f in fs])
            out[s, fs] = logits64(w, win)
            valid[s, fs] = True
    return out, valid


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def mask_bits(mask_words):
    """[..., 4] uint32 -> [..., 128] bool, bit k = word k // 32, bit k % 32"""
    m = np.ascontiguousarray(mask_words).view(np.uint32)
    return np.unpackbits(m.view(np.uint8), axis=-1, bitorder="little").astype(bool)
