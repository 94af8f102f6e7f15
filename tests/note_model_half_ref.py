"""The note model of a PVQ_NOTE_BF16 / PVQ_NOTE_F16 handle in float64 (Q64): tests/note_model_ref.py's model with the rounding points
of the rule in include/pvq.h restated through torch dtype casts — each pooled feature, every dense weight and every hidden activation
cast to the type once; everything else (conv, sums, bias, ReLU, logits) in float64.  L64 is the unrounded note_model_ref.logits64.
Also the two bars every test of the 16-bit path applies, and the logits behind the probabilities the host face returns."""
import numpy as np
import torch
import torch.nn.functional as F

import note_model_ref as R

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
BAR_A, BAR_B = 1.5, 0.5


def _q(x, dt):
    return x.to(dt).double()


def logits_q64(w, windows, precision):
    """windows [rows][L] -> float64 logits [rows][128] under the rule's rounding"""
    dt = DTYPES[precision]
    d = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    x = torch.from_numpy(np.ascontiguousarray(windows)).double()
    h = F.conv1d(x.unsqueeze(1), d["conv1.weight"].double(), d["conv1.bias"].double(), stride=2)
    h = _q(F.max_pool1d(F.relu(h), 2).flatten(1), dt)
    h = _q(F.relu(F.linear(h, _q(d["fc1.weight"], dt), d["fc1.bias"].double())), dt)
    i = 0
    while f"layers.{i}.weight" in d:
        h = _q(F.relu(F.linear(h, _q(d[f"layers.{i}.weight"], dt), d[f"layers.{i}.bias"].double())), dt)
        i += 1
    return F.linear(h, _q(d["output.weight"], dt), d["output.bias"].double()).numpy()


def rows_q64(w, db, n_frames, t_frames, precision):
    """note_model_ref.rows64 for Q64: [streams][stride][128], zero outside the model rows"""
    S, stride, nb = db.shape
    out = np.zeros((S, stride, 128))
    for s in range(S):
        fs = np.arange(t_frames - 1, n_frames[s])
        if fs.size:
            flat = db[s].reshape(-1)
            out[s, fs] = logits_q64(w, np.stack([flat[(f - t_frames + 1) * nb:(f + 1) * nb] for f in fs]), precision)
    return out


def logit_of(prob):
    """the logit behind an f32 probability, in float64.  The f32 rounding of p moves it by at most 6e-8 p / (p (1 - p)): under 2e-6 for
    |logit| < 3.5, against a quantisation effect of 7e-5 and more on every shape the tests use."""
    p = np.asarray(prob, np.float64)
    return np.log(p) - np.log1p(-p)


def ratios(got, q64, l64):
    """(a) max |got - L64| / max |Q64 - L64|, (b) rms(got - Q64) / rms(Q64 - L64), and max |Q64 - L64| itself"""
    quant = float(np.abs(q64 - l64).max())
    a = float(np.abs(got - l64).max()) / quant
    b = float(np.sqrt(np.mean((got - q64) ** 2)) / np.sqrt(np.mean((q64 - l64) ** 2)))
    return a, b, quant
