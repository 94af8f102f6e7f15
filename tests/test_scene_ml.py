"""The scene stage's `ml` branch (update.rs:247-255, display_system/util.rs:23-31) without a GPU: the host face
(SceneState.update(..., ml_prob=...), pvq_ml_scene_state_update) against tests/scene_ml_model.py, and the pitch of a bin
(pvq_ml_midi_pitch) against its f32 restatement.

Bars: everything test_scene.py holds the host to (scene_model.compare), and alpha bit-identical to the model's — the branch is one
compare and at most one f32 product.  (Where alpha is NaN — 0 / 0 of an all-zero list — both must be NaN.)

The three new entry points carry the prefix pvq_ml_, not pvq_scene_: the set of pvq_scene_ symbols is pinned by tests/test_scene.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pitchvis_amd as P
import scene_ml_model as MM
import scene_model as M
from pitchvis_amd import _lib
from pitchvis_amd import scene as PS
from test_render import CHROMA_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DT = 33_333_333
GEOMS = [(61.74, 2, 24), (55.0, 8, 24), (55.0, 7, 36)]
THRESH = f32(0.35)
ABOVE = np.nextafter(THRESH, f32(1.0))


def alpha_bits_equal(got, want):
    g, w = np.asarray(got["ball_rgba"])[..., 3], np.asarray(want["ball_rgba"])[..., 3]
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32))


def planted_probs(n_frames, seed):
    """random probabilities with the threshold's neighbourhood planted: exactly 0.35 (dim), the next f32 above (lit), NaN (dim), 0, 1"""
    rng = np.random.default_rng(seed)
    p = rng.random((n_frames, 128)).astype(f32)
    special = np.array([THRESH, ABOVE, np.nan, 0.0, 1.0], f32)
    pick = rng.random((n_frames, 128)) < 0.4
    p[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return p


def test_symbols_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in ("pvq_ml_scene_state_update", "pvq_ml_midi_pitch", "pvq_ml_scene_batch_frames_device"):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert "Left out: the `ml` branch" not in hdr
    assert PS.midi_pitch(36, 0) == 33


@pytest.mark.parametrize("octaves,bpo", [(7, 36), (8, 12), (8, 24), (5, 39), (16, 64)])
def test_midi_pitch_is_the_f32_restatement(octaves, bpo):
    got = [PS.midi_pitch(bpo, b) for b in range(octaves * bpo)]
    assert got == [MM.midi_pitch(bpo, b) for b in range(octaves * bpo)]
    assert got[0] == 33 and got[bpo] == 45
    if bpo == 12:
        assert got[94] == 127 and got[95] is None and got[:95] == list(range(33, 128))
    if bpo == 24:      # odd bins land on .5, which rounds away from zero
        assert got[188] == 127 and got[189] is None and got[1] == 34 and got[2] == 34 and got[3] == 35 and got[187] == 127


def test_midi_pitch_arguments():
    L = _lib.load()
    out = C.c_uint32(5)
    assert L.pvq_ml_midi_pitch(0, 3, C.byref(out)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_ml_midi_pitch(12, 3, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_ml_midi_pitch(12, 0xFFFFFFFF, C.byref(out)) == _lib.PVQ_OK and out.value == 0xFFFFFFFF
    assert L.pvq_ml_midi_pitch(1, 94, C.byref(out)) == _lib.PVQ_OK and out.value == 0xFFFFFFFF     # 94 octaves up


def _run(octaves, bpo, frames, probs, dts=None):
    """host with ml_prob, model with ml_prob, and a twin host without: compared after every frame"""
    host, twin = P.SceneState(P.VqtRange(55.0, octaves, bpo)), P.SceneState(P.VqtRange(55.0, octaves, bpo))
    model = MM.SceneMlModel(octaves, bpo)
    n = octaves * bpo
    keyed_lit = keyed_dim = keyed_none = 0
    for i, (pk, calm, acc, dev, scene) in enumerate(frames):
        dt = DT if dts is None else dts[i]
        host.update(pk, calm, acc, dev, scene, dt, ml_prob=probs[i])
        model.update(pk, calm, acc, dev, scene, dt, ml_prob=probs[i])
        twin.update(pk, calm, acc, dev, scene, dt)
        g, w, t = host.get(), model.get(), twin.get()
        M.compare(g, w, CHROMA_REL)
        assert alpha_bits_equal(g, w), i
        # the twin differs only in the alpha of balls keyed at some frame so far (the fade carries an alpha on)
        for k in ("ball_xyzs", "ball_params", "ball_visible", "bass_rgba"):
            assert np.array_equal(g[k], t[k], equal_nan=True), k
        assert g["bass_lit"] == t["bass_lit"] and g["bloom"] == t["bloom"]
        assert np.array_equal(g["ball_rgba"][:, :3], t["ball_rgba"][:, :3], equal_nan=True)
        keys = {M.as_usize(np.trunc(f32(c))) for c, _ in pk}
        keys = {k for k in keys if k < n}
        for idx in range(n):
            if idx not in keys and i == 0:
                assert g["ball_rgba"][idx, 3] == t["ball_rgba"][idx, 3]
        for idx in keys:
            m = MM.midi_pitch(bpo, idx)
            a = g["ball_rgba"][idx, 3]
            if m is None:
                keyed_none += 1
                assert a == t["ball_rgba"][idx, 3] or np.isnan(a)
            elif probs[i][m] > THRESH:
                keyed_lit += 1
                assert a == f32(1.0)
            else:
                keyed_dim += 1
                tw = t["ball_rgba"][idx, 3]
                assert np.isnan(a) if np.isnan(tw) else a == f32(tw * f32(0.1))
    return keyed_lit, keyed_dim, keyed_none


@pytest.mark.parametrize("geom,seed", list(zip(GEOMS, (131, 132, 133))))
def test_host_matches_model_on_analysis_state_frames(geom, seed):
    min_freq, octaves, bpo = geom
    frames = M.oracle_frames(min_freq, octaves, bpo, 40, seed)
    lit, dim, none = _run(octaves, bpo, frames, planted_probs(40, seed))
    print(f"{octaves} x {bpo}: keyed balls lit {lit}, dim {dim}, above pitch 127 {none}")
    assert lit >= 10 and dim >= 10
    if (octaves, bpo) == (8, 24):
        assert MM.midi_pitch(bpo, octaves * bpo - 1) is None


@pytest.mark.parametrize("geom,seed", list(zip(GEOMS, (141, 142, 143))))
def test_host_matches_model_on_crafted_frames(geom, seed):
    _, octaves, bpo = geom
    crafted = M.crafted_frames(octaves * bpo, bpo, seed)
    frames = [c[1:] for c in crafted]
    lit, dim, none = _run(octaves, bpo, frames, planted_probs(len(frames), seed), dts=[DT if i % 2 else 16_666_667 for i in range(len(frames))])
    assert lit and dim
    if (octaves, bpo) == (8, 24):        # the last bin (keyed by "first_and_last_bin") lies above pitch 127
        assert none >= 1


def test_none_is_update_bit_for_bit():
    octaves, bpo = 7, 36
    frames = M.oracle_frames(55.0, octaves, bpo, 12, 151)
    a, b = P.SceneState(P.VqtRange(55.0, octaves, bpo)), P.SceneState(P.VqtRange(55.0, octaves, bpo))
    L = _lib.load()
    fp = C.POINTER(C.c_float)
    for pk, calm, acc, dev, scene in frames:
        a.update(pk, calm, acc, dev, scene, DT)
        # the new entry point with a NULL row, under the Python face
        ctr, sz = np.asarray([p[0] for p in pk] or [0.0], f32), np.asarray([p[1] for p in pk] or [0.0], f32)
        assert L.pvq_ml_scene_state_update(b._h, ctr.ctypes.data_as(fp), sz.ctypes.data_as(fp), len(pk), calm.ctypes.data_as(fp),
                                           acc.ctypes.data_as(fp), dev.ctypes.data_as(fp), float(scene), DT, None) == _lib.PVQ_OK
        ga, gb = a.get(), b.get()
        for k in ga:
            assert np.array_equal(np.asarray(ga[k]).view(np.uint32) if np.asarray(ga[k]).dtype == f32 else ga[k],
                                  np.asarray(gb[k]).view(np.uint32) if np.asarray(gb[k]).dtype == f32 else gb[k]), k
    assert L.pvq_ml_scene_state_update(None, None, None, 0, None, None, None, 0.0, DT, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_ml_scene_state_update(b._h, None, None, 1, None, None, None, 0.0, DT, None) == _lib.PVQ_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        a.update([], calm, acc, dev, 0.0, DT, ml_prob=np.zeros(127, f32))


@pytest.mark.parametrize("who", ["host", "model"])
def test_threshold_known_answers(who):
    """two peaks of sizes 12 and 6 at bins 40 and 100 of 7 x 36: pitches 46 and 66; coef 1 and 1 - 0.25 = 0.75"""
    octaves, bpo = 7, 36
    n = octaves * bpo
    z = np.zeros(n, f32)
    pk = [(40.3, 12.0), (100.6, 6.0)]
    assert (MM.midi_pitch(bpo, 40), MM.midi_pitch(bpo, 100)) == (46, 66)

    def alpha(prob):
        s = P.SceneState(P.VqtRange(55.0, octaves, bpo)) if who == "host" else MM.SceneMlModel(octaves, bpo)
        s.update(pk, z, z, z, 0.0, DT, ml_prob=prob)
        g = s.get()
        return g["ball_rgba"][40, 3], g["ball_rgba"][100, 3], g
    assert alpha(None)[:2] == (f32(1.0), f32(0.75))
    assert alpha(np.ones(128, f32))[:2] == (f32(1.0), f32(1.0))                               # all inferred: exactly 1
    assert alpha(np.zeros(128, f32))[:2] == (f32(f32(1.0) * f32(0.1)), f32(f32(0.75) * f32(0.1)))   # none: coef * 0.1f, the initial vec![0.0; 128]
    p = np.zeros(128, f32)
    p[46], p[66] = THRESH, ABOVE
    assert alpha(p)[:2] == (f32(0.1), f32(1.0))                                               # > 0.35 is strict
    p[46], p[66] = ABOVE, np.nan
    assert alpha(p)[:2] == (f32(1.0), f32(f32(0.75) * f32(0.1)))                              # a NaN takes the dim side
    # only the keyed pitches are read: every other entry may be anything
    q = np.full(128, np.nan, f32)
    q[46], q[66] = 1.0, 0.0
    a40, a100, g = alpha(q)
    assert (a40, a100) == (f32(1.0), f32(f32(0.75) * f32(0.1)))
    base = alpha(None)[2]
    keep = np.ones(n, bool)
    keep[[40, 100]] = False
    assert np.array_equal(g["ball_rgba"][keep], base["ball_rgba"][keep]) and np.array_equal(g["ball_xyzs"], base["ball_xyzs"])
    assert np.array_equal(g["bass_rgba"], base["bass_rgba"]) and g["bass_lit"] == base["bass_lit"]   # the bass spiral's alpha is its own
    # the fade lifts a dim ball to 0.7 on its next frame (update.rs:166-168), as in the viewer
    s = P.SceneState(P.VqtRange(55.0, octaves, bpo)) if who == "host" else MM.SceneMlModel(octaves, bpo)
    s.update(pk, z, z, z, 0.0, DT, ml_prob=np.zeros(128, f32))
    s.update([], z, z, z, 0.0, DT, ml_prob=np.zeros(128, f32))
    assert s.get()["ball_rgba"][40, 3] == f32(0.7)
