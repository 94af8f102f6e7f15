"""The pitch-ball scene (pvq_scene_state_*, pvq_scene_batch_*) as far as it goes without a GPU: the symbols, the argument checks and
the host-only handle, what the compiler made of the kernels, known answers derived from the reference text alone, and the host
SceneState against tests/scene_model.py on frames of an oracle AnalysisState and on crafted frames.

Bars (host against model; tests/test_scene_gpu.py holds the device to the same ones): scale, z, the visible mask, the three params,
bass_lit and bloom bit-identical — they touch no libm beyond the fade table; x, y and the eight colour channels within
CHROMA_REL * max(1, |want|) (x and y pass through zero)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pitchvis_amd as P
import scene_cases as SC
import scene_model as M
from pitchvis_amd import _lib
from pitchvis_amd import scene as PS
from test_render import CHROMA_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32
DT = 33_333_333
GEOMS = [(61.74, 2, 24), (55.0, 7, 36), (55.0, 7, 84)]


def visible_bins(g):
    return list(np.nonzero(np.unpackbits(g["ball_visible"].view(np.uint8), bitorder="little"))[0])


def zeros(n):
    z = np.zeros(n, f32)
    return z, z, z


def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    names = sorted(set(re.findall(r"\b(pvq_scene_\w+)\s*\(", hdr)))
    assert len(names) == 12 and "pvq_scene_batch_frames_device" in names and "pvq_scene_state_update" in names
    for name in names:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert P.SceneState is PS.SceneState and P.SceneBatch is PS.SceneBatch
    assert (PS.FULL, PS.ZEN, PS.PERFORMANCE, PS.GALAXY) == (M.FULL, M.ZEN, M.PERFORMANCE, M.GALAXY) == (0, 1, 2, 3)


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    h = C.c_void_p()
    create = L.pvq_scene_batch_create
    assert create(-1, 7, 36, None, 4, None) == _lib.PVQ_ERR_INVALID_ARG
    for dev in (-1, 0):   # rejected before any device is touched
        for bad in ((0, 36, 4), (7, 0, 4), (7, 36, 0)):
            assert create(dev, bad[0], bad[1], None, bad[2], C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, 1, 2, None, 4, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value       # 2 bins
        assert create(dev, 25, 41, None, 4, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value     # 1025 bins
        assert "1024" in L.pvq_last_error().decode()
        cfg = _lib.CSceneSettings(4, 1, None, 60.0, 1.3)                                                # unknown mode
        assert create(dev, 7, 36, C.byref(cfg), 4, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert "mode" in L.pvq_last_error().decode()
    for octaves, bpo in ((1, 3), (7, 36), (16, 64)):
        assert create(-1, octaves, bpo, None, 2, C.byref(h)) == _lib.PVQ_OK and h.value
        L.pvq_scene_batch_destroy(h)
    assert create(-1, 7, 36, None, 3, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        assert L.pvq_scene_batch_n_segments(h) == 167
        buf = np.zeros(4096, f32)
        p = buf.ctypes.data   # stands for device memory; a host-only handle never dereferences it
        call = L.pvq_scene_batch_frames_device
        full = dict(center=p, size=p, peak_count=p, max_peaks=8, calmness=p, pitch_accuracy=p, pitch_deviation=p, scene_calmness=p)

        def ins(**kw):
            i = _lib.CSceneInputs()
            for k, v in {**full, **kw}.items():
                setattr(i, k, v)
            return C.byref(i)
        o = _lib.CSceneOutputs()
        o.bloom = p
        assert call(None, 1, ins(), DT, None, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, ins(), DT, None, C.byref(o), None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
        assert call(h, 1, ins(), DT, None, None, None) == _lib.PVQ_ERR_NO_DEVICE
        assert call(h, 1, None, DT, None, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG                   # null tables
        for name in ("center", "size", "peak_count", "calmness", "pitch_accuracy", "pitch_deviation", "scene_calmness"):
            assert call(h, 1, ins(**{name: None}), DT, None, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG, name
        assert call(h, 1, ins(max_peaks=0), DT, None, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG       # peak inputs given, no room
        assert "max_peaks" in L.pvq_last_error().decode()
        o2 = _lib.CSceneOutputs()
        o2.ball_xyzs = p + 4
        assert call(h, 1, ins(), DT, None, C.byref(o2), None) == _lib.PVQ_ERR_INVALID_ARG                 # float4 stores
        assert call(h, 1 << 31, ins(), DT, None, C.byref(o), None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_scene_batch_get_state(h, 3, None, None, None, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_scene_batch_get_state(h, 0, None, None, None, None, None, None, None) == _lib.PVQ_ERR_NO_DEVICE
    finally:
        L.pvq_scene_batch_destroy(h)
    L.pvq_scene_batch_destroy(None)
    L.pvq_scene_state_destroy(None)
    cfg = _lib.CSceneSettings(-1, 1, None, 60.0, 1.3)
    assert L.pvq_scene_state_create(7, 36, C.byref(cfg), C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    assert L.pvq_scene_state_create(0, 36, None, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    b = P.SceneBatch(P.VqtRange(55.0, 7, 36), 5, device=None)
    assert b.n_bins == 252 and b.output_shape("ball_visible", 3) == ((5, 3, 8), np.uint32)
    assert b.output_shape("ball_params", 2) == ((5, 2, 252, 3), np.float32) and len(b.OUTPUTS) == 7
    with pytest.raises(P.PvqError) as e:
        b.frames_device({k: p for k in PS.INPUTS}, outputs={"bloom": p}, n_frames=1, max_peaks=4)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        b.frames_device({k: p for k in PS.INPUTS if k != "size"}, outputs={"bloom": p}, n_frames=1, max_peaks=4)
    with pytest.raises(ValueError):
        b.frames_device({k: p for k in PS.INPUTS}, outputs={"nonsense": p}, n_frames=1, max_peaks=4)
    with pytest.raises(ValueError):
        P.SceneState(P.VqtRange(55.0, 7, 36), visuals_mode=7)
    with pytest.raises(P.PvqError):
        P.SceneBatch(P.VqtRange(55.0, 13, 84), 2, device=None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """one scene_frames instantiation per 64-chunk of bins, no kernel of the unit uses scratch; LDS and VGPRs recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "scene_batch.hip")
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
    kern = {int(re.search(r"scene_framesILi(\d+)E", k).group(1)): u for k, u in usage.items() if "scene_frames" in k}
    assert sorted(kern) == list(range(1, 17)), list(usage)
    peaks = [u for k, u in usage.items() if "scene_peaks" in k]
    assert len(peaks) == 1
    print(f"scene_peaks: {peaks[0]}")
    assert peaks[0]["ScratchSize"] == 0 and peaks[0]["VGPRs"] + peaks[0].get("AGPRs", 0) <= 256
    for nk, u in sorted(kern.items()):
        print(f"scene_frames<{nk}>: {u}")
        assert u["ScratchSize"] == 0, (nk, u)
        assert u["LDS"] == 60 * 64 * nk, (nk, u)              # fifteen dwords a bin: the LDS of a chunk count, not of 1024 bins
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (nk, u)   # four waves per SIMD by registers


# ---- known answers, from the reference text alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("who", ["host", "model"])
def test_known_answers(who):
    F = M.F
    make = (lambda **kw: P.SceneState(P.VqtRange(55.0, 7, 36), **kw)) if who == "host" else \
           (lambda visuals_mode=0, enable_bloom=True: M.SceneModel(7, 36, visuals_mode, enable_bloom))
    n = 252
    s = make()
    g = s.get()
    assert visible_bins(g) == list(range(0, n, 17))                                     # setup.rs:106
    assert np.all(g["ball_xyzs"][::17, 3] == 3.0) and np.count_nonzero(g["ball_xyzs"][:, 3]) == len(range(0, n, 17))
    assert np.all(g["ball_xyzs"][:, 2] == f32(-0.01)) and g["bass_lit"] == 0 and g["bloom"] == 0.0 and s.n_segments == 167
    assert abs(g["ball_xyzs"][0, 0] + 0.6) < 1e-6 and abs(g["ball_xyzs"][0, 1]) < 1e-6  # bin 0: radius 0.6 at angle 2 pi
    assert np.all(g["ball_params"] == 0.0) and np.allclose(g["ball_rgba"][5], [1.0, 0.4479884, 0.3185468, 1.0], atol=1e-6)
    # one fade at 1 / 30 s: dropoff of ball 0 is 0.85^(30 * (1 / 30)): 30 * 0.033333335 rounds to 1.0 in f32
    s.update([], *zeros(n), 0.9, DT)
    g1 = s.get()
    assert g1["ball_xyzs"][0, 3] == f32(f32(f32(f32(3.0) / F) * f32(0.85)) * F)
    assert g1["ball_xyzs"][0, 2] == f32(f32(-0.01) - f32(f32(f32(0.001) * f32(30.0)) * M.secs_f32(DT)))
    assert g1["ball_rgba"][0, 3] == f32(0.85) and g1["ball_rgba"][1, 3] == 1.0         # a ball below the cutoff does not fade
    # a frame without peaks changes nothing but the fade: positions, colours, params, bass and bloom as before
    assert np.array_equal(g1["ball_xyzs"][:, :2], g["ball_xyzs"][:, :2]) and np.array_equal(g1["ball_rgba"][:, :3], g["ball_rgba"][:, :3])
    assert g1["bass_lit"] == 0 and g1["bloom"] == 0.0 and visible_bins(g1) == visible_bins(g)
    # a single peak (40.3, 20.0) with calmness 0.5 under it
    calm = np.full(n, 0.5, f32)
    acc, dev = np.full(n, 0.25, f32), np.full(n, -0.125, f32)
    s.update([(40.3, 20.0)], calm, acc, dev, 0.8, DT)
    g2 = s.get()
    c = f32(f32(0.5) - f32(0.27))
    assert g2["ball_rgba"][40, 3] == 1.0                                                # 1 - (1 - 20 / 20)^2
    assert g2["ball_xyzs"][40, 2] == f32(f32(f32(1.0) - f32(1.01)) * f32(12.5)) and abs(g2["ball_xyzs"][40, 2] + 0.125) < 1e-6
    assert g2["ball_xyzs"][40, 3] == f32(f32(f32(f32(20.0) * f32(1.0)) * F) * f32(f32(1.0) + f32(f32(0.2) * c)))
    assert list(g2["ball_params"][40]) == [c, f32(0.25), f32(-0.125)] and 40 in visible_bins(g2)
    assert g2["bloom"] == 1.0                                                           # 0.8 * 1.3 clamps at 1
    assert g2["bass_lit"] == 13 * 6 and g2["bass_rgba"][3] == 1.0                       # round(40.3 / 36 * 12 = 13.43) * 6
    # the hide range at bpo 36 is round(c +- 0.69): 40.3 -> 40 ..= 41; a visible neighbour hides and keeps its scale
    s2 = make()
    s2.update([(33.6, 10.0)], *zeros(n), 0.0, DT)                                       # round(32.91) ..= round(34.29): 33, 34 — ball 34 is an intro ball
    g3 = s2.get()
    assert 34 not in visible_bins(g3) and 33 in visible_bins(g3) and g3["ball_xyzs"][34, 3] > 2.0
    assert set(range(0, n, 17)) - set(visible_bins(g3)) == {34}
    # bass: first peak at centre 6.2 -> round(2.0667) * 6 = 12 lit; a semitone that reaches the last segment lights none
    s2.update([(6.2, 5.0), (100.0, 9.0)], *zeros(n), 0.1, DT)
    g4 = s2.get()
    assert g4["bass_lit"] == 12 and g4["bass_rgba"][3] == f32(f32(1.0) - f32(f32(f32(1.0) - f32(f32(5.0) / f32(9.0))) ** 2))
    assert g4["bloom"] == f32(f32(0.1) * f32(1.3))
    kept = g4["bass_rgba"].copy()
    s2.update([(84.0, 5.0)], *zeros(n), 0.1, DT)                                        # semitone 28: 168 >= 167
    assert s2.get()["bass_lit"] == 0 and np.array_equal(s2.get()["bass_rgba"], kept)
    s2.update([(81.0, 5.0)], *zeros(n), 0.1, DT)                                        # semitone 27: 162 < 167
    assert s2.get()["bass_lit"] == 162
    # Galaxy lights none; Performance scales by 0.7 and has bloom 0; bloom disabled gives 0
    gal = make(visuals_mode=M.GALAXY)
    gal.update([(6.2, 5.0)], *zeros(n), 0.5, DT)
    assert gal.get()["bass_lit"] == 0 and gal.get()["bloom"] == f32(f32(0.5) * f32(1.3))
    perf = make(visuals_mode=M.PERFORMANCE)
    perf.update([(40.3, 20.0)], calm, acc, dev, 0.8, DT)
    assert perf.get()["ball_xyzs"][40, 3] == f32(f32(f32(f32(20.0) * f32(0.7)) * F) * f32(f32(1.0) + f32(f32(0.2) * c)))
    assert perf.get()["bloom"] == 0.0 and perf.get()["bass_lit"] == 78
    dark = make(enable_bloom=False)
    dark.update([(40.3, 20.0)], calm, acc, dev, 0.8, DT)
    assert dark.get()["bloom"] == 0.0


@pytest.mark.parametrize("who", ["host", "model"])
def test_hide_range_at_bpo_84(who):
    """radius (84 / 12) * 0.23 = 1.61: a peak at 120.2 marks round(118.59) ..= round(121.81) = 119 ..= 122, and keeps 120"""
    n = 7 * 84
    s = P.SceneState(P.VqtRange(55.0, 7, 84)) if who == "host" else M.SceneModel(7, 84)
    s.update([(float(b) + 0.5, 30.0) for b in range(117, 125)], *zeros(n), 0.0, DT)     # light 117 .. 124
    assert set(range(117, 125)) <= set(visible_bins(s.get()))
    s.update([(120.2, 30.0)], *zeros(n), 0.0, DT)
    vis = set(visible_bins(s.get()))
    assert {117, 118, 120, 123, 124} <= vis and not ({119, 121, 122} & vis)


# ---- host against model -------------------------------------------------------------------------------------------------------
def run_both(octaves, bpo, frames, dts=None, also=None, **kw):
    host = P.SceneState(P.VqtRange(55.0, octaves, bpo), **kw)
    model = M.SceneModel(octaves, bpo, kw.get("visuals_mode", 0), kw.get("enable_bloom", True))
    worst = 0.0
    for i, (pk, calm, acc, dev, scene) in enumerate(frames):
        dt = DT if dts is None else dts[i]
        host.update(pk, calm, acc, dev, scene, dt)
        model.update(pk, calm, acc, dev, scene, dt)
        worst = max(worst, M.compare(host.get(), model.get(), CHROMA_REL))
        if also is not None:
            also(host.get(), model.get())
    return worst, host, model


@pytest.mark.parametrize("geom,seed", list(zip(GEOMS, (31, 32, 33))))
def test_host_matches_model_on_analysis_state_frames(geom, seed):
    min_freq, octaves, bpo = geom
    frames = M.oracle_frames(min_freq, octaves, bpo, 40, seed)
    assert sum(len(f[0]) for f in frames) >= 40                                         # the stimulus really lights the scene
    worst, host, _ = run_both(octaves, bpo, frames)
    print(f"{octaves} x {bpo}: host vs model over 40 oracle frames: max |d| / max(1, |want|) = {worst:.2e}")
    assert host.get()["bass_lit"] >= 0 and len(visible_bins(host.get())) > 0


@pytest.mark.parametrize("geom,seed", list(zip(GEOMS, (41, 42, 43))))
def test_host_matches_model_on_crafted_frames(geom, seed):
    _, octaves, bpo = geom
    n = octaves * bpo
    crafted = M.crafted_frames(n, bpo, seed)
    names = [c[0] for c in crafted]
    frames = [c[1:] for c in crafted]
    worst, _, _ = run_both(octaves, bpo, frames, dts=[DT if i % 2 else 16_666_667 for i in range(len(frames))])
    print(f"{n} bins: host vs model over the crafted frames: max |d| / max(1, |want|) = {worst:.2e}")
    assert len(frames[names.index("seventy")][0]) == 70
    # the later entry of a key wins, and the order of the pair decides the ball
    m = n // 2
    ab, ba = frames[names.index("same_key_ab")], frames[names.index("same_key_ba")]
    for who in (lambda: P.SceneState(P.VqtRange(55.0, octaves, bpo)), lambda: M.SceneModel(octaves, bpo)):
        a, b = who(), who()
        a.update(*ab, DT)
        b.update(*ba, DT)
        ga, gb = a.get(), b.get()
        assert ga["ball_rgba"][m, 3] == 1.0 and gb["ball_rgba"][m, 3] < 1.0 and not np.array_equal(ga["ball_xyzs"][m], gb["ball_xyzs"][m])
        z = who()
        z.update(*frames[names.index("all_zero_sizes")], DT)                             # 0 / 0: NaN alpha and z, scale 0
        gz = z.get()
        assert np.isnan(gz["ball_rgba"][m - 4, 3]) and np.isnan(gz["ball_xyzs"][m - 4, 2]) and gz["ball_xyzs"][m - 4, 3] == 0.0
        e = who()
        e.update(*frames[names.index("full_a")], DT)
        before = e.get()
        e.update(*frames[names.index("empty")], DT)
        after = e.get()
        assert after["bass_lit"] == before["bass_lit"] and after["bloom"] == before["bloom"]
        assert np.array_equal(after["ball_params"], before["ball_params"]) and after["ball_xyzs"][m + 2, 3] < before["ball_xyzs"][m + 2, 3]


# ---- the cases of tests/scene_cases.py: edge geometries, long lists, hide ranges, odd entries, frame times ---------------------------
def model_accepts(frame, octaves, bpo):
    try:
        M.SceneModel(octaves, bpo).update(*frame[1:], DT)
        return True
    except ValueError:
        return False


@pytest.mark.parametrize("geom", SC.GEOMS_EDGE)
def test_host_matches_model_on_edge_cases(geom):
    """the crafted frames, the long lists, the hide cases, the odd entries and the odd fields in one walk; a list the model refuses
    (a NaN centre) is left out of the walk and held on the host alone by test_nan_centre_on_the_host"""
    octaves, bpo = geom
    n = octaves * bpo
    cases = M.crafted_frames(n, bpo, 50 + n) + SC.long_lists(n, bpo, 60 + n)
    for hc in SC.hide_cases(octaves, bpo):
        cases += hc[1]
    cases += SC.edge_entries(n) + SC.edge_fields(n)
    refused = [c[0] for c in cases if "nan_centre" in c[0] and not model_accepts(c, octaves, bpo)]
    frames = [c[1:] for c in cases if c[0] not in refused]
    assert len(frames) >= len(cases) - 2 and max(len(f[0]) for f in frames) == 200
    worst, _, _ = run_both(octaves, bpo, frames, dts=[DT if i % 3 else 16_666_667 for i in range(len(frames))],
                           also=lambda g, w: SC.close_with_specials(g, w, CHROMA_REL))
    print(f"{octaves} x {bpo}: host vs model over {len(frames)} edge frames ({len(refused)} refused): max |d| / max(1, |want|) = {worst:.2e}")


@pytest.mark.parametrize("geom", [(1, 1024), (7, 9), (1, 12), (1, 11), (5, 13), (11, 93)])
@pytest.mark.parametrize("who", ["host", "model"])
def test_hide_known_answers(who, geom):
    octaves, bpo = geom
    cases = SC.hide_cases(octaves, bpo)
    assert len(cases) == len(SC.HIDE_TABLE.get(geom, [0]))
    for case in cases:
        s = P.SceneState(P.VqtRange(55.0, octaves, bpo)) if who == "host" else M.SceneModel(octaves, bpo)
        for fr in case[1]:
            s.update(*fr[1:], DT)
        SC.hide_holds(s.get(), case)


@pytest.mark.parametrize("who", ["host", "model"])
def test_long_lists_honour_list_order(who):
    """the builder's own check, on both faces: a long list and its reversal leave different balls, and key A of the list — entered
    in chunk 0 only — carries its LAST entry (index 40), not an earlier one"""
    octaves, bpo, n = 7, 36, 252
    for fr in SC.long_lists(n, bpo, 5):
        pk = fr[1]
        a = int(pk[40][0])
        first = next(i for i, (c, _) in enumerate(pk) if int(c) == a)
        assert first <= 3 and int(pk[3][0]) == a and all(int(c) != a for c, _ in pk[41:])
        got = []
        for lst in (pk, pk[::-1]):
            s = P.SceneState(P.VqtRange(55.0, octaves, bpo)) if who == "host" else M.SceneModel(octaves, bpo)
            s.update(lst, *fr[2:], DT)
            got.append(s.get())
        assert not np.array_equal(SC.balls(got[0]), SC.balls(got[1]), equal_nan=True), fr[0]
        big = max(z for _, z in pk)
        want = lambda z: f32(f32(f32(f32(z) / f32(big)) - f32(1.01)) * f32(12.5))           # update.rs:233
        assert got[0]["ball_xyzs"][a, 2] == want(pk[40][1]) and got[1]["ball_xyzs"][a, 2] == want(pk[first][1]), fr[0]


def test_nan_centre_on_the_host():
    """what the reference text gives for a NaN centre: trunc(NaN) as usize is 0 (update.rs:211), so the entry lands on ball 0, whose
    x and y become NaN (util.rs:9-20); every other ball is as without the entry"""
    n = 252
    named = {c[0]: c for c in SC.edge_entries(n)}
    for name in ("nan_centre", "nan_centre_first"):
        fr = named[name]
        with_nan, without = P.SceneState(P.VqtRange(55.0, 7, 36)), P.SceneState(P.VqtRange(55.0, 7, 36))
        with_nan.update(*fr[1:], DT)
        without.update([p for p in fr[1] if p[0] == p[0]], *fr[2:], DT)
        g, w = with_nan.get(), without.get()
        size = next(z for c, z in fr[1] if c != c)
        assert np.isnan(g["ball_xyzs"][0, 0]) and np.isnan(g["ball_xyzs"][0, 1])
        assert g["ball_xyzs"][0, 3] == f32(f32(f32(size) * M.F) * f32(f32(1.0) + f32(f32(0.2) * g["ball_params"][0, 0])))
        assert np.array_equal(g["ball_xyzs"][1:, :2], w["ball_xyzs"][1:, :2]) and np.array_equal(g["ball_rgba"][1:, :3], w["ball_rgba"][1:, :3])
        assert g["bass_lit"] == (0 if name == "nan_centre_first" else w["bass_lit"])     # round(NaN) as usize is 0 segments


@pytest.mark.parametrize("geom", [(7, 36), (1, 3)])
def test_frame_times_at_the_edges(geom):
    """Duration::as_secs_f32 at 0 ns, 1 ns, 1 s, 5 s + 7 ns and 2^40 ns: host against model, and the split itself"""
    octaves, bpo = geom
    n = octaves * bpo
    assert M.secs_f32(5_000_000_007) == f32(f32(5.0) + f32(f32(7.0) / f32(1e9))) and M.secs_f32(2 ** 40) == f32(f32(1099.0) + f32(f32(511627776.0) / f32(1e9)))
    frames = [c[1:] for c in SC.plain_frames(n, 3 * len(SC.FRAME_TIMES_NS), 17)]
    dts = [SC.FRAME_TIMES_NS[i // 3] if i % 3 == 1 else DT for i in range(len(frames))]
    worst, host, _ = run_both(octaves, bpo, frames, dts=dts)
    print(f"{n} bins: host vs model over frame times {SC.FRAME_TIMES_NS}: max |d| / max(1, |want|) = {worst:.2e}")
    s = P.SceneState(P.VqtRange(55.0, octaves, bpo))
    before = s.get()
    s.update([], *zeros(n), 0.0, 0)                                                       # 0 ns: dropoff x^0 = 1, z step 0
    after = s.get()
    for k in ("ball_xyzs", "ball_rgba"):
        assert np.array_equal(before[k], after[k]), k
