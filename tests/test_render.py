"""The render stage (pvq_spectrogram_row, pvq_chroma_row, pvq_render_batch_*) as far as it goes without a GPU: the symbols, the
argument checks and the host-only handle, what the compiler made of the kernel, and the two host functions against
tests/render_model.py — the literal restatement of pitchvis_viewer/src/display_system/update.rs:961-1065 and :1102-1131 — first on
known answers derived from the reference text alone (host functions and model both), then on rows of an oracle AnalysisState.

Bars (host against model; tests/test_render_gpu.py holds the device to the same ones):
  * u8 outputs never more than one level apart; at most 1 % of the bytes differ at all.  Both sides evaluate the same f32 expressions;
    a byte flips only where (x * 255) * 1.2, x * 254 or the sRGB * 255 rounding sits within an ulp or two of an integer, and where
    powf / expf / cosf of two libms differ in the last place: of order 1e-3 per byte.
  * chroma within 1e-5 relative per entry, the project's magnitude bar: <= 49 positive terms, each a powf a few ulp off, summed in
    the same order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import pitchvis_amd as P
import render_cases as RC
import render_model as M
from helpers import get_geom, white_noise
from pitchvis_amd import _lib
from pitchvis_amd import consumers as PC
from synth import piano_roll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("pvq_spectrogram_row", "pvq_chroma_row", "pvq_render_batch_create", "pvq_render_batch_destroy", "pvq_render_batch_rows_device")
U8_LEVELS, U8_SHARE, CHROMA_REL = 1, 0.01, 1e-5
fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def both(fn):
    """the host function and the model, called alike"""
    return [("host", getattr(PC, fn)), ("model", getattr(M, fn))]


def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert (PC.SPECTROGRAM_VQT, PC.SPECTROGRAM_PEAKS) == (M.VQT, M.PEAKS) == (0, 1)
    assert P.RenderBatch is PC.RenderBatch and P.spectrogram_row is PC.spectrogram_row and P.chroma_row is PC.chroma_row


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    h = C.c_void_p()
    create = L.pvq_render_batch_create
    assert create(-1, 55.0, 7, 36, None, 60.0, 1.3, None) == _lib.PVQ_ERR_INVALID_ARG
    for bad in ((0.0, 7, 36), (-1.0, 7, 36), (float("nan"), 7, 36), (55.0, 0, 36), (55.0, 7, 0)):
        for dev in (-1, 0):   # rejected before any device is touched
            assert create(dev, bad[0], bad[1], bad[2], None, 60.0, 1.3, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    for dev in (-1, 0):
        assert create(dev, 55.0, 1, 2, None, 60.0, 1.3, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value     # 2 bins
        assert create(dev, 55.0, 13, 84, None, 60.0, 1.3, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value   # 1092 bins
        assert "1024" in L.pvq_last_error().decode()
    for octaves, bpo in ((1, 3), (5, 36), (7, 36), (7, 84), (10, 84), (16, 64)):   # what pvq_analysis_batch_create takes: 3 .. 1024 bins
        assert create(-1, 55.0, octaves, bpo, None, 60.0, 1.3, C.byref(h)) == _lib.PVQ_OK and h.value
        L.pvq_render_batch_destroy(h)
    pal = np.ascontiguousarray(PC.SERIAL_COLORS, np.float32)
    assert create(-1, 55.0, 7, 36, pal.ctypes.data_as(fp), 5.0, 2.3, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        # the pointers stand for device memory; a host-only handle never dereferences them
        buf = np.zeros(4096, np.float32)
        p = buf.ctypes.data
        rows = L.pvq_render_batch_rows_device

        def outs(**kw):
            o = _lib.CRenderOutputs()
            for k, v in kw.items():
                setattr(o, k, v)
            return C.byref(o)
        assert rows(None, 1, p, p, p, p, 8, outs(chroma=p), None) == _lib.PVQ_ERR_INVALID_ARG                 # null handle
        assert rows(h, 1, p, p, p, p, 8, outs(spectrogram_vqt=p, spectrogram_peaks=p, chroma=p, led=p), None) == _lib.PVQ_ERR_NO_DEVICE
        assert "GPU" in L.pvq_last_error().decode()
        assert rows(h, 1, p, None, None, None, 0, outs(spectrogram_vqt=p, chroma=p), None) == _lib.PVQ_ERR_NO_DEVICE
        assert rows(h, 1, None, p, p, p, 8, outs(spectrogram_peaks=p, led=p), None) == _lib.PVQ_ERR_NO_DEVICE
        for name in ("spectrogram_vqt", "chroma"):                                                           # need x_vqt_smoothed
            assert rows(h, 1, None, p, p, p, 8, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert "x_vqt_smoothed" in L.pvq_last_error().decode()
        for name in ("spectrogram_peaks", "led"):                                                            # need all three peak arrays
            assert rows(h, 1, p, None, p, p, 8, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert rows(h, 1, p, p, None, p, 8, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert rows(h, 1, p, p, p, None, 8, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert rows(h, 1, p, p, p, p, 0, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
        assert rows(h, 1, p, p, p, p, 8, outs(spectrogram_vqt=p + 2), None) == _lib.PVQ_ERR_INVALID_ARG       # RGBA: dword stores
        assert rows(h, 1 << 31, p, p, p, p, 8, outs(chroma=p), None) == _lib.PVQ_ERR_INVALID_ARG
        assert rows(h, 1, p, p, p, p, 8, None, None) == _lib.PVQ_ERR_NO_DEVICE                                # (checked before "nothing to do")
    finally:
        L.pvq_render_batch_destroy(h)
    L.pvq_render_batch_destroy(None)
    r = P.RenderBatch(P.VqtRange(55.0, 7, 36), device=None)
    assert r.n_bins == 252 and r.output_shape("led", 5) == ((5, 759), np.uint8)
    with pytest.raises(P.PvqError) as e:
        r.rows_device(x_vqt_smoothed=buf.ctypes.data, n_rows=1, outputs={"chroma": buf.ctypes.data})
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        r.rows_device(center=buf.ctypes.data, n_rows=1, max_peaks=4, outputs={"led": buf.ctypes.data})      # size and peak_count missing
    with pytest.raises(ValueError):
        r.rows_device(x_vqt_smoothed=buf.ctypes.data, n_rows=1, outputs={"nonsense": buf.ctypes.data})
    with pytest.raises(ValueError):
        P.RenderBatch(P.VqtRange(55.0, 0, 36), device=None)
    with pytest.raises(P.PvqError):
        P.RenderBatch(P.VqtRange(55.0, 13, 84), device=None)
    # the host functions' own checks
    out = np.zeros((252, 4), np.uint8)
    x = np.zeros(252, np.float32)
    col = np.ascontiguousarray(PC.COLORS, np.float32).ctypes.data_as(fp)
    call = L.pvq_spectrogram_row
    assert call(2, 252, 36, x.ctypes.data_as(fp), None, None, 0, col, 60.0, 1.3, out.ctypes.data_as(bp)) == _lib.PVQ_ERR_INVALID_ARG
    assert call(0, 252, 0, x.ctypes.data_as(fp), None, None, 0, col, 60.0, 1.3, out.ctypes.data_as(bp)) == _lib.PVQ_ERR_INVALID_ARG
    assert call(0, 252, 36, None, None, None, 0, col, 60.0, 1.3, out.ctypes.data_as(bp)) == _lib.PVQ_ERR_INVALID_ARG
    assert call(1, 252, 36, None, None, None, 3, col, 60.0, 1.3, out.ctypes.data_as(bp)) == _lib.PVQ_ERR_INVALID_ARG
    assert call(1, 252, 36, None, None, None, 0, col, 60.0, 1.3, out.ctypes.data_as(bp)) == _lib.PVQ_OK
    assert call(0, 252, 36, x.ctypes.data_as(fp), None, None, 0, None, 60.0, 1.3, out.ctypes.data_as(bp)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_chroma_row(55.0, 252, 0, x.ctypes.data_as(fp), x.ctypes.data_as(fp)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_chroma_row(55.0, 252, 36, None, x.ctypes.data_as(fp)) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_chroma_row(55.0, 252, 36, x.ctypes.data_as(fp), None) == _lib.PVQ_ERR_INVALID_ARG


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """in the manner of test_kernel_resources.py: one instantiation per 64-chunk of bins, none may use scratch; LDS and VGPRs recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "render_batch.hip")
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
    kern = {int(re.search(r"render_rowsILi(\d+)E", k).group(1)): u for k, u in usage.items() if "render_rows" in k}
    assert sorted(kern) == list(range(1, 17)), list(usage)
    for nk, u in sorted(kern.items()):
        print(f"render_rows<{nk}>: {u}")
        assert u["ScratchSize"] == 0, (nk, u)
        assert u["LDS"] <= 32 * 1024, (nk, u)          # at least five workgroups (waves) per CU by LDS
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (nk, u)   # two waves per SIMD


# ---- known answers, from the reference text alone -------------------------------------------------------------------------------
def test_bin_0_pitch_class_of_55_hz():
    """12 log2(55 / 261.626) = -27.0 -> (-27 % 12 + 12) % 12 = 9 (A)"""
    assert M.bin_0_pitch_class(55.0) == 9
    # the host: a row whose only energy is bin 0 peaks in class 9
    x = np.full(252, -1000.0, np.float32)   # 10^-100 underflows to 0
    x[0] = 10.0
    for who, fn in both("chroma_row"):
        c = fn(55.0, 252, 36, x)
        assert c[9] == 1.0 and np.count_nonzero(c) == 1, who


def test_chroma_of_an_all_zero_row():
    """10^0 = 1 per bin, 252 / 12 = 21 bins per class -> 21 / 21"""
    counts = np.zeros(12, int)
    for b in range(252):
        counts[(int(np.floor(b * 12 / 36 + 0.5)) + 9) % 12] += 1
    assert np.all(counts == 21)
    for who, fn in both("chroma_row"):
        c = fn(55.0, 252, 36, np.zeros(252, np.float32))
        assert c.dtype == np.float32 and np.array_equal(c, np.ones(12, np.float32)), who


@pytest.mark.parametrize("who,fn", both("spectrogram_row"))
def test_vqt_mode_known_answers(who, fn):
    n, bpo = 252, 36
    shift = bpo - 3 * (bpo // 12)
    row = fn(M.VQT, n, bpo, np.zeros(n, np.float32))
    assert row.shape == (n, 4) and row.dtype == np.uint8
    assert not row[:, 3].any()                                       # max == 0: every alpha 0 ...
    want = np.array([[M._texel(c) for c in O.consumers.calculate_color(bpo, float((b + shift) % bpo), M.COLORS, 60.0, 1.3)] for b in range(n)])
    assert np.array_equal(row[:, :3], want) and row[:, :3].any()     # ... RGB still the bin colours
    # palette entry A (1.00, 0.96, 0.03) on tone: 255 and 244 as u8, 255 / 255 * 255 * 1.2 and 244 / 255 * 255 * 1.2 both clamp to 255
    on_a = [b for b in range(n) if (b + shift) % bpo == 9 * (bpo // 12)]
    assert on_a and on_a[0] == 0
    assert all(row[b, 0] == 255 and row[b, 1] == 255 for b in on_a)
    x = np.linspace(0.0, 40.0, n).astype(np.float32)
    x[100] = 55.0
    row2 = fn(M.VQT, n, bpo, x)
    assert row2[100, 3] == 255                                       # the row's maximum: (1 - (1 - 55 / 55.001)^2) * 1.5 clamps to 1
    assert row2[0, 3] == 0 and np.array_equal(row2[:, :3], row[:, :3])
    assert np.all(np.diff(row2[:100, 3].astype(int)) >= 0)          # brightness rises with the value
    # half the maximum: (1 - 0.25) * 1.5 = 1.125 -> 1 -> 255; a quarter: (1 - 0.5625) * 1.5 = 0.65625 -> 0.65625 * 306 = 200.8
    x3 = np.zeros(n, np.float32)
    x3[10], x3[20] = 1000.0, 250.0
    assert fn(M.VQT, n, bpo, x3)[20, 3] in (200, 201)


@pytest.mark.parametrize("who,fn", both("spectrogram_row"))
def test_peaks_mode_known_answers(who, fn):
    n, bpo = 252, 36
    assert not fn(M.PEAKS, n, bpo, None, []).any()                   # no peaks
    assert not fn(M.PEAKS, n, bpo, None, [(50.0, 0.0), (80.5, -3.0)]).any()   # all sizes <= 0: max_size > 0 fails
    c = 100
    row = fn(M.PEAKS, n, bpo, None, [(float(c), 7.5)])
    assert list(np.nonzero(row.any(axis=1))[0]) == [c - 2, c - 1, c, c + 1]   # c + 2 is not written: the range is exclusive
    assert list(row[c - 2:c + 2, 3]) == [41, 185, 255, 185]          # exp(-2), exp(-1/2), 1, exp(-1/2), times 306, truncated
    assert len({tuple(px[:3]) for px in row[c - 2:c + 2]}) == 1 and row[c, :3].any()
    # clipped at the edges: floor(0.3 - 2).max(0) = 0 .. ceil(2.3) = 3; floor(n - 2.4) = n - 3 .. ceil(n + 1.6).min(n) = n
    row = fn(M.PEAKS, n, bpo, None, [(0.3, 5.0), (n - 0.4, 5.0)])
    assert list(np.nonzero(row.any(axis=1))[0]) == [0, 1, 2, n - 2, n - 1]   # |n - 3 - (n - 0.4)| = 2.6 > 2
    assert row[0, 3] == M._texel(np.float32(np.exp(np.float32(-0.3 * 0.3 / 2))))
    # two peaks 2.5 bins apart: the later one owns the overlap (bin 102; 103 is 2 from the first but past its exclusive upper bound)
    a, b = (101.0, 9.0), (103.5, 4.0)
    row = fn(M.PEAKS, n, bpo, None, [a, b])
    only_b = fn(M.PEAKS, n, bpo, None, [(0.0, 9.0), b])             # (the same max_size)
    only_a = fn(M.PEAKS, n, bpo, None, [a])
    assert list(np.nonzero(row.any(axis=1))[0]) == [99, 100, 101, 102, 103, 104, 105]
    assert np.array_equal(row[102:106], only_b[102:106]) and np.array_equal(row[99:102], only_a[99:102])
    assert not np.array_equal(only_a[102], only_b[102])
    swapped = fn(M.PEAKS, n, bpo, None, [b, a])                      # list order decides, not the centre
    assert np.array_equal(swapped[102], only_a[102]) and np.array_equal(swapped[103:106], only_b[103:106])
    # a peak in the last bucket
    row = fn(M.PEAKS, n, bpo, None, [(float(n - 1), 2.0)])
    assert list(np.nonzero(row.any(axis=1))[0]) == [n - 3, n - 2, n - 1] and row[n - 1, 3] == 255


@pytest.mark.parametrize("who,fn", both("spectrogram_row"))
def test_nan_gives_zero_bytes(who, fn):
    """f32::max ignores a NaN; `as u8` maps it to 0: the bin's alpha is 0, its neighbours are as without it"""
    n, bpo = 180, 36
    x = np.linspace(1.0, 30.0, n).astype(np.float32)
    clean = fn(M.VQT, n, bpo, x)
    x[40] = np.nan
    row = fn(M.VQT, n, bpo, x)
    assert row[40, 3] == 0 and np.array_equal(row[:, :3], clean[:, :3])
    assert np.array_equal(np.delete(row[:, 3], 40), np.delete(clean[:, 3], 40))
    assert not fn(M.VQT, n, bpo, np.full(n, np.nan, np.float32))[:, 3].any()
    # peaks mode: a NaN size is ignored by the maximum and paints alpha 0; a NaN centre paints nothing
    pk = [(50.0, np.nan), (90.0, 3.0)]
    if who == "host":
        pk.append((np.nan, 3.0))   # (oracle/consumers.py's calculate_color rounds through math.floor, which refuses a NaN)
    row = fn(M.PEAKS, n, bpo, None, pk)
    assert list(np.nonzero(row.any(axis=1))[0]) == [48, 49, 50, 51, 88, 89, 90, 91]
    assert not row[48:52, 3].any() and row[90, 3] == 255
    ch = dict(both("chroma_row"))[who](55.0, n, bpo, x)
    assert np.isnan(ch).any()                                        # the sum carries it, as in the reference


# ---- host against model on rows of an oracle AnalysisState ----------------------------------------------------------------------
def _oracle_state_rows(geom, seed, n_rows):
    """the recipe of tests/test_consumers_gpu.py without a GPU: synth.piano_roll + noise -> oracle VQT dB frames ->
    oracle.analysis_state.OracleAnalysisState"""
    _, op = get_geom(geom)
    hop = 2048
    pcm, _ = piano_roll(op.sr, (3 * n_rows + 1) * hop / op.sr, seed)
    pcm = (pcm * 2.0 + white_noise(pcm.size, seed, amp=0.004)).astype(np.float32)
    db = O.OracleVqt(op).calculate_batch(pcm, hop, 3 * n_rows)
    return op, M.oracle_rows(op.min_freq, op.octaves, op.buckets_per_octave, n_rows, seed, db_frames=db)


@pytest.mark.parametrize("geom,seed", [("serial_22k_180", 21), ("bench_48k_252", 22), ("default_22k_588", 23)])
def test_host_matches_model_on_analysis_state_rows(geom, seed):
    op, (smoothed, peaks) = _oracle_state_rows(geom, seed, 24)
    n, bpo = op.octaves * op.buckets_per_octave, op.buckets_per_octave
    assert sum(len(p) for p in peaks) >= 24 and smoothed.max() > 10.0           # the stimulus really lights the row
    got = {"vqt": [], "peaks": [], "chroma": []}
    want = {"vqt": [], "peaks": [], "chroma": []}
    for x, pk in zip(smoothed, peaks):
        got["vqt"].append(PC.spectrogram_row(PC.SPECTROGRAM_VQT, n, bpo, x))
        want["vqt"].append(M.spectrogram_row(M.VQT, n, bpo, x))
        got["peaks"].append(PC.spectrogram_row(PC.SPECTROGRAM_PEAKS, n, bpo, None, pk))
        want["peaks"].append(M.spectrogram_row(M.PEAKS, n, bpo, None, pk))
        got["chroma"].append(PC.chroma_row(op.min_freq, n, bpo, x))
        want["chroma"].append(M.chroma_row(op.min_freq, n, bpo, x))
    for k in ("vqt", "peaks"):
        levels, share = M.compare_u8(got[k], want[k])
        print(f"{geom} spectrogram_{k}: host vs model: max {levels} level(s), {share:.2e} of the bytes differ")
        assert levels <= U8_LEVELS and share <= U8_SHARE, (k, levels, share)
    assert np.asarray(want["peaks"]).any()
    g, w = np.asarray(got["chroma"], np.float64), np.asarray(want["chroma"], np.float64)
    rel = float(np.max(np.abs(g - w) / w))
    print(f"{geom} chroma: host vs model: max relative difference {rel:.2e}")
    assert rel <= CHROMA_REL and np.all(w.max(axis=1) == 1.0)


# ---- crafted rows (tests/render_cases.py): the builder's own conditions, then host against model ---------------------------------
CRAFTED = [(61.74, 2, 24), (55.0, 7, 36), (32.70, 16, 64)]   # 48, 252 and 1024 bins: one 64-chunk of bins, the benchmark's, sixteen


def test_class_table_reaches_every_class_and_four_pitch_classes():
    ns = [o * b for _, o, b in RC.CLASS_TABLE]
    assert sorted({(n + 63) // 64 for n in ns}) == list(range(1, 17))
    assert {3, 64, 65, 128, 961, 1024} <= set(ns)                                # both ends of NK = 1 (3: the admitted end), 2 and 16
    bpos = [b for _, _, b in RC.CLASS_TABLE]
    assert min(bpos) < 12 and max(bpos) > 100 and any(b > 12 and b % 12 for b in bpos)
    classes = {M.bin_0_pitch_class(f) for f, _, _ in RC.CLASS_TABLE}
    assert {0, 11} <= classes and len(classes) >= 4, classes
    for f, o, b in RC.CLASS_TABLE:                                               # the host's class: a row whose only energy is bin 0
        x = np.full(o * b, -1000.0, np.float32)
        x[0] = 10.0
        assert int(np.argmax(PC.chroma_row(f, o * b, b, x))) == M.bin_0_pitch_class(f), f
        n = o * b
        _, lists = RC.class_rows(n, n)
        assert (len(lists[3]) > 64) == (n >= 100) and all(0.0 <= c < n for pk in lists for c, _ in pk)


@pytest.mark.parametrize("min_freq,octaves,bpo", CRAFTED)
def test_crafted_lists_depend_on_their_order(min_freq, octaves, bpo):
    """Conditions on the INPUTS, from the model alone: reversing any crafted list repaints at least 5 % of the bytes either picture
    lights (observed: spectrogram 64 - 95 %, LED 6 - 34 %), and the two orders of the chunk-straddling pair differ in the contested
    bin.  A kernel that ignored list order could not pass on such lists."""
    n = octaves * bpo
    cases = RC.list_cases(n, n)
    assert ("straddle_pq" in cases) == (n >= 97) and len(cases) >= 12
    assert n < 140 or {len(pk) for pk in cases.values()} >= set(RC.LONG_COUNTS)
    for name, pk in cases.items():
        assert all(0.0 <= c < n for c, _ in pk) and len({s for _, s in pk}) == len(pk), name
        gaps = np.diff(sorted(c for c, _ in pk))
        assert gaps.min() >= 1.0 and (name.startswith("straddle") or 1.249 <= gaps.min() and gaps.max() <= 3.001), (name, gaps.min(), gaps.max())
        spec, led = RC.order_dependence(n, bpo, pk)
        print(f"{n} bins, {name} ({len(pk)} peaks): reversal repaints {spec:.3f} of the spectrogram bytes, {led:.3f} of the LED bytes")
        assert spec >= RC.MIN_ORDER_SHARE and led >= RC.MIN_ORDER_SHARE, (name, spec, led)
    if "straddle_pq" in cases:
        a, b, B = RC.straddle_pair(n, n)
        assert a == cases["straddle_pq"] and a[:63] == b[:63] and a[65:] == b[65:] and (a[63], a[64]) == (b[64], b[63])
        (sa, la), (sb, lb) = RC.model_of_peaks(n, bpo, a), RC.model_of_peaks(n, bpo, b)
        assert np.any(sa[B, :3] != sb[B, :3]) and np.any(la[3 + 3 * B:6 + 3 * B] != lb[3 + 3 * B:6 + 3 * B])
        only_q = RC.model_of_peaks(n, bpo, a[:63] + [a[64]] + a[65:])[0]           # P then Q: Q's pixel stands; Q then P: not Q's
        assert np.array_equal(sa[B], only_q[B]) and not np.array_equal(sb[B], only_q[B])


def _host_rows(min_freq, n, bpo, xs, peak_lists):
    led = lambda pk: np.frombuffer(PC.led_frame(n, bpo, pk, PC.COLORS, PC.GRAY_LEVEL, PC.EASING_POW), np.uint8)
    return {"spectrogram_vqt": np.asarray([PC.spectrogram_row(PC.SPECTROGRAM_VQT, n, bpo, x) for x in xs]),
            "chroma": np.asarray([PC.chroma_row(min_freq, n, bpo, x) for x in xs]),
            "spectrogram_peaks": np.asarray([PC.spectrogram_row(PC.SPECTROGRAM_PEAKS, n, bpo, None, pk) for pk in peak_lists]),
            "led": np.asarray([led(pk) for pk in peak_lists])}


def hold_to_the_bars(tag, got, want, who="host"):
    """the file's bars on the four outputs of a set of rows; chroma: NaN / inf where the model has them, the rest within CHROMA_REL"""
    for k in ("spectrogram_vqt", "spectrogram_peaks", "led"):
        assert got[k].shape == want[k].shape and got[k].dtype == np.uint8
        levels, share = M.compare_u8(got[k], want[k])
        print(f"{tag} {k}: {who} vs model: max {levels} level(s), {share:.2e} of the bytes differ")
        assert levels <= U8_LEVELS and share <= U8_SHARE, (tag, k, levels, share)
    same = int(sum(np.array_equal(g, w) for g, w in zip(got["led"], want["led"])))
    print(f"{tag} led: {same}/{len(want['led'])} rows byte-identical")   # (a figure: crafted rows hold hundreds of peaks)
    rel = RC.chroma_agrees(got["chroma"], want["chroma"], CHROMA_REL)
    print(f"{tag} chroma: {who} vs model: max relative difference {rel:.2e}")


@pytest.mark.parametrize("min_freq,octaves,bpo", CRAFTED)
def test_host_matches_model_on_crafted_rows(min_freq, octaves, bpo):
    """the sequential loops of the host face — the device's second reference — on long lists in every order and on the edge rows"""
    n = octaves * bpo
    cases = RC.list_cases(n, n)
    xs = list(RC.db_rows(n, n).values())
    lists = list(cases.values())
    hold_to_the_bars(f"{n} bins, lists", _host_rows(min_freq, n, bpo, xs, lists), RC.model_rows(min_freq, n, bpo, xs, lists))
    edge = RC.edge_rows(n, n)
    xs, lists = [x for x, _ in edge.values()], [pk for _, pk in edge.values()]
    got, want = _host_rows(min_freq, n, bpo, xs, lists), RC.model_rows(min_freq, n, bpo, xs, lists)
    hold_to_the_bars(f"{n} bins, edges", got, want)
    check_edge_rows(n, edge, got)


def check_edge_rows(n, edge, got):
    """known answers of the edge rows (RC.edge_rows): a NaN brightness is a 0 byte; sizes all zero paint nothing"""
    names = list(edge)
    at = (2 * n) // 3
    for name in ("db_nan", "db_plus_inf"):                                        # NaN; inf / (inf + 0.001) -> NaN
        assert got["spectrogram_vqt"][names.index(name), at, 3] == 0 and got["spectrogram_vqt"][names.index(name), at, :3].any()
        assert np.isnan(got["chroma"][names.index(name)]).any()
    assert not got["spectrogram_vqt"][names.index("db_negative"), :, 3].any()     # max_val stays 0
    assert np.isfinite(got["chroma"][names.index("db_negative")]).all() and got["chroma"][names.index("db_negative")].max() == 1.0
    assert np.isnan(got["chroma"][names.index("db_overflow")]).sum() == 1         # inf / inf in one class, 0 in the others
    for name in ("edges_all_zero", "short_all_zero"):
        r = names.index(name)
        assert not got["spectrogram_peaks"][r].any() and not got["led"][r, 3:].any()   # max_size > 0 fails; 0 / 0 -> NaN -> 0
    for name in ("edges_equal", "short_one_zero", "edges_reversed"):
        r = names.index(name)
        assert got["spectrogram_peaks"][r].any() and got["led"][r, 3:].any()
    assert np.all(got["led"][:, 0] == 0xFF) and np.all(got["led"][:, 1].astype(int) * 256 + got["led"][:, 2] == n)
