"""Every bin-count class of the hot path's kernels, at its edges, against the oracle.

Four stages pick a kernel instantiation from the bin count, each compiling its class's bounds in (a fixed LDS row stride, a
fixed register count, `__builtin_assume`):

  kernel product + dB, block-DFT fp32   blockdft_dots.hip  <= 256 lds260 | 257-304 lds308 | 305-368 lds372 | 369-592 lds596 |
                                                           593-848 lds852 | 849-1020 lds1028 | 1021-1024 db1x8 (banddots_db<1, 8>)
  the same, split-bf16 GEMM             blockdft_dots.hip  <= 256 bf2x4 | 257-1024 bf1x4
  peaks (launch_peaks_frames)           peaks_frames.hip   lean kernel NK in {4, 5, 6, 8, 10, 12, 16} x DENSE (n > 64 (NK - 1)) x DIST
                                                           (min_distance > 1); the generic kernel behind it <4/8/12/16>
  AnalysisBatch                         analysis_batch.hip ab_recurrence<NK, DENSE>, ab_frames<NK, DIST, DENSE>, NK in {4, 6, 8, 10, 12, 16}

and the FFT path's dB epilogue covers max(1024, 4 T) bins with T threads per frame (fftdb: up to 1 024 bins, fftdb-wide: more).

VQT_ROWS and AB_ROWS below are the one table of geometries: the GPU tests here run it, tests/test_bin_classes.py restates the
dispatch rules in Python, reads their thresholds out of the kernel sources and checks that every row lands in the classes it
claims and that every class has rows at both of its edges (EDGE_NOTES says why an edge itself cannot be built and which count
stands in for it)."""
import numpy as np
import pytest

import oracle as O
import pitchvis_amd as P
from oracle import model_f64 as MF
from helpers import geom_pair, mask_to_indices, white_noise

pytestmark = pytest.mark.gpu

FFT, BD32, BD16 = "fft", "bd32", "bd16"
BD = (FFT, BD32, BD16)

# VQT geometries: (sr, min_freq, octaves, bpo, bins, hop, claimed classes, paths).  The block-DFT paths run where a power-of-two hop
# (64 ... 4096) divides every window, at most 256 hop blocks per window; rows above 1 024 bins run the FFT path only.
VQT_ROWS = [
    (22050.0, 440.0, 3, 1, 3, 64, ("lds260", "bf2x4", "pk4s-nodist", "fftdb"), BD),          # windows 256 ... 64
    (22050.0, 110.0, 6, 2, 12, 256, ("pk4s-nodist", "fftdb"), (FFT,)),                        # a 32-sample window: no block-DFT hop
    (96000.0, 55.0, 9, 7, 63, 128, ("lds260", "bf2x4", "pk4s-nodist", "fftdb"), BD),         # 8 window groups
    (48000.0, 440.0, 5, 13, 65, 256, ("lds260", "bf2x4", "pk4s-nodist", "fftdb"), BD),
    (48000.0, 55.0, 8, 32, 256, 256, ("lds260", "bf2x4", "pk4d-nodist", "fftdb"), BD),
    (22050.0, 440.0, 1, 257, 257, 256, ("lds308", "bf1x4", "pk5d-dist", "fftdb"), BD),
    (48000.0, 55.0, 8, 38, 304, 256, ("lds308", "bf1x4", "pk5d-nodist", "fftdb"), BD),
    (48000.0, 440.0, 5, 61, 305, 256, ("lds372", "bf1x4", "pk5d-dist", "fftdb"), BD),
    (96000.0, 110.0, 8, 46, 368, 256, ("lds372", "bf1x4", "pk6d-dist", "fftdb"), BD),
    (96000.0, 55.0, 9, 41, 369, 256, ("lds596", "bf1x4", "pk6d-nodist", "fftdb"), BD),
    (96000.0, 110.0, 8, 74, 592, 256, ("lds596", "bf1x4", "pk10d-dist", "fftdb"), BD),
    (22050.0, 440.0, 1, 593, 593, 256, ("lds852", "bf1x4", "pk10d-dist", "fftdb"), BD),
    (96000.0, 55.0, 9, 66, 594, 256, ("lds852", "bf1x4", "pk10d-dist", "fftdb"), BD),
    (48000.0, 55.0, 8, 106, 848, 256, ("lds852", "bf1x4", "pk16s-dist", "fftdb"), BD),
    (22050.0, 110.0, 3, 283, 849, 256, ("lds1028", "bf1x4", "pk16s-dist", "fftdb"), BD),
    (96000.0, 27.5, 10, 102, 1020, 256, ("lds1028", "bf1x4", "pk16d-dist", "fftdb"), BD),
    (22050.0, 440.0, 1, 1021, 1021, 256, ("db1x8", "bf1x4", "pk16d-dist", "fftdb"), BD),
    (96000.0, 220.0, 7, 146, 1022, 256, ("db1x8", "bf1x4", "pk16d-dist", "fftdb"), BD),
    (96000.0, 110.0, 8, 128, 1024, 256, ("db1x8", "bf1x4", "pk16d-dist", "fftdb"), BD),
    (48000.0, 440.0, 5, 205, 1025, 256, ("fftdb-wide",), (FFT,)),                             # windows 16 384 ...
    (96000.0, 440.0, 6, 180, 1080, 256, ("fftdb-wide",), (FFT,)),                             # windows 32 768 ...
    (22050.0, 880.0, 2, 540, 1080, 256, ("fftdb-wide",), (FFT,)),                             # one 4 096-sample window: T = 128
]

# AnalysisBatch ranges (min_freq 55 Hz, no sample rate: the batch takes a bare VqtRange): (octaves, bpo, bins, claimed classes).  Its
# frame-parallel pre-pass is launch_peaks_frames, so these rows also reach the peak classes no buildable VQT geometry reaches (DIST
# false needs bpo <= 44: 24 octaves and more for 1 024 bins).  One row per edge of every (NK, DENSE, DIST) class.
AB_ROWS = [
    (1, 3, 3, ("ab4s-nodist", "pk4s-nodist")), (6, 32, 192, ("ab4s-nodist", "pk4s-nodist")),
    (1, 45, 45, ("ab4s-dist", "pk4s-dist")), (1, 192, 192, ("ab4s-dist", "pk4s-dist")),
    (5, 39, 195, ("ab4d-nodist", "pk4d-nodist")), (8, 32, 256, ("ab4d-nodist", "pk4d-nodist")),
    (1, 193, 193, ("ab4d-dist", "pk4d-dist")), (1, 256, 256, ("ab4d-dist", "pk4d-dist")),
    (6, 43, 258, ("ab6s-nodist", "pk5d-nodist")), (8, 40, 320, ("ab6s-nodist", "pk5d-nodist")),
    (1, 257, 257, ("ab6s-dist", "pk5d-dist")), (1, 320, 320, ("ab6s-dist", "pk5d-dist")),
    (14, 23, 322, ("ab6d-nodist", "pk6d-nodist")), (12, 32, 384, ("ab6d-nodist", "pk6d-nodist")),
    (1, 321, 321, ("ab6d-dist", "pk6d-dist")), (1, 384, 384, ("ab6d-dist", "pk6d-dist")),
    (11, 35, 385, ("ab8s-nodist", "pk8s-nodist")), (14, 32, 448, ("ab8s-nodist", "pk8s-nodist")),
    (1, 385, 385, ("ab8s-dist", "pk8s-dist")), (1, 448, 448, ("ab8s-dist", "pk8s-dist")),
    (15, 30, 450, ("ab8d-nodist", "pk8d-nodist")), (16, 32, 512, ("ab8d-nodist", "pk8d-nodist")),
    (1, 449, 449, ("ab8d-dist", "pk8d-dist")), (1, 512, 512, ("ab8d-dist", "pk8d-dist")),
    (19, 27, 513, ("ab10s-nodist", "pk10s-nodist")), (16, 36, 576, ("ab10s-nodist", "pk10s-nodist")),
    (1, 513, 513, ("ab10s-dist", "pk10s-dist")), (1, 576, 576, ("ab10s-dist", "pk10s-dist")),
    (17, 34, 578, ("ab10d-nodist", "pk10d-nodist")), (16, 40, 640, ("ab10d-nodist", "pk10d-nodist")),
    (1, 577, 577, ("ab10d-dist", "pk10d-dist")), (1, 640, 640, ("ab10d-dist", "pk10d-dist")),
    (23, 28, 644, ("ab12s-nodist", "pk12s-nodist")), (16, 44, 704, ("ab12s-nodist", "pk12s-nodist")),
    (1, 641, 641, ("ab12s-dist", "pk12s-dist")), (1, 704, 704, ("ab12s-dist", "pk12s-dist")),
    (23, 31, 713, ("ab12d-nodist", "pk12d-nodist")), (24, 32, 768, ("ab12d-nodist", "pk12d-nodist")),
    (1, 705, 705, ("ab12d-dist", "pk12d-dist")), (1, 768, 768, ("ab12d-dist", "pk12d-dist")),
    (22, 35, 770, ("ab16s-nodist", "pk16s-nodist")), (24, 40, 960, ("ab16s-nodist", "pk16s-nodist")),
    (1, 769, 769, ("ab16s-dist", "pk16s-dist")), (1, 960, 960, ("ab16s-dist", "pk16s-dist")),
    (31, 31, 961, ("ab16d-nodist", "pk16d-nodist")), (32, 32, 1024, ("ab16d-nodist", "pk16d-nodist")),
    (1, 961, 961, ("ab16d-dist", "pk16d-dist")), (1, 1024, 1024, ("ab16d-dist", "pk16d-dist")),
]
AB_MAX_OCTAVES = 32   # what "buildable" means for an AnalysisBatch range here

# class edges that no row can sit on: the count that stands in for each, and why
EDGE_NOTES = {
    ("pk4s-dist", 3): (45, "DIST needs bpo >= 45: the smallest such count"),
    ("ab4s-dist", 3): (45, "DIST needs bpo >= 45: the smallest such count"),
    ("pk4d-nodist", 193): (195, "193 is prime and > 44: no octaves x bpo with bpo <= 44"),
    ("ab4d-nodist", 193): (195, "193 is prime and > 44: no octaves x bpo with bpo <= 44"),
    ("pk5d-nodist", 257): (258, "257 is prime"),
    ("ab6s-nodist", 257): (258, "257 is prime"),
    ("pk6d-nodist", 321): (322, "321 = 3 x 107"),
    ("ab6d-nodist", 321): (322, "321 = 3 x 107"),
    ("pk8d-nodist", 449): (450, "449 is prime"),
    ("ab8d-nodist", 449): (450, "449 is prime"),
    ("pk10d-nodist", 577): (578, "577 is prime"),
    ("ab10d-nodist", 577): (578, "577 is prime"),
    ("pk12s-nodist", 641): (644, "641 is prime, 642 = 2 x 3 x 107, 643 is prime"),
    ("ab12s-nodist", 641): (644, "641 is prime, 642 = 2 x 3 x 107, 643 is prime"),
    ("pk12d-nodist", 705): (713, "705 ... 712 have no factor pair with bpo <= 44 and octaves <= 32"),
    ("ab12d-nodist", 705): (713, "705 ... 712 have no factor pair with bpo <= 44 and octaves <= 32"),
    ("pk16s-nodist", 769): (770, "769 is prime"),
    ("ab16s-nodist", 769): (770, "769 is prime"),
    ("fftdb-wide", 4096): (1080, "the tests run 1 025 and 1 080 bins: up to 4 096 the epilogue forms with 512 and 1 024 threads cover "
                                 "the bins, beyond them the FFT path refuses (test_fft_path_refuses_what_no_form_covers)"),
}


def _id(r):
    return f"{r[4]}-{r[6][0]}"


def _vqt(row, device=0):
    sr, fmin, octaves, bpo = row[:4]
    pp, op = geom_pair(sr, fmin, octaves, bpo)
    return P.Vqt.new(pp, device), op


def _set_path(v, path):
    if path == FFT:
        v.set_algo(P.ALGO_FFT)
        return P.ALGO_FFT
    v.set_algo(P.ALGO_BLOCKDFT)
    v.set_gemm_precision(P.GEMM_BF16X3 if path == BD16 else P.GEMM_F32)
    return P.ALGO_BLOCKDFT


def _run(v, d_pcm, hop, nf, lead):
    import torch
    d_db = torch.full((nf, v.n_bins), -1.0, device="cuda")   # a value the dB output never takes: no row may keep it
    d_cx = torch.zeros((nf, v.n_bins, 2), device="cuda")
    v.calculate_batch_db_device(d_pcm, hop, nf, d_db, n_lead=lead, d_out_cplx=d_cx)
    torch.cuda.synchronize()
    return d_db.cpu().numpy(), d_cx.cpu().numpy().view(np.complex64)[..., 0]


_ORACLE = {}


def _oracle(row, hop, nf, lead):
    """white noise, the oracle's dB and complex output, the float64 model's first 8 frames (cached per row: three paths share it)"""
    key = row[:6]
    if key not in _ORACLE:
        _, op = geom_pair(*row[:4])
        ov = O.OracleVqt(op)
        pcm = white_noise(lead + hop * nf, 0xB1C0 + row[4])
        wdb, wcx = ov.calculate_batch(pcm, hop, nf, n_lead=lead, want_complex=True)
        truth = MF.from_oracle_params(op, values_from=ov).batch_complex(pcm, hop, 8, n_lead=lead)
        _ORACLE[key] = (pcm, wdb, wcx, truth)
    return _ORACLE[key]


LEAD = 33003   # no multiple of 4, longer than any window
VQT_PATH_CASES = [pytest.param(r, p, id=f"{_id(r)}-{p}") for r in VQT_ROWS for p in r[7] if r[4] <= 1024]


@pytest.mark.parametrize("row,path", VQT_PATH_CASES)
def test_vqt_parity_per_class_and_path(row, path):
    """130 frames (two whole 64-frame tiles and 2 frames of a third) and 72 (one tile and 8 frames: a partial 32-frame half tile)
    of white noise against the oracle; the float64 model as truth on 8 frames"""
    import torch
    from test_parity_gpu import assert_parity
    v, _ = _vqt(row)
    hop = row[5]
    pcm, wdb, wcx, truth = _oracle(row, hop, 130, LEAD)
    algo = _set_path(v, path)
    d_pcm = torch.from_numpy(pcm).cuda()
    for nf in (130, 72):
        db, cx = _run(v, d_pcm, hop, nf, LEAD)
        assert v.last_algo() == algo, (nf, v.last_algo())
        assert (db != -1.0).all(), (nf, np.argwhere(db == -1.0)[:5])
        assert_parity(db[:8], cx[:8], wdb[:8], wcx[:8], truth)
        assert_parity(db, cx, wdb[:nf], wcx[:nf])


WIDE_CASES = [pytest.param(r, id=f"{r[4]}-{r[0] / 1000:g}k-fftdb-wide") for r in VQT_ROWS if r[4] > 1024]


@pytest.mark.parametrize("row", WIDE_CASES)
def test_fft_path_above_1024_bins(row):
    """Above 1 024 bins only the FFT path runs: a batch of 400 frames (vqt_fft_group + db_rows_batch: at least 64 frames, and more
    than 1 500 (frames per workgroup, window group) pairs, below which the group split takes a batch of several window groups), one of
    20 (the walk, or the group split + db_rows), one frame (calculate_vqt_instant_in_db): every bin of every frame against the oracle"""
    import torch
    from test_parity_gpu import assert_parity
    v, op = _vqt(row)
    hop = row[5]
    assert 400 * len(v.kernel().window_groups) > 1500 or len(v.kernel().window_groups) == 1
    pcm, wdb, wcx, truth = _oracle(row, hop, 400, LEAD)
    d_pcm = torch.from_numpy(pcm).cuda()
    for nf in (400, 20):
        db, cx = _run(v, d_pcm, hop, nf, LEAD)
        assert v.last_algo() == P.ALGO_FFT
        assert (db != -1.0).all(), (nf, np.argwhere(db == -1.0)[:5])
        assert_parity(db[:8], cx[:8], wdb[:8], wcx[:8], truth)
        assert_parity(db, cx, wdb[:nf], wcx[:nf])
    x = white_noise(op.n_fft, 0x1A57 + row[4])
    got, want = v.calculate_vqt_instant_in_db(x), O.OracleVqt(op).calculate_vqt_instant_in_db(x)
    assert got.shape == want.shape == (v.n_bins,)
    assert np.abs(got - want).max() <= 1e-2, float(np.abs(got - want).max())


def test_peaks_and_analysis_refuse_above_1024_bins():
    """1 025 bins: the FFT path computes them, peak detection and AnalysisBatch refuse with PVQ_ERR_UNSUPPORTED (7) and a message,
    their outputs untouched"""
    import torch
    row = next(r for r in VQT_ROWS if r[4] == 1025)
    v, _ = _vqt(row)
    nb = v.n_bins
    assert nb == 1025
    with pytest.raises(P.PvqError) as e:
        v.analyze_batch(np.zeros((4, nb), np.float32))
    assert e.value.status == 7 and P.last_error()
    hop, nf, lead = 256, 16, 16384
    d_pcm = torch.from_numpy(white_noise(lead + hop * nf, 3)).cuda()
    d_db = torch.full((nf, nb), -1.0, device="cuda")
    d_mask = torch.full((nf, (nb + 31) // 32), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((nf,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(P.PvqError) as e:
        v.vqt_analyze_batch_device(d_pcm, hop, nf, d_db, d_mask, d_cnt, n_lead=lead)
    torch.cuda.synchronize()
    assert e.value.status == 7 and P.last_error()
    assert bool((d_db == -1.0).all()) and bool((d_mask == -1).all()) and bool((d_cnt == -1).all())
    with pytest.raises(P.PvqError) as e:
        P.AnalysisBatch(P.VqtRange(440.0, 5, 205), 2)
    assert e.value.status == 7 and P.last_error()


@pytest.mark.parametrize("sr,fmin,octaves,bpo,bins", [pytest.param(22050.0, 55.0, 1, 4097, 4097, id="4097-bins"),
                                                      pytest.param(96000.0, 27.5, 10, 310, 3100, id="3100-bins-lds")])
def test_fft_path_refuses_what_no_form_covers(sr, fmin, octaves, bpo, bins):
    """beyond 4 096 bins (what the dB epilogue covers with 1 024 threads per frame), or where a frame's largest FFT and its bins
    need more than 160 KB of LDS (3 100 bins beside a 16 384-point FFT), the FFT path refuses with PVQ_ERR_UNSUPPORTED and a
    message, for a single frame, a short batch and a long one alike; the output stays untouched"""
    import torch
    pp, _ = geom_pair(sr, fmin, octaves, bpo)
    v = P.Vqt.new(pp, 0)
    assert v.n_bins == bins
    hop = 256
    d_pcm = torch.from_numpy(white_noise(hop * 64, 5)).cuda()
    for nf in (1, 8, 64):
        d_db = torch.full((nf, bins), -1.0, device="cuda")
        with pytest.raises(P.PvqError) as e:
            v.calculate_batch_db_device(d_pcm, hop, nf, d_db)
        torch.cuda.synchronize()
        assert e.value.status == 7 and "FFT path" in P.last_error()
        assert bool((d_db == -1.0).all())


def _tie_frames(n, n_frames, seed):
    """random dB frames with two- and three-sample plateaus (the generic kernel takes the longer ones) and ties at the edges, as
    test_peaks_gpu.py::test_random_ties_two_and_three_sample_plateaus, for any n >= 3"""
    rng = np.random.default_rng(seed)
    frames = np.abs(rng.normal(0, 9, (n_frames, n))).astype(np.float32)
    for f in range(n_frames):
        for _ in range(int(rng.integers(1, 2 + n // 24))):
            ln = 2 if f % 3 else int(rng.integers(2, 5))
            i = int(rng.integers(0, max(n - ln, 0) + 1))
            frames[f, i:i + ln] = frames[f, i]
        if f % 7 == 0:
            frames[f, 0:2] = frames[f, 0]              # tie at the left edge
        if f % 11 == 0:
            frames[f, n - 2:n] = 35.0                  # tie at the right edge: never a peak
        if f % 13 == 0 and n >= 8:
            j = n // 2 - 2
            frames[f, j:j + 2] = 30.0; frames[f, j + 2:j + 4] = 31.0   # rising plateau then a plateau peak
    return frames


PEAK_CASES = [pytest.param(r, id=f"{r[4]}-{next(c for c in r[6] if c.startswith('pk'))}") for r in VQT_ROWS if r[4] <= 1024]


@pytest.mark.parametrize("row", PEAK_CASES)
def test_peaks_per_class(row):
    """Vqt.analyze_batch on random frames with ties: peak indices bit-identical to oracle.analyze_frame, centre and size at the bars
    of test_peaks_gpu.py"""
    v, op = _vqt(row)
    n = v.n_bins
    frames = _tie_frames(n, 96, row[4])
    mask, count, center, size = v.analyze_batch(frames, max_peaks=n)
    for f in range(frames.shape[0]):
        wp, wce, wsz = O.analyze_frame(frames[f], op.min_freq, op.octaves, op.buckets_per_octave)
        assert np.array_equal(mask_to_indices(mask[f], n), wp), f
        assert count[f] == wp.size
        k = wp.size
        ctol = np.maximum(1e-4, 4 * np.spacing(np.abs(wce).astype(np.float32)))
        assert (np.abs(center[f, :k] - wce) <= ctol).all(), f
        assert (np.abs(size[f, :k] - wsz) <= 2e-3 + 40.0 * ctol).all(), f


def _ab_frames(n_streams, n_frames, nb, seed):
    """dB-like frames for any nb >= 3 (test_analysis_batch_gpu.py's _frames needs 7 bins and 200 frames): a noise floor, notes that
    start, hold, glide and stop, a silent stretch, exact ties of neighbours"""
    rng = np.random.default_rng(seed)
    x = (rng.random((n_streams, n_frames, nb), dtype=np.float32) * 6.0).astype(np.float32)
    for s in range(n_streams):
        for _ in range(int(rng.integers(2, 7))):
            b0 = int(rng.integers(1, nb - 1))
            t0 = int(rng.integers(0, n_frames - 8))
            t1 = min(n_frames, t0 + int(rng.integers(8, n_frames)))
            lvl = float(rng.uniform(18.0, 50.0))
            for t in range(t0, t1):
                b = int(np.clip(b0 + (t - t0) // 13 * int(rng.integers(-1, 2)), 1, nb - 2))
                x[s, t, b] = lvl + 0.3 * np.sin(t / 7.0)
                x[s, t, b - 1] = max(x[s, t, b - 1], lvl - 9.0)
                x[s, t, b + 1] = max(x[s, t, b + 1], lvl - 11.0)
        q = int(rng.integers(0, n_frames - 6))
        x[s, q:q + 5] = 0.0
        for t in range(0, n_frames, 5):
            i = int(rng.integers(0, nb - 1))
            x[s, t, i:i + 2] = x[s, t, i]
    return x


AB_CASES = [pytest.param(r, id=f"{r[2]}-{r[3][0]}") for r in AB_ROWS]


@pytest.mark.parametrize("row", AB_CASES)
def test_analysis_batch_per_class(row):
    """AnalysisBatch (pre-pass launch_peaks_frames, ab_recurrence, ab_frames) at every (NK, DENSE, DIST) class edge: every pub field of
    every frame of 4 streams against the oracle, in two calls so that the state carries over"""
    import torch
    from test_analysis_batch_gpu import FIELDS, TOL, _Tally, _alloc_outputs, _compare_stream, _oracle_reference, _to_host
    octaves, bpo, nb, _ = row
    rng_ = P.VqtRange(55.0, octaves, bpo)
    n_streams, n_frames, max_peaks = 4, 40, 64
    dt = 256.0 / 48000.0 * 3
    x = _ab_frames(n_streams, n_frames, nb, 77 + nb)
    d_db = torch.from_numpy(x).cuda()
    b = P.AnalysisBatch(rng_, n_streams)
    outs = _alloc_outputs(n_streams, n_frames, nb, max_peaks)
    cut = 15
    first = {k: t[:, :cut].contiguous() for k, t in outs.items()}
    b.preprocess_device(d_db[:, :cut].contiguous(), cut, dt, first, max_peaks=max_peaks)
    rest = {k: t[:, cut:].contiguous() for k, t in outs.items()}
    b.preprocess_device(d_db[:, cut:].contiguous(), n_frames - cut, dt, rest, max_peaks=max_peaks)
    torch.cuda.synchronize()
    g = _to_host({k: torch.cat([first[k], rest[k]], dim=1) for k in outs}, nb)
    tally = _Tally()
    for s in range(n_streams):
        _compare_stream(tally, g, s, _oracle_reference(rng_, x[s], int(round(dt * 1e9)), "default"), n_frames, max_peaks, TOL, "oracle")
    for k in FIELDS:
        assert np.array_equal(b.field(n_streams - 1, k), g[k][n_streams - 1, -1]), k


@pytest.mark.parametrize("bins", [pytest.param(849, id="849-lds1028"), pytest.param(1020, id="1020-lds1028")])
def test_streams_equal_single_stream_calls_at_the_widest_stride(bins):
    """one many-streams call on the block-DFT path (lds1028: more than 64 KB of dynamic LDS) equals the per-stream calls bit for bit"""
    from test_streams_gpu import _check_equal, _streams
    row = next(r for r in VQT_ROWS if r[4] == bins)
    v, _ = _vqt(row)
    hop = row[5]
    frames = [130, 64, 1, 37, 0, 72]
    leads = [0, 5003, 0, v.window_union - hop, 0, 123]
    pcms = _streams(len(frames), hop, frames, leads, 4000 + bins)
    v.set_algo(P.ALGO_BLOCKDFT)
    _check_equal(v, pcms, hop, frames, leads, stride=160)
    assert v.last_algo() == P.ALGO_BLOCKDFT
