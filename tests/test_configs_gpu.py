"""BASELINE.json configs 3-5 as parity-test cases (config 2 is the bench line, config 1 is
tests/test_parity_gpu.py::test_sweep_parity)."""
import numpy as np
import pytest

import oracle as O
import pitchvis_amd as P
from pitchvis_amd.sharding import plan_shard
from helpers import get_geom, white_noise, mask_to_indices, report
from synth import piano_roll, active_notes
from test_parity_gpu import assert_parity, input_peak

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _run(v, pcm, hop, nf, n_lead=0):
    d_pcm = torch.from_numpy(np.ascontiguousarray(pcm, np.float32)).cuda()
    d_db = torch.empty((nf, v.n_bins), device="cuda")
    words = (v.n_bins + 31) // 32
    d_mask = torch.zeros((nf, words), dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(nf, dtype=torch.int32, device="cuda")
    d_c = torch.zeros((nf, 64), device="cuda")
    d_s = torch.zeros((nf, 64), device="cuda")
    v.vqt_analyze_batch_device(d_pcm, hop, nf, d_db, d_mask, d_cnt, d_c, d_s, 64, n_lead=n_lead)
    torch.cuda.synchronize()
    return (d_db.cpu().numpy(), d_mask.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy(), d_c.cpu().numpy(),
            d_s.cpu().numpy())


@pytest.mark.parametrize("world", [2, 8])
def test_config3_sharded_equals_unsharded(world):
    """config 3 geometry (48 kHz, 8 oct x 36 = 288 bins, hop 256): frame shards with their window-union
    halo reproduce the unsharded batch bit for bit (no collective on the data path)."""
    pp, op = get_geom("bench_48k_288")
    v = P.Vqt.new(pp, 0)
    hop, nf = 256, 8192
    pcm = white_noise(hop * nf, 0x5EED0003)
    full = _run(v, pcm, hop, nf)
    assert v.last_algo() == P.ALGO_BLOCKDFT
    for r in range(world):
        s = plan_shard(nf, hop, v.window_union, r, world)
        part = _run(v, pcm[s.sample_begin:s.sample_end], hop, s.n_frames, n_lead=s.n_lead)
        sl = slice(s.first_frame, s.first_frame + s.n_frames)
        assert np.array_equal(part[0], full[0][sl]) and np.array_equal(part[1], full[1][sl])
        assert np.array_equal(part[2], full[2][sl])
    # spot parity of the unsharded result
    ov = O.OracleVqt(op)
    for f in (0, 63, 4095, nf - 1):
        end = (f + 1) * hop
        x = np.zeros(op.n_fft, np.float32)
        beg = max(end - op.n_fft, 0)
        x[op.n_fft - (end - beg):] = pcm[beg:end]
        assert np.abs(full[0][f] - ov.calculate_vqt_instant_in_db(x)).max() <= 1e-2


@pytest.mark.parametrize("name", ["hires_96k_360", "hires_96k_840"])
def test_config4_96k_stereo_hop128(name):
    """config 4: 96 kHz, hop 128, 10 octaves from 27.5 Hz (55 Hz would exceed Nyquist);
    the reference is mono end to end, so the two channels are two independent streams."""
    pp, op = get_geom(name)
    with pytest.raises(P.AboveNyquist):
        P.Vqt.new(P.VqtParameters(sr=96000.0, range=P.VqtRange(55.0, 10, pp.range.buckets_per_octave)), None)
    v = P.Vqt.new(pp, 0)
    v.set_algo(P.ALGO_BLOCKDFT)   # (left to itself PVQ_ALGO_AUTO sends fewer than 384 frames to the FFT path: 192 per channel here)
    ov = O.OracleVqt(op)
    hop, nf, n_lead = 128, 192, 40000
    chans = [white_noise(n_lead + hop * nf, seed) for seed in (0x5EED0004, 0x5EED0005)]   # left, right
    d_chans = [torch.from_numpy(c).cuda() for c in chans]
    # the stereo pair as ONE many-streams call (pvq_vqt_calculate_batch_db_streams: both channels share every launch) ...
    d_both = torch.empty((2, nf, v.n_bins), device="cuda")
    v.batch_streams_device(d_chans, hop, [nf, nf], d_both, nf, n_leads=[n_lead, n_lead]); torch.cuda.synchronize()
    assert v.last_algo() == P.ALGO_BLOCKDFT  # 256 hop blocks per 32768-sample window
    for ch, (pcm, d_pcm) in enumerate(zip(chans, d_chans)):
        # ... equals the single-stream call channel by channel (which also hands out the complex coefficients for the parity bars)
        d_db = torch.empty((nf, v.n_bins), device="cuda"); d_cx = torch.empty((nf, v.n_bins, 2), device="cuda")
        v.calculate_batch_db_device(d_pcm, hop, nf, d_db, n_lead=n_lead, d_out_cplx=d_cx); torch.cuda.synchronize()
        assert v.last_algo() == P.ALGO_BLOCKDFT
        assert torch.equal(d_both[ch], d_db)
        wdb, wcx = ov.calculate_batch(pcm, hop, nf, n_lead=n_lead, want_complex=True)
        assert_parity(d_both[ch].cpu().numpy(), d_cx.cpu().numpy().view(np.complex64)[..., 0], wdb, wcx,
                      xpeak=input_peak(pcm, hop, nf, n_lead, v.window_union), sr=op.sr)


@pytest.mark.parametrize("algo", [P.ALGO_FFT, P.ALGO_BLOCKDFT])
def test_config4_fp16_twiddles(algo):
    """config 4's "fp16 FFT twiddles" variant: every twiddle factor rounded to IEEE half, fp32 accumulation.  Parity is
    relaxed and reported (expected ~1e-3 relative); switching back restores full parity."""
    pp, op = get_geom("hires_96k_360")
    v = P.Vqt.new(pp, 0)
    v.set_algo(algo)
    ov = O.OracleVqt(op)
    hop, nf, n_lead = 128, 96, 40000
    pcm = white_noise(n_lead + hop * nf, 0x5EED0004)
    d_pcm = torch.from_numpy(pcm).cuda()
    wdb, wcx = ov.calculate_batch(pcm, hop, nf, n_lead=n_lead, want_complex=True)
    fmax = np.abs(wcx).max(axis=1, keepdims=True)

    def run():
        d_db = torch.empty((nf, v.n_bins), device="cuda"); d_cx = torch.empty((nf, v.n_bins, 2), device="cuda")
        v.calculate_batch_db_device(d_pcm, hop, nf, d_db, n_lead=n_lead, d_out_cplx=d_cx); torch.cuda.synchronize()
        return d_db.cpu().numpy(), d_cx.cpu().numpy().view(np.complex64)[..., 0]

    db32, cx32 = run()
    v.set_twiddle_fp16(True)
    db16, cx16 = run()
    v.set_twiddle_fp16(False)
    db32b, cx32b = run()
    e32 = (np.abs(cx32 - wcx) / fmax).max()
    e16 = (np.abs(cx16 - wcx) / fmax).max()
    strong = wdb > 10.0
    print(f"fp16 twiddles ({'fft' if algo == P.ALGO_FFT else 'blockdft'}): rel err {e16:.2e} (fp32 twiddles {e32:.2e}); "
          f"dB err on bins > 10 dB: {np.abs(db16 - wdb)[strong].max():.3f}")
    assert e32 <= 1e-5
    assert 1e-5 < e16 <= 5e-3                      # the quantisation is really in effect, and bounded
    assert np.abs(db16 - wdb)[strong].max() <= 0.1
    assert np.array_equal(cx32, cx32b) and np.array_equal(db32, db32b)


def test_config5_polyphonic_notes():
    """config 5 with a synthetic additive piano roll (no SoundFont / MIDI assets exist here): the note
    lists of the GPU path equal the CPU oracle's, and both recover the ground truth."""
    pp, op = get_geom("bench_48k_252")
    v = P.Vqt.new(pp, 0)
    ov = O.OracleVqt(op)
    pcm, notes = piano_roll(op.sr, 12.0, 5)
    hop = 2048
    nf = len(pcm) // hop
    db, mask, cnt, ctr, sz = _run(v, pcm, hop, nf)
    wdb = ov.calculate_batch(pcm, hop, nf)
    tp = fp = fn = explained = ndet = 0
    mismatched = 0
    for f in range(nf):
        t = (f + 1) * hop / op.sr - v.delay
        truth = set(active_notes(notes, t))
        k = int(cnt[f])
        det = set(int(round(c * 12 / 36)) + 33 for c, s in zip(ctr[f, :k], sz[f, :k]) if s > 12.0)  # A1 = MIDI 33 (train.rs:34)
        _, wce, wsz = O.analyze_frame(wdb[f], op.min_freq, op.octaves, op.buckets_per_octave)
        wdet = set(int(round(c * 12 / 36)) + 33 for c, s in zip(wce, wsz) if s > 12.0)
        mismatched += det != wdet
        if not truth:
            continue
        tp += len(det & truth); fp += len(det - truth); fn += len(truth - det)
        partials = set(int(round(m + 12 * np.log2(h))) for m in truth for h in range(1, 7))
        explained += len(det & partials); ndet += len(det)
    recall, precision, spectral_precision = tp / (tp + fn), tp / (tp + fp), explained / ndet
    report("parity_evidence_r02.txt", f"# config5: note recall {recall:.3f}, note precision {precision:.3f} (overtones count as false), "
          f"peaks explained by a partial of an active note {spectral_precision:.3f}; "
          f"frames whose GPU note list differs from the oracle's: {mismatched}/{nf}")
    assert mismatched <= nf // 50          # only threshold-straddling peaks (size within tolerance of 12 dB) may differ
    assert recall >= 0.9 and spectral_precision >= 0.9


def test_two_handles_two_streams():
    """Handles are independent (one per thread / stream): two of them driven on two non-default streams,
    interleaved, give the same bits as each alone."""
    pp, _ = get_geom("bench_48k_252")
    va, vb = P.Vqt.new(pp, 0), P.Vqt.new(pp, 0)
    hop, nf = 256, 1500
    pa = torch.from_numpy(white_noise(hop * nf, 71)).cuda()
    pb = torch.from_numpy(white_noise(hop * nf, 72)).cuda()
    words = (va.n_bins + 31) // 32

    def bufs():
        return (torch.empty((nf, va.n_bins), device="cuda"), torch.zeros((nf, words), dtype=torch.int32, device="cuda"),
                torch.zeros(nf, dtype=torch.int32, device="cuda"))

    ra, rb = bufs(), bufs()
    va.vqt_analyze_batch_device(pa, hop, nf, *ra)
    vb.vqt_analyze_batch_device(pb, hop, nf, *rb)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    qa, qb = bufs(), bufs()
    for _ in range(3):
        va.vqt_analyze_batch_device(pa, hop, nf, *qa, stream=sa)
        vb.vqt_analyze_batch_device(pb, hop, nf, *qb, stream=sb)
    torch.cuda.synchronize()
    for x, y in zip(ra + rb, qa + qb):
        assert torch.equal(x, y)


def test_gemm_precision_switch_on_one_handle():
    """One handle, one batch shape, fp32 -> split-bf16 -> fp32 GEMM arithmetic (what bench.py does for its `other_gemm` line): the
    two kernels keep their tile lists apart (the fp32 kernel pairs column tiles into 64-column entries, the split-bf16 kernel takes
    32-column tiles only), and each arithmetic gives the bits a fresh handle gives."""
    pp, _ = get_geom("bench_48k_288")
    hop, nf, n_lead = 256, 3000, 16128
    pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 5)).cuda()

    def run(v):
        db = torch.empty((nf, v.n_bins), device="cuda")
        v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead)
        torch.cuda.synchronize()
        return db.cpu().numpy()

    v = P.Vqt.new(pp, 0)
    v.set_algo(P.ALGO_BLOCKDFT)
    a1 = run(v)
    v.set_gemm_precision(P.GEMM_BF16X3)
    b1 = run(v)
    v.set_gemm_precision(P.GEMM_F32)
    a2 = run(v)
    w = P.Vqt.new(pp, 0)
    w.set_algo(P.ALGO_BLOCKDFT)
    w.set_gemm_precision(P.GEMM_BF16X3)
    b0 = run(w)
    assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32))
    assert np.array_equal(b1.view(np.uint32), b0.view(np.uint32))
    loud = a1 > a1.max() - 40
    assert np.abs(a1 - b1)[loud].max() <= 2e-2


def test_tile_list_cache_evicts_and_rebuilds_under_work_in_flight():
    """ONE handle walked through twelve distinct launch shapes and back, without a synchronisation between the calls: (frames, lead,
    stream length, GEMM arithmetic, single stream / several streams, power-of-two / general hop).  The fused kernels' tile lists —
    which tiles lie wholly inside their stream and may take 16-byte loads / pair up — are cached in eight slots keyed on exactly that
    geometry, so this sequence evicts and rebuilds lists while earlier launches are still queued.  Round 3's in-round GPU fault
    ("The tile-list fault of round 3") was a list reused for a geometry it was not built for; here every call must give
    the bits a FRESH handle gives for the same shape, on the first pass and on the way back."""
    pp, _ = get_geom("bench_48k_252")
    hop = 256
    shapes = [  # (frames, lead, arithmetic, n_streams, hop)
        (3000, 0, P.GEMM_F32, 1, 256), (3000, 16128, P.GEMM_F32, 1, 256), (1000, 0, P.GEMM_F32, 1, 256), (1000, 500, P.GEMM_BF16X3, 1, 256),
        (5000, 0, P.GEMM_F32, 1, 256), (3000, 0, P.GEMM_BF16X3, 1, 256), (700, 123, P.GEMM_F32, 3, 256), (2999, 0, P.GEMM_F32, 1, 256),
        (4000, 0, P.GEMM_F32, 1, 256), (2000, 300, P.GEMM_F32, 1, 256), (1500, 0, P.GEMM_BF16X3, 1, 256),
        (600, 77, P.GEMM_F32, 1, 1600),
    ]
    pcms = {}
    for i, (nf, lead, _, ns, hp) in enumerate(shapes):
        pcms[i] = [torch.from_numpy(white_noise(lead + hp * nf, 900 + 7 * i + s)).cuda() for s in range(ns)]

    def call(v, i, out):
        nf, lead, arith, ns, hp = shapes[i]
        v.set_gemm_precision(arith)
        if ns == 1:
            v.calculate_batch_db_device(pcms[i][0], hp, nf, out[0], n_lead=lead)
        else:
            v.batch_streams_device(pcms[i], hp, [nf] * ns, out, nf, n_leads=[lead] * ns)

    v = P.Vqt.new(pp, 0)
    v.set_algo(P.ALGO_BLOCKDFT)
    order = list(range(len(shapes))) + list(range(len(shapes) - 1, -1, -1)) + [0, 4, 1, 6, 11, 3, 9]
    outs = []
    for i in order:   # no synchronisation in between: the next call's list upload meets the previous launches still in flight
        o = torch.full((shapes[i][3], shapes[i][0], v.n_bins), -1.0, device="cuda")
        call(v, i, o)
        outs.append((i, o))
    torch.cuda.synchronize()
    v.input_status()
    fresh = {}
    for i in range(len(shapes)):
        w = P.Vqt.new(pp, 0)
        w.set_algo(P.ALGO_BLOCKDFT)
        o = torch.full((shapes[i][3], shapes[i][0], v.n_bins), -1.0, device="cuda")
        call(w, i, o)
        torch.cuda.synchronize()
        fresh[i] = o
    for i, o in outs:
        assert torch.equal(o, fresh[i]), (i, shapes[i], int((o != fresh[i]).sum()))


def test_unfused_fallback_stages_in_a_subprocess():
    """The unfused GEMM + combine stages (taken when a geometry has more than 8 window groups; developer knob
    PVQ_NO_FUSE=1) against the FFT path, in a child process because the knob is read once per process."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, os
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        import numpy as np, torch
        import pitchvis_amd as P
        from helpers import get_geom, white_noise
        for name, hop in (("bench_48k_252", 256), ("hires_96k_360", 128)):
            pp, op = get_geom(name)
            v = P.Vqt.new(pp, 0)
            nf, n_lead = 200, 70000   # full windows from the first frame on (n_fft <= 65536)
            pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 5)).cuda()
            out = {}
            for algo in (P.ALGO_BLOCKDFT, P.ALGO_FFT):
                v.set_algo(algo)
                cx = torch.zeros((nf, v.n_bins, 2), device="cuda")
                db = torch.empty((nf, v.n_bins), device="cuda")
                v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead, d_out_cplx=cx)
                torch.cuda.synchronize()
                assert v.last_algo() == algo
                out[algo] = cx.cpu().numpy().view(np.complex64)[..., 0]
                launches = v.last_kernel_launches() if hasattr(v, "last_kernel_launches") else {}
            a, b = out[P.ALGO_BLOCKDFT], out[P.ALGO_FFT]
            err = (np.abs(a - b) / np.abs(b).max(axis=1, keepdims=True)).max()
            assert err <= 1e-5, (name, err)
        print("UNFUSED_OK")
    """)
    env = dict(os.environ, PVQ_NO_FUSE="1", PVQ_DEV_LIB="1")   # the developer library: the product build reads no environment
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "UNFUSED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_tile_shapes_bit_identical_in_subprocesses():
    """Every tile shape of the hop-DFT + tree stage computes the same bits on every test geometry — same sums, same k order, same
    tree levels: a frame's value must not depend on the tile that produced it.  The product (256 rows, neighbouring column tiles
    paired into 64-column wide tiles except at the stream's ends and in the launch's tail, queues evened out; 128 x 32 rows for a
    launch of fewer than ~1 400 tiles), 128 x 32 rows always (PVQ_FUSED_BM=128), 256 rows always (=256), 256 x 32 only (PVQ_WIDE=0,
    unbalanced queues), wide tiles wherever they fit (PVQ_WIDE=2) — knobs of the
    developer library libpvq_dev.so — and the product library against the developer one.
    Child processes: the knobs are read once per process."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys, os
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        import numpy as np, torch
        import pitchvis_amd as P
        from helpers import GEOMS, get_geom, white_noise
        out = {}
        for name in GEOMS:
            pp, op = get_geom(name)
            hop = 128 if op.sr > 90000 else 256
            v = P.Vqt.new(pp, 0)
            v.set_algo(P.ALGO_BLOCKDFT)
            nf, n_lead = 1500, 777
            pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 11)).cuda()
            cx = torch.zeros((nf, v.n_bins, 2), device="cuda")
            db = torch.empty((nf, v.n_bins), device="cuda")
            v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead, d_out_cplx=cx)
            torch.cuda.synchronize()
            out[name + "_db"] = db.cpu().numpy()
            out[name + "_cx"] = cx.cpu().numpy()
        # other hops on one geometry: 64 (one double k group per tile: the K loops' shortest form), 512 and 1024 (the slice of E is
        # staged in two / four passes; 1024 = the shortest window: no tree level at all in its group)
        pp, op = get_geom("bench_48k_252")
        for hop in (64, 512, 1024, 1600, 800):   # (1 600, 800: the general-hop kernel, blockdft_gemm_gen)
            v = P.Vqt.new(pp, 0)
            v.set_algo(P.ALGO_BLOCKDFT)
            nf, n_lead = 40000 // (hop // 64), 333
            pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 13)).cuda()
            db = torch.empty((nf, v.n_bins), device="cuda")
            v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead)
            torch.cuda.synchronize()
            out["hop%d_db" % hop] = db.cpu().numpy()
        np.savez(sys.argv[1], **out)
        print("FORM_OK")
    """)
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    res = {}
    for tag, env in (("base", {}), ("dev", {"PVQ_DEV_LIB": "1"}), ("bm128", {"PVQ_DEV_LIB": "1", "PVQ_FUSED_BM": "128"}), ("bm256", {"PVQ_DEV_LIB": "1", "PVQ_FUSED_BM": "256"}),
                     ("narrow", {"PVQ_DEV_LIB": "1", "PVQ_WIDE": "0", "PVQ_BALANCE": "0"}), ("wide_all", {"PVQ_DEV_LIB": "1", "PVQ_WIDE": "2"})):
        f = os.path.join(root, "gpurun_out", f"forms_{tag}.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0 and "FORM_OK" in r.stdout, tag + r.stdout[-2000:] + r.stderr[-2000:]
        res[tag] = dict(np.load(f))
        os.remove(f)
    for tag in ("dev", "bm128", "bm256", "narrow", "wide_all"):
        for k, a in res["base"].items():
            assert np.array_equal(a.view(np.uint32), res[tag][k].view(np.uint32)), (tag, k)


def test_fft_batch_kernels_equal_the_walk_in_subprocesses():
    """The FFT path's batch form (vqt_fft_group: one kernel instantiation per window size, round 5) against the walk (vqt_fft_frames, which the
    developer library keeps for batches too with PVQ_FFT_CT=0): the same bits on every test geometry, at a power-of-two hop and at an odd one
    (735 = pitchvis_serial's cadence at 22 050 Hz), stream start included.  Both forms share every arithmetic helper and fft_path.hip
    compiles with FMA contraction off (fused multiply-adds are written where wanted), so this holds by construction; the test keeps it so.
    (tests/test_handles_gpu.py::test_few_frames_on_the_fft_path_equal_the_same_frames_of_a_batch compares the few-frames forms of the walk with
    the batch form in one process.)"""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys, os
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        import numpy as np, torch
        import pitchvis_amd as P
        from helpers import GEOMS, get_geom, white_noise
        out = {}
        for name in GEOMS:
            pp, op = get_geom(name)
            for hop in ((128 if op.sr > 90000 else 256), 735):
                v = P.Vqt.new(pp, 0)
                v.set_algo(P.ALGO_FFT)
                nf, n_lead = 2500, 0 if hop == 735 else 4321
                pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 17)).cuda()
                cx = torch.zeros((nf, v.n_bins, 2), device="cuda")
                db = torch.empty((nf, v.n_bins), device="cuda")
                v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead, d_out_cplx=cx)
                torch.cuda.synchronize()
                out[f"{name}_{hop}_db"] = db.cpu().numpy()
                out[f"{name}_{hop}_cx"] = cx.cpu().numpy()
        np.savez(sys.argv[1], **out)
        print("FFT_OK")
    """)
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    res = {}
    for tag, env in (("batch", {}), ("walk", {"PVQ_DEV_LIB": "1", "PVQ_FFT_CT": "0"})):
        f = os.path.join(root, "gpurun_out", f"fftforms_{tag}.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0 and "FFT_OK" in r.stdout, tag + r.stdout[-2000:] + r.stderr[-2000:]
        res[tag] = dict(np.load(f))
        os.remove(f)
    for k, a in res["batch"].items():
        assert np.array_equal(a.view(np.uint32), res["walk"][k].view(np.uint32)), k


@pytest.mark.parametrize("name", ["default_22k_588", "bench_48k_252", "bench_48k_288", "hires_96k_360", "hires_96k_840", "serial_22k_180"])
def test_same_input_same_output_every_geometry(name):
    """Reference convention: same input => same output.  Three runs of the whole path per geometry and
    arithmetic, every output compared bit for bit (scripts/dev_soak.py is the long version of this)."""
    pp, op = get_geom(name)
    hop = 128 if op.sr > 90000 else 256
    nf, n_lead = 6000, 321
    d_pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 31)).cuda()
    for prec in (P.GEMM_F32, P.GEMM_BF16X3):
        v = P.Vqt.new(pp, 0)
        v.set_algo(P.ALGO_BLOCKDFT); v.set_gemm_precision(prec)
        words = (v.n_bins + 31) // 32
        ref = None
        for _ in range(3):
            d_db = torch.empty((nf, v.n_bins), device="cuda"); d_cx = torch.empty((nf, v.n_bins, 2), device="cuda")
            d_mask = torch.zeros((nf, words), dtype=torch.int32, device="cuda"); d_cnt = torch.zeros(nf, dtype=torch.int32, device="cuda")
            d_c = torch.zeros((nf, 64), device="cuda"); d_s = torch.zeros((nf, 64), device="cuda")
            v.calculate_batch_db_device(d_pcm, hop, nf, d_db, n_lead=n_lead, d_out_cplx=d_cx)
            v.analyze_batch_device(d_db, nf, d_mask, d_cnt, d_c, d_s, 64)
            torch.cuda.synchronize()
            cur = (d_db, d_cx, d_mask, d_cnt, d_c, d_s)
            if ref is None:
                ref = cur
            else:
                assert all(torch.equal(a, b) for a, b in zip(ref, cur)), (name, prec)


def test_config3_full_size_shard_on_one_gpu():
    """BASELINE configs[2] at its real per-GPU size: rank 3 of 8's shard of the 1 M-hop stream (seed 0x5EED0003, 48 kHz,
    8 x 36 = 288 bins, hop 256): 131 072 frames with their 16 128-sample halo, exactly what bench.py --gpus 8 hands that
    rank.  Size-independent properties (the same stream analysed without the shard cut gives the same bits around both
    shard edges; determinism; finite, 0..60 dB) plus oracle spot frames at the edges and inside."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pitchvis_amd.sharding import stream_slice
    pp, op = get_geom("bench_48k_288")
    v = P.Vqt.new(pp, 0)
    hop, F, world, rank = 256, 131072, 8, 3
    s = plan_shard(world * F, hop, v.window_union, rank, world)
    assert s.n_frames == F and s.n_lead == v.window_union - hop == 16128
    # the stream around this shard (the whole 1 GiB stream is never needed: it is a function of the sample index)
    s_lo, s_hi = s.sample_begin - 2048 * hop - 40000, s.sample_end + 2048 * hop
    around = stream_slice(0x5EED0003, s_lo, s_hi, "cuda")

    class _Stream:   # global sample indices into the piece that was generated
        def __getitem__(self, sl):
            return around[sl.start - s_lo:sl.stop - s_lo]
    stream = _Stream()
    d_pcm = stream[s.sample_begin:s.sample_end].clone()
    words = (v.n_bins + 31) // 32

    def run(pcm, nf, n_lead):
        d_db = torch.empty((nf, v.n_bins), device="cuda")
        d_mask = torch.zeros((nf, words), dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(nf, dtype=torch.int32, device="cuda")
        v.vqt_analyze_batch_device(pcm, hop, nf, d_db, d_mask, d_cnt, n_lead=n_lead)
        torch.cuda.synchronize()
        return d_db, d_mask, d_cnt

    a = run(d_pcm, F, s.n_lead)
    assert v.last_algo() == P.ALGO_BLOCKDFT and v.last_frames_per_launch() == 131072   # one sub-batch per rank
    b = run(d_pcm, F, s.n_lead)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                                  # same input, same output
    assert torch.isfinite(a[0]).all() and float(a[0].min()) >= 0.0 and float(a[0].max()) <= 60.0 and int(a[2].sum()) > F
    v.input_status()
    # the unsharded stream around both edges of the shard: 4 096 frames straddling each, with all the history they want
    for edge in (s.first_frame, s.first_frame + F):
        f0 = edge - 2048
        lead = min(f0 * hop, 40000)
        piece = stream[f0 * hop - lead:(f0 + 4096) * hop]
        c = run(piece, 4096, lead)
        lo, hi = max(f0, s.first_frame), min(f0 + 4096, s.first_frame + F)
        for x, y in zip(a, c):
            assert torch.equal(x[lo - s.first_frame:hi - s.first_frame], y[lo - f0:hi - f0])
    # oracle spot frames
    ov = O.OracleVqt(op)
    host = stream[s.sample_begin:s.sample_end].cpu().numpy()
    db = a[0].cpu().numpy()
    mask = a[1].cpu().numpy().view(np.uint32)
    for f in (0, 1, 65535, 65536, 99999, F - 1):
        end = s.n_lead + (f + 1) * hop
        beg = max(end - op.n_fft, 0)
        x = np.zeros(op.n_fft, np.float32)
        x[op.n_fft - (end - beg):] = host[beg:end]
        wdb = ov.calculate_vqt_instant_in_db(x)
        assert np.abs(db[f] - wdb).max() <= 1e-2 and np.abs(db[f] - wdb)[wdb > wdb.max() - 20].max() <= 2e-3
        assert np.array_equal(mask_to_indices(mask[f], v.n_bins), O.find_peaks_split(db[f], 36))


def test_bench_two_ranks_gloo_on_one_gpu():
    """bench.py's N > 1 path end to end on the one-GPU box: two ranks (both on cuda:0, gloo for the barrier and the
    max-over-ranks reduce) on two consecutive shards of one stream.  The 8-GPU RCCL run is the driver's; this checks that the
    line it will get is well-formed and that `value` at N = 2 is measured on the SAME workload as at N = 1 (BASELINE
    configs[1], what the metric is quoted on: a 1 -> 8 curve must compare like with like), with configs[2] under its extra key."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    common = ["--steps", "3", "--warmup", "1", "--frames", "16384", "--full"]   # (--full: roofline and the config2 key)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo"] + common
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--no-cpu-baseline"] + common, capture_output=True, text=True,
                        timeout=600, cwd=root)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-3000:]
    j1 = json.loads([ln for ln in r1.stdout.splitlines() if ln.startswith("{")][-1])
    # the headline of both lines is BASELINE configs[1], word for word the same workload
    assert j["config"]["workload"] == j1["config"]["workload"] == bench.WORKLOADS[1]["name"].format(F=16384, T=0, N=0)
    assert "configs[1]" in j["config"]["workload"] and j["config"]["n_bins"] == j1["config"]["n_bins"] == 252
    assert j["n_gpus"] == 2 and j1["n_gpus"] == 1 and j["scaling"] == j1["scaling"] == "weak"
    assert j["config"]["frames_per_gpu_per_step"] == j1["config"]["frames_per_gpu_per_step"] == 16384
    for line, n in ((j, 2), (j1, 1)):
        assert line["value"] > 0 and 0 < line["roofline"]["frac"] <= 1.0 and line["roofline"]["bound"] == "mfma"
        assert abs(line["value"] - n * 16384 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-3
    # configs[2] rides along under its own key, on the same N
    c2, c21 = j["config2"], j1["config2_single_gpu"]
    assert c2["n_bins"] == c21["n_bins"] == 288 and "configs[2]" in c2["workload"] and c2["n_gpus"] == 2 and c21["n_gpus"] == 1
    assert abs(c2["value"] - 2 * 16384 * 3 / (c2["ms_per_step"] * 3e-3)) / c2["value"] < 1e-3


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """bench.py without --full: the headline line alone, and --dump-outputs writes what the timed path computed — the same bits this
    process gets from one call of the path on the same seeded input."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from pitchvis_amd.sharding import stream_slice
    F = 16384
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--frames", str(F),
                        "--settle-ms", "0", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["metric"] == "vqt_frames_per_sec" and j["unit"] == "frames/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["steps"] == 3 and j["value"] > 0 and abs(j["value"] - F * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 1e-3
    assert not {"roofline", "alt_gemm", "cold_start", "config2_single_gpu", "cpu_baseline"} & set(j)
    got = {n[:-4]: np.load(os.path.join(tmp_path, n)) for n in os.listdir(tmp_path)}
    assert set(got) == {"frames", "db", "peaks", "peak_count", "peak_center", "peak_size"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["frames"], np.arange(F))   # (F <= the sample size: every frame)
    # the same step in this process: the bench's workload, its shard, its settings
    W = bench.WORKLOADS[1]
    v = P.Vqt.new(P.VqtParameters(sr=bench.SR, range=P.VqtRange(55.0, W["octaves"], 36)), 0)
    v.set_algo(P.ALGO_AUTO); v.set_gemm_precision(P.GEMM_F32)
    s = plan_shard(F, bench.HOP, v.window_union, 0, 1)
    d_pcm = stream_slice(W["seed"], s.sample_begin, s.sample_end, "cuda")
    db, mask, cnt, ctr, sz = _run(v, d_pcm.cpu().numpy(), bench.HOP, F, n_lead=s.n_lead)
    peaks = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:, :v.n_bins]
    for name, want in (("db", db), ("peaks", peaks), ("peak_count", cnt), ("peak_center", ctr), ("peak_size", sz)):
        assert np.array_equal(got[name], want.astype(np.float32)), name
    assert int(cnt.sum()) > 0
