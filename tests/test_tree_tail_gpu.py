"""The fused GEMM's epilogue evaluates a tile's last one or two tree levels (strides 16 and 32: window groups of 32 and 64 hop blocks)
on the way from LDS to memory, in the store's thread mapping, instead of as an LDS pass of their own before the store.  The calls and
their order are those of the level pass, so every bit of X and Y must stay what it was.

Checked here, in child processes (the developer knobs are read once per process): the former epilogue (developer library,
PVQ_TREE_TAIL=0) and the new one give equal complex output and dB on every case, with the launch's own tile shape and with 256-row
tiles forced (PVQ_FUSED_BM=256: S = 193 complete frames per tile of the 64-block group, 225 of the 32-block group — the frame counts
below sit around those and around the 64-frame X tiles); the product library equals the developer one; and the block path stays
within 1e-5 of the frame peak of the FFT path.  bench_48k_252 at hop 256 has 32- and 64-block groups (the single and the double fused
pass; its shallower groups take the plain store); hires_96k_360 at hop 128 has 256 blocks: 64-block sums go to Y and on to
blockdft_tree_finish.  n_lead 777 reaches the stream-edge K loop and tiles whose last frames do not exist."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM_HOPS = (("bench_48k_252", 256), ("hires_96k_360", 128))
FRAMES = (1, 63, 64, 65, 192, 193, 194, 225, 226, 449, 451, 1500)   # 1 500: past the 128-row kernel's switch (hires_96k_360)
LEADS = (0, 777)
STREAM_FRAMES = (65, 193, 450)
FFT_BAR = 1e-5   # the project's bar for block-DFT path against FFT path, relative to the frame's peak magnitude

CHILD = textwrap.dedent("""
    import sys, os
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import numpy as np, torch
    import pitchvis_amd as P
    from helpers import get_geom, white_noise
    geom_hops, frames, leads, stream_frames = eval(sys.argv[2])
    with_fft = sys.argv[3] == "1"
    out = {}
    for name, hop in geom_hops:
        pp, op = get_geom(name)
        v = P.Vqt.new(pp, 0)
        for nf in frames:
            for n_lead in leads:
                pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 100 + nf)).cuda()
                res = {}
                for algo in (P.ALGO_BLOCKDFT, P.ALGO_FFT) if with_fft else (P.ALGO_BLOCKDFT,):
                    v.set_algo(algo)
                    cx = torch.zeros((nf, v.n_bins, 2), device="cuda")
                    db = torch.empty((nf, v.n_bins), device="cuda")
                    v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead, d_out_cplx=cx)
                    torch.cuda.synchronize()
                    assert v.last_algo() == algo
                    res[algo] = (cx.cpu().numpy(), db.cpu().numpy())
                key = "%s/%d/%d" % (name, nf, n_lead)
                out[key + "/cx"], out[key + "/db"] = res[P.ALGO_BLOCKDFT]
                if with_fft:
                    a, b = (res[k][0].view(np.complex64)[..., 0] for k in (P.ALGO_BLOCKDFT, P.ALGO_FFT))
                    fmax = np.abs(b).max(axis=1)
                    # the project's bar (tests/test_parity_gpu.py: assert_parity, test_blockdft_tile_boundaries): a frame that sees little of
                    # the signal (a stream's first frames: the samples sit in the window's tails, the coefficients are the residue of
                    # cancelling terms) is measured against 1 % of the response a sine of its input's peak amplitude would give
                    x = np.abs(pcm.cpu().numpy())
                    ends = n_lead + hop * (1 + np.arange(nf))
                    xpeak = np.array([x[max(e - v.window_union, 0):e].max() for e in ends])
                    d = np.abs(a - b).max(axis=1)
                    out[key + "/err"] = np.float64((d / np.maximum(fmax, 0.01 * np.sqrt(op.sr) * xpeak)).max())
                    out[key + "/err_unfloored"] = np.float64((d / fmax).max())
        # many streams in one call against the single-stream calls (dB: the streams entry point has no complex output)
        v.set_algo(P.ALGO_BLOCKDFT)
        pcms = [torch.from_numpy(white_noise(777 + hop * nf, 200 + nf)).cuda() for nf in stream_frames]
        stride = max(stream_frames)
        multi = torch.full((len(pcms), stride, v.n_bins), -1.0, device="cuda")
        v.batch_streams_device(pcms, hop, stream_frames, multi, stride, n_leads=[777] * len(pcms))
        torch.cuda.synchronize()
        assert v.last_algo() == P.ALGO_BLOCKDFT
        out[name + "/multi"] = multi.cpu().numpy()
        for s, nf in enumerate(stream_frames):
            db = torch.empty((nf, v.n_bins), device="cuda")
            v.calculate_batch_db_device(pcms[s], hop, nf, db, n_lead=777)
            torch.cuda.synchronize()
            out["%s/single%d" % (name, s)] = db.cpu().numpy()
    np.savez(sys.argv[1], **out)
    print("TAIL_OK")
""")

RUNS = {   # the product library; the developer library: new / former epilogue, with the launch's own tile shape and with 256-row tiles
    "product": {},
    "dev": {"PVQ_DEV_LIB": "1"},
    "dev_old": {"PVQ_DEV_LIB": "1", "PVQ_TREE_TAIL": "0"},
    "dev256": {"PVQ_DEV_LIB": "1", "PVQ_FUSED_BM": "256"},
    "dev256_old": {"PVQ_DEV_LIB": "1", "PVQ_FUSED_BM": "256", "PVQ_TREE_TAIL": "0"},
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every form once, each in its own child process; the arrays are shared by the tests below and not modified"""
    d = tmp_path_factory.mktemp("tree_tail")
    res = {}
    for tag, env in RUNS.items():
        f = str(d / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD, f, repr((GEOM_HOPS, FRAMES, LEADS, STREAM_FRAMES)), "1" if tag == "product" else "0"],
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0 and "TAIL_OK" in r.stdout, tag + r.stdout[-2000:] + r.stderr[-2000:]
        with np.load(f) as z:
            res[tag] = {k: z[k] for k in z.files}
    return res


def _cases():
    return ["%s/%d/%d" % (name, nf, n_lead) for name, _ in GEOM_HOPS for nf in FRAMES for n_lead in LEADS]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_block_path_within_the_bar_of_the_fft_path(runs):
    """Block-DFT path against FFT path, every frame of every case, in units of the frame's peak magnitude with the floor the parity
    tests give frames that see little of their input (CHILD).  Without that floor the first frames of a stream (lead 0 and 777: at
    most the first 27 frames, windows mostly empty) reach 3.7e-4 at bench_48k_252 / 1 500 frames / lead 0 and 2.6e-4 at hires_96k_360
    / 1 frame — the same figures, to every digit, before and after the epilogue change, and 7e-7 once the windows are full; the
    unfloored figure is printed."""
    errs = {k: float(runs["product"][k + "/err"]) for k in _cases()}
    raw = {k: float(runs["product"][k + "/err_unfloored"]) for k in _cases()}
    worst, worst_raw = max(errs, key=errs.get), max(raw, key=raw.get)
    print("worst block-DFT / FFT difference: %.3e of the floored frame peak (%s); %.3e of the bare frame peak (%s)"
          % (errs[worst], worst, raw[worst_raw], worst_raw))
    assert errs[worst] <= FFT_BAR, (worst, errs[worst])


@pytest.mark.parametrize("new,old", [("dev", "dev_old"), ("dev256", "dev256_old")])
def test_former_and_fused_epilogue_bit_identical(runs, new, old):
    a, b = runs[new], runs[old]
    for k in _cases():
        for part in ("/cx", "/db"):
            assert _same_bits(a[k + part], b[k + part]), (k + part, int((a[k + part].view(np.uint32) != b[k + part].view(np.uint32)).sum()))
    for name, _ in GEOM_HOPS:
        assert _same_bits(a[name + "/multi"], b[name + "/multi"]), name


def test_product_library_equals_the_developer_one_and_every_tile_shape(runs):
    keys = sorted(runs["dev"])
    assert len(keys) == 2 * len(_cases()) + len(GEOM_HOPS) * (1 + len(STREAM_FRAMES))
    for tag in ("dev", "dev256"):
        for k in keys:
            assert _same_bits(runs["product"][k], runs[tag][k]), (tag, k)


@pytest.mark.parametrize("tag", list(RUNS))
def test_many_streams_equal_single_stream_calls(runs, tag):
    r = runs[tag]
    for name, _ in GEOM_HOPS:
        multi = r[name + "/multi"]
        for s, nf in enumerate(STREAM_FRAMES):
            assert _same_bits(multi[s, :nf], r["%s/single%d" % (name, s)]), (name, s)
            assert not np.any(multi[s, nf:]), (name, s)   # rows a stream does not fill: zero frames
