"""Mixed column tiles of the fused GEMM (blockdft_plan.hpp: MixedPair): the partial last column tiles of two window groups share one
32-column tile — one K loop, one epilogue — and each part is stored to the X columns it always had.  An MFMA output does not depend
on its column's position in the tile and the tree is the same tree_cmadd calls per column, so every bit of X and of the dB frames
must stay what it was.

Checked here, in child processes (the developer knobs are read once per process): the developer library with 256-row tiles forced
(PVQ_FUSED_BM=256: the mixed entries' kernel; launches this small take 128-row tiles otherwise) with the mixed list and with the
former list (PVQ_MIXED_TILES=0), and the product library, give equal complex output and dB, bit for bit, on every case.
bench_48k_252 pairs its (32, 16)- and (8, 4)-block groups (one and no tail level in the store; 3 and 2 register levels),
bench_48k_288 its (32, 16) and (4, 2), default_22k_588 its 2- and 11-column tiles in a half tile, all at hop 256; hires_96k_360 at
hop 128 has groups that leave Y partial sums, with which no pair forms.  The frame counts sit at the 64-frame X tiles, at the row
strides 225 / 241 / 249 / 253 of the groups of 32 / 16 / 8 / 4 blocks and 8 frames either side of 225 (the 32- and 16-block groups'
windows begin 8 hops apart); n_lead 777 reaches the stream-edge K loop, next to which the second group's frames come from cover
entries."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM_HOPS = (("bench_48k_252", 256), ("bench_48k_288", 256), ("default_22k_588", 256), ("hires_96k_360", 128))
FRAMES = (1, 7, 8, 9, 63, 64, 65, 217, 224, 225, 226, 233, 241, 242, 249, 250, 253, 254, 450, 451, 1500)
LEADS = (0, 777)
STREAM_FRAMES = (65, 193, 450)

CHILD = textwrap.dedent("""
    import sys, os
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import numpy as np, torch
    import pitchvis_amd as P
    from helpers import get_geom, white_noise
    geom_hops, frames, leads, stream_frames = eval(sys.argv[2])
    out = {}
    for name, hop in geom_hops:
        pp, op = get_geom(name)
        v = P.Vqt.new(pp, 0)
        v.set_algo(P.ALGO_BLOCKDFT)
        for nf in frames:
            for n_lead in leads:
                pcm = torch.from_numpy(white_noise(n_lead + hop * nf, 100 + nf)).cuda()
                cx = torch.zeros((nf, v.n_bins, 2), device="cuda")
                db = torch.empty((nf, v.n_bins), device="cuda")
                v.calculate_batch_db_device(pcm, hop, nf, db, n_lead=n_lead, d_out_cplx=cx)
                torch.cuda.synchronize()
                assert v.last_algo() == P.ALGO_BLOCKDFT
                key = "%s/%d/%d" % (name, nf, n_lead)
                out[key + "/cx"], out[key + "/db"] = cx.cpu().numpy(), db.cpu().numpy()
        # many streams in one call against the single-stream calls (dB: the streams entry point has no complex output)
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
    print("MIXED_OK")
""")

RUNS = {   # the product library; the developer library on 256-row tiles: the mixed list / the former list
    "product": {},
    "dev": {"PVQ_DEV_LIB": "1", "PVQ_FUSED_BM": "256"},
    "dev_off": {"PVQ_DEV_LIB": "1", "PVQ_FUSED_BM": "256", "PVQ_MIXED_TILES": "0"},
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every form once, each in its own child process; the arrays are shared by the tests below and not modified"""
    d = tmp_path_factory.mktemp("mixed_tiles")
    res = {}
    for tag, env in RUNS.items():
        f = str(d / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD, f, repr((GEOM_HOPS, FRAMES, LEADS, STREAM_FRAMES))],
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0 and "MIXED_OK" in r.stdout, tag + r.stdout[-2000:] + r.stderr[-2000:]
        with np.load(f) as z:
            res[tag] = {k: z[k] for k in z.files}
    return res


def _cases():
    return ["%s/%d/%d" % (name, nf, n_lead) for name, _ in GEOM_HOPS for nf in FRAMES for n_lead in LEADS]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("other", ["dev_off", "product"])
def test_mixed_list_bit_identical(runs, other):
    a, b = runs["dev"], runs[other]
    keys = sorted(a)
    assert len(keys) == 2 * len(_cases()) + len(GEOM_HOPS) * (1 + len(STREAM_FRAMES)) and keys == sorted(b)
    for k in keys:
        assert _same_bits(a[k], b[k]), (other, k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()))


@pytest.mark.parametrize("tag", list(RUNS))
def test_many_streams_equal_single_stream_calls(runs, tag):
    r = runs[tag]
    for name, _ in GEOM_HOPS:
        multi = r[name + "/multi"]
        for s, nf in enumerate(STREAM_FRAMES):
            assert _same_bits(multi[s, :nf], r["%s/single%d" % (name, s)]), (name, s)
            assert not np.any(multi[s, nf:]), (name, s)   # rows a stream does not fill: zero frames
