"""The kernel product's stage-stream loop (blockdft_banddots4c_db: one operand ring per wave over all its blocks) against the block
loop it replaced (blockdft_banddots4c_blocks_db, developer library, knob PVQ_DOTS_BLOCKS=1): the same MFMAs in the same order, so
every bit of the dB rows and of the complex output must be equal.  One geometry per LDS stride class of the kernel (260, 308, 372,
596, 852, 1028) and the smallest bin count; 150 frames behind a lead of 777 samples (two full X tiles and a partial one of 22 live
frames); a many-streams call (the X-tile map); a NaN sample (status flag, untouched frames).
Child processes: the knob is read once per process."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = textwrap.dedent("""
    import sys, os
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import numpy as np, torch
    import pitchvis_amd as P
    from helpers import geom_pair, get_geom, white_noise
    from test_bin_classes_gpu import VQT_ROWS
    out = {}
    NF, LEAD = 150, 777

    def run(tag, pp, hop):
        v = P.Vqt.new(pp, 0)
        v.set_algo(P.ALGO_BLOCKDFT)
        v.set_gemm_precision(P.GEMM_F32)
        pcm = torch.from_numpy(white_noise(LEAD + hop * NF, 11)).cuda()
        cx = torch.zeros((NF, v.n_bins, 2), device="cuda")
        db = torch.full((NF, v.n_bins), -1.0, device="cuda")
        v.calculate_batch_db_device(pcm, hop, NF, db, n_lead=LEAD, d_out_cplx=cx)
        torch.cuda.synchronize()
        v.input_status()
        assert v.last_algo() == P.ALGO_BLOCKDFT
        out[tag + "_db"] = db.cpu().numpy()
        out[tag + "_cx"] = cx.cpu().numpy()
        return v

    # one geometry per stride class: 260, 308, 372 (32-frame tiles), 596, 852
    for name, hop in (("bench_48k_252", 256), ("bench_48k_288", 256), ("hires_96k_360", 128), ("default_22k_588", 256), ("hires_96k_840", 128)):
        v = run(name, get_geom(name)[0], hop)
        if name == "bench_48k_252":
            # many streams in one call: rows through the X-tile map
            nfs = [100, 64, 37]
            pcms = [torch.from_numpy(white_noise(LEAD + hop * n, 21 + i)).cuda() for i, n in enumerate(nfs)]
            db = torch.full((3, 100, v.n_bins), -1.0, device="cuda")
            v.batch_streams_device(pcms, hop, nfs, db, 100, n_leads=[LEAD] * 3)
            torch.cuda.synchronize()
            v.input_status()
            out["streams_db"] = db.cpu().numpy()
            # a NaN sample: its frames are flagged, every other frame is what it was
            host = white_noise(LEAD + hop * NF, 11)
            at = LEAD + hop * 75
            host[at] = np.nan
            pcm = torch.from_numpy(host).cuda()
            cx = torch.zeros((NF, v.n_bins, 2), device="cuda")
            db = torch.full((NF, v.n_bins), -1.0, device="cuda")
            v.calculate_batch_db_device(pcm, hop, NF, db, n_lead=LEAD, d_out_cplx=cx)
            torch.cuda.synchronize()
            flagged = 0
            try:
                v.input_status()
            except P.PvqError as e:
                flagged = int(e.status)
            out["nan_flag"] = np.array([flagged])
            out["nan_db"] = db.cpu().numpy()
            out["nan_cx"] = cx.cpu().numpy()
    # the 1028 class at both ends and the smallest bin count, by the rows of the bin-class table
    for bins in (3, 849, 1020):
        row = next(r for r in VQT_ROWS if r[4] == bins)
        run("row%d" % bins, geom_pair(*row[:4])[0], row[5])
    np.savez(sys.argv[1], **out)
    print("STREAM_OK")
""")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_stage_stream_equals_block_loop_bit_for_bit(tmp_path):
    res = {}
    for tag, env in (("stream", {}), ("blocks", {"PVQ_DEV_LIB": "1", "PVQ_DOTS_BLOCKS": "1"})):
        f = str(tmp_path / f"dots_stream_{tag}.npz")
        r = subprocess.run([sys.executable, "-c", CODE, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0 and "STREAM_OK" in r.stdout, (tag, r.stdout[-2000:] + r.stderr[-2000:])
        with np.load(f) as z:
            res[tag] = {k: z[k] for k in z.files}
    a, b = res["stream"], res["blocks"]
    assert set(a) == set(b) and len(a) == 2 * 8 + 4
    from pitchvis_amd import _lib
    assert int(a["nan_flag"][0]) == int(b["nan_flag"][0]) == _lib.PVQ_ERR_NONFINITE_INPUT
    for k in sorted(a):
        if k == "nan_flag":
            continue
        assert a[k].shape == b[k].shape, k
        if k.startswith("nan_"):   # the frames the NaN reaches hold it in their complex rows on both sides; every other frame bit for bit
            hit_a, hit_b = (~np.isfinite(x["nan_cx"]).all(axis=(1, 2)) for x in (a, b))
            assert np.array_equal(hit_a, hit_b)
            assert 1 <= hit_a.sum() <= 65, int(hit_a.sum())   # (the longest window of the geometry, 16 384 samples, spans 64 hops)
            assert np.array_equal(_bits(a[k][~hit_a]), _bits(b[k][~hit_a])), k
            continue
        assert np.isfinite(a[k]).all(), k
        if k.endswith("_db"):
            assert (a[k] >= 0.0).all(), k   # no row keeps the fill value
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, int((_bits(a[k]) != _bits(b[k])).sum()))
    s = a["streams_db"]
    assert (s >= 0).all() and (s[1, 64:] == 0.0).all() and (s[2, 37:] == 0.0).all()   # rows a stream does not fill are zero frames
