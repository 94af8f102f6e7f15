"""The panels stage on the GPU (pvq_panels_batch_rows_device, pvq_panels_batch_graph_device) against the host face (pvq_spectrum_mesh,
pvq_calmness_histogram_mesh, pvq_calmness_graph_*), which tests/test_panels.py holds to tests/panels_model.py bit for bit.

The bar is the bits of the host face: the device evaluates only IEEE + - * / and sqrt on the same inputs, with tables from the
host, so there is no tolerance to measure.  Every test prints the number of differing 32-bit words before it asserts zero; a
difference is a finding whose operation is to be named, not a tolerance to be widened."""
import numpy as np
import pytest

import panels_cases as PC
import panels_model as M
import pitchvis_amd as P
from helpers import get_geom

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = 40


def _upload(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _differing(tag, got, want):
    """{name: differing 32-bit words} of device tensors against host arrays, printed"""
    diff = {k: M.same_bits(got[k].cpu().numpy().reshape(want[k].shape), want[k]) for k in want}
    print(f"{tag}: differing 32-bit words, device vs host face: {diff}")
    return diff


@pytest.mark.parametrize("max_peaks", [1, 12, 70])
@pytest.mark.parametrize("min_freq,octaves,bpo", PC.GEOMETRIES)
def test_rows_match_the_host_face_on_oracle_fields(min_freq, octaves, bpo, max_peaks):
    n = octaves * bpo
    case = PC.make(min_freq, octaves, bpo, ROWS, 100 + n, max_peaks)
    count = case["count"]
    assert count.min() == 0 and count.max() == max_peaks and np.isnan(case["center"][count == 0]).all()
    d_x, d_c, d_s, d_n, d_calm = _upload(case["x"], case["center"], case["size"], count, case["calmness"])
    b = P.PanelsBatch(P.VqtRange(min_freq, octaves, bpo), 1)
    out = b.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n, calmness=d_calm)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(P.PanelsBatch.OUTPUTS)
    want = PC.host_rows(P, case)
    diff = _differing(f"{n} bins, max_peaks {max_peaks}, {ROWS} rows", out, want)
    assert not any(diff.values()), diff
    # list entries beyond a row's count are NaN in the inputs: none shows, and the disc slots beyond the count are all zero
    dp, dc = out["disc_pos"].cpu().numpy(), out["disc_rgba"].cpu().numpy()
    for r in range(ROWS):
        assert not dp[r, count[r]:].view(np.uint32).any() and not dc[r, count[r]:].view(np.uint32).any(), r
    finite_rows = [r for r, pk in enumerate(case["peaks"]) if all(c == c for c, _ in pk)]
    assert np.isfinite(dp[finite_rows]).all() and np.isfinite(dc).all()
    # a count above max_peaks is taken as max_peaks
    raised = count.astype(np.int64)
    full = np.nonzero(count == max_peaks)[0]
    raised[full[0]] = max_peaks + 1
    raised[full[-1]] = 0xFFFFFFFF
    d_raised = torch.from_numpy(raised.astype(np.uint32).view(np.int32)).cuda()
    again = b.rows_device(center=d_c, size=d_s, peak_count=d_raised, outputs=["disc_pos", "disc_rgba"])
    # each output requested alone gives the bits it has when requested with the others
    alone = {}
    for name in P.PanelsBatch.OUTPUTS:
        alone.update(b.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n, calmness=d_calm, outputs=[name]))
    torch.cuda.synchronize()
    for name in ("disc_pos", "disc_rgba"):
        assert torch.equal(_bits(again[name]), _bits(out[name])), name
    for name in P.PanelsBatch.OUTPUTS:
        assert torch.equal(_bits(alone[name]), _bits(out[name])), name


@pytest.fixture(scope="module")
def chain():
    """PCM -> preprocess_pcm -> rows_device / graph_device at 252 bins, nothing copied between the stages"""
    pp, _ = get_geom("bench_48k_252")
    v = P.Vqt.new(pp, 0)
    n_streams, nf, hop, max_peaks = 2, 64, 1024, 32
    rng = np.random.default_rng(11)
    t = np.arange(nf * hop) / 48000.0
    pcms = []
    for s in range(n_streams):
        x = 0.01 * rng.standard_normal(t.size)
        for f0 in rng.uniform(80.0, 3000.0, 5):
            x += 0.15 * np.sin(2 * np.pi * f0 * t) * (t > rng.uniform(0, 0.6))
        pcms.append(torch.from_numpy(x.astype(np.float32)).cuda())
    n = v.n_bins
    fields = {"x_vqt_smoothed": torch.zeros((n_streams, nf, n), device="cuda"), "calmness": torch.zeros((n_streams, nf, n), device="cuda"),
              "peak_count": torch.zeros((n_streams, nf), dtype=torch.int32, device="cuda"),
              "center": torch.zeros((n_streams, nf, max_peaks), device="cuda"), "size": torch.zeros((n_streams, nf, max_peaks), device="cuda"),
              "scene_calmness": torch.zeros((n_streams, nf), device="cuda")}
    a = P.AnalysisBatch(pp.range, n_streams)
    b = P.PanelsBatch(pp.range, n_streams)
    a.preprocess_pcm(v, pcms, nf, hop, outputs=fields, max_peaks=max_peaks)
    out = b.rows_device(fields)                 # the dict preprocess_pcm filled, as it stands
    graph = b.graph_device(fields["scene_calmness"])
    torch.cuda.synchronize()
    return dict(pp=pp, fields=fields, out=out, graph=graph, b=b, n_streams=n_streams, nf=nf, max_peaks=max_peaks)


def test_rows_match_the_host_face_on_the_analysis_batch_outputs(chain):
    f, n = chain["fields"], 252
    n_rows = chain["n_streams"] * chain["nf"]
    x = f["x_vqt_smoothed"].cpu().numpy().reshape(n_rows, n)
    calm = f["calmness"].cpu().numpy().reshape(n_rows, n)
    cnt = f["peak_count"].cpu().numpy().reshape(n_rows)
    ctr = f["center"].cpu().numpy().reshape(n_rows, -1)
    sz = f["size"].cpu().numpy().reshape(n_rows, -1)
    rows = list(range(5, n_rows, 3))[:ROWS]     # the first frames of a stream hold little
    assert len(rows) == ROWS and int(cnt[rows].sum()) > ROWS // 2 and all(t.is_cuda for t in chain["out"].values())
    peaks = [list(zip(ctr[i, :cnt[i]].tolist(), sz[i, :cnt[i]].tolist())) for i in rows]
    case = dict(n=n, bpo=chain["pp"].range.buckets_per_octave, x=x[rows], calmness=calm[rows], peaks=peaks, max_peaks=chain["max_peaks"])
    want = PC.host_rows(P, case)
    got = {k: t.reshape((n_rows,) + tuple(t.shape[1:]))[rows] for k, t in chain["out"].items()}
    diff = _differing("analysis batch outputs, 252 bins", got, want)
    assert not any(diff.values()), diff
    # the graph of the newest frame from the batch's own scene calmness, at the viewer's capacity
    sc = f["scene_calmness"].cpu().numpy()
    for s in range(chain["n_streams"]):
        h = P.CalmnessGraph()
        for v in sc[s]:
            h.push(float(v))
        hm = h.mesh()
        g = {"pos": chain["graph"]["graph_pos"][s, 0], "rgba": chain["graph"]["graph_rgba"][s, 0]}
        d = _differing(f"graph of stream {s}", g, {"pos": hm["pos"], "rgba": hm["rgba"]})
        assert not any(d.values()) and M.same_bits(chain["b"].history(s), hm["history"]) == 0


def _host_graph(capacity, vals):
    """per stream and frame: (pos, rgba) of the host handle after each push, and the final histories"""
    n_streams, nf = vals.shape
    pos = np.zeros((n_streams, nf, 4 * (capacity - 1), 3), f32)
    rgba = np.zeros((n_streams, nf, 4 * (capacity - 1), 4), f32)
    hist = np.zeros((n_streams, capacity), f32)
    for s in range(n_streams):
        h = P.CalmnessGraph(capacity)
        for f in range(nf):
            h.push(float(vals[s, f]))
            m = h.mesh()
            pos[s, f], rgba[s, f], hist[s] = m["pos"], m["rgba"], m["history"]
    return pos, rgba, hist


GRAPH_CASES = [(c, k) for c in (2, 64, 65) for k in sorted({1, c - 1, c, c + 1, 2 * c + 3})] + [(300, 5), (129, 1), (129, 131), (1024, 3)]


@pytest.mark.parametrize("capacity,n_frames", GRAPH_CASES)
def test_graph_matches_the_host_handle(capacity, n_frames):
    n_streams = 3
    rng = np.random.default_rng(1000 * capacity + n_frames)
    vals = rng.random((n_streams, n_frames), dtype=f32)
    vals[:, ::4] = np.resize(np.array([0.7, 0.3, 0.71, 0.31, 0.0, 1.5, -0.2], f32), vals[:, ::4].shape)
    want_pos, want_rgba, want_hist = _host_graph(capacity, vals)
    rng_ = P.VqtRange(55.0, 7, 36)

    def run(pieces, first_of_last=0):
        """the frames in `pieces` calls; every call emits all its frames but the last, which starts at first_of_last"""
        b = P.PanelsBatch(rng_, n_streams, graph_capacity=capacity)
        edges = np.linspace(0, n_frames, pieces + 1).astype(int)
        outs = []
        for i in range(pieces):
            lo, hi = int(edges[i]), int(edges[i + 1])
            if hi == lo:
                continue
            first = first_of_last if i == pieces - 1 else 0
            o = b.graph_device(_upload(vals[:, lo:hi])[0], first_emitted=first)
            outs.append((lo + first, o))
        torch.cuda.synchronize()
        return b, outs

    b, outs = run(1)
    got = {"graph_pos": outs[0][1]["graph_pos"], "graph_rgba": outs[0][1]["graph_rgba"]}
    diff = _differing(f"capacity {capacity}, {n_frames} frames, one call", got, {"graph_pos": want_pos, "graph_rgba": want_rgba})
    assert not any(diff.values()), diff
    hist = np.stack([b.history(s) for s in range(n_streams)])
    assert M.same_bits(hist, want_hist) == 0
    for pieces in (2, 3):
        b2, outs2 = run(pieces)
        for first, o in outs2:
            k = o["graph_pos"].shape[1]
            assert torch.equal(_bits(o["graph_pos"]), _bits(got["graph_pos"][:, first:first + k])), (pieces, first)
            assert torch.equal(_bits(o["graph_rgba"]), _bits(got["graph_rgba"][:, first:first + k])), (pieces, first)
        assert M.same_bits(np.stack([b2.history(s) for s in range(n_streams)]), want_hist) == 0, pieces
    # the newest frame alone (the default), and a call that only advances the history
    b3, outs3 = run(1, first_of_last=n_frames - 1)
    assert outs3[0][1]["graph_pos"].shape == (n_streams, 1, 4 * (capacity - 1), 3)
    assert torch.equal(_bits(outs3[0][1]["graph_pos"]), _bits(got["graph_pos"][:, -1:])) and torch.equal(_bits(outs3[0][1]["graph_rgba"]), _bits(got["graph_rgba"][:, -1:]))
    b4 = P.PanelsBatch(rng_, n_streams, graph_capacity=capacity)
    assert b4.graph_device(_upload(vals)[0], outputs=[]) == {}
    assert M.same_bits(np.stack([b4.history(s) for s in range(n_streams)]), want_hist) == 0
    assert M.same_bits(np.stack([b3.history(s) for s in range(n_streams)]), want_hist) == 0


SENTINEL, GUARD = 0xA5, 256


def _carved(shape):
    """a contiguous float32 tensor of `shape`, 16-byte aligned, GUARD bytes into a sentinel-filled byte buffer; (view, buffer, first, last)"""
    nbytes = int(np.prod(shape)) * 4
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8).cuda()
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD:GUARD + nbytes].view(torch.float32).view(shape)
    assert view.data_ptr() == buf.data_ptr() + GUARD and view.is_contiguous()
    return view, buf, GUARD, GUARD + nbytes


def test_outputs_land_where_they_are_told_and_nowhere_else_on_a_second_stream():
    """195 bins (four 64-chunks, the last one nearly empty), 70 peak slots, 7 rows: each output asked for alone, the others NULL, on a
    stream of its own: the bits of the plain call, the guard bands either side untouched"""
    min_freq, octaves, bpo, max_peaks, n_rows = 55.0, 5, 39, 70, 7
    case = PC.make(min_freq, octaves, bpo, n_rows, 77, max_peaks)
    d_x, d_c, d_s, d_n, d_calm = _upload(case["x"], case["center"], case["size"], case["count"], case["calmness"])
    b = P.PanelsBatch(P.VqtRange(min_freq, octaves, bpo), 2, graph_capacity=65)
    ins = dict(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n, calmness=d_calm)
    plain = b.rows_device(**ins)
    vals = _upload(np.random.default_rng(5).random((2, 9), dtype=f32))[0]
    plain_graph = b.graph_device(vals, first_emitted=2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for name in P.PanelsBatch.OUTPUTS:
        view, buf, first, last = _carved(b.output_shape(name, n_rows, max_peaks))
        with torch.cuda.stream(side):
            b.rows_device(**ins, outputs={name: view})
        side.synchronize()
        assert torch.equal(_bits(view), _bits(plain[name])), name
        assert bool((buf[:first] == SENTINEL).all()) and bool((buf[last:] == SENTINEL).all()), name
    for name in P.PanelsBatch.GRAPH_OUTPUTS:
        b2 = P.PanelsBatch(P.VqtRange(min_freq, octaves, bpo), 2, graph_capacity=65)
        view, buf, first, last = _carved(b2.output_shape(name, 7))
        with torch.cuda.stream(side):
            b2.graph_device(vals, outputs={name: view}, first_emitted=2)
        side.synchronize()
        assert torch.equal(_bits(view), _bits(plain_graph[name])), name
        assert bool((buf[:first] == SENTINEL).all()) and bool((buf[last:] == SENTINEL).all()), name


# ---- the edges of arg_max, the disc chunk loop, the graph's largest capacity ------------------------------------------------------
@pytest.mark.parametrize("min_freq,octaves,bpo", PC.EDGE_GEOMETRIES)
def test_arg_max_edges_match_the_host_face(min_freq, octaves, bpo):
    """tests/panels_cases.edge_spectra through panels_rows' per-lane scan and wave reduction: both signs of zero as the first
    maximum (one lane's two chunks, two lanes), NaN at bin 0, in all of a lane's bins and scattered, rows that never exceed f32::MIN
    (all NaN, all -inf, all -FLT_MAX), a +inf maximum, the maximum at bins 63, 64 and n - 1"""
    n = octaves * bpo
    spectra = PC.edge_spectra(n, 700 + n)
    names = list(spectra)
    x = np.stack([spectra[k][0] for k in names])
    out = P.PanelsBatch(P.VqtRange(min_freq, octaves, bpo), 1).rows_device(x_vqt_smoothed=_upload(x)[0])
    torch.cuda.synchronize()
    assert sorted(out) == ["line_pos", "line_rgba"]
    host = [P.spectrum_mesh(n, bpo, row) for row in x]
    want = {k: np.stack([h[k] for h in host]) for k in ("line_pos", "line_rgba")}
    per_row = {name: sum(M.same_bits(out[k][r].cpu().numpy(), want[k][r]) for k in want) for r, name in enumerate(names)}
    print(f"{n} bins, crafted spectra: differing 32-bit words, device vs host face, per row: {per_row}")
    diff = _differing(f"{n} bins, {len(names)} crafted spectra", out, want)
    assert not any(diff.values()) and not any(per_row.values()), (diff, per_row)
    for name in ("zeros_first_and_last", "zeros_one_lane", "zeros_two_lanes"):       # (so one answer cannot fit both rows)
        a, b = names.index(name), names.index(name + "_swapped")
        assert M.same_bits(want["line_rgba"][a], want["line_rgba"][b]) >= 4 * (n - 3), name


@pytest.mark.parametrize("max_peaks", sorted(PC.DISC_COUNTS))
def test_disc_lists_on_both_sides_of_the_chunk(max_peaks):
    """rows of 63, 64 and 65 discs (128 and 129 at 129 slots) among short and empty ones: the chunk loop's `live`, its barriers, the
    zeros beyond the count in the chunk that holds the count and in the chunks after it"""
    counts = PC.DISC_COUNTS[max_peaks]
    case = PC.list_case(55.0, 5, 39, max_peaks, counts, 800 + max_peaks)
    assert list(case["count"]) == counts and np.isnan(case["center"][np.arange(max_peaks)[None, :] >= case["count"][:, None]]).all()
    d_x, d_c, d_s, d_n, d_calm = _upload(case["x"], case["center"], case["size"], case["count"], case["calmness"])
    out = P.PanelsBatch(P.VqtRange(55.0, 5, 39), 1).rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n, calmness=d_calm)
    torch.cuda.synchronize()
    diff = _differing(f"max_peaks {max_peaks}, counts {counts}", out, PC.host_rows(P, case))
    assert not any(diff.values()), diff
    dp, dc = out["disc_pos"].cpu().numpy(), out["disc_rgba"].cpu().numpy()
    for r, c in enumerate(counts):
        assert not dp[r, c:].view(np.uint32).any() and not dc[r, c:].view(np.uint32).any(), r
        assert c == 0 or (dp[r, c - 1].view(np.uint32).any() and dc[r, c - 1].view(np.uint32).any()), r


def test_graph_at_capacity_1024_over_a_call_longer_than_the_ring():
    """1027 frames at the largest capacity in one call that emits the last 3, and as 1024 + 3; the histories after each call"""
    capacity, n_streams, nf, emit = 1024, 2, 1027, 3
    vals = np.random.default_rng(1027).random((n_streams, nf), dtype=f32)
    vals[:, ::5] = np.resize(np.array([0.7, 0.3, 0.71, 0.31, 0.0, 1.5, -0.2], f32), vals[:, ::5].shape)
    want = {"graph_pos": np.zeros((n_streams, emit, 4 * (capacity - 1), 3), f32), "graph_rgba": np.zeros((n_streams, emit, 4 * (capacity - 1), 4), f32)}
    hist = np.zeros((2, n_streams, capacity), f32)                                    # after 1024 frames, after 1027
    for s in range(n_streams):
        h = P.CalmnessGraph(capacity)
        for f in range(nf):
            h.push(float(vals[s, f]))
            if f == nf - emit - 1:
                hist[0, s] = h.mesh()["history"]
            if f >= nf - emit:
                m = h.mesh()
                want["graph_pos"][s, f - (nf - emit)], want["graph_rgba"][s, f - (nf - emit)], hist[1, s] = m["pos"], m["rgba"], m["history"]
    assert np.array_equal(hist[0], vals[:, :capacity]) and np.array_equal(hist[1], vals[:, emit:])
    rng_ = P.VqtRange(55.0, 7, 36)
    one = P.PanelsBatch(rng_, n_streams, graph_capacity=capacity)
    got = one.graph_device(_upload(vals)[0], first_emitted=nf - emit)
    torch.cuda.synchronize()
    diff = _differing(f"capacity {capacity}, {nf} frames in one call, the last {emit} emitted", got, want)
    assert not any(diff.values()), diff
    assert M.same_bits(np.stack([one.history(s) for s in range(n_streams)]), hist[1]) == 0
    two = P.PanelsBatch(rng_, n_streams, graph_capacity=capacity)
    assert two.graph_device(_upload(vals[:, :capacity])[0], outputs=[]) == {}
    assert M.same_bits(np.stack([two.history(s) for s in range(n_streams)]), hist[0]) == 0
    got2 = two.graph_device(_upload(vals[:, capacity:])[0], first_emitted=0)
    torch.cuda.synchronize()
    diff = _differing(f"capacity {capacity}, 1024 + {emit} frames", got2, want)
    assert not any(diff.values()), diff
    assert M.same_bits(np.stack([two.history(s) for s in range(n_streams)]), hist[1]) == 0


# ---- the stride loops: a workgroup's second row ---------------------------------------------------------------------------------
FILL = 0xA5A5A5A5 - (1 << 32)                                                          # the sentinel byte as an int32 word


def _carved_on_device(shape):
    """_carved, filled on the device (the large calls): (view, buffer, first, last)"""
    nbytes = int(np.prod(shape)) * 4
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf[GUARD:GUARD + nbytes].view(torch.float32).view(shape), buf, GUARD, GUARD + nbytes


def _guards_hold(buf, first, last):
    return bool((buf[:first] == SENTINEL).all()) and bool((buf[last:] == SENTINEL).all())


def test_rows_stride_with_a_different_row_each_time():
    """panels_rows<2>: 8192 workgroups over 8192 + 61 rows of 61 distinct ones (tests/panels_cases.stride_case; tests/test_panels.py
    holds the orders: an empty list after a full one, a short one after one that crosses the 64-chunk, a NaN spectrum after an
    ordinary one).  As 8192 = 134 x 61 + 18, the 61 workgroups that take a second row meet a row of another kind with s_cx, s_cy and
    s_at as the first left them.  Every row of the large call is, bit for bit, that row of the 61-row call, which is the host face's."""
    cap, m = 8192, PC.STRIDE_ROWS
    case, kinds = PC.stride_case()
    want = PC.host_rows(P, case)
    differ = lambda i, j: all(M.same_bits(want[k][i], want[k][j]) for k in want) and all(
        not np.array_equal(case[k][i], case[k][j], equal_nan=True) for k in ("x", "calmness", "center", "size"))
    pairs = PC.stride_follows(m, cap, differ)
    orders = {(kinds[i][0], kinds[j][0]) for i, j in pairs} | {(kinds[i][1], kinds[j][1]) for i, j in pairs}
    assert {("full", "empty"), ("crossing", "short"), ("ordinary", "nan")} <= orders, orders
    empty =[r for r in range(m) if not want["disc_pos"][r].view(np.uint32).any()]
    assert 4 * len(empty) <= m and empty == [r for r in range(m) if kinds[r][0] == "empty"]
    total = cap + m
    idx = _upload(np.arange(total, dtype=np.int64) % m)[0]
    ins = dict(zip(("x_vqt_smoothed", "center", "size", "peak_count", "calmness"),
                   _upload(case["x"], case["center"], case["size"], case["count"], case["calmness"])))
    b = P.PanelsBatch(P.VqtRange(55.0, 5, 13), 1)
    small = b.rows_device(**ins)
    torch.cuda.synchronize()
    diff = _differing(f"{m} distinct rows", small, want)
    assert not any(diff.values()), diff
    model = PC.model_rows(M, case)
    assert not any(M.same_bits(want[k], model[k]) for k in want)
    carved = {name: _carved_on_device(b.output_shape(name, total, case["max_peaks"])) for name in P.PanelsBatch.OUTPUTS}
    b.rows_device(**{k: t[idx].contiguous() for k, t in ins.items()}, outputs={k: v[0] for k, v in carved.items()})
    torch.cuda.synchronize()
    differing, unwritten = {}, {}
    for name, (view, buf, first, last) in carved.items():
        differing[name] = int((_bits(view) != _bits(small[name])[idx]).sum())
        assert not bool((_bits(small[name]) == FILL).any()), name                   # no row's answer is the fill value,
        unwritten[name] = int((_bits(view)[cap:] == FILL).sum())                    # so none of rows cap .. total may hold it
        assert _guards_hold(buf, first, last), name
    print(f"{total} rows over {cap} workgroups: differing 32-bit words against the {m}-row call: {differing}; "
          f"words of rows {cap} .. still the fill value: {unwritten}")
    assert not any(differing.values()) and not any(unwritten.values()), (differing, unwritten)


def test_graph_stride_over_130_streams():
    """panels_graph: capacity 3, 130 streams x 64 frames, all emitted: 8320 rows over 8192 workgroups; stream s is pattern s % 61,
    so row r + 8192 (stream s + 128, the same frame) is pattern + 6's"""
    cap, m, capacity, n_streams, nf = 8192, 61, 3, 130, 64
    vals = np.random.default_rng(3130).random((m, nf), dtype=f32)
    vals[::7, 5::9] = np.nan
    want_pos, want_rgba, want_hist = _host_graph(capacity, vals)
    step = cap // nf
    assert cap % nf == 0 and n_streams * nf > cap and step % m != 0
    for p in range(m):                                                              # a workgroup's second row is another pattern's
        q = (p + step) % m
        assert all(M.same_bits(want_pos[p, f], want_pos[q, f]) for f in range(nf)) and M.same_bits(vals[p], vals[q]) == nf, (p, q)
    idx = np.arange(n_streams) % m
    rng_ = P.VqtRange(55.0, 7, 36)
    d_vals = _upload(vals)[0]
    small = P.PanelsBatch(rng_, m, graph_capacity=capacity).graph_device(d_vals, first_emitted=0)
    torch.cuda.synchronize()
    diff = _differing(f"capacity {capacity}, {m} distinct streams", small, {"graph_pos": want_pos, "graph_rgba": want_rgba})
    assert not any(diff.values()), diff
    b = P.PanelsBatch(rng_, n_streams, graph_capacity=capacity)
    carved = {name: _carved_on_device(b.output_shape(name, nf)) for name in P.PanelsBatch.GRAPH_OUTPUTS}
    d_idx = _upload(idx.astype(np.int64))[0]
    b.graph_device(d_vals[d_idx].contiguous(), outputs={k: v[0] for k, v in carved.items()}, first_emitted=0)
    torch.cuda.synchronize()
    differing, unwritten = {}, {}
    for name, (view, buf, first, last) in carved.items():
        differing[name] = int((_bits(view) != _bits(small[name])[d_idx]).sum())
        unwritten[name] = int((_bits(view).reshape(n_streams * nf, -1)[cap:] == FILL).sum())
        assert _guards_hold(buf, first, last) and not bool((_bits(small[name]) == FILL).any()), name
    print(f"{n_streams * nf} graph rows over {cap} workgroups: differing 32-bit words against the {m}-stream call: {differing}; "
          f"words of rows {cap} .. still the fill value: {unwritten}")
    assert not any(differing.values()) and not any(unwritten.values()), (differing, unwritten)
    for s in (0, 1, n_streams - 2, n_streams - 1):
        assert M.same_bits(b.history(s), want_hist[idx[s]]) == 0, s


def test_history_stride_over_520_streams():
    """panels_history: 520 streams x capacity 1024 = 532 480 entries over 2048 x 256 = 524 288 lanes, in two calls that emit nothing;
    stream s is pattern s % 61, so entry t + 524 288 (stream s + 512) is pattern + 24's.  The history is the last 1024 entries of
    [zeros | values]; streams 512 .. 519 are the second trip's."""
    lanes, m, capacity, n_streams, calls = 2048 * 256, 61, 1024, 520, (700, 500)
    vals = np.random.default_rng(520).random((m, sum(calls)), dtype=f32)
    vals[:, ::11] = np.resize(np.array([0.0, -0.0, np.nan, 1.5], f32), vals[:, ::11].shape)
    step = lanes // capacity
    assert lanes % capacity == 0 and n_streams * capacity > lanes and step % m != 0
    for p in range(m):
        assert M.same_bits(vals[p], vals[(p + step) % m]) > vals.shape[1] // 2, p
    idx = np.arange(n_streams) % m
    d_vals, d_idx = _upload(vals)[0], _upload(idx.astype(np.int64))[0]
    b = P.PanelsBatch(P.VqtRange(55.0, 7, 36), n_streams, graph_capacity=capacity)
    padded = np.concatenate([np.zeros((m, capacity), f32), vals], axis=1)
    f0, differing = 0, {}
    for k in calls:
        assert b.graph_device(d_vals[d_idx][:, f0:f0 + k].contiguous(), outputs=[]) == {}
        f0 += k
        want = padded[:, f0:f0 + capacity]                                            # the last `capacity` of [zeros | the values so far]
        got = np.stack([b.history(s) for s in range(n_streams)])
        differing[f0] = M.same_bits(got, want[idx])
        assert M.same_bits(got[step:], np.zeros_like(got[step:])) > 0
    print(f"{n_streams * capacity} history entries over {lanes} lanes: differing 32-bit words after {list(differing)} frames: {list(differing.values())}")
    assert not any(differing.values()), differing
    h = P.CalmnessGraph(capacity)                                                     # and the host handle agrees about what a history is
    for v in vals[idx[-1]]:
        h.push(float(v))
    assert M.same_bits(h.mesh()["history"], got[-1]) == 0
