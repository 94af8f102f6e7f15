"""The render stage on the GPU (pvq_render_batch_rows_device): spectrogram rows in both modes, chroma and LED frames for many rows,
against tests/render_model.py (pitchvis_viewer/src/display_system/update.rs:961-1065, :1102-1131) and oracle/consumers.py's
led_frame (pitchvis_serial/src/main.rs:122-175).

The device gets inputs identical to the model's: (a) oracle-made AnalysisState fields are uploaded, (b) the GPU AnalysisBatch's own
outputs are downloaded and fed to the model.  No analysis tolerance enters either way; what differs is the device's libm.  The bars
are those of tests/test_render.py (one level, 1 % of the bytes, 1e-5 relative for chroma), plus >= 97 % of the LED rows
byte-identical, the figure tests/test_consumers_gpu.py holds."""
import itertools

import numpy as np
import pytest

import pitchvis_amd as P
import render_cases as RC
import render_model as M
from helpers import get_geom
from pitchvis_amd import consumers as PC
from test_render import CHROMA_REL, U8_LEVELS, U8_SHARE, check_edge_rows, hold_to_the_bars

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LED_ROWS_IDENTICAL = 0.97
# 180 / 252 / 588 / 840 bins, and 192 | 195: either side of a 64-chunk edge (3 and 4 chunks)
GEOMETRIES = [(55.0, 5, 36), (55.0, 7, 36), (55.0, 7, 84), (27.5, 10, 84), (55.0, 8, 24), (55.0, 5, 39)]


def _edge_row(n, max_peaks, rng):
    """max_peaks peaks in ascending centre: within 2 of either edge, two bins apart, 2.5 apart, in the last bucket"""
    centers = [0.3, 2.3, 4.3, 6.8, float(n - 6), n - 3.5, n - 0.4]
    k = 0
    while len(centers) < max_peaks:
        centers.append(20.0 + 3.25 * k)
        k += 1
    centers = sorted(centers[:max_peaks])
    return [(float(np.float32(c)), float(np.float32(rng.uniform(1.0, 40.0)))) for c in centers]


def _fields(min_freq, octaves, bpo, n_rows, seed):
    """(a): rows of an oracle AnalysisState, plus a row without peaks, rows with max_peaks peaks, a last-bucket peak"""
    n = octaves * bpo
    smoothed, peaks = M.oracle_rows(min_freq, octaves, bpo, n_rows - 4, seed)
    rng = np.random.default_rng(seed)
    max_peaks = max(12, max(len(p) for p in peaks))
    extra_x = (rng.random((4, n), dtype=np.float32) * 30.0).astype(np.float32)
    extra_x[0] = 0.0
    extra = [[], _edge_row(n, max_peaks, rng), [(float(n - 1), 3.0)], _edge_row(n, max_peaks, rng)[::2]]
    smoothed = np.concatenate([smoothed, extra_x])
    peaks = peaks + extra
    center = np.full((n_rows, max_peaks), np.nan, np.float32)     # entries beyond a row's count are never read
    size = np.full((n_rows, max_peaks), np.nan, np.float32)
    count = np.zeros(n_rows, np.int32)
    for r, pk in enumerate(peaks):
        count[r] = len(pk)
        center[r, :len(pk)] = [p[0] for p in pk]
        size[r, :len(pk)] = [p[1] for p in pk]
    assert count.min() == 0 and count.max() == max_peaks
    return smoothed, peaks, center, size, count


def _model(min_freq, n, bpo, smoothed, peaks, colors=M.COLORS, gray=M.GRAY_LEVEL, easing=M.EASING_POW):
    want = {"spectrogram_vqt": [], "spectrogram_peaks": [], "chroma": [], "led": []}
    for x, pk in zip(smoothed, peaks):
        want["spectrogram_vqt"].append(M.spectrogram_row(M.VQT, n, bpo, x, colors=colors, gray_level=gray, easing_pow=easing))
        want["spectrogram_peaks"].append(M.spectrogram_row(M.PEAKS, n, bpo, None, pk, colors=colors, gray_level=gray, easing_pow=easing))
        want["chroma"].append(M.chroma_row(min_freq, n, bpo, x))
        want["led"].append(np.frombuffer(M.led_frame(n, bpo, pk, colors, gray, easing), np.uint8))
    return {k: np.asarray(v) for k, v in want.items()}


def _hold_to_the_bars(tag, got, want):
    for k in ("spectrogram_vqt", "spectrogram_peaks", "led"):
        levels, share = M.compare_u8(got[k], want[k])
        print(f"{tag} {k}: device vs model: max {levels} level(s), {share:.2e} of the bytes differ")
        assert got[k].shape == want[k].shape
        assert levels <= U8_LEVELS and share <= U8_SHARE, (tag, k, levels, share)
    assert want["spectrogram_peaks"].any() and want["led"][:, 3:].any()
    same = int(sum(np.array_equal(g, w) for g, w in zip(got["led"], want["led"])))
    print(f"{tag} led: {same}/{len(want['led'])} rows byte-identical")
    assert same >= int(LED_ROWS_IDENTICAL * len(want["led"])), (tag, same)
    assert np.all(got["led"][:, 0] == 0xFF) and got["led"][:, 3:].max() <= 0xFE
    g, w = got["chroma"].astype(np.float64), want["chroma"].astype(np.float64)
    rel = float(np.max(np.abs(g - w) / w))
    print(f"{tag} chroma: device vs model: max relative difference {rel:.2e}")
    assert rel <= CHROMA_REL, (tag, rel)


def _upload(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("min_freq,octaves,bpo", GEOMETRIES)
def test_rows_match_the_model_on_oracle_fields(min_freq, octaves, bpo):
    n, n_rows = octaves * bpo, 40
    smoothed, peaks, center, size, count = _fields(min_freq, octaves, bpo, n_rows, 100 + n)
    d_x, d_c, d_s, d_n = _upload(smoothed, center, size, count)
    r = P.RenderBatch(P.VqtRange(min_freq, octaves, bpo))
    out = r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(P.RenderBatch.OUTPUTS)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    _hold_to_the_bars(f"{n} bins", got, _model(min_freq, n, bpo, smoothed, peaks))
    # the rows without peaks: an all-zero peaks row, an all-zero LED payload (0 / 0 -> NaN -> 0, main.rs:162)
    for row in np.nonzero(count == 0)[0]:
        assert not got["spectrogram_peaks"][row].any() and not got["led"][row, 3:].any()


def test_led_strip_palette_on_the_serial_geometry():
    """the serial consumer's own palette (main.rs:44-59) on a handle of its own"""
    pp, op = get_geom("serial_22k_180")
    n, bpo = 180, 36
    smoothed, peaks, center, size, count = _fields(op.min_freq, op.octaves, bpo, 40, 7)
    d_c, d_s, d_n = _upload(center, size, count)
    r = P.RenderBatch(pp.range, PC.SERIAL_COLORS, PC.SERIAL_GRAY_LEVEL, PC.SERIAL_EASING_POW)
    got = r.rows_device(center=d_c, size=d_s, peak_count=d_n, outputs=["led"])["led"].cpu().numpy()
    want = np.asarray([np.frombuffer(M.led_frame(n, bpo, pk, PC.SERIAL_COLORS, PC.SERIAL_GRAY_LEVEL, PC.SERIAL_EASING_POW), np.uint8) for pk in peaks])
    host = np.asarray([np.frombuffer(P.led_frame(n, bpo, pk), np.uint8) for pk in peaks])
    for tag, ref in (("model", want), ("host", host)):
        levels, share = M.compare_u8(got, ref)
        same = int(sum(np.array_equal(g, w) for g, w in zip(got, ref)))
        print(f"serial led: device vs {tag}: max {levels} level(s), {share:.2e} of the bytes differ, {same}/{len(ref)} rows identical")
        assert levels <= U8_LEVELS and share <= U8_SHARE and same >= int(LED_ROWS_IDENTICAL * len(ref))


class _Spy:
    """the library with one entry point's arguments recorded"""

    def __init__(self, L, name):
        self._L, self._name, self.calls = L, name, []

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if name != self._name:
            return f

        def call(*a):
            self.calls.append(a)
            return f(*a)
        return call


@pytest.fixture(scope="module")
def chain():
    """(b): PCM -> preprocess_pcm -> rows_device at 252 bins, nothing copied between the stages; everything downloaded afterwards"""
    pp, _ = get_geom("bench_48k_252")
    v = P.Vqt.new(pp, 0)
    n_streams, nf, hop, max_peaks = 4, 64, 1024, 32
    rng = np.random.default_rng(11)
    t = np.arange(nf * hop) / 48000.0
    pcms = []
    for s in range(n_streams):
        x = 0.01 * rng.standard_normal(t.size)
        for f0 in rng.uniform(80.0, 3000.0, 5):
            x += 0.15 * np.sin(2 * np.pi * f0 * t) * (t > rng.uniform(0, 0.6))
        pcms.append(torch.from_numpy(x.astype(np.float32)).cuda())
    n = v.n_bins
    fields = {"x_vqt_smoothed": torch.zeros((n_streams, nf, n), device="cuda"), "peak_count": torch.zeros((n_streams, nf), dtype=torch.int32, device="cuda"),
              "center": torch.zeros((n_streams, nf, max_peaks), device="cuda"), "size": torch.zeros((n_streams, nf, max_peaks), device="cuda"),
              "scene_calmness": torch.zeros((n_streams, nf), device="cuda")}
    b = P.AnalysisBatch(pp.range, n_streams)
    r = P.RenderBatch(pp.range)
    spy_a, spy_r = _Spy(b._L, "pvq_analysis_batch_preprocess_pcm"), _Spy(r._L, "pvq_render_batch_rows_device")
    b._L, r._L = spy_a, spy_r
    b.preprocess_pcm(v, pcms, nf, hop, outputs=fields, max_peaks=max_peaks)
    out = r.rows_device(fields)                 # the dict preprocess_pcm filled, as it stands
    b._L, r._L = spy_a._L, spy_r._L
    torch.cuda.synchronize()
    return dict(pp=pp, fields=fields, out=out, r=r, spy_a=spy_a, spy_r=spy_r, n_rows=n_streams * nf, max_peaks=max_peaks)


def test_chain_stays_on_the_device(chain):
    """what rows_device read is, pointer for pointer, what preprocess_pcm wrote"""
    (ca,), (cr,) = chain["spy_a"].calls, chain["spy_r"].calls
    o = ca[8]._obj                              # the pvq_analysis_batch_outputs behind byref()
    f = chain["fields"]
    assert (cr[1], cr[6]) == (chain["n_rows"], chain["max_peaks"])
    assert cr[2] == o.x_vqt_smoothed == f["x_vqt_smoothed"].data_ptr()
    assert cr[3] == o.center == f["center"].data_ptr() and cr[4] == o.size == f["size"].data_ptr()
    assert cr[5] == o.peak_count == f["peak_count"].data_ptr()
    assert all(t.is_cuda for t in chain["out"].values()) and int(f["peak_count"].sum()) > chain["n_rows"] // 2


def test_rows_match_the_model_on_the_analysis_batch_outputs(chain):
    f, n_rows, n = chain["fields"], chain["n_rows"], 252
    x = f["x_vqt_smoothed"].cpu().numpy().reshape(n_rows, n)
    cnt = f["peak_count"].cpu().numpy().reshape(n_rows)
    ctr = f["center"].cpu().numpy().reshape(n_rows, -1)
    sz = f["size"].cpu().numpy().reshape(n_rows, -1)
    rows = list(range(3, n_rows, 5))            # the first frames of a stream hold little; every fifth row after them
    peaks = [list(zip(ctr[i, :cnt[i]].tolist(), sz[i, :cnt[i]].tolist())) for i in rows]
    rng_ = chain["pp"].range
    want = _model(rng_.min_freq, n, rng_.buckets_per_octave, x[rows], peaks)
    got = {k: t.cpu().numpy()[rows] for k, t in chain["out"].items()}
    _hold_to_the_bars("analysis batch outputs, 252 bins", got, want)


def test_every_subset_of_outputs_and_row_counts(chain):
    f, r, n_rows, out = chain["fields"], chain["r"], chain["n_rows"], chain["out"]
    names = P.RenderBatch.OUTPUTS
    for k in range(1, len(names)):
        for subset in itertools.combinations(names, k):
            part = {}
            for name in subset:
                shape, dt = r.output_shape(name, n_rows)
                part[name] = torch.full(shape, 0x5A if dt == np.uint8 else -1.0, dtype=torch.uint8 if dt == np.uint8 else torch.float32, device="cuda")
            res = r.rows_device(f, part)
            torch.cuda.synchronize()
            assert res is part and all(torch.equal(part[name], out[name]) for name in subset), subset
    flat = {k: f[k].reshape((n_rows,) + tuple(f[k].shape[2:])) for k in ("x_vqt_smoothed", "center", "size", "peak_count")}
    for m in (1, 7):
        res = r.rows_device({k: t[:m].contiguous() for k, t in flat.items()})
        torch.cuda.synchronize()
        assert all(torch.equal(res[name], out[name][:m]) for name in names), m
    # 4 096 x 64 rows: 64 distinct rows, 4 096 times over
    reps, m = 4096, 64
    big = {k: t[:m].repeat((reps,) + (1,) * (t.dim() - 1)).contiguous() for k, t in flat.items()}
    res = r.rows_device(big)
    torch.cuda.synchronize()
    for name in names:
        got = res[name].reshape((reps, m) + tuple(res[name].shape[1:]))
        assert torch.equal(got, out[name][:m].unsqueeze(0).expand_as(got)), name
    del big, res
    # a second call, on another stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        again = r.rows_device(f)
    s.synchronize()
    assert all(torch.equal(again[name], out[name]) for name in names)


# ---- crafted rows (tests/render_cases.py): long lists in any order, every class, the row stride, value edges, placement ------------
# The bars are the file's (test_render.hold_to_the_bars).  The share of byte-identical LED rows is printed, not asserted: its 97 % was
# set on rows of about a dozen peaks; a crafted row holds hundreds.
def _range(min_freq, octaves, bpo):
    return P.VqtRange(min_freq, octaves, bpo)


def _inputs(xs, peak_lists, max_peaks):
    center, size, count = RC.pack(peak_lists, max_peaks)
    return _upload(np.asarray(xs, np.float32), center, size, count)


def _render(r, xs, peak_lists, max_peaks):
    d_x, d_c, d_s, d_n = _inputs(xs, peak_lists, max_peaks)
    out = r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("min_freq,octaves,bpo", RC.CLASS_TABLE)
def test_every_bin_count_class(min_freq, octaves, bpo):
    """render_rows<1> .. <16>, 3 and 1024 bins included (tests/test_render.py holds the table to its coverage): an ordinary row, a
    peakless all-zero row, the centre edges, and a shuffled list of as many peaks as fit"""
    n = octaves * bpo
    xs, lists = RC.class_rows(n, n)
    got = _render(P.RenderBatch(_range(min_freq, octaves, bpo)), xs, lists, max(len(pk) for pk in lists))
    hold_to_the_bars(f"class {(n + 63) // 64}, {n} bins", got, RC.model_rows(min_freq, n, bpo, xs, lists), "device")
    assert not got["spectrogram_peaks"][1].any() and not got["led"][1, 3:].any() and not got["spectrogram_vqt"][1, :, 3].any()
    assert got["spectrogram_peaks"][[0, 2, 3]].any(axis=(1, 2)).all() and got["led"][[0, 2, 3], 3:].any(axis=1).all()
    assert np.all(got["led"][:, 0] == 0xFF) and np.all(got["led"][:, 1].astype(int) * 256 + got["led"][:, 2] == n)


def _list_call(n, max_peaks):
    """(dB rows, peak lists): every crafted list of at most max_peaks peaks in every order, among rows of 0, 1, 64, 65 and max_peaks
    peaks; three dB rows in turn"""
    cases = RC.list_cases(n, n)
    lists = [pk for pk in cases.values() if len(pk) <= max_peaks]
    mix = [[], [(n / 2 + 0.25, 5.0)]] + [RC.spaced_list(n, c, n + 7 * c) for c in (64, 65, max_peaks) if c <= max_peaks]
    mix = [pk if i % 2 else pk[::-1] for i, pk in enumerate(mix)]
    assert all(pk is not None for pk in mix) and sorted({len(pk) for pk in mix}) == sorted({0, 1, max_peaks} | ({64, 65} if max_peaks > 64 else {64}))
    lists = [pk for pair in itertools.zip_longest(lists, mix) for pk in pair if pk is not None]   # short after long, peakless after crowded
    db = RC.db_rows(n, n)
    xs = [(db["ordinary"], np.zeros(n, np.float32), db["negative"])[i % 3] for i in range(len(lists))]
    return xs, lists, cases


LIST_GEOMETRIES = [(55.0, 7, 36), (32.70, 16, 64)]   # 252 and 1024 bins
FULLEST = {252: len(RC.spaced_list(252, None, 252 + 999)), 1024: len(RC.spaced_list(1024, None, 1024 + 999))}


@pytest.mark.parametrize("max_peaks", [64, 65, 129, 200, "fullest"])
@pytest.mark.parametrize("min_freq,octaves,bpo", LIST_GEOMETRIES)
def test_long_lists_in_every_order(min_freq, octaves, bpo, max_peaks):
    """Rows of 64, 65, 127, 128, 129 peaks and of as many as fit, ascending, descending and shuffled, and the pair of lists whose
    deciding two peaks sit either side of the chunk edge: the chunk loop, its barriers, the `p < cnt` tail of a later chunk, a later
    chunk repainting an earlier one's bins.  (tests/test_render.py: reversing any of these lists repaints 64 - 95 % of the spectrogram
    bytes and 6 - 34 % of the LED bytes, so no rule but "the last in list order" passes.)  The width of the arrays does not matter:
    what a row gives at max_peaks 64 it gives at 487, entries beyond its count being NaN."""
    n = octaves * bpo
    if max_peaks == "fullest":
        max_peaks = max(FULLEST[n], 130)
    xs, lists, cases = _list_call(n, max_peaks)
    if max_peaks >= 129:
        assert all(pk in lists for pk in cases.values()) or max_peaks < FULLEST[n]
    assert any(len(pk) == max_peaks for pk in lists) and [] in lists
    got = _render(P.RenderBatch(_range(min_freq, octaves, bpo)), xs, lists, max_peaks)
    hold_to_the_bars(f"{n} bins, max_peaks {max_peaks}, {len(lists)} rows", got, RC.model_rows(min_freq, n, bpo, xs, lists), "device")
    for r, pk in enumerate(lists):                                                # a row at a time: no row hides in the aggregate
        want = RC.model_of_peaks(n, bpo, pk)
        for g, w, k in ((got["spectrogram_peaks"][r], want[0], "spectrogram_peaks"), (got["led"][r], want[1], "led")):
            levels, share = M.compare_u8(g, w)
            assert levels <= U8_LEVELS and share <= U8_SHARE, (r, len(pk), k, levels, share)


def test_straddle_pair_on_the_device():
    """entries 63 and 64 swapped: the contested bin takes the later one's pixel both ways round, the rest of the row is the same"""
    n, bpo = 252, 36
    a, b, B = RC.straddle_pair(n, n)
    got = _render(P.RenderBatch(_range(55.0, 7, bpo)), [np.zeros(n, np.float32)] * 2, [a, b], 67)
    for k, sl in (("spectrogram_peaks", slice(B, B + 1)), ("led", slice(3 + 3 * B, 6 + 3 * B))):
        wa, wb = (RC.model_of_peaks(n, bpo, pk)[k == "led"] for pk in (a, b))
        assert np.any(wa[sl] != wb[sl])
        assert np.abs(got[k][0][sl].astype(int) - wa[sl]).max() <= U8_LEVELS and np.abs(got[k][1][sl].astype(int) - wb[sl]).max() <= U8_LEVELS
        assert np.abs(got[k][0][sl].astype(int) - got[k][1][sl]).max() > 2 * U8_LEVELS       # (so the two could not both match one answer)
    far = got["spectrogram_peaks"][:, :B - 3]
    assert np.array_equal(far[0], far[1]) and far.any()


def test_peak_count_above_max_peaks_is_max_peaks():
    """include/pvq.h: "a count above max_peaks is taken as max_peaks" — max_peaks + 1 and 0xFFFFFFFF on rows whose lists are full"""
    n, max_peaks = 252, 65
    xs, lists, _ = _list_call(n, max_peaks)
    d_x, d_c, d_s, d_n = _inputs(xs, lists, max_peaks)
    r = P.RenderBatch(_range(55.0, 7, 36))
    base = r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n)
    count = d_n.cpu().numpy().astype(np.int64)
    full = np.nonzero(count == max_peaks)[0]
    assert len(full) >= 4
    count[full[0::2]] = max_peaks + 1
    count[full[1::2]] = 0xFFFFFFFF
    raised = torch.from_numpy(count.astype(np.uint32).view(np.int32)).cuda()
    out = r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=raised)
    torch.cuda.synchronize()
    for k in P.RenderBatch.OUTPUTS:
        assert torch.equal(out[k].view(torch.uint8), base[k].view(torch.uint8)), k
    assert base["spectrogram_peaks"].cpu().numpy()[full].any(axis=(1, 2)).all()


def test_row_stride_with_a_different_row_each_time():
    """8192 workgroups stride over 2 x 8192 + 61 rows of 61 distinct ones: as 8192 = 134 x 61 + 18, a workgroup's next row is
    another row (peakless after crowded, a short list after a long one, a NaN row after an ordinary one), so whatever a row leaves
    in LDS or registers meets a row it does not fit.  Every row must be, bit for bit, what the 61-row call gives, which the model pins."""
    n, bpo, m, max_peaks = 252, 36, 61, 129
    cases, db = RC.list_cases(n, n), RC.db_rows(n, n)
    crowded = [pk for name, pk in cases.items() if len(pk) >= 64]
    short = [pk for name, pk in cases.items() if len(pk) <= 12] + [RC.centre_edges(n, n)]
    xs, lists = [], []
    for i in range(m):
        kind = i % 4
        xs.append((np.zeros(n, np.float32), db["ordinary"], db["nan"], db["negative"])[kind] if i % 8 < 4 else
                  (db["ordinary"], db["plus_inf"], db["ordinary"], db["overflow"])[kind])
        lists.append(([], crowded[(i // 4) % len(crowded)], short[(i // 4) % len(short)], crowded[(i // 4 + 7) % len(crowded)][:64 + i])[kind])
    assert sum(not pk for pk in lists) >= 15 and max(len(pk) for pk in lists) == max_peaks
    total = 2 * 8192 + m
    idx = _upload(np.arange(total, dtype=np.int64) % m)[0]
    assert 8192 % m == 18 and all(lists[i] != lists[(i + 8192) % m] or xs[i] is not xs[(i + 8192) % m] for i in range(m))
    d_x, d_c, d_s, d_n = _inputs(xs, lists, max_peaks)
    r = P.RenderBatch(_range(55.0, 7, bpo))
    small = r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n)
    big = r.rows_device(x_vqt_smoothed=d_x[idx].contiguous(), center=d_c[idx].contiguous(), size=d_s[idx].contiguous(), peak_count=d_n[idx].contiguous())
    torch.cuda.synchronize()
    for k in P.RenderBatch.OUTPUTS:
        want = small[k].view(torch.uint8 if k != "chroma" else torch.int32)[idx]                # chroma by its bits: NaN rows
        assert torch.equal(big[k].view(want.dtype), want), k
    hold_to_the_bars(f"{m} distinct rows", {k: t.cpu().numpy() for k, t in small.items()}, RC.model_rows(55.0, n, bpo, xs, lists), "device")


def test_value_edges_on_the_device():
    """all-negative, NaN, +inf, -inf and overflowing dB rows; integer centres, centres in the last bucket and at n - 1; equal sizes,
    all-zero sizes, one zero size"""
    n, bpo = 252, 36
    edge = RC.edge_rows(n, n)
    xs, lists = [x for x, _ in edge.values()], [pk for _, pk in edge.values()]
    got = _render(P.RenderBatch(_range(55.0, 7, bpo)), xs, lists, 12)
    hold_to_the_bars(f"{n} bins, value edges", got, RC.model_rows(55.0, n, bpo, xs, lists), "device")
    check_edge_rows(n, edge, got)


SENTINEL, GUARD = 0xA5, 64


def _carved(shape, dtype, offset):
    """a contiguous tensor of `shape` starting `GUARD + offset` bytes into a sentinel-filled byte buffer; (view, buffer, first, last)"""
    nbytes = int(np.prod(shape)) * (1 if dtype == torch.uint8 else 4)
    buf = torch.full((GUARD + offset + nbytes + GUARD + 4,), SENTINEL, dtype=torch.uint8).cuda()
    assert buf.data_ptr() % 4 == 0
    first = GUARD + offset
    view = buf[first:first + nbytes]
    view = (view if dtype == torch.uint8 else view.view(torch.float32)).view(shape)
    assert view.data_ptr() == buf.data_ptr() + first and view.is_contiguous()
    return view, buf, first, first + nbytes


@pytest.mark.parametrize("min_freq,octaves,bpo", [(32.70, 1, 3), (49.0, 7, 25), (32.70, 16, 64)])   # 3, 175 and 1024 bins
def test_outputs_land_where_they_are_told_and_nowhere_else(min_freq, octaves, bpo):
    """the LED output at byte offsets 0 .. 3 of a dword (its rows, 3 + 3 n bytes long, then start at every offset the head and tail
    logic knows), the RGBA outputs and chroma at their natural alignment: the same bytes as a plain call, and the 64 bytes either
    side untouched"""
    n = octaves * bpo
    xs, lists = RC.class_rows(n, n)
    xs, lists = xs + xs[:3], lists + [lists[3], lists[0], lists[2][::-1]]          # 7 rows
    max_peaks = max(len(pk) for pk in lists)
    d_x, d_c, d_s, d_n = _inputs(xs, lists, max_peaks)
    r = P.RenderBatch(_range(min_freq, octaves, bpo))
    plain = r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n)
    torch.cuda.synchronize()
    assert plain["led"][:, 3:].any() and plain["spectrogram_peaks"].any()
    for offset in range(4):
        carved = {}
        for name in P.RenderBatch.OUTPUTS:
            shape, dt = r.output_shape(name, len(lists))
            carved[name] = _carved(shape, torch.uint8 if dt == np.uint8 else torch.float32, offset if name == "led" else 0)
        assert carved["led"][0].data_ptr() % 4 == offset
        r.rows_device(x_vqt_smoothed=d_x, center=d_c, size=d_s, peak_count=d_n, outputs={k: v[0] for k, v in carved.items()})
        torch.cuda.synchronize()
        for name, (view, buf, first, last) in carved.items():
            assert torch.equal(view.view(torch.uint8), plain[name].view(torch.uint8)), (name, offset)
            assert bool((buf[:first] == SENTINEL).all()) and bool((buf[last:] == SENTINEL).all()), (name, offset)
