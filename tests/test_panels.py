"""The debug panels (pvq_spectrum_mesh, pvq_calmness_histogram_mesh, pvq_calmness_graph_*, pvq_panel_topology, pvq_panels_batch_*) as
far as they go without a GPU: the symbols, the argument checks and the host-only handle, what the compiler made of the kernels, known
answers derived from the reference text alone, and the host face against tests/panels_model.py.

The bar is the model's bits: both sides evaluate IEEE + - * / and sqrt in one order, the colour table through one libm (the
host's).  Arrays are compared as uint32 views; a NaN matches a NaN."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import panels_cases as PC
import panels_model as M
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import panels as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32


def test_symbols_exported_and_abi_version():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    names = sorted(set(re.findall(r"\b(pvq_(?:panels_batch|panel|calmness_graph|calmness_histogram|spectrum)_\w+)\s*\(", hdr)))
    assert len(names) == 14 and "pvq_panels_batch_rows_device" in names and "pvq_spectrum_mesh" in names, names
    for name in names:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4
    assert P.PanelsBatch is PP.PanelsBatch and P.CalmnessGraph is PP.CalmnessGraph and P.spectrum_mesh is PP.spectrum_mesh
    assert P.calmness_histogram_mesh is PP.calmness_histogram_mesh and P.panel_topology is PP.panel_topology


def test_host_only_handle_and_argument_checks():
    L = _lib.load()
    h = C.c_void_p()
    create = L.pvq_panels_batch_create
    assert create(-1, 7, 36, None, 60.0, 4, 0, None) == _lib.PVQ_ERR_INVALID_ARG
    for dev in (-1, 0):   # rejected before any device is touched
        for bad in ((0, 36, 4), (7, 0, 4), (7, 36, 0)):
            assert create(dev, bad[0], bad[1], None, 60.0, bad[2], 0, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, 1, 2, None, 60.0, 4, 0, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value       # 2 bins
        assert create(dev, 25, 41, None, 60.0, 4, 0, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value     # 1025 bins
        assert "1024" in L.pvq_last_error().decode()
        for cap in (1, 1025):
            assert create(dev, 7, 36, None, 60.0, 4, cap, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "capacity" in L.pvq_last_error().decode()
    for octaves, bpo, cap, want in ((1, 3, 0, 300), (7, 36, 2, 2), (16, 64, 1024, 1024)):
        assert create(-1, octaves, bpo, None, 60.0, 2, cap, C.byref(h)) == _lib.PVQ_OK and h.value
        assert L.pvq_panels_batch_graph_capacity(h) == want
        L.pvq_panels_batch_destroy(h)
    assert create(-1, 7, 36, None, 60.0, 3, 0, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        buf = np.zeros(4096, f32)
        p = buf.ctypes.data & ~15   # stands for device memory; a host-only handle never dereferences it
        rows, graph = L.pvq_panels_batch_rows_device, L.pvq_panels_batch_graph_device

        def outs(**kw):
            o = _lib.CPanelsOutputs()
            for k, v in kw.items():
                setattr(o, k, v)
            return C.byref(o)
        assert rows(None, 1, p, p, p, p, 8, p, outs(line_pos=p), None) == _lib.PVQ_ERR_INVALID_ARG
        assert rows(h, 1, p, p, p, p, 8, p, outs(line_pos=p, disc_rgba=p, hist_pos=p), None) == _lib.PVQ_ERR_NO_DEVICE
        assert "GPU" in L.pvq_last_error().decode()
        assert rows(h, 1, p, p, p, p, 8, p, None, None) == _lib.PVQ_ERR_NO_DEVICE
        # a requested output without its input
        for name in ("line_pos", "line_rgba"):
            assert rows(h, 1, None, p, p, p, 8, p, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert rows(h, 1, p, None, None, None, 0, None, outs(**{name: p}), None) == _lib.PVQ_ERR_NO_DEVICE, name
        for name in ("hist_pos", "hist_rgba"):
            assert rows(h, 1, p, p, p, p, 8, None, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, name
            assert rows(h, 1, None, None, None, None, 0, p, outs(**{name: p}), None) == _lib.PVQ_ERR_NO_DEVICE, name
        for name in ("disc_pos", "disc_rgba"):
            for miss in range(3):
                a = [p, p, p]
                a[miss] = None
                assert rows(h, 1, p, a[0], a[1], a[2], 8, p, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG, (name, miss)
            assert rows(h, 1, p, p, p, p, 0, p, outs(**{name: p}), None) == _lib.PVQ_ERR_INVALID_ARG and "max_peaks" in L.pvq_last_error().decode()
            assert rows(h, 1, None, p, p, p, 8, None, outs(**{name: p + 4}), None) == _lib.PVQ_ERR_NO_DEVICE         # dword stores
            assert rows(h, 1, None, p, p, p, 8, None, outs(**{name: p + 2}), None) == _lib.PVQ_ERR_INVALID_ARG
        for name in ("line_pos", "line_rgba", "hist_pos", "hist_rgba"):
            assert rows(h, 1, p, p, p, p, 8, p, outs(**{name: p + 4}), None) == _lib.PVQ_ERR_INVALID_ARG, name       # 16-byte stores
        assert rows(h, 1 << 31, p, p, p, p, 8, p, outs(line_pos=p), None) == _lib.PVQ_ERR_INVALID_ARG
        assert graph(None, 1, p, 0, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert graph(h, 1, p, 0, p, p, None) == _lib.PVQ_ERR_NO_DEVICE
        assert graph(h, 1, None, 0, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert graph(h, 2, p, 3, p, p, None) == _lib.PVQ_ERR_INVALID_ARG and "first_emitted" in L.pvq_last_error().decode()
        assert graph(h, 2, p, 0, p + 4, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert graph(h, 1 << 31, p, 0, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_panels_batch_get_history(h, 3, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_panels_batch_get_history(h, 0, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_panels_batch_get_history(h, 0, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.PVQ_ERR_NO_DEVICE
    finally:
        L.pvq_panels_batch_destroy(h)
    L.pvq_panels_batch_destroy(None)
    L.pvq_calmness_graph_destroy(None)
    # the host face: null arrays, bin counts, capacities
    fp = C.POINTER(C.c_float)
    x = np.zeros(16, f32)
    col = np.ascontiguousarray(PP.COLORS, f32)
    xa, ca = x.ctypes.data_as(fp), col.ctypes.data_as(fp)
    assert L.pvq_spectrum_mesh(4, 12, xa, None, None, 0, ca, 60.0, None, None, None, None) == _lib.PVQ_OK
    assert L.pvq_spectrum_mesh(1, 12, xa, None, None, 0, ca, 60.0, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_spectrum_mesh(4, 0, xa, None, None, 0, ca, 60.0, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_spectrum_mesh(4, 12, xa, None, None, 0, None, 60.0, None, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_spectrum_mesh(4, 12, None, None, None, 0, ca, 60.0, xa, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_spectrum_mesh(4, 12, xa, None, xa, 1, ca, 60.0, None, None, xa, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_calmness_histogram_mesh(4, None, None, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_calmness_histogram_mesh(1, xa, None, None) == _lib.PVQ_ERR_INVALID_ARG
    for cap in (1, 1025):
        assert L.pvq_calmness_graph_create(cap, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    assert L.pvq_calmness_graph_create(2, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_calmness_graph_push(None, 0.5) == _lib.PVQ_ERR_INVALID_ARG
    assert P.CalmnessGraph().capacity == 300 and P.CalmnessGraph(0).capacity == 300 and P.CalmnessGraph(1024).capacity == 1024
    with pytest.raises(ValueError):
        P.CalmnessGraph(1)
    with pytest.raises(ValueError):
        P.spectrum_mesh(4, 12, np.zeros(5, f32))
    b = P.PanelsBatch(P.VqtRange(55.0, 7, 36), 5, device=None)
    assert b.n_bins == 252 and b.graph_capacity == 300 and len(b.OUTPUTS) == 6
    assert b.output_shape("line_pos", 3) == (3, 1004, 3) and b.output_shape("disc_rgba", 2, 7) == (2, 7, 13, 4)
    assert b.output_shape("graph_rgba", 2) == (5, 2, 1196, 4)
    with pytest.raises(P.PvqError) as e:
        b.rows_device({"x_vqt_smoothed": p}, outputs={"line_pos": p}, n_rows=1)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        b.rows_device({"x_vqt_smoothed": p}, outputs={"hist_pos": p}, n_rows=1)
    with pytest.raises(ValueError):
        b.rows_device({"x_vqt_smoothed": p}, outputs={"nonsense": p}, n_rows=1)
    with pytest.raises(P.PvqError) as e:
        b.graph_device(p, outputs={"graph_pos": p}, n_frames=1)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(P.PvqError):
        P.PanelsBatch(P.VqtRange(55.0, 13, 84), 2, device=None)
    with pytest.raises(ValueError):
        P.PanelsBatch(P.VqtRange(55.0, 7, 36), 2, graph_capacity=1025, device=None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """one panels_rows instantiation per 64-chunk of bins; no kernel of the unit uses scratch; at most 128 registers each"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "panels_batch.hip")
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
    rows = {int(re.search(r"panels_rowsILi(\d+)E", k).group(1)): u for k, u in usage.items() if "panels_rows" in k}
    assert sorted(rows) == list(range(1, 17)), list(usage)
    others = {k: u for k, u in usage.items() if "panels_rows" not in k}
    assert len(others) == 2 and any("panels_graph" in k for k in others) and any("panels_history" in k for k in others), list(others)
    for k, u in list(sorted(rows.items())) + list(others.items()):
        print(f"{k if isinstance(k, str) else 'panels_rows<%d>' % k}: {u}")
        assert u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (k, u)


# ---- known answers, from the reference text alone -------------------------------------------------------------------------------
FACES = {"host": (P.spectrum_mesh, P.calmness_histogram_mesh, P.CalmnessGraph, P.panel_topology),
         "model": (M.spectrum_mesh, M.calmness_histogram_mesh, M.CalmnessGraph, M.panel_topology)}


@pytest.mark.parametrize("who", ["host", "model"])
def test_known_answers(who):
    spectrum, histogram, Graph, topology = FACES[who]
    n, bpo = 252, 36
    # a flat spectrum at level a: dy = 0, so v = 0 and u = -0.011 * 0.02 * 0.5 / 0.011: v0.x = v1.x and v0.y - v1.y = +-0.02
    flat = spectrum(n, bpo, np.full(n, 12.5, f32))
    q = flat["line_pos"].reshape(n - 1, 4, 3)
    assert np.array_equal(q[:, 0, 0], q[:, 1, 0]) and np.array_equal(q[:, 2, 0], q[:, 3, 0])
    d = q[:, 0, 1] - q[:, 1, 1]
    assert np.all(np.abs(np.abs(d.astype(np.float64)) - 0.02) < 5e-7) and np.all(q[:, :, 2] == 0.0)
    assert np.array_equal(q[:, 0, 0], (np.arange(n - 1, dtype=f32) * f32(0.011)).astype(f32))
    assert np.all(flat["line_rgba"][:, 3] == 1.0)                                     # every bin is the maximum: 1 - sqrt(0.5 - 1 / 2)
    idx, uvs = topology(n - 1, 0)
    assert np.array_equal(idx.reshape(n - 1, 6), 4 * np.arange(n - 1)[:, None] + np.array([2, 1, 0, 2, 0, 3]))
    assert np.array_equal(uvs.reshape(n - 1, 8), np.tile(np.array([0, 1, 0, 0, 1, 0, 1, 1], f32), (n - 1, 1)))
    # the maximum bin has alpha exactly 1.0, a bin at half the maximum 1 - sqrt(0.25) = 0.5, a bin at zero 1 - sqrt(0.5)
    x = np.full(n, 10.0, f32)
    x[100], x[7] = 20.0, 0.0
    m = spectrum(n, bpo, x, [(40.3, 20.0)])
    a = m["line_rgba"].reshape(n - 1, 4, 4)
    assert np.all(a[100, :, 3] == 1.0) and np.all(a[3, :, 3] == 0.5) and np.all(a[7, :, 3] == f32(1.0) - np.sqrt(f32(0.5)))
    assert np.array_equal(a[5, 0, :3], a[5 + bpo, 0, :3]) and not np.array_equal(a[5, 0, :3], a[8, 0, :3])   # the colour is i % bpo's (5 and 8: another semitone)
    # the disc: centre (center * 0.011, size / 10), vertex 1 at (cx + 0.08, cy), 13 vertices at alpha 0.9 in the colour of round(40.3) = 40
    dp, dc = m["disc_pos"][0], m["disc_rgba"][0]
    cx, cy = f32(f32(40.3) * f32(0.011)), f32(f32(20.0) / f32(10.0))
    assert tuple(dp[0]) == (cx, cy, 0.0) and tuple(dp[1]) == (f32(cx + f32(0.08)), cy, 0.0)
    assert abs(float(dp[4, 0]) - float(cx)) < 5e-7 and abs(float(dp[4, 1]) - float(cy) - 0.08) < 5e-7               # a_3 = TAU / 4
    assert np.all(dc[:, 3] == f32(0.9)) and np.all(dc[:, :3] == a[40, 0, :3])
    idx, uvs = topology(2, 2)
    assert idx.max() == 2 * 4 + 2 * 13 - 1 and len(idx) == 12 + 72 and uvs.shape == (34, 2)
    assert list(idx[12:18]) == [8, 9, 10, 8, 10, 11] and list(idx[12 + 33:12 + 36]) == [8, 20, 9] and list(idx[48:51]) == [21, 22, 23]
    assert tuple(uvs[8]) == (0.5, 0.5) and tuple(uvs[9]) == (1.0, 0.5) and tuple(uvs[21]) == (0.5, 0.5) and tuple(uvs[22]) == (1.0, 0.5)
    # round reaches n: the table index wraps to bucket 0; a negative or NaN centre saturates to bucket 0
    w = spectrum(n, bpo, x, [(0.3, 5.0), (float(f32(n - 0.4)), 7.0), (-0.3, 1.0), (float("nan"), 1.0)])
    for k in range(4):
        assert np.all(w["disc_rgba"][k, :, :3] == a[0, 0, :3]), k
    assert np.isnan(w["disc_pos"][3, :, 0]).all() and w["disc_pos"][3, 0, 1] == f32(f32(1.0) / f32(10.0))
    # an all-zero spectrum: 0 / 0 makes every alpha NaN, the positions are finite
    z = spectrum(n, bpo, np.zeros(n, f32))
    assert np.isnan(z["line_rgba"][:, 3]).all() and np.isfinite(z["line_pos"]).all() and np.isfinite(z["line_rgba"][:, :3]).all()
    # calmness_to_color at averages 0.71, 0.7 (not above: yellow), 0.31 and 0.3 (red)
    c = np.array([0.71, 0.71, 0.7, 0.7, 0.31, 0.31, 0.3, 0.3], f32)
    h = histogram(8, c)
    col = h["rgba"].reshape(7, 4, 4)[:, 0]
    cyan, yellow, red = [0.5, 0.8, 1.0, 1.0], [1.0, 1.0, 0.5, 1.0], [1.0, 0.5, 0.5, 1.0]
    assert np.array_equal(col[[0, 2, 4, 6]], np.asarray([cyan, yellow, yellow, red], f32))
    hp = h["pos"].reshape(7, 4, 3)
    assert h["pos"].shape == (28, 3) and np.all(np.abs(np.abs((hp[::2, 0, 1] - hp[::2, 1, 1]).astype(np.float64)) - 0.01) < 5e-7)
    assert abs(float(hp[0, 0, 1]) - (0.355 + 0.005)) < 1e-6                           # 0.71 * 0.5 - u, u = -0.005
    # a graph of capacity 4 after pushes 0.1, 0.5, 0.9
    g = Graph(4)
    for v in (0.1, 0.5, 0.9):
        g.push(v)
    gm = g.mesh()
    assert np.array_equal(gm["history"], np.asarray([0.0, 0.1, 0.5, 0.9], f32))
    gp = gm["pos"].reshape(3, 4, 3)
    mid = (gp[:, 0, :2].astype(np.float64) + gp[:, 1, :2]) / 2                           # v0 and v1 straddle p
    assert np.allclose(mid[:, 0], [-0.5, -0.25, 0.0], atol=1e-7) and np.allclose(mid[:, 1], [0.0, 0.1, 0.5], atol=1e-7)
    mid_q = (gp[2, 2, :2].astype(np.float64) + gp[2, 3, :2]) / 2
    assert np.allclose(mid_q, [0.25, 0.9], atol=1e-7)
    assert np.array_equal(gm["rgba"].reshape(3, 4, 4)[:, 0], np.asarray([red, red, yellow], f32))


# ---- host against model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_freq,octaves,bpo", PC.GEOMETRIES)
def test_host_matches_model(min_freq, octaves, bpo):
    n = octaves * bpo
    case = PC.make(min_freq, octaves, bpo, 11, 300 + n)
    assert any(len(pk) == case["max_peaks"] for pk in case["peaks"]) and [] in case["peaks"] and not case["x"][-5].any()
    worst = {}
    for r, pk in enumerate(case["peaks"]):
        got, want = P.spectrum_mesh(n, bpo, case["x"][r], pk), M.spectrum_mesh(n, bpo, case["x"][r], pk)
        hg, hw = P.calmness_histogram_mesh(n, case["calmness"][r]), M.calmness_histogram_mesh(n, case["calmness"][r])
        assert hw["skipped"] == 0                                                     # the `l < 0.0001` skip never fires
        for k, g, w in [(k, got[k], want[k]) for k in got] + [("hist_" + k, hg[k], hw[k]) for k in hg]:
            worst[k] = max(worst.get(k, 0), M.same_bits(g, w))
    print(f"{n} bins: host vs model over {len(case['peaks'])} rows, differing 32-bit words: {worst}")
    assert not any(worst.values()), worst
    zero = P.spectrum_mesh(n, bpo, case["x"][-5], [])
    assert np.isnan(zero["line_rgba"][:, 3]).all() and np.isfinite(zero["line_pos"]).all() and zero["disc_pos"].shape == (0, 13, 3)


def _line_differs(n, bpo, x, y):
    """differing 32-bit words of line_rgba between two spectra on the host face"""
    return M.same_bits(P.spectrum_mesh(n, bpo, x)["line_rgba"], P.spectrum_mesh(n, bpo, y)["line_rgba"])


@pytest.mark.parametrize("min_freq,octaves,bpo", PC.EDGE_GEOMETRIES)
def test_arg_max_edges_host_matches_model(min_freq, octaves, bpo):
    """util::arg_max on rows it was not written for (tests/panels_cases.edge_spectra): both signs of zero as the maximum, NaN, rows
    that never exceed f32::MIN, +inf, the maximum on a 64-chunk edge and in the last bin.  max_size is x[arg_max]; its value and
    its sign show in every alpha of the row."""
    n = octaves * bpo
    spectra = PC.edge_spectra(n, 700 + n)
    assert len(spectra) == 16
    worst = {}
    for name, (x, at) in spectra.items():
        assert M.arg_max(x) == (0 if at is None else at), name                       # the model's fold finds what the case was built for
        if at is None:
            assert not (x > M.F32_MIN).any()
        elif name != "plus_inf":
            assert x[at] == np.nanmax(x) and (name.startswith("zeros") or int(np.sum(x == x[at])) == 1), name
        assert (x < 0).any() or name == "all_nan", name
        got, want = P.spectrum_mesh(n, bpo, x), M.spectrum_mesh(n, bpo, x)
        worst[name] = sum(M.same_bits(got[k], want[k]) for k in got)
        alpha = got["line_rgba"].reshape(n - 1, 4, 4)[:, 0, 3]
        ms = x[0 if at is None else at]
        with np.errstate(all="ignore"):
            expect = (f32(1.0) - np.sqrt(f32(0.5) - x[:-1] / ms / f32(2.0))).astype(f32)
        assert M.same_bits(alpha, expect) == 0, name                                 # the alphas of THIS max_size, sign included
    print(f"{n} bins: host vs model, differing 32-bit words per crafted spectrum: {worst}")
    assert not any(worst.values()), worst
    for name in ("zeros_first_and_last", "zeros_one_lane", "zeros_two_lanes"):       # -0 first and +0 first are told apart
        a, b = spectra[name][0], spectra[name + "_swapped"][0]
        assert np.array_equal(a, b) and np.signbit(a[spectra[name][1]]) and not np.signbit(b[spectra[name][1]])
        d = _line_differs(n, bpo, a, b)
        assert d >= 4 * (n - 3), (name, d)                                            # every negative bin: +inf against -inf under the root
        al = P.spectrum_mesh(n, bpo, a)["line_rgba"][:, 3]
        assert np.isnan(al).all(), name                                               # x / -0 = +inf: sqrt(0.5 - inf) is NaN
        assert np.isneginf(P.spectrum_mesh(n, bpo, b)["line_rgba"][:, 3]).sum() >= 4 * (n - 3), name
    nan_row = P.spectrum_mesh(n, bpo, spectra["all_nan"][0])
    assert np.isnan(nan_row["line_rgba"][:, 3]).all()
    flt = P.spectrum_mesh(n, bpo, spectra["all_minus_flt_max"][0])["line_rgba"][:, 3]
    assert np.all(flt == 1.0)                                                         # max_size = x[0] = every entry
    inf_row = P.spectrum_mesh(n, bpo, spectra["plus_inf"][0])["line_rgba"].reshape(n - 1, 4, 4)[:, 0, 3]
    assert np.isnan(inf_row[n // 3]) and np.all(np.delete(inf_row, n // 3) == f32(1.0) - np.sqrt(f32(0.5)))


@pytest.mark.parametrize("max_peaks", sorted(PC.DISC_COUNTS))
def test_long_disc_lists_host_matches_model(max_peaks):
    """lists of 63, 64, 65, 128 and 129 discs (tests/test_panels_gpu.py takes them through the device's 64-chunk loop)"""
    counts = PC.DISC_COUNTS[max_peaks]
    assert {63, 64}.issubset(counts) and max(counts) == max_peaks and 0 in counts and all(c <= max_peaks for c in counts)
    case = PC.list_case(55.0, 5, 39, max_peaks, counts, 800 + max_peaks)
    got, want = PC.host_rows(P, case), PC.model_rows(M, case)
    diff = {k: M.same_bits(got[k], want[k]) for k in got}
    print(f"max_peaks {max_peaks}, counts {counts}: host vs model, differing 32-bit words: {diff}")
    assert not any(diff.values()), diff
    assert np.isnan(case["center"][np.arange(max_peaks)[None, :] >= case["count"][:, None]]).all()


def test_stride_rows_host_matches_model():
    """the 61 rows of the device's row-stride test: the model's bits, and the orders the test is there for"""
    case, kinds = PC.stride_case()
    m = PC.STRIDE_ROWS
    got, want = PC.host_rows(P, case), PC.model_rows(M, case)
    diff = {k: M.same_bits(got[k], want[k]) for k in got}
    print(f"{m} stride rows: host vs model, differing 32-bit words: {diff}")
    assert not any(diff.values()), diff
    empty = [r for r in range(m) if not got["disc_pos"][r].view(np.uint32).any() and not got["disc_rgba"][r].view(np.uint32).any()]
    assert empty == [r for r in range(m) if kinds[r][0] == "empty"] and 4 * len(empty) <= m
    differ = lambda i, j: all(M.same_bits(got[k][i], got[k][j]) for k in got) and all(
        not np.array_equal(case[k][i], case[k][j], equal_nan=True) for k in ("x", "calmness", "center", "size"))     # (two counts may both be 65)
    pairs = PC.stride_follows(m, 8192, differ)
    orders = {(kinds[i][0], kinds[j][0]) for i, j in pairs} | {(kinds[i][1], kinds[j][1]) for i, j in pairs}
    assert {("full", "empty"), ("crossing", "short"), ("ordinary", "nan")} <= orders, orders


@pytest.mark.parametrize("capacity", [2, 5, 64, 65, 129, 1024])
def test_graph_handle_matches_model(capacity):
    rng = np.random.default_rng(capacity)
    for k in (1, capacity - 1, capacity, capacity + 1, 2 * capacity + 3):
        vals = rng.random(k, dtype=f32)
        vals[::3] = [0.7, 0.3, 0.71, 0.31, 0.0][k % 5]
        h, m = P.CalmnessGraph(capacity), M.CalmnessGraph(capacity)
        for v in vals:
            h.push(float(v))
            m.push(v)
        got, want = h.mesh(), m.mesh()
        diff = {key: M.same_bits(got[key], want[key]) for key in got}
        assert not any(diff.values()), (capacity, k, diff)
        tail = np.concatenate([np.zeros(capacity, f32), vals])[-capacity:]
        assert np.array_equal(got["history"], tail)


def test_graph_handle_at_the_viewer_capacity():
    h, m = P.CalmnessGraph(), M.CalmnessGraph()
    for v in np.random.default_rng(3).random(301, dtype=f32):
        h.push(float(v))
        m.push(v)
    got, want = h.mesh(), m.mesh()
    assert got["pos"].shape == (4 * 299, 3) and not any(M.same_bits(got[k], want[k]) for k in got)


def test_panel_topology():
    for nq, nc in ((0, 0), (1, 0), (0, 1), (251, 12), (1023, 70)):
        idx, uvs = P.panel_topology(nq, nc)
        mi, mu = M.panel_topology(nq, nc)
        assert np.array_equal(idx, mi) and M.same_bits(uvs, mu) == 0, (nq, nc)
        assert idx.shape == (6 * nq + 36 * nc,) and uvs.shape == (4 * nq + 13 * nc, 2)
        if nq + nc:
            assert idx.min() == 0 and idx.max() == 4 * nq + 13 * nc - 1
        if nc:
            discs = idx[6 * nq:].reshape(nc, 12, 3)
            assert np.array_equal(discs[:, 0, 0], 4 * nq + 13 * np.arange(nc))     # disc bases follow the quads
            assert np.all(discs[:, :, 1] - discs[:, :, 0] == np.arange(1, 13)) and np.all(discs[:, 11, 2] == discs[:, 0, 1])
            assert np.all((uvs >= 0.0) & (uvs <= 1.0))
