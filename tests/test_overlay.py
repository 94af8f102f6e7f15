"""The overlay stage (pvq_overlay_*: the scrolling spectrogram quad and the chroma boxes in front of the balls) as far as it goes
without a GPU: the symbols, the argument checks and the host-only handle, what the compiler made of the kernels, known answers of
the rule worked from its statement alone, and the host face against tests/overlay_model.py, which keeps the texture literally.

The bar, here and in tests/test_overlay_gpu.py: no differing bit in any pixel channel."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import overlay_cases as OC
import overlay_model as M
import pitchvis_amd as P
from pitchvis_amd import _lib
from pitchvis_amd import overlay as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32 = np.float32
NAMES = ["pvq_overlay_batch_create", "pvq_overlay_batch_destroy", "pvq_overlay_batch_frames_device", "pvq_overlay_batch_get_texture",
         "pvq_overlay_frame", "pvq_overlay_quad", "pvq_overlay_state_create", "pvq_overlay_state_destroy", "pvq_overlay_state_push",
         "pvq_overlay_state_texture"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, want, tag):
    diff = bits(got) != bits(want)
    assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ---- 1. symbols and arguments ---------------------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pvq.h")).read()
    assert sorted(set(re.findall(r"\b(pvq_overlay_\w+)\s*\(", hdr))) == NAMES
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pvq_abi_version() == 4   # additive: nothing that existed changed
    assert P.OverlayBatch is PO.OverlayBatch and P.OverlayState is PO.OverlayState
    assert P.overlay_frame is PO.overlay_frame and P.overlay_quad is PO.overlay_quad


def test_left_out_lists_name_only_what_is_left():
    """the two lists of include/pvq.h and the two of DESIGN.md no longer name the quad and the boxes as missing"""
    for path in ("include/pvq.h", "DESIGN.md"):
        text = open(os.path.join(ROOT, path)).read()
        lists = re.findall(r"Left out:.*?(?:\*/|\n\n)", text, flags=re.S)
        assert lists, path
        for item in lists:
            flat = " ".join(item.split())
            if "chroma boxes" in flat:
                assert "overlay stage" in flat, (path, flat[:200])


@pytest.mark.parametrize("h,n", [(200, 252), (0, 252), (2, 3), (4096, 1024), (5, 24)])
def test_overlay_quad(h, n):
    q = P.overlay_quad(n, h)
    hh = h or 200
    same(q, M.quad(n, hh), (h, n))
    same(q, np.asarray([-7.0, 6.0, 12.0, f32(12.0) * f32(f32(hh) / f32(n))], f32), (h, n))
    assert abs(float(q[3]) - 12.0 * hh / n) <= 1e-6 * 12.0 * hh / n


def test_argument_ranges_and_host_only_handle():
    L = _lib.load()
    buf = np.zeros(4096, f32)
    p = buf.ctypes.data   # stands for device memory; a host-only handle never dereferences it
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    bp = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    bad_quads = [(0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, -1.0), (math.nan, 0.0, 1.0, 1.0), (0.0, 0.0, math.inf, 1.0), (0.0, math.inf, 1.0, 1.0)]
    # pvq_overlay_quad and the state
    for n, h in ((2, 200), (1025, 200), (252, 1), (252, 4097)):
        assert L.pvq_overlay_quad(n, h, fp) == _lib.PVQ_ERR_INVALID_ARG, (n, h)
        s = C.c_void_p()
        assert L.pvq_overlay_state_create(n, h, C.byref(s)) == _lib.PVQ_ERR_INVALID_ARG and not s.value, (n, h)
    assert L.pvq_overlay_quad(252, 200, None) == _lib.PVQ_ERR_INVALID_ARG
    assert L.pvq_overlay_state_create(252, 200, None) == _lib.PVQ_ERR_INVALID_ARG
    s = C.c_void_p()
    assert L.pvq_overlay_state_create(3, 2, C.byref(s)) == _lib.PVQ_OK and s.value
    try:
        assert L.pvq_overlay_state_push(s, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_overlay_state_push(None, bp) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_overlay_state_texture(None, bp, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_overlay_state_texture(s, None, None) == _lib.PVQ_OK
        # the host face
        frame = L.pvq_overlay_frame
        assert frame(s, 8, 8, 0.0, 0.0, None, fp, None, fp) == _lib.PVQ_OK
        assert frame(None, 8, 8, 0.0, 1.0, None, fp, None, fp) == _lib.PVQ_OK
        assert frame(s, 8, 8, 0.0, 1.0, None, None, None, fp) == _lib.PVQ_OK
        assert frame(None, 8, 8, 0.0, 1.0, None, None, None, fp) == _lib.PVQ_ERR_INVALID_ARG      # neither layer
        assert frame(s, 8, 8, 0.0, 1.0, None, fp, None, None) == _lib.PVQ_ERR_INVALID_ARG         # no image
        for w, hh in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
            assert frame(s, w, hh, 0.0, 1.0, None, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG and "4096" in L.pvq_last_error().decode()
        for vh in (-1.0, math.inf, math.nan):
            assert frame(s, 8, 8, vh, 1.0, None, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG and "viewport_height" in L.pvq_last_error().decode()
        for ui in (-1.0, math.inf, math.nan):
            assert frame(s, 8, 8, 0.0, ui, None, fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG and "ui_scale" in L.pvq_last_error().decode()
        for q in bad_quads:
            assert frame(s, 8, 8, 0.0, 1.0, (C.c_float * 4)(*q), fp, None, fp) == _lib.PVQ_ERR_INVALID_ARG and "quad" in L.pvq_last_error().decode()
    finally:
        L.pvq_overlay_state_destroy(s)
    L.pvq_overlay_state_destroy(None)
    # the batch handle: every range, rejected before any device is touched
    create = L.pvq_overlay_batch_create
    h = C.c_void_p()
    assert create(-1, 7, 36, 200, 0.0, 1.0, None, None, 2, 64, 64, None) == _lib.PVQ_ERR_INVALID_ARG
    for dev in (-1, 0):
        for o, b, ns in ((0, 36, 4), (7, 0, 4), (7, 36, 0)):
            assert create(dev, o, b, 200, 0.0, 1.0, None, None, ns, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        assert create(dev, 1, 2, 200, 0.0, 1.0, None, None, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
        assert create(dev, 25, 41, 200, 0.0, 1.0, None, None, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_UNSUPPORTED and not h.value
        assert "1024" in L.pvq_last_error().decode()
        for hr in (1, 4097):
            assert create(dev, 7, 36, hr, 0.0, 1.0, None, None, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
            assert "history_rows" in L.pvq_last_error().decode()
        for w, hh in ((0, 64), (64, 0), (4097, 64), (64, 4097)):
            assert create(dev, 7, 36, 200, 0.0, 1.0, None, None, 4, w, hh, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        for vh in (-1.0, math.inf, math.nan):
            assert create(dev, 7, 36, 200, vh, 1.0, None, None, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        for ui in (-0.5, math.inf, math.nan):
            assert create(dev, 7, 36, 200, 0.0, ui, None, None, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
        for q in bad_quads:
            assert create(dev, 7, 36, 200, 0.0, 1.0, (C.c_float * 4)(*q), None, 4, 64, 64, C.byref(h)) == _lib.PVQ_ERR_INVALID_ARG and not h.value
    for o, b, hr, w, hh, ui in ((1, 3, 2, 1, 1, 0.0), (7, 36, 0, 4096, 4096, 1.0), (16, 64, 4096, 129, 33, 0.25)):
        assert create(-1, o, b, hr, 20.0, ui, None, None, 2, w, hh, C.byref(h)) == _lib.PVQ_OK and h.value
        L.pvq_overlay_batch_destroy(h)
    assert create(-1, 7, 36, 0, 0.0, 0.0, (C.c_float * 4)(0.0, 0.0, 4.0, 3.0), fp, 3, 64, 48, C.byref(h)) == _lib.PVQ_OK and h.value
    try:
        call = L.pvq_overlay_batch_frames_device
        assert call(None, 1, p, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1, p, p, p, None) == _lib.PVQ_ERR_NO_DEVICE and "GPU" in L.pvq_last_error().decode()
        assert call(h, 1, None, p, p, None) == _lib.PVQ_ERR_NO_DEVICE          # boxes alone
        assert call(h, 1, p, None, p, None) == _lib.PVQ_ERR_NO_DEVICE          # quad alone
        assert call(h, 1, None, None, p, None) == _lib.PVQ_ERR_INVALID_ARG     # neither layer
        assert call(h, 1, p, p, None, None) == _lib.PVQ_ERR_INVALID_ARG        # no image
        assert call(h, 1, p, p, p + 8, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in L.pvq_last_error().decode()
        assert call(h, 1, p + 2, p, p, None) == _lib.PVQ_ERR_INVALID_ARG and "aligned" in L.pvq_last_error().decode()
        assert call(h, 1, p, p + 1, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert call(h, 1 << 31, p, p, p, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_overlay_batch_get_texture(h, 0, bp, None) == _lib.PVQ_ERR_NO_DEVICE
        assert L.pvq_overlay_batch_get_texture(h, 3, bp, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_overlay_batch_get_texture(h, 0, None, None) == _lib.PVQ_ERR_INVALID_ARG
        assert L.pvq_overlay_batch_get_texture(None, 0, bp, None) == _lib.PVQ_ERR_INVALID_ARG
    finally:
        L.pvq_overlay_batch_destroy(h)
    L.pvq_overlay_batch_destroy(None)
    # the Python face
    b = P.OverlayBatch(P.VqtRange(55.0, 7, 36), 5, 64, 48, device=None)
    assert (b.n_bins, b.width, b.height, b.history_rows) == (252, 64, 48, 200)
    with pytest.raises(P.PvqError) as e:
        b.frames(1, p, rows=p, chroma=p)
    assert e.value.status == _lib.PVQ_ERR_NO_DEVICE
    with pytest.raises(P.PvqError):
        b.texture(0)
    with pytest.raises(ValueError):
        b.frames(1, p)
    with pytest.raises(ValueError):
        P.OverlayBatch(P.VqtRange(55.0, 7, 36), 5, 64, 5000, device=None)
    with pytest.raises(ValueError):
        P.OverlayBatch(P.VqtRange(55.0, 7, 36), 5, 64, 48, quad=(0.0, 0.0, 1.0), device=None)
    with pytest.raises(ValueError):
        P.OverlayBatch(P.VqtRange(55.0, 7, 36), 5, 64, 48, colors=np.zeros((11, 3)), device=None)
    with pytest.raises(ValueError):
        P.OverlayState(24, 5).push(np.zeros((23, 4), np.uint8))
    with pytest.raises(ValueError):
        P.overlay_frame(np.zeros((4, 4, 4), f32), chroma=np.zeros(11, f32))


# ---- 2. kernel resources --------------------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """no kernel of the unit uses scratch; VGPRs, LDS and occupancy recorded"""
    src = os.path.join(ROOT, "pitchvis_amd", "csrc", "overlay_batch.hip")
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
    kern = {}
    for want in ("overlay_draw", "overlay_keep"):
        found = [u for k, u in usage.items() if want in k]
        assert len(found) == 1, (want, list(usage))
        kern[want] = found[0]
        print(f"{want}: {found[0]}")
    assert len(usage) == 2, list(usage)
    for k, u in kern.items():
        assert u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64, (k, u)       # a pixel's state is small: full occupancy
        assert u["Occupancy"] >= 8, (k, u)
    assert kern["overlay_draw"]["LDS"] == 548 * 4                 # the decode tables: 256 + 256 + 36 floats
    assert kern["overlay_keep"]["LDS"] == 0


# ---- 3. the ring, kept literally ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [2, 3, 5, 7])
def test_state_texture_matches_model(h):
    n = 9
    rows = OC.rows(1, 2 * h + 1, n, 10 + h)[0]
    for pushes in (0, 1, h - 1, h, 2 * h + 1):
        st, tex = P.OverlayState(n, h), M.Texture(n, h)
        for r in rows[:pushes]:
            st.push(r)
            tex.push(r)
        got, w = st.texture()
        assert np.array_equal(got, tex.tex) and w == tex.write_index == pushes % h, (h, pushes)
        assert not got[h - 1 - w].any()                              # the next line is cleared
        if pushes:
            assert np.array_equal(got[h - 1 - (pushes - 1) % h], rows[pushes - 1])   # the newest row, flipped
        if pushes == 0:
            assert not got.any()
    assert P.OverlayState(9, 0).history_rows == 200


def test_scroll_known_answers():
    """h = 4 rows of 3 bins over a 4 x 3 image, the quad over the whole image: a column is a texture row, a pixel row a bin.  The
    newest row shows in the rightmost column, the zeroed row in the leftmost; bins run bottom to top."""
    n, h, W, H = 3, 4, 4, 3
    q = OC.full_quad(W, H)
    bg = np.full((H, W, 4), 0.5, f32)
    assert np.array_equal(P.overlay_frame(bg, P.OverlayState(n, h), viewport_height=3.0, quad=q), bg)   # a never-written ring
    st = P.OverlayState(n, h)
    for k in range(1, 8):
        row = np.zeros((n, 4), np.uint8)
        row[:, 0], row[:, 1], row[:, 3] = 10 * k, np.arange(n) + 1, 255        # red tells the frame, green the bin; opaque
        st.push(row)
        img = P.overlay_frame(bg, st, viewport_height=3.0, quad=q)
        same(img, M.frame(bg, _texture_of(st), viewport_height=3.0, quad_=q), k)
        assert np.array_equal(img[:, 0], bg[:, 0])                              # the zeroed row, at the left edge
        for age, col in enumerate((3, 2, 1)):
            frame = k - age
            for j, b in enumerate((2, 1, 0)):                                   # pixel row 0 is the top: the highest bin
                want = bg[j, col] if frame < 1 else [M.LINEAR[10 * frame], M.LINEAR[b + 1], M.LINEAR[0], 1.0]
                assert np.array_equal(img[j, col], np.asarray(want, f32)), (k, age, b)


def _texture_of(st):
    """the model's Texture standing as a host state stands"""
    tex = M.Texture(st.n_bins, st.history_rows)
    tex.tex, tex.write_index = st.texture()
    return tex


# ---- 4. the host face against the model -----------------------------------------------------------------------------------------
HOST_CASES = [(1, 1, 24, 5, 7), (7, 5, 24, 5, 7), (16, 16, 24, 5, 7), (17, 33, 24, 5, 7), (129, 33, 24, 5, 7), (40, 24, 3, 6, 9),
              (40, 24, 252, 6, 9), (40, 24, 1024, 6, 9), (4, 1030, 1024, 3, 4), (24, 8, 24, 2, 5), (260, 3, 24, 200, 230)]


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: "%dx%d-%dbins-h%d-%df" % c)
def test_frames_match_model(case):
    W, H, n, h, nf = case
    rows, chroma, imgs = OC.rows(1, nf, n, 20 + W)[0], OC.chroma(1, nf, 21)[0], OC.images(1, nf, W, H, 22, nans=True)[0]
    q = OC.full_quad(W, H)
    info = []
    want, tex = OC.model_chain(n, h, rows, chroma, imgs, info=info, viewport_height=3.0, quad_=q)
    got, st = OC.host_chain(n, h, rows, chroma, imgs, viewport_height=3.0, quad_=q)
    same(got, want, case)
    assert np.array_equal(st.texture()[0], tex.tex)
    if (W, H) != (1, 1):
        assert not np.array_equal(got, imgs)
        ages = set().union(*(d["ages"] for d in info))
        assert len(ages) >= min(h - 1, 4) and max(ages) <= h - 2, (case, sorted(ages))
        assert len(set().union(*(d["bins"] for d in info))) >= min(n, H, 4)
    untouched = bits(got) == bits(imgs)
    assert untouched.all(-1).any() or (W, H) == (1, 1)               # the zeroed row's column keeps its bits, NaN payloads included


def test_reference_quad_and_view():
    """quad=None and viewport_height=0 at 252 bins: the viewer's placement, top left of the picture"""
    n, h, W, H, nf = 252, 200, 64, 36, 3
    rows, chroma, imgs = OC.rows(1, nf, n, 30)[0], OC.chroma(1, nf, 31)[0], OC.images(1, nf, W, H, 32)[0]
    info = []
    want, _ = OC.model_chain(n, h, rows, chroma, imgs, info=info, before=OC.rows(1, 230, n, 33)[0])
    got, _ = OC.host_chain(n, h, rows, chroma, imgs, before=OC.rows(1, 230, n, 33)[0])
    same(got, want, "reference quad")
    assert info[-1]["drawn"] > 0.1 * W * H and len(info[-1]["ages"]) > 20 and len(info[-1]["bins"]) > 10
    changed = (bits(got[-1]) != bits(imgs[-1])).any(-1)
    ys, xs = np.nonzero(changed)
    s = float(M.RM.VIEWPORT_HEIGHT) / H
    assert xs.max() < W / 2 + (-7.0 + 6.0) / s + 1 and ys.max() < H / 2 - (6.0 - 0.5 * 12.0 * 200 / 252) / s + 1


@pytest.mark.parametrize("mode", [_lib.SPECTROGRAM_VQT, _lib.SPECTROGRAM_PEAKS])
def test_rows_of_both_spectrogram_modes(mode):
    """rows as pvq_spectrogram_row returns them: in Peaks mode most texels are zeros and leave the picture alone"""
    n, bpo, h, W, H, nf = 24, 12, 5, 20, 24, 6
    rng = np.random.default_rng(40 + mode)
    rows = []
    for f in range(nf):
        x = rng.uniform(0.0, 1.0, n).astype(f32)
        peaks = [(float(c), float(z)) for c, z in zip(rng.uniform(1.0, n - 2.0, 3), rng.uniform(0.2, 1.0, 3))]
        rows.append(P.spectrogram_row(mode, n, bpo, x, peaks))
    rows, imgs = np.asarray(rows), OC.images(1, nf, W, H, 41)[0]
    q = OC.full_quad(W, H)
    info = []
    want, _ = OC.model_chain(n, h, rows, None, imgs, info=info, viewport_height=3.0, quad_=q)
    got, _ = OC.host_chain(n, h, rows, None, imgs, viewport_height=3.0, quad_=q)
    same(got, want, mode)
    assert info[-1]["drawn"] > 0 and (mode == _lib.SPECTROGRAM_VQT or info[-1]["drawn"] < 0.5 * W * H)


# ---- 5. the chroma boxes --------------------------------------------------------------------------------------------------------
def rule_box(i, j, H, s):
    """the box of pixel (i, j) straight from the rule's statement, in doubles (every value the two scales below produce is exact)"""
    px, py = i + 0.5, j + 0.5
    y0, y1, r = H - 50 * s, H - 10 * s, 4 * s
    if not y0 <= py < y1:
        return None
    for pc in range(12):
        x0 = (400 + 45 * pc) * s
        x1 = x0 + 40 * s
        if x0 <= px < x1:
            cx, cy = min(max(px, x0 + r), x1 - r), min(max(py, y0 + r), y1 - r)     # the nearest point of the inner rectangle
            if cx != px and cy != py and (px - cx) ** 2 + (py - cy) ** 2 > r * r:  # in a corner square, outside its circle
                return None
            return pc
    return None


@pytest.mark.parametrize("scale,W,H", [(1.0, 960, 56), (0.25, 240, 14)])
def test_boxes_known_answers(scale, W, H):
    bg = OC.images(1, 1, W, H, 50)[0, 0]
    c = np.linspace(0.3, 1.0, 12).astype(f32)
    c[3], c[7], c[9] = np.nan, 0.0, -1.0
    img = P.overlay_frame(bg, None, c, ui_scale=scale)
    same(img, M.frame(bg, None, c, ui_scale=scale), scale)
    changed = (bits(img) != bits(bg)).any(-1)
    box = np.asarray([[rule_box(i, j, H, scale) for i in range(W)] for j in range(H)], object)
    want = np.asarray([[b is not None and b not in (3, 7, 9) for b in row] for row in box])   # NaN, 0 and negative strengths draw nothing
    assert np.array_equal(changed, want)
    assert want.sum() > 9 * 0.9 * (40 * scale) ** 2
    # positions, half-open edges and rounded corners of box 0, whose left edge is at x = 400 s and top edge at y = H - 50 s
    left, top = int(400 * scale), math.ceil(H - 50 * scale - 0.5)
    side, mid = int(40 * scale), int(20 * scale)
    assert not changed[top + mid, left - 1] and changed[top + mid, left] and changed[top + mid, left + side - 1] and not changed[top + mid, left + side]
    assert not changed[top - 1, left + mid] and changed[top, left + mid] and changed[top + side - 1, left + mid] and not changed[top + side, left + mid]
    # A corner pixel is outside, its diagonal neighbour inside.  At s = 1 a corner pixel's centre is (3.5, 3.5) from the circle's
    # centre: 24.5 > 16.  At s = 0.25 and H = 14 the box spans y = 1.5 .. 11.5: a top corner pixel's centre lies on the top edge,
    # (0.5, 1) from the circle's centre, 1.25 > 1; a bottom one lies level with the circle's centre, in no corner square: inside.
    for jj, ii, dj, di in ((top, left, 1, 1), (top, left + side - 1, 1, -1), (top + side - 1, left, -1, 1), (top + side - 1, left + side - 1, -1, -1)):
        assert changed[jj, ii] == (scale == 0.25 and dj == -1) and changed[jj + dj, ii + di], (jj, ii)
    lin = [[M.RM.srgb_to_linear(x) for x in rgb] for rgb in M.COLORS]
    for pc in (0, 4, 11):
        j, i = top + mid, int((400 + 45 * pc) * scale) + mid
        k = f32(1.0) - c[pc]
        px = [f32(lin[pc][ch]) * c[pc] + bg[j, i, ch] * k for ch in range(3)] + [c[pc] + bg[j, i, 3] * k]
        assert box[j, i] == pc and np.array_equal(img[j, i], np.asarray(px, f32)), pc


def test_boxes_with_palette_and_default_scale():
    bg = np.full((60, 960, 4), 0.25, f32)
    c = np.full(12, 0.5, f32)
    pal = np.random.default_rng(51).uniform(0.0, 1.0, (12, 3)).astype(f32)
    same(P.overlay_frame(bg, None, c, colors=pal), M.frame(bg, None, c, colors=pal), "palette")
    same(P.overlay_frame(bg, None, c, ui_scale=0.0), P.overlay_frame(bg, None, c, ui_scale=1.0), "ui_scale 0 means 1")
    assert not np.array_equal(P.overlay_frame(bg, None, c, colors=pal), P.overlay_frame(bg, None, c))
