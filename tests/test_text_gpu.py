"""The text stage on the device (pvq_text_batch_*) against the host face (pvq_text_frame).  The bar: no differing bit in the
coverage layer or in any pixel channel — the device adds the host face's segment areas in the host face's order.

All fonts come from outline arrays (the fixture's nine DejaVuSans glyphs, or the synthetic fonts of tests/text_cases.py), so the
GPU machine needs neither a font file nor fontTools.  Shapes are chosen for where the kernels can go wrong: sides that are no
multiple of the 16 x 16 tile or the 8 x 8 wave block, labels cut by every image edge, tiles with several labels, more segments
than one LDS chunk, more rows than the blend's grid."""

import numpy as np
import pytest

import pitchvis_amd as P
import text_cases as TC
from pitchvis_amd import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32
bits, same = TC.bits, TC.same


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def dejavu():
    return TC.font_of(TC.fixture())


@pytest.fixture(scope="module")
def syn():
    return TC.font_of(TC.SYNTHETIC)


def hold(tag, font, labels, W, H, vh, n_rows, seed):
    """a fresh handle's layer and one call over n_rows pictures against the host face -> (device images, host coverages)"""
    imgs = TC.images(n_rows, W, H, seed)
    imgs[0, 0, 0, :] = np.nan                                  # payloads pass through untouched pixels, and blend as NaN elsewhere
    host = [P.text_frame(font, labels, im, viewport_height=vh, coverage=True) for im in imgs[:3]]
    cov = host[0][1]
    b = P.TextBatch(font, labels, W, H, viewport_height=vh)
    for l in range(len(labels)):
        same(b.coverage(l), cov[l], (tag, "layer of label", l))
    same(b.coverage(), cov.max(0), (tag, "layer"))
    image = to_device(imgs)
    assert b.rows(n_rows, image) is image
    got = download(image)
    want = np.asarray([h[0] for h in host] + [P.text_frame(font, labels, im, viewport_height=vh) for im in imgs[3:]], f32)
    print(f"{tag}: {int((cov > 0).any(0).sum())} of {W * H} pixels covered, {int((bits(got) != bits(want)).sum())} channels differ")
    same(got, want, tag)
    return got, imgs, cov


@pytest.mark.parametrize("case", TC.HOST_CASES, ids=lambda c: "%s-%dx%d-vh%g" % c)
def test_bits_of_layer_and_image(dejavu, case):
    """the twelve labels (and the em of 200 pixels) at 64 x 64, 256 x 256 and 301 x 173; 3 streams x 2 frames of rows"""
    kind, W, H, vh = case
    got, imgs, cov = hold(str(case), dejavu, TC.case_labels(kind), W, H, vh, 6, 200 + W)
    covered = (cov > 0).any(0)
    assert covered.sum() > 30 and not covered.all()
    changed = (bits(got) != bits(imgs)).any(-1)
    assert not changed[:, ~covered].any()                                   # uncovered pixels keep their bits, the NaN payload included
    assert changed[:, covered].sum() > 0.8 * got.shape[0] * covered.sum()   # (a coverage near 1e-8 may leave a channel's bits alone)


def test_synthetic_known_answers(syn):
    """the known answers of tests/test_text.py, on the device: squares on and off pixel boundaries, the triangle, the hole, the
    overlap, the reversed and the degenerate contour, each in its own label of one picture"""
    W, H = 64, 32
    texts = ["s", "s", "t", "o", "d", "r", "h"]
    labels = [P.TextLabel(t, -28.0 + 9.0 * k + (0.25 if k == 1 else 0.0), 3.0 - (0.25 if k == 1 else 0.0), 64.0, 1.0, (0.1 * k, 1.0 - 0.1 * k, 0.5))
              for k, t in enumerate(texts)]
    got, imgs, cov = hold("synthetic", syn, labels, W, H, float(H), 2, 31)
    b = P.TextBatch(syn, labels, W, H, viewport_height=float(H))
    layer = [b.coverage(l) for l in range(len(labels))]
    x0 = [W / 2 + lab.x - (2.0 if t in "srh" else 3.0) for lab, t in zip(labels, texts)]     # the glyph origin's pixel column
    y1 = H / 2 - 3.0                                                                       # the baseline's pixel row
    same(layer[0], TC.rect_coverage(W, H, x0[0], y1 - 4, x0[0] + 4, y1), "square")
    same(layer[1], TC.rect_coverage(W, H, x0[1], y1 + 0.25 - 4, x0[1] + 4, y1 + 0.25), "shifted square")
    assert sorted(set(np.unique(layer[1]))) == [0.0, 0.0625, 0.1875, 0.25, 0.5625, 0.75, 1.0]
    tri = [(x0[2], y1), (x0[2] + 6, y1), (x0[2], y1 - 3)]
    want = np.asarray([[TC.clip_area(tri, i, j) for i in range(W)] for j in range(H)])
    assert np.abs(layer[2] - want).max() <= 2.0 ** -22 and abs(layer[2].sum() - 9.0) <= 1e-6
    want = TC.rect_coverage(W, H, x0[3], y1 - 6, x0[3] + 6, y1) - TC.rect_coverage(W, H, x0[3] + 2, y1 - 4, x0[3] + 4, y1 - 2)
    same(layer[3], want, "hole")
    want = np.maximum(TC.rect_coverage(W, H, x0[4], y1 - 4, x0[4] + 4, y1), TC.rect_coverage(W, H, x0[4] + 2, y1 - 6, x0[4] + 6, y1 - 2))
    same(layer[4], want, "overlap counts once")
    same(layer[5], TC.rect_coverage(W, H, x0[5], y1 - 4, x0[5] + 4, y1), "reversed contour")
    assert not layer[6].any()


def test_overlap_blends_in_label_order(syn):
    """two labels of different colours over the same pixels, and a third cut by the tile boundary at x = 16: swapping the first two
    changes the picture, and each order equals the host face's"""
    W, H = 40, 24
    a, b2, c = (P.TextLabel("o", 1.5, 2.5, 64.0, 1.0, (1.0, 0.1, 0.1)), P.TextLabel("d", 2.25, 0.5, 64.0, 1.0, (0.1, 0.2, 1.0)),
                P.TextLabel("s", -4.5, 1.25, 64.0, 1.0, (0.3, 0.9, 0.2)))
    first, imgs, cov = hold("a over b", syn, [a, b2, c], W, H, float(H), 2, 41)
    assert ((cov[0] > 0) & (cov[1] > 0) & (cov[0] < 1) & (cov[1] < 1)).sum() >= 4            # partial coverages of both meet
    second, _, _ = hold("b over a", syn, [b2, a, c], W, H, float(H), 2, 41)
    both = (cov[0] > 0) & (cov[1] > 0)
    assert (bits(first[:, both]) != bits(second[:, both])).any(-1).sum() >= both.sum()       # the order shows where both cover
    assert (bits(first[:, ~both]) == bits(second[:, ~both])).all()


def test_off_image_labels_make_the_call_a_no_op(syn):
    W, H = 33, 17
    labels = [P.TextLabel("s", 100.0, 0.0, 64.0, 1.0), P.TextLabel("o", 0.0, -50.0, 64.0, 1.0), P.TextLabel("h", 0.0, 0.0, 64.0, 1.0)]
    assert not any(d["on_image"] for d in P.text_layout(syn, labels, W, H, float(H)))
    b = P.TextBatch(syn, labels, W, H, viewport_height=float(H))
    imgs = TC.images(3, W, H, 51)
    imgs[1] = np.nan
    image = to_device(imgs)
    b.rows(3, image)
    same(download(image), imgs, "nothing on the image")
    assert not b.coverage().any() and not b.coverage(1).any()


@pytest.mark.parametrize("edge", ["left", "right", "top", "bottom", "corner"])
def test_untouched_memory_and_edges(syn, edge):
    """a glyph hanging off each image edge on a 21 x 13 picture between NaN-filled guard bands: uncovered pixels and the bands keep
    their bits"""
    import torch
    W, H, n_rows, guard = 21, 13, 3, 4096
    x, y = {"left": (-W / 2.0 - 0.25, 0.0), "right": (W / 2.0 + 0.25, 0.0), "top": (0.5, H / 2.0 - 1.5), "bottom": (0.5, -H / 2.0 - 2.25),
            "corner": (W / 2.0, -H / 2.0 - 2.0)}[edge]
    lab = P.TextLabel("s", x, y, 64.0, 1.0, (0.2, 0.5, 0.9))
    imgs = TC.images(n_rows, W, H, 61)
    flat = np.full(2 * guard + imgs.size, np.nan, f32)
    flat.view(np.uint32)[:guard] = 0x7FC0BEEF
    flat.view(np.uint32)[-guard:] = 0x7FC0CAFE
    flat[guard:-guard] = imgs.ravel()
    dev = to_device(flat)
    b = P.TextBatch(syn, [lab], W, H, viewport_height=float(H))
    b.rows(n_rows, dev[guard:guard + imgs.size])
    out = download(dev)
    assert (out.view(np.uint32)[:guard] == 0x7FC0BEEF).all() and (out.view(np.uint32)[-guard:] == 0x7FC0CAFE).all()
    got = out[guard:-guard].reshape(imgs.shape)
    x0, y1 = W / 2.0 + x - 2.0, H / 2.0 - y
    want_cov = TC.rect_coverage(W, H, x0, y1 - 4.0, x0 + 4.0, y1)
    same(b.coverage(0), want_cov, edge)
    same(got, np.asarray([P.text_frame(syn, [lab], im, viewport_height=float(H)) for im in imgs]), edge)
    assert np.array_equal((bits(got) != bits(imgs)).any(-1), np.broadcast_to(want_cov > 0, got.shape[:3]))


def test_arguments_on_the_device(syn):
    import torch
    W, H = 16, 16
    b = P.TextBatch(syn, [TC.unit_label("s")], W, H, viewport_height=float(H))
    image = torch.zeros(2 * W * H * 4 + 4, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError) as e:
        P.text._checked(b._L, b._L.pvq_text_batch_rows_device(b._h, 2, image.data_ptr() + 4, None))
    assert "aligned" in str(e.value)
    with pytest.raises(ValueError):
        b.rows(2, image)                                        # the wrong number of elements
    with pytest.raises(ValueError):
        P.text._checked(b._L, b._L.pvq_text_batch_rows_device(b._h, 2, None, None))
    assert b._L.pvq_text_batch_rows_device(b._h, 0, image.data_ptr(), None) == _lib.PVQ_OK      # no rows: nothing to do
    assert not download(image).any()
    with pytest.raises(ValueError):
        b.coverage(1)


def test_row_stride_past_the_blend_grid_cap(syn):
    """text_blend (gridDim.y 65 535) over 65 539 rows of an 8 x 8 picture with one label (67 MB): rows 0 .. 3 have a second trip, to
    rows 65 535 .. 65 538, which exist only if the kernel strides by the very cap the host clamps to.  Every row holds its own
    number, so a row blended twice or not at all shows."""
    import torch
    W = H = 8
    n_rows, cap = 65539, 65535
    lab = P.TextLabel("s", 0.25, -0.25, 64.0, 1.0, (0.9, 0.4, 0.1))
    b = P.TextBatch(syn, [lab], W, H, viewport_height=float(H))
    base = TC.images(1, W, H, 71)[0]
    image = to_device(base).repeat(n_rows, 1, 1, 1)
    image[..., 1] += torch.arange(n_rows, device="cuda", dtype=torch.float32)[:, None, None] / 65536.0
    before = {r: download(image[r]).copy() for r in (0, 1, cap - 1, cap, cap + 1, n_rows - 1)}
    assert image.numel() * 4 == n_rows * W * H * 16
    b.rows(n_rows, image)
    torch.cuda.synchronize()
    for r, bg in before.items():
        same(download(image[r]), P.text_frame(syn, [lab], bg, viewport_height=float(H)), ("row", r))
        assert not np.array_equal(download(image[r]), bg)
    # every row was blended exactly once: the covered pixels' alpha is a function of the coverage and the shared background alone
    cov = b.coverage(0)
    want_alpha = P.text_frame(syn, [lab], base, viewport_height=float(H))[..., 3]
    alpha = image[..., 3]
    assert bool((alpha == to_device(want_alpha)[None]).all())
    assert (cov > 0).sum() == 25


def test_repeat_call_blends_twice(dejavu):
    W, H, vh = 64, 64, 0.0
    labels = TC.pitch_labels()
    b = P.TextBatch(dejavu, labels, W, H, viewport_height=vh)
    imgs = TC.images(2, W, H, 81)
    image = to_device(imgs)
    b.rows(2, image)
    b.rows(2, image)
    want = np.asarray([P.text_frame(dejavu, labels, P.text_frame(dejavu, labels, im)) for im in imgs])
    same(download(image), want, "two calls on one handle and stream")


@pytest.mark.parametrize("H,text", [(64, "G♯"), (256, "B♭")])
def test_long_label_spans_lds_chunks(dejavu, H, text):
    """an em of 600 pixels on a picture 1024 wide.  64 high, most of the outline lies above and below the picture and its segments
    are dropped; 256 high, the label keeps more segments than one LDS chunk of 256, so text_coverage stages two"""
    W = 1024
    s = float(f32(TC.M.VIEWPORT_HEIGHT) / f32(H))
    labels = [P.TextLabel(text, 0.2, 0.3, 40.0, 600.0 * s / 40.0, (0.95, 0.54, 0.23))]
    lay = P.text_layout(dejavu, labels, W, H)[0]
    assert lay["n_tiles"] > 50 and (lay["n_segments"] > 256 if H == 256 else lay["n_segments"] < 256), lay
    got, imgs, cov = hold("long label", dejavu, labels, W, H, 0.0, 2, 91)
    assert (cov == 1.0).sum() > 1000 and ((cov > 0) & (cov < 1)).sum() > 100


def test_chain_balls_text_overlay(dejavu):
    """BackdropBatch.frames -> RasterBatch.frames_over -> TextBatch.rows -> OverlayBatch.frames on one small lit scene, 2 streams x 3
    frames: every row equals the host faces chained, text_frame then overlay_frame, over the device's own picture of the balls"""
    import overlay_cases as OC
    import scene_cases as SC
    import torch
    geom, ns, nf, W, H, mp, vh, h = (55.0, 7, 36), 2, 3, 96, 72, 16, 0.0, 4
    n = 252
    rng = P.VqtRange(*geom)
    streams = [[c[1:] for c in SC.plain_frames(n, nf, 900 + s, most=9, every_empty=5)] for s in range(ns)]
    a = {"center": np.full((ns, nf, mp), -7.0, f32), "size": np.full((ns, nf, mp), -7.0, f32), "peak_count": np.zeros((ns, nf), np.int32),
         "calmness": np.zeros((ns, nf, n), f32), "pitch_accuracy": np.zeros((ns, nf, n), f32), "pitch_deviation": np.zeros((ns, nf, n), f32),
         "scene_calmness": np.zeros((ns, nf), f32)}
    for s, frames in enumerate(streams):
        for f, (pk, calm, acc, dev, scene) in enumerate(frames):
            a["peak_count"][s, f] = len(pk)
            for p, (c, z) in enumerate(pk):
                a["center"][s, f, p], a["size"][s, f, p] = c, z
            a["calmness"][s, f], a["pitch_accuracy"][s, f], a["pitch_deviation"][s, f], a["scene_calmness"][s, f] = calm, acc, dev, scene
    d = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    d["x_vqt_smoothed"] = torch.from_numpy(np.random.default_rng(8).uniform(0.0, 30.0, (ns, nf, n)).astype(f32)).cuda()
    rendered = P.RenderBatch(rng).rows_device(d, outputs=("spectrogram_vqt", "chroma"))
    scene = P.SceneBatch(rng, ns).frames_device(d, frame_time=1.0 / 30.0)
    el = (2.0 + 0.0333 * np.arange(nf)).astype(f32)
    r = {k: download(v).reshape((ns, nf) + v.shape[1:]) for k, v in rendered.items()}
    back = P.BackdropBatch(rng, ns, W, H, viewport_height=vh).frames(nf, scene)
    P.RasterBatch(rng, ns, W, H, viewport_height=vh).frames_over(back, scene, d, elapsed=el)
    under = download(back).copy()
    labels = P.pitch_name_labels(geom[1])
    text = P.TextBatch(dejavu, labels, W, H, viewport_height=vh)
    assert text.rows(ns * nf, back) is back
    lettered = download(back).copy()
    ov = P.OverlayBatch(rng, ns, W, H, history_rows=h, viewport_height=vh, ui_scale=0.05)
    assert ov.frames(nf, back, rendered) is back
    img = download(back)
    for s in range(ns):
        with_text = np.asarray([P.text_frame(dejavu, labels, u, viewport_height=vh) for u in under[s]])
        same(lettered[s], with_text, ("text over the balls", s))
        host, _ = OC.host_chain(n, h, r["spectrogram_vqt"][s], r["chroma"][s], with_text, viewport_height=vh, ui_scale=0.05)
        same(img[s], host, ("chain", s))
    assert not np.array_equal(lettered, under) and not np.array_equal(img, lettered)
