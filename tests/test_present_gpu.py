"""The present stage on the device (pvq_present_batch_*) against the host face (pvq_present_frame) at the bars of
tests/present_cases.py: the bloomed linear picture within 1e-5 of the image's largest finite value with the same NaNs and
infinities, bytes at most one level apart and at most 1 % of them different.  Host and device share every operation of the linear
picture — the first pass's power is taken in double arithmetic without libm on both — so out_hdr is also held to its bits
against the host face, as is any row against the same row in another place, another cut or another call.  The bytes go through
each side's own expf and powf and are held to the bars.

Shapes are the crafted cases' (present_cases.py): images that are no multiple of the 16 x 16 tile or the 8 x 8 wave block, one texel,
more than one tile, mips one texel wide, 1 to 8 mips.  The picture's two passes stage their tiles' source footprints in LDS where
they fit and sample device memory where they do not: the first pass does not at 64 x 64 with a 4 x 4 or 8 x 8 mip 0 and at 129 x 33
with a 16 x 4 one, the last pass does not at 33 x 17 with a 994 x 512 mip 0 (a magnified picture)."""
import numpy as np
import pytest

import present_cases as PC
import pitchvis_amd as P
from test_present import bits

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 0x5A5A5A5A
SEVEN = (0.3, 0.0, 1.0, float("nan"), 0.0, 0.01, 1.0)


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def present(b, imgs, intensity, **kw):
    """one device call -> (bytes, hdr) as host arrays"""
    import torch
    image = to_device(imgs)
    hdr = torch.empty_like(image)
    out = b.rows_device(image, None if intensity is None else to_device(np.asarray(intensity, f32)), hdr=hdr, **kw)
    assert np.array_equal(bits(download(image)), bits(imgs))                    # the image is never written
    return download(out), download(hdr)


def seven_rows(W=33, H=17, seed=70):
    return np.stack([PC.specials(W, H, seed) if r == 2 else PC.random_hdr(W, H, seed + r) for r in range(7)])


def same(tag, got, want):
    """no differing bit, in bytes or in the linear picture"""
    for g, w, what in ((got[0], want[0], "bytes"), (bits(got[1]), bits(want[1]), "hdr")):
        diff = g != w
        assert not diff.any(), (tag, what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("name", PC.IDS)
def test_cases_match_host(name):
    _, img, intensity, kw = PC.CASES[PC.IDS.index(name)]
    H, W = img.shape[:2]
    want_out, want_hdr = P.present_frame(img, intensity, hdr=True, **kw)
    out, hdr = present(P.PresentBatch(W, H, **kw), img[None], [intensity])
    PC.compare(name + " (device against host)", out[0], hdr[0], want_out, want_hdr, img)
    PC.compare(name + " (device against model)", out[0], hdr[0], *PC.model(name), img)
    differing = int((bits(hdr[0]) != bits(want_hdr)).sum())
    print(f"{name}: {differing} of {hdr[0].size} channels of out_hdr differ in a bit from the host face")
    assert differing == 0
    assert np.array_equal(bits(hdr[0][..., 3]), bits(img[..., 3]))
    if not (np.isfinite(intensity) and intensity > 0):
        assert np.array_equal(bits(hdr[0]), bits(img))


def test_seven_rows_each_as_alone():
    """intensities (0.3, 0, 1, NaN, 0, 0.01, 1): the rows at 0 and NaN skip bloom; every row is bit-identical to itself alone"""
    W, H, kw = 33, 17, dict(max_mip_dimension=16)
    imgs = seven_rows(W, H)
    b = P.PresentBatch(W, H, **kw)
    out, hdr = present(b, imgs, SEVEN)
    for r, intensity in enumerate(SEVEN):
        same(("row", r), (out[r], hdr[r]), [a[0] for a in present(b, imgs[r:r + 1], [intensity])])
        want = P.present_frame(imgs[r], intensity, hdr=True, **kw)
        PC.compare(f"row {r} at {intensity}", out[r], hdr[r], *want, imgs[r])
        blooms = np.isfinite(intensity) and intensity > 0
        assert np.array_equal(bits(hdr[r]), bits(imgs[r])) != blooms, r
    assert not np.array_equal(out[2], out[6])


@pytest.mark.parametrize("pieces", [(3, 3, 1), (1,) * 7])
def test_workspace_pieces(pieces):
    W, H, kw = 33, 17, dict(max_mip_dimension=16)
    imgs = seven_rows(W, H, 80)
    per_row = 16 * sum(w * h for w, h in P.present_mips(W, H, 16))
    whole = present(P.PresentBatch(W, H, **kw), imgs, SEVEN)
    b = P.PresentBatch(W, H, **kw)
    b.set_workspace_limit(pieces[0] * per_row + (per_row // 2 if pieces[0] > 1 else -per_row + 1))   # 3.5 rows' worth, or one byte
    same(pieces, present(b, imgs, SEVEN), whole)
    same((pieces, "again, the workspace grown"), present(b, imgs, SEVEN), whole)


def test_row_position_independence():
    W, H, kw = 40, 24, dict(max_mip_dimension=64, composite_mode=0)
    imgs = np.stack([PC.random_hdr(W, H, 90 + r) for r in range(6)])
    imgs[5] = imgs[0]
    intensity = [0.7, 0.2, 0.0, 1.0, 0.5, 0.7]
    out, hdr = present(P.PresentBatch(W, H, **kw), imgs, intensity)
    same("rows 0 and 5", (out[0], hdr[0]), (out[5], hdr[5]))
    assert not np.array_equal(out[0], out[1])


def test_guards_side_stream_hdr_in_place_and_no_intensity():
    """64 bytes of guard either side of both outputs, a side stream; then d_hdr == d_image; then d_intensity NULL"""
    import torch
    W, H, kw = 129, 33, dict(max_mip_dimension=64)
    imgs = seven_rows(W, H, 100)
    b = P.PresentBatch(W, H, **kw)
    want_out, want_hdr = present(b, imgs, SEVEN)
    n = imgs.size
    gb = torch.full((n // 4 + 32,), GUARD, dtype=torch.int32, device="cuda")      # bytes: n of them, 16 guard words either side
    gh = torch.full((n + 32,), GUARD, dtype=torch.int32, device="cuda")
    out_t = gb[16:-16].view(torch.uint8).view(imgs.shape)
    hdr_t = gh[16:-16].view(torch.float32).view(imgs.shape)
    image, intensity = to_device(imgs), to_device(np.asarray(SEVEN, f32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert b.rows_device(image, intensity, out=out_t, hdr=hdr_t, stream=side) is out_t
    side.synchronize()
    for g in (gb, gh):
        edge = g.cpu().numpy().view(np.uint32)
        assert np.all(edge[:16] == GUARD) and np.all(edge[-16:] == GUARD)
    same("side stream, guarded", (download(out_t), download(hdr_t)), (want_out, want_hdr))
    out = b.rows_device(image, intensity, hdr=image)                              # the linear picture over the image
    same("hdr in place", (download(out), download(image)), (want_out, want_hdr))
    plain_out, plain_hdr = present(b, imgs, None)                                  # no intensities: no row blooms
    assert np.array_equal(bits(plain_hdr), bits(imgs))
    same("no intensity", (plain_out, plain_hdr), present(b, imgs, np.zeros(7, f32)))
    for r in (0, 2):
        PC.compare(f"no intensity, row {r}", plain_out[r], plain_hdr[r], *P.present_frame(imgs[r], 0.0, hdr=True, **kw), imgs[r])


def test_chain():
    """SceneBatch -> BackdropBatch.frames -> RasterBatch.frames_over -> PresentBatch.rows_device, fed with the scene's bloom buffer where
    it lies, on 2 streams x 3 frames at 64 x 64: every row against the host face on the same picture and intensity"""
    import scene_cases as SC
    import torch
    geom, ns, nf, W, H, mp, vh = (55.0, 7, 36), 2, 3, 64, 64, 16, 20.0
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
    scene = P.SceneBatch(rng, ns).frames_device(d, frame_time=1.0 / 30.0)
    el = (2.0 + 0.0333 * np.arange(nf)).astype(f32)
    back = P.BackdropBatch(rng, ns, W, H, viewport_height=vh).frames(nf, scene)
    P.RasterBatch(rng, ns, W, H, viewport_height=vh).frames_over(back, scene, d, elapsed=el)
    hdr = torch.empty_like(back)
    out = P.PresentBatch(W, H).rows_device(back, scene["bloom"], hdr=hdr)
    assert tuple(out.shape) == (ns, nf, H, W, 4)
    picture, bloom, out, hdr = download(back), download(scene["bloom"]), download(out), download(hdr)
    assert bloom.shape == (ns, nf) and (bloom > 0).any()
    for s in range(ns):
        for f in range(nf):
            want = P.present_frame(picture[s, f], float(bloom[s, f]), hdr=True)
            PC.compare(f"chain, stream {s} frame {f}, intensity {bloom[s, f]:.3f}", out[s, f], hdr[s, f], *want, picture[s, f])
    assert len(np.unique(out[..., :3])) > 16
