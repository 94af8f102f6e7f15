"""The present stage on the device (pvq_present_batch_*) against the host face (pvq_present_frame) at the bars of
tests/present_cases.py: the bloomed linear picture within 1e-5 of the image's largest finite value with the same NaNs and
infinities, bytes at most one level apart and at most 1 % of them different.  Host and device share every operation of the linear
picture — the first pass's power is taken in double arithmetic without libm on both — so out_hdr is also held to its bits
against the host face, as is any row against the same row in another place, another cut or another call.  The bytes go through
each side's own expf and powf and are held to the bars.

Shapes are the crafted cases' (present_cases.py): images that are no multiple of the 16 x 16 tile or the 8 x 8 wave block, one texel,
more than one tile, mips one texel wide, 1 to 11 mips, a mip 0 of 16 384 x 4.  The picture's two passes stage their tiles' source
footprints in LDS where they fit and sample device memory where they do not: the first pass does not at 64 x 64 with a 4 x 4, 8 x 8
or 16 x 16 mip 0 and at 129 x 33 with a 16 x 4 one, the last pass does not at 33 x 17 with a 994 x 512 mip 0, at 40 x 24 with a
167 x 100 one and at 1 x 64 with a 64 x 4096 one (magnified pictures).  tests/test_present.py::test_every_kernel_form_has_a_case
holds the cases to that list."""
import numpy as np
import pytest

import present_cases as PC
import present_model as M
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


@pytest.mark.parametrize("mode", [0, 1])
def test_intensities_outside_0_to_1(mode):
    """8 rows at 17 x 9, d 16, intensities -0.5, -0.0, +inf, -inf, 2.5, 2.5, 1, 0.3, in both composite modes: a negative, a negative zero
    and an infinite intensity do not bloom (out_hdr is the image in bits); 2.5 does, with 1 - b and lf negative where the mode conserves
    energy.  Every row against the host face (out_hdr in bits) and the model (the bars); rows 4 and 5 are one picture and one result."""
    W, H, kw = 17, 9, dict(max_mip_dimension=16, composite_mode=mode)
    intensity = [-0.5, -0.0, float("inf"), float("-inf"), 2.5, 2.5, 1.0, 0.3]
    imgs = np.stack([PC.random_hdr(W, H, 120 + r) for r in range(8)])
    imgs[5] = imgs[4]
    assert np.signbit(f32(intensity[1]))
    out, hdr = present(P.PresentBatch(W, H, **kw), imgs, intensity)
    for r, v in enumerate(intensity):
        want_out, want_hdr = P.present_frame(imgs[r], v, hdr=True, **kw)
        PC.compare(f"mode {mode}, row {r} at {v} (device against host)", out[r], hdr[r], want_out, want_hdr, imgs[r])
        PC.compare(f"mode {mode}, row {r} at {v} (device against model)", out[r], hdr[r], *M.present(imgs[r], v, **kw), imgs[r])
        assert np.array_equal(bits(hdr[r]), bits(want_hdr)), r
        assert np.array_equal(bits(hdr[r]), bits(imgs[r])) == (r < 4), r
    same("rows 4 and 5", (out[4], hdr[4]), (out[5], hdr[5]))
    assert not np.array_equal(bits(hdr[4]), bits(hdr[6]))


@pytest.mark.parametrize("W,H,d,total", PC.STRIDE_SHAPES, ids=[f"{s[0]}x{s[1]}-d{s[2]}-{s[3]}rows" for s in PC.STRIDE_SHAPES])
def test_row_stride_past_the_grid_cap(W, H, d, total):
    """Every launch of a call (gridDim.y 65 535) over 3 x 65 535 + 3 rows of 5 x 4 and 2 x 65 535 + 3 rows of 24 x 10, in one piece: a
    workgroup makes 3 (2) trips through its row loop and those of rows 0 .. 2 one more.  All four launches are the staged forms at both
    shapes (test_present.py::test_every_kernel_form_has_a_case), so every trip after the first stages its footprint in the LDS array
    that the trip before sampled.  A wave without an inside lane is through with a row at once (`if (!inside) continue`), and where the
    footprint has more than 64 texels it stages part of the next row's: at 5 x 4 wave 1, in the mip 0 -> mip 1 pass and in the last pass
    (mip 0 is 10 x 8, both targets 5 x 4, wave 0's alone); at 24 x 10 waves 2 and 3 in the first pass (the whole picture under a tile of
    16 x 8) and waves 1 and 2 in the mip 0 -> mip 1 pass (19 x 8 under 9 x 4).  The last pass at 24 x 10 has two tiles, the second
    partial, and inside lanes in all four waves of the first.

    Row r is pattern r % 61 of present_cases.stride_rows, which a 61-row call pins against the host face (out_hdr in bits, bytes at
    the bars).  65 535 % 61 = 21: the workgroup of pattern p goes on to p + 21 and p + 42, every such pair a different picture with a
    different result, a quarter of them at most skipping bloom.

    What a wrong kernel would show.  A stride larger than the clamp, or a loop that makes one trip: rows 65 535 .. are the second and
    later trips' alone, and some of their words keep the fill value.  No leading barrier in stage_footprint: a wave that is through
    with row r (at once, where it has no inside lane) stages row r + 65 535's footprint while a slower wave still samples row r's; the
    asserted pairs say that the two pictures and their results differ and that bloom -> bloom, bloom -> skip, skip -> bloom and
    bloom -> skip -> bloom all occur, so the slow wave's texels would carry another picture's light and differ from the 61-row call's.
    That is a race: the test can catch it, not prove its absence.  A barrier that only some lanes of a workgroup reach: in present_up
    the inside and the outside lanes meet the same barriers only because none follows `if (!inside) continue`, whatever the order of
    blooming and skipping rows; wrong texels or a hang otherwise.

    Not run past the cap: the unstaged forms.  An unstaged first pass needs a picture of more than 1 936 texels and an unstaged last
    pass a mip 0 of that size, 2 to 6 GB for 65 538 rows; their row loops have no barrier and share grid_of with the staged ones.  Nor
    element offsets beyond 2^32."""
    import torch
    m, cap = PC.STRIDE_PATTERNS, 65535
    per_row = 16 * sum(w * h for w, h in P.present_mips(W, H, d))
    assert total > 2 * cap and per_row * total < 1 << 30                            # one piece: the strides are taken, not cut away
    imgs, intensity = PC.stride_rows(W, H, 7000)
    blooms = [bool(np.isfinite(v) and v > 0) for v in intensity]
    assert 4 * blooms.count(False) <= m and 0.0 < min(v for v, b in zip(intensity, blooms) if b) and max(intensity[blooms]) == 1.0
    kw = dict(max_mip_dimension=d)
    host = [P.present_frame(imgs[p], float(intensity[p]), hdr=True, **kw) for p in range(m)]
    host_out, host_hdr = np.stack([h[0] for h in host]), np.stack([h[1] for h in host])
    assert cap % m == 21
    orders = {(blooms[p], blooms[(p + 21) % m]) for p in range(m)}
    assert {(True, True), (True, False), (False, True)} <= orders, orders
    assert any(blooms[p] and not blooms[(p + 21) % m] and blooms[(p + 42) % m] for p in range(m))
    for p in range(m):
        assert (bits(host_hdr[p]) != bits(host_hdr[(p + 21) % m])).any(), p
        assert blooms[p] != np.array_equal(bits(host_hdr[p]), bits(imgs[p])), p
    assert not (bits(host_hdr) == GUARD).any() and not (host_out.view(np.uint32) == GUARD).any()

    small_img, small_int = to_device(imgs), to_device(intensity)
    small_hdr = torch.empty_like(small_img)
    small_out = P.PresentBatch(W, H, **kw).rows_device(small_img, small_int, hdr=small_hdr)
    got_out, got_hdr = download(small_out), download(small_hdr)
    differing = int((bits(got_hdr) != bits(host_hdr)).sum())
    print(f"{m} distinct rows of {W} x {H}: {differing} of {got_hdr.size} channels of out_hdr differ in a bit from the host face")
    assert differing == 0
    for p in range(m):
        PC.compare(f"pattern {p} at {intensity[p]}", got_out[p], got_hdr[p], host_out[p], host_hdr[p], imgs[p])
    assert not (bits(got_hdr) == GUARD).any() and not (got_out.view(np.uint32) == GUARD).any()

    idx = torch.arange(total, device="cuda") % m
    n = total * H * W                                                               # pixels: a word of bytes, four of out_hdr
    image, big_int = small_img[idx].contiguous(), small_int[idx].contiguous()
    gb = torch.full((n + 32,), GUARD, dtype=torch.int32, device="cuda")             # 16 guard words either side of both outputs
    gh = torch.full((4 * n + 32,), GUARD, dtype=torch.int32, device="cuda")
    out_t = gb[16:-16].view(torch.uint8).view(image.shape)
    hdr_t = gh[16:-16].view(torch.float32).view(image.shape)
    b = P.PresentBatch(W, H, **kw)
    b.rows_device(image, big_int, out=out_t, hdr=hdr_t)
    torch.cuda.synchronize()
    want_b, want_h = small_out.view(torch.int32).view(m, -1), small_hdr.view(torch.int32).view(m, -1)
    big_b, big_h = gb[16:-16].view(total, -1), gh[16:-16].view(total, -1)
    differing = int((big_b != want_b[idx]).sum()), int((big_h != want_h[idx]).sum())
    unwritten = int((big_b[cap:] == GUARD).sum()), int((big_h[cap:] == GUARD).sum())    # of the second and later trips' rows
    written_on = int((image.view(torch.int32).view(total, -1) != small_img.view(torch.int32).view(m, -1)[idx]).sum())
    guards = all(bool((g[:16] == GUARD).all()) and bool((g[-16:] == GUARD).all()) for g in (gb, gh))
    print(f"{total} rows of {W} x {H} over {cap} grid rows: differing 32-bit words against the {m}-row call: {differing[0]} of bytes, "
          f"{differing[1]} of out_hdr; words of rows {cap} .. that are still the fill value: {unwritten[0]} and {unwritten[1]}; "
          f"words of the image written on: {written_on}; guards intact: {guards}")
    assert differing == (0, 0) and unwritten == (0, 0) and written_on == 0 and guards

    del b                                                                           # its workspace with it
    again = P.PresentBatch(W, H, **kw)
    again.set_workspace_limit(100000 * per_row)                                     # two pieces: the first strides, the second starts at row 100 000
    hdr2 = torch.empty_like(image)
    out2 = again.rows_device(image, big_int, hdr=hdr2)
    torch.cuda.synchronize()
    differing = int((out2.view(torch.int32).view(total, -1) != big_b).sum()), int((hdr2.view(torch.int32).view(total, -1) != big_h).sum())
    print(f"in pieces of 100000 and {total - 100000} rows: {differing[0]} words of bytes and {differing[1]} of out_hdr differ from the call in one piece")
    assert differing == (0, 0)


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
