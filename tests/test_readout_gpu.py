"""The readout stage on the device (pvq_readout_batch_*) against the host face (pvq_readout_frame, itself held to the NumPy model
bit for bit by tests/test_readout.py).  The bar: no differing bit, in any atlas cell and in any pixel channel — the device formats
the value in integer arithmetic, folds the pen in the host's order and adds the host face's chord areas in the host face's order.

Both fonts come from outline arrays (tests/readout_cases.py).  Shapes are chosen for where the kernels can go wrong: sides that
are no multiple of the 16 x 16 tile, a box cut by the left edge, a box edge on a pixel centre, strings of 17 to 25 slots in one
call, more rows than the draw grid's cap."""

import numpy as np
import pytest

import pitchvis_amd as P
import readout_cases as K
import readout_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def host_frames(case):
    name, W, H, scale = case
    return np.asarray([K.host_frame(name, W, H, scale, index) for index in range(len(K.VALUES))], f32)


@pytest.mark.parametrize("name,scale", [("synthetic", 4.0), ("curved", 0.0), ("curved", 0.5), ("curved", 1.3), ("curved", 6.0)])
def test_atlas_equals_the_host_faces(name, scale):
    """every cell of the device's atlas, both fonts; at ui_scale 6 an em is 96 pixels: cells of several tiles, glyphs of more chords"""
    font = K.lib_font(name)
    device, host = P.ReadoutBatch(font, 64, 64, scale), P.ReadoutBatch(font, 64, 64, scale, device=None)
    pixels = 0
    for ch in M.CODEPOINTS:
        got, want = device.atlas(ch), host.atlas(ch)
        assert got[:3] == want[:3] and got[3].shape == want[3].shape, ch
        K.same(got[3], want[3], (name, scale, ch))
        pixels += int((got[3] > 0).sum())
    assert pixels > 23


@pytest.mark.parametrize("case", K.GPU_CASES, ids=lambda c: "%s-%dx%d-%g" % c)
def test_one_call_over_the_value_list(case):
    """a row a value of the list: every channel of every row equals the host face's picture of that value; outside the row's box
    and covered cell pixels the bits are kept, the NaN's payload included"""
    name, W, H, scale = case
    base, want = K.background(W, H), host_frames(case)
    batch = P.ReadoutBatch(K.lib_font(name), W, H, scale)
    image = to_device(np.broadcast_to(base, want.shape))
    values = to_device(np.asarray(K.VALUES, f32))
    assert batch.rows(values, image) is image
    got = download(image)
    print(f"{case}: {int((K.bits(got) != K.bits(want)).sum())} channels differ")
    atlas = K.model_atlas(name, scale)
    for index, value in enumerate(K.VALUES):
        K.compare(got[index], want[index], M.frame(atlas, value, base)[1], base, (case, value))


def test_streams_by_frames_equal_flat_rows():
    """rows as [3 streams][7 frames] with a values tensor of that shape, as AnalysisBatch leaves tuning_grid_inaccuracy, against
    the same 21 rows fed flat"""
    name, W, H, scale = "curved", 301, 173, 0.0
    base = K.background(W, H)
    batch = P.ReadoutBatch(K.lib_font(name), W, H, scale)
    vals = np.asarray(K.VALUES[:21], f32)
    flat = download(batch.rows(to_device(vals), to_device(np.broadcast_to(base, (21, H, W, 4)))))
    shaped = download(batch.rows(to_device(vals.reshape(3, 7)), to_device(np.broadcast_to(base, (3, 7, H, W, 4)))))
    K.same(shaped.reshape(flat.shape), flat, "3 x 7 against flat")
    K.same(flat, host_frames((name, W, H, scale))[:21], "flat against the host face")


def test_more_rows_than_the_grid_cap():
    """24 x 8 at ui_scale 0.25 and 65 535 + 38 rows: the draw kernel's stride loop over rows takes some rows twice round; the
    values cycle through the list, and every row is compared with the host picture of its value"""
    name, W, H, scale = "curved", 24, 8, 0.25
    n_rows = 65535 + 38
    base = np.random.default_rng(24).uniform(0.0, 1.0, (H, W, 4)).astype(f32)   # finite: at this size the box reaches every corner
    want = np.asarray([P.readout_frame(K.lib_font(name), value, base, scale) for value in K.VALUES], f32)
    index = np.arange(n_rows) % len(K.VALUES)
    batch = P.ReadoutBatch(K.lib_font(name), W, H, scale)
    image = to_device(np.broadcast_to(base, (n_rows, H, W, 4)))
    batch.rows(to_device(np.asarray(K.VALUES, f32)[index]), image)
    got = download(image)
    diff = (K.bits(got) != K.bits(want[index])).reshape(n_rows, -1).any(1)
    assert not diff.any(), (int(diff.sum()), np.flatnonzero(diff)[:8].tolist())
    assert (K.bits(want) != K.bits(base)).reshape(len(K.VALUES), -1).any(1).all()   # every value draws something at this size


def test_two_calls_on_a_stream_give_the_bits_of_one():
    """the stage is stateless after create: two calls of one handle on a non-default stream, each over fresh pictures, both give what
    one call gives"""
    import torch
    case = ("synthetic", 64, 64, 4.0)
    name, W, H, scale = case
    want = host_frames(case)
    batch = P.ReadoutBatch(K.lib_font(name), W, H, scale)
    values = to_device(np.asarray(K.VALUES, f32))
    first, second = (to_device(np.broadcast_to(K.background(W, H), want.shape)) for _ in range(2))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    batch.rows(values, first, stream=stream)
    batch.rows(values, second, stream=stream)
    stream.synchronize()
    K.same(download(first), want, "first call")
    K.same(download(second), want, "second call")
