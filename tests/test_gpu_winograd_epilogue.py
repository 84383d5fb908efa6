"""GPU tests of the Winograd kernel's epilogue (conv_wino.hip): the MFMA takes the weights as its first operand, so a lane
owns ONE tile and four consecutive channels of each 16-wide half, runs the output transform on the four at once and stores
16 bytes per output pixel and half; a quad that reaches past cout is stored channel by channel.  The 16-byte store is
dword-aligned, so a channel stride of 75 or an offset of 3 takes the same path as a dense 128-wide tensor.

Every destination is a flat buffer pre-filled with a sentinel, with spare floats before, after and between the pixels'
channels; the conv is written into it through `out_view`, and every float outside the written region must still hold the
sentinel.  Values are held to fp64 oracle.tfops.conv2d within the Winograd tests' 2e-5 abs on O(1) data (weights scaled
1 / sqrt(9 cin)); the kernel name is asserted.  Shapes: one or two 64-tile blocks, 4 or 8 chunks of 8 channels; odd sizes,
tiles past the end, every cout class whose last quad or second half is cut."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import tfops as T
from sentinel_dest import SENT, Dest

RNG = np.random.default_rng(181)
ATOL = 2e-5
ACT = {None: lambda v: v, "relu": T.relu, "sigmoid": T.sigmoid}


def rnd(*shape, scale=1.0):
    return (RNG.normal(size=shape) * scale).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from masklab_hip import _lib, ops
    _lib.check(_lib.load().ml_device_check(), "ml_device_check")
    ops.set_conv_math("f32")


def _weights(cin, cout):
    return rnd(3, 3, cin, cout, scale=1.0 / np.sqrt(9 * cin)), rnd(cout)


def _dc(w, b):
    from masklab_hip import ops, packing
    return ops.DeviceConv(packing.pack_dense(w, b), "cuda")


def _names(fn):
    from masklab_hip import ops
    ops.PROFILE = []
    try:
        r = fn()
        torch.cuda.synchronize()
        return r, [rec["kernel"] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _wino(x, dc, dest, act=None, **kw):
    from masklab_hip import _lib, ops
    _, names = _names(lambda: ops.conv2d(x, dc, act=_lib.ACT_BY_NAME[act], out_view=dest.view, **kw))
    assert names == ["conv_wino_f32"], names
    return dest.read()


def _check(got, x, w, b, act=None):
    ref = ACT[act](T.conv2d(x.astype(np.float64), w, b))
    print(f"\nepilogue {x.shape} -> {w.shape[3]}: max abs vs fp64 {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


def test_odd_height_and_width_and_tiles_past_the_end():
    """2 x 5 x 7 -> 128: 12 tiles per image, 40 tiles of the block past the end; the last tile row and column have one
    pixel row / column only (the y1 / x1 guards of the vector store)."""
    x = rnd(2, 5, 7, 32)
    w, b = _weights(32, 128)
    got = _wino(dev(x), _dc(w, b), Dest((2, 5, 7), 128, 132, head=4), act="relu")
    _check(got, x, w, b, "relu")


def test_cout_75_at_a_channel_stride_of_75_behind_a_row_offset():
    """The class tower's destination: channel stride 75 and a start 3 rows in, so a pixel's quads are dword-aligned only.
    Two channel blocks, the second with a dead half; its quad 72..75 has three live channels, stored one by one."""
    x = rnd(2, 6, 6, 32)
    w, b = _weights(32, 75)
    got = _wino(dev(x), _dc(w, b), Dest((2, 6, 6), 75, 75, head=3 * 75, tail=2 * 75), act="sigmoid")
    _check(got, x, w, b, "sigmoid")


def test_cout_60_aligned_with_a_partly_dead_half():
    """One channel block; the second half holds channels 32..59: its quads 60.. are past cout and store nothing."""
    x = rnd(2, 6, 6, 32)
    w, b = _weights(32, 60)
    _check(_wino(dev(x), _dc(w, b), Dest((2, 6, 6), 60, 64, head=8)), x, w, b)


def test_cout_20_dead_second_half_and_a_quad_past_cout():
    """One block, waves 4-7 dead; of the first half, quads 0..16 are stored whole and quad 20..23 not at all."""
    x = rnd(2, 6, 6, 32)
    w, b = _weights(32, 20)
    _check(_wino(dev(x), _dc(w, b), Dest((2, 6, 6), 20, 24, head=4)), x, w, b)


def test_channel_offsets_4_and_3_in_a_stride_of_132_give_the_same_values():
    """cout 128 into channels [4, 132) of a 132-wide buffer (16-byte aligned, not dense), then into [3, 131) (dword-aligned):
    the same bits, and the fp64 reference."""
    x = rnd(2, 6, 6, 32)
    w, b = _weights(32, 128)
    dc, xd = _dc(w, b), dev(x)
    at4 = _wino(xd, dc, Dest((2, 6, 6), 128, 132, coff=4), act="relu")
    at3 = _wino(xd, dc, Dest((2, 6, 6), 128, 132, coff=3), act="relu")
    assert np.array_equal(at4, at3)
    _check(at4, x, w, b, "relu")


def test_two_problems_in_one_launch():
    """1 x 16 x 16 (one block) and 2 x 8 x 8 (32 tiles of its block): the problem boundary inside the grid."""
    from masklab_hip import _lib, ops
    xs = [rnd(1, 16, 16, 64), rnd(2, 8, 8, 64)]
    ws = [_weights(64, 128) for _ in xs]
    dests = [Dest(x.shape[:3], 128, 132, head=4) for x in xs]
    probs = [dict(x=dev(x), dc=_dc(w, b), act=_lib.ACT_RELU, out_view=d.view) for x, (w, b), d in zip(xs, ws, dests)]
    _, names = _names(lambda: ops.conv2d_multi(probs))
    assert names == ["conv_wino_f32"], names
    for x, (w, b), d in zip(xs, ws, dests):
        _check(d.read(), x, w, b, "relu")


def test_gn_partials_sum_the_kernels_own_output_and_fill_every_slot():
    """2 x 16 x 16, 64 -> 128: one block per image and 64-channel half, two 128-pixel flattened tiles each; a lane sums 2
    halves x 4 channels x 4 pixels of its tile in fp64.  The launch-size rule of gn_partials is met by a filler problem.
    Every slot starts as NaN."""
    from masklab_hip import _lib, ops
    B, hw, cin = 2, 16, 64
    x = rnd(B, hw, hw, cin)
    w, b = _weights(cin, 128)
    side = 16 * int(np.ceil(np.sqrt(128.0 * ops._gn_min_launch_tiles()) / 16))
    filler = dict(x=dev(rnd(1, side, side, 32)), dc=_dc(*_weights(32, 128)), act=_lib.ACT_RELU)
    tiles = B * hw * hw // 128
    part = torch.full((tiles, 4, 2), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((B, hw, hw, 128), SENT, device="cuda")
    _, names = _names(lambda: ops.conv2d_multi([dict(x=dev(x), dc=_dc(w, b), act=_lib.ACT_RELU, out=out, gn_partials=part), filler]))
    assert names == ["conv_wino_f32"], names
    y, pt = host(out), host(part)
    assert np.isfinite(pt).all()
    yd = y.astype(np.float64).reshape(tiles, 128, 4, 32)      # [128-pixel tile][pixel][32-channel group][channel]
    np.testing.assert_allclose(pt[..., 0], yd.sum(axis=(1, 3)), rtol=1e-9)
    np.testing.assert_allclose(pt[..., 1], (yd * yd).sum(axis=(1, 3)), rtol=1e-9)
    _check(y, x, w, b, "relu")


def test_live_batch_of_8_slots_with_5_live():
    """8 slots of 14 x 14 (49 tiles each), 5 live: live slots equal the launch without `live` bit for bit; a block with no
    live slot stores nothing.  Block 3 (tiles 192..255) holds the end of live slot 4 and the first 11 tiles of slot 5, which
    it computes like any other; every other tile of slots 5..7 keeps the sentinel."""
    from masklab_hip import _lib, ops
    cap, nlive = 8, 5
    x = rnd(cap, 14, 14, 32)
    w, b = _weights(32, 128)
    dc, xd = _dc(w, b), dev(x)
    full = _wino(xd, dc, Dest((cap, 14, 14), 128, 132, head=4), act="relu")
    dest = Dest((cap, 14, 14), 128, 132, head=4)
    live = torch.tensor([nlive], dtype=torch.int32, device="cuda")
    _, names = _names(lambda: ops.conv2d_multi([dict(x=xd, dc=dc, act=_lib.ACT_RELU, out_view=dest.view, live=(live, cap))]))
    assert names == ["conv_wino_f32"], names
    got = dest.read()
    last_live_block = (nlive * 49 - 1) // 64
    for i in range(cap):
        if i < nlive:
            assert np.array_equal(got[i], full[i]), i
            continue
        for t in range(49):
            ty, tx = divmod(t, 7)
            tile = got[i, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]
            if (i * 49 + t) // 64 <= last_live_block:
                assert np.array_equal(tile, full[i, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]), (i, t)
            else:
                assert (tile == SENT).all(), (i, t)
    _check(got[:nlive], x[:nlive], w, b, "relu")


def test_five_launches_give_the_same_bits_and_an_image_does_not_depend_on_its_batch():
    """5 x 6 x 10 (15 tiles per image: image 2 shares its block with the four others), cout 75 at stride 75: launched five
    times, then image 2 alone."""
    x = rnd(5, 6, 10, 32)
    w, b = _weights(32, 75)
    dc, xd = _dc(w, b), dev(x)
    runs = [_wino(xd, dc, Dest((5, 6, 10), 75, 75, head=75), act="sigmoid") for _ in range(5)]
    assert all(np.array_equal(runs[0], r) for r in runs[1:])
    alone = _wino(dev(x[2:3]), dc, Dest((1, 6, 10), 75, 75, head=75), act="sigmoid")
    assert np.array_equal(alone[0], runs[0][2])
    _check(runs[0], x, w, b, "sigmoid")
