"""GPU tests of the Winograd kernel's 8-channel patch chunks (conv_wino.hip: a patch ring of 3 slots of 8 channels = two K
steps, a weight ring of 4 slots of one K step, one barrier per chunk, the gn exchange laid over the ring's head).  The
shapes are the smallest at which each path of the loop can go wrong: 4 chunks (the prologue stages half of them), 8 and 20
(neither a multiple of the 3 patch slots), fewer than 64 tiles, every border tap out of range, blocks shared by images, a
channel slice as input, two problems in one launch, a fixed-capacity batch.  Every case is checked against fp64
oracle.tfops.conv2d and against the direct kernel chosen by an explicit tile code, within the dense conv tests' 2e-5 abs on
O(1) data."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import tfops as T

RNG = np.random.default_rng(83)
ATOL = 2e-5


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


def _packed(cin, cout=128, tile=0):
    from masklab_hip import packing
    w, b = rnd(3, 3, cin, cout, scale=1.0 / np.sqrt(9 * cin)), rnd(cout)
    return w, b, packing.pack_dense(w, b, tile=tile)


def _names(fn):
    from masklab_hip import ops
    ops.PROFILE = []
    try:
        r = fn()
        torch.cuda.synchronize()
        return r, [rec["kernel"] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _wino(x, dc, **kw):
    """The conv on the Winograd kernel through ops.conv2d; the launch log must say so."""
    from masklab_hip import _lib, ops
    got, names = _names(lambda: ops.conv2d(x, dc, act=_lib.ACT_RELU, **kw))
    assert names == ["conv_wino_f32"], names
    return host(got)


def _direct(x, w, b, **kw):
    """The same conv on the direct 128 x 128 kernel (tile code 1)."""
    from masklab_hip import _lib, ops, packing
    dc = ops.DeviceConv(packing.pack_dense(w, b, tile=1), "cuda")
    got, names = _names(lambda: ops.conv2d(x, dc, act=_lib.ACT_RELU, **kw))
    assert names[0].startswith("conv_mfma"), names
    return host(got)


def _check(got, x, w, b, direct):
    ref = T.relu(T.conv2d(x.astype(np.float64), w, b))
    err, derr = np.abs(got - ref).max(), np.abs(got - direct).max()
    print(f"\nchunk8 {x.shape} -> {w.shape[3]}: max abs vs fp64 {err:.3e}, vs the direct kernel {derr:.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(got, direct, rtol=0, atol=ATOL)


@pytest.mark.parametrize("cin", [32, 64, 160])
def test_chunk_counts_on_an_odd_image_smaller_than_a_block(cin):
    """1 x 5 x 7: 12 tiles of a 64-tile block, every border tap out of range; 4, 8 and 20 chunks of 8 channels."""
    from masklab_hip import ops
    x = rnd(1, 5, 7, cin)
    w, b, p = _packed(cin)
    _check(_wino(dev(x), ops.DeviceConv(p, "cuda")), x, w, b, _direct(dev(x), w, b))


def test_cout_36_through_the_c_entry_point():
    """36 output channels in a 128-wide packing: ops.conv2d packs such a conv 64 wide and keeps it on the direct kernel, so
    the launch is made on the C entry point with tile = 6.  Channels 36.. of the second 32-channel group are not stored."""
    from masklab_hip import _lib, ops
    cin, cout = 64, 36
    x = rnd(1, 5, 7, cin)
    w, b, p = _packed(cin, cout, tile=1)
    assert p.n_pad == 128
    dc = ops.DeviceConv(p, "cuda")
    xd = dev(x)
    out = torch.full((1, 5, 7, cout + 4), -2.5, device="cuda")
    d, _, _ = ops._conv_desc(xd, dc, act=_lib.ACT_RELU, out=out)
    d.tile, d.wgt = 6, dc.wgt_wino.data_ptr()
    lib = _lib.load()
    assert lib.ml_conv2d_wino_eligible(C.byref(d))
    ws = ops.workspace(int(lib.ml_conv2d_workspace_bytes()), xd.device, "conv")
    _lib.check(lib.ml_conv2d_multi_f32((_lib.ConvDesc * 1)(d), 1, ops._ptr(ws), ws.numel(), ops._stream()), "ml_conv2d_multi_f32")
    got = host(out)
    assert (got[..., cout:] == -2.5).all()
    _check(got[..., :cout], x, w, b, _direct(xd, w, b))


def test_blocks_shared_by_several_images():
    """3 x 8 x 8: 16 tiles per image, one block holds all three and 16 tiles past the end."""
    from masklab_hip import ops
    x = rnd(3, 8, 8, 64)
    w, b, p = _packed(64)
    _check(_wino(dev(x), ops.DeviceConv(p, "cuda")), x, w, b, _direct(dev(x), w, b))


def test_image_alone_equals_image_in_batch():
    """6 x 10 = 15 tiles per image: in a batch of 5 image 2 straddles nothing it owns alone; its bits do not change."""
    from masklab_hip import ops
    x = rnd(5, 6, 10, 64)
    w, b, p = _packed(64)
    dc = ops.DeviceConv(p, "cuda")
    batch = _wino(dev(x), dc)
    alone = _wino(dev(x[2:3]), dc)
    assert np.array_equal(alone[0], batch[2])
    _check(batch, x, w, b, _direct(dev(x), w, b))
    _check(alone, x[2:3], w, b, _direct(dev(x[2:3]), w, b))


def test_gn_partials_sum_the_kernels_own_output():
    """2 x 16 x 16 x 128: one block per image and 64-channel half, two 128-pixel tiles each.  The launch-size rule of
    gn_partials (ml_conv2d_gn_min_launch_tiles) is met by a second, plain problem in the same launch.  The sums are laid
    over the head of the LDS ring the K loop has just left."""
    from masklab_hip import _lib, ops
    B, hw, cin = 2, 16, 64
    x = rnd(B, hw, hw, cin)
    w, b, p = _packed(cin)
    dc = ops.DeviceConv(p, "cuda")
    side = 16 * int(np.ceil(np.sqrt(128.0 * ops._gn_min_launch_tiles()) / 16))
    filler = dict(x=dev(rnd(1, side, side, 32)), dc=ops.DeviceConv(_packed(32)[2], "cuda"), act=_lib.ACT_RELU)
    tiles = B * hw * hw // 128
    part = torch.full((tiles, 4, 2), float("nan"), dtype=torch.float64, device="cuda")
    outs, names = _names(lambda: ops.conv2d_multi([dict(x=dev(x), dc=dc, act=_lib.ACT_RELU, gn_partials=part), filler]))
    assert names == ["conv_wino_f32"], names
    y, pt = host(outs[0]), host(part)
    assert np.isfinite(pt).all()
    yd = y.astype(np.float64).reshape(tiles, 128, 4, 32)      # [128-pixel tile][pixel][32-channel group][channel]
    np.testing.assert_allclose(pt[..., 0], yd.sum(axis=(1, 3)), rtol=1e-9)
    np.testing.assert_allclose(pt[..., 1], (yd * yd).sum(axis=(1, 3)), rtol=1e-9)
    _check(y, x, w, b, _direct(dev(x), w, b))


def test_channel_slice_input():
    """Channels [32, 96) of a 96-channel tensor, as the decoder reads its concat buffer."""
    from masklab_hip import ops
    x = rnd(2, 5, 7, 96)
    w, b, p = _packed(64)
    xs = np.ascontiguousarray(x[..., 32:])
    got = _wino(dev(x), ops.DeviceConv(p, "cuda"), in_coff=32)
    _check(got, xs, w, b, _direct(dev(x), w, b, in_coff=32))


def test_two_problems_in_one_launch():
    from masklab_hip import _lib, ops
    xs = [rnd(1, 16, 16, 64), rnd(2, 8, 8, 64)]
    ps = [_packed(64) for _ in xs]
    probs = [dict(x=dev(x), dc=ops.DeviceConv(p, "cuda"), act=_lib.ACT_RELU) for x, (_, _, p) in zip(xs, ps)]
    outs, names = _names(lambda: ops.conv2d_multi(probs))
    assert names == ["conv_wino_f32"], names
    for x, (w, b, _), o in zip(xs, ps, outs):
        _check(host(o), x, w, b, _direct(dev(x), w, b))


def test_live_batch_of_capacity_6():
    """14 x 14 = 49 tiles per slot, capacity 6, 2 live: 64-tile blocks straddle slots.  Live slots equal the conv without
    `live` bit for bit; a block with no live slot stores nothing, so dead slots keep their canary -- except the tiles of
    slot 2 that share block 1 (tiles 64..127) with live slot 1, which that block computes like any other."""
    from masklab_hip import _lib, ops
    cap = 6
    x = rnd(cap, 14, 14, 64)
    w, b, p = _packed(64)
    dc = ops.DeviceConv(p, "cuda")
    full = _wino(dev(x), dc)
    out = torch.full((cap, 14, 14, 128), -9.5, device="cuda")
    live = torch.tensor([2], dtype=torch.int32, device="cuda")
    _, names = _names(lambda: ops.conv2d_multi([dict(x=dev(x), dc=dc, act=_lib.ACT_RELU, out=out, live=(live, cap))]))
    assert names == ["conv_wino_f32"], names
    got = host(out)
    for i in range(cap):
        if i < 2:
            assert np.array_equal(got[i], full[i]), i
            continue
        for t in range(49):
            ty, tx = divmod(t, 7)
            tile = got[i, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]
            if (i * 49 + t) // 64 == 1:             # in the block that also holds the end of live slot 1
                assert np.array_equal(tile, full[i, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]), (i, t)
            else:
                assert (tile == -9.5).all(), (i, t)
    _check(got[:2], x[:2], w, b, _direct(dev(x[:2]), w, b))
