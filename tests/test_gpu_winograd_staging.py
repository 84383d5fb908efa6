"""GPU tests of the Winograd kernel's staging (conv_wino.hip: LDS-DMA ring of 4-channel chunks, 64 tiles x 64 channels per
block, the patch resource rebased per block): channel counts, levels where one block spans several images, partial tiles,
fixed-capacity batches, an input above 4 GiB.  Each case is checked against fp64 and the direct kernel within the dense
conv tests' 2e-5 abs on O(1) data."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import tfops as T

RNG = np.random.default_rng(31)


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


@pytest.mark.parametrize("cin,B,hw", [
    (32, 2, (16, 16)),        # the fewest chunks the rule allows (8 of 4 channels)
    (160, 2, (33, 35)),       # odd Ho / Wo: partial last tile row and column
    (96, 3, (20, 18)),
    (128, 8, (8, 8)),         # 16 tiles per image: one block spans 4 images
    (128, 20, (4, 4)),        # 4 tiles per image: one block spans 16 images
    (128, 5, (13, 17)),       # partial tiles and blocks that straddle images
    (160, 2, (1, 1)),
])
def test_staging_against_fp64_and_the_direct_kernel(cin, B, hw):
    from masklab_hip import _lib, ops
    x = rnd(B, hw[0], hw[1], cin)
    w, b, p = _packed(cin)
    ref = T.relu(T.conv2d(x.astype(np.float64), w, b))
    got, names = _names(lambda: host(ops.conv2d(dev(x), ops.DeviceConv(p, "cuda"), act=_lib.ACT_RELU)))
    assert names == ["conv_wino_f32"]
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5)
    p.tile = 1
    direct, names = _names(lambda: host(ops.conv2d(dev(x), ops.DeviceConv(p, "cuda"), act=_lib.ACT_RELU)))
    assert names[0].startswith("conv_mfma")
    np.testing.assert_allclose(got, direct, rtol=0, atol=2e-5)


@pytest.mark.parametrize("hw", [(8, 8), (4, 4), (13, 17)])
def test_image_in_a_shared_block_equals_image_alone(hw):
    """Where one 64-tile block holds several images, an image's bits do not depend on its neighbours or position."""
    from masklab_hip import _lib, ops
    x = rnd(11, hw[0], hw[1], 128)
    _, _, p = _packed(128)
    dc = ops.DeviceConv(p, "cuda")
    xb = dev(x)
    runs = [ops.conv2d(xb, dc, act=_lib.ACT_RELU) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    for i in (0, 5, 10):
        alone = ops.conv2d(dev(x[i:i + 1]), dc, act=_lib.ACT_RELU)
        assert torch.equal(alone[0], runs[0][i]), i


def test_live_batch_leaves_dead_slots_untouched():
    """16 x 16 images = one 64-tile block each: with 2 of every 4 slots live, the dead slots keep their canary and the live
    ones equal the same conv without `live`, bit for bit."""
    from masklab_hip import _lib, ops
    B, period = 12, 4
    x = rnd(B, 16, 16, 128)
    w, b, p = _packed(128)
    dc = ops.DeviceConv(p, "cuda")
    full = host(ops.conv2d(dev(x), dc, act=_lib.ACT_RELU))
    out = torch.full((B, 16, 16, 128), -9.5, device="cuda")
    live = torch.tensor([2], dtype=torch.int32, device="cuda")
    _, names = _names(lambda: ops.conv2d_multi([dict(x=dev(x), dc=dc, act=_lib.ACT_RELU, out=out, live=(live, period))]))
    assert names == ["conv_wino_f32"]
    got = host(out)
    for i in range(B):
        if i % period < 2:
            assert np.array_equal(got[i], full[i]), i
        else:
            assert (got[i] == -9.5).all(), i
    np.testing.assert_allclose(got[0], T.relu(T.conv2d(x[:1].astype(np.float64), w, b))[0], rtol=0, atol=2e-5)


def test_input_above_4gib_on_sampled_images():
    """A channel slice of an input tensor of 4.6 GB: the per-block rebased buffer resource reaches images far past 4 GiB.
    Sampled images are checked against fp64 and against the same image in a launch of its own."""
    from masklab_hip import _lib, ops
    B, H, W, C = 1100, 64, 64, 256
    if torch.cuda.get_device_properties(0).total_memory < 16 * 2 ** 30:
        pytest.skip("needs 16 GiB of device memory")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    x = torch.randn((B, H, W, C), generator=g, device="cuda", dtype=torch.float32)
    assert x.numel() * 4 > 4 * 2 ** 30
    w, b, p = _packed(128)
    dc = ops.DeviceConv(p, "cuda")
    y, names = _names(lambda: ops.conv2d(x, dc, act=_lib.ACT_RELU, in_coff=128))
    assert names == ["conv_wino_f32"]
    for i in (0, 700, B - 1):                  # byte offsets 0, 2.9 GB, 4.6 GB
        xi = x[i:i + 1, :, :, 128:].contiguous()
        ref = T.relu(T.conv2d(host(xi).astype(np.float64), w, b))
        np.testing.assert_allclose(host(y[i:i + 1]), ref, rtol=0, atol=2e-5, err_msg=str(i))
        alone = ops.conv2d(xi, dc, act=_lib.ACT_RELU)
        assert torch.equal(alone[0], y[i]), i
    del x, y
    torch.cuda.empty_cache()
