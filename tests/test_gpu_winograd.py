"""GPU tests of the Winograd F(2x2,3x3) conv kernel (conv_wino.hip, ml_conv2d_desc.tile = 6) against an fp64 conv and the
direct kernel.  Tolerance: the dense-conv tests' 2e-5 abs (test_gpu_ops.py) on O(1) data."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import tfops as T

RNG = np.random.default_rng(29)


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


def _packed(cin, cout, tile=0):
    from masklab_hip import packing
    w, b = rnd(3, 3, cin, cout, scale=1.0 / np.sqrt(9 * cin)), rnd(cout)
    return w, b, packing.pack_dense(w, b, tile=tile)


def _logged(fn):
    """Run fn with the profiler hook on -> (result, kernel names of the launches)."""
    from masklab_hip import ops
    ops.PROFILE = []
    try:
        r = fn()
        torch.cuda.synchronize()
        return r, [rec["kernel"] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None


@pytest.mark.parametrize("cin,hw,act,bias", [
    (128, (33, 35), "relu", True), (160, (16, 16), "relu", True), (128, (13, 17), None, True),
    (128, (14, 14), "relu", False), (128, (1, 1), None, True), (160, (8, 9), None, False),
])
def test_winograd_against_fp64_and_the_direct_kernel(cin, hw, act, bias):
    from masklab_hip import _lib, ops
    B = 2
    x = rnd(B, hw[0], hw[1], cin)
    w, b, p = _packed(cin, 128)
    if not bias:
        p.bias, b = None, np.zeros(128, np.float32)
    ref = T.conv2d(x.astype(np.float64), w, b)
    ref = T.relu(ref) if act else ref
    a = _lib.ACT_BY_NAME[act]
    got, names = _logged(lambda: host(ops.conv2d(dev(x), ops.DeviceConv(p, "cuda"), act=a)))
    assert names == ["conv_wino_f32"]
    err = np.abs(got - ref)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5)
    p.tile = 1                                                 # the direct 128 x 128 kernel on the same weights
    direct, names = _logged(lambda: host(ops.conv2d(dev(x), ops.DeviceConv(p, "cuda"), act=a)))
    assert names[0].startswith("conv_mfma")
    derr = np.abs(direct - ref)
    np.testing.assert_allclose(got, direct, rtol=0, atol=2e-5)
    print(f"\nwinograd cin={cin} {hw}: max abs {err.max():.3e}, max rel {(err / (np.abs(ref) + 1e-3)).max():.3e}; "
          f"direct: max abs {derr.max():.3e}, max rel {(derr / (np.abs(ref) + 1e-3)).max():.3e}")


def test_winograd_five_level_launch_and_slice_destination():
    """128^2 .. 8^2 in one launch; the first level writes into channels [32, 160) of a 192-channel buffer whose other
    channels keep their canary."""
    from masklab_hip import _lib, ops
    B = 1
    levels = [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)]
    xs = [rnd(B, h, w_, 128) for h, w_ in levels]
    ps = [_packed(128, 128) for _ in levels]
    canvas = torch.full((B, 128, 128, 192), 7.25, device="cuda")
    probs = [dict(x=dev(x), dc=ops.DeviceConv(p, "cuda"), act=_lib.ACT_RELU) for x, (_, _, p) in zip(xs, ps)]
    probs[0]["out"], probs[0]["out_coff"] = canvas, 32
    outs, names = _logged(lambda: ops.conv2d_multi(probs))
    assert names == ["conv_wino_f32"]
    for k, (x, (w, b, _), o) in enumerate(zip(xs, ps, outs)):
        ref = T.relu(T.conv2d(x.astype(np.float64), w, b))
        got = host(o)[..., 32:160] if k == 0 else host(o)
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5, err_msg=str(levels[k]))
    c = host(canvas)
    assert (c[..., :32] == 7.25).all() and (c[..., 160:] == 7.25).all()


def test_winograd_out_view_writes_only_its_rows():
    from masklab_hip import ops
    B, h, w_, nc = 2, 10, 6, 128
    x = rnd(B, h, w_, 128)
    w, b, p = _packed(128, nc)
    total = h * w_ + 7
    pred = torch.full((B, total + 3, nc), -3.5, device="cuda")
    ops.conv2d(dev(x), ops.DeviceConv(p, "cuda"), out_view=(pred, 3 * nc, nc, (total + 3) * nc))
    got = host(pred)
    np.testing.assert_allclose(got[:, 3:3 + h * w_], T.conv2d(x.astype(np.float64), w, b).reshape(B, -1, nc), atol=2e-5)
    assert (got[:, :3] == -3.5).all() and (got[:, 3 + h * w_:] == -3.5).all()


@pytest.mark.parametrize("hw", [(128, 128), (64, 64), (32, 32), (256, 256)])
def test_winograd_gn_partials_equal_a_statistics_pass(hw):
    from masklab_hip import _lib, ops
    B = max(2, -(-600 * 128 // (hw[0] * hw[1])))               # a launch above ml_conv2d_gn_min_launch_tiles()
    groups = min(32, hw[0] * hw[1] // 128)                 # whole 128-pixel tiles per chunk
    x = rnd(B, hw[0], hw[1], 128)
    _, _, p = _packed(128, 128)
    M = B * hw[0] * hw[1]
    part = torch.full((M // 128, 4, 2), float("nan"), dtype=torch.float64, device="cuda")
    y = ops.conv2d(dev(x), ops.DeviceConv(p, "cuda"), act=_lib.ACT_RELU, gn_partials=part)
    yd = host(y).astype(np.float64).reshape(B, groups, -1)    # chunk = contiguous HWC / groups floats
    pt = host(part)
    assert np.isfinite(pt).all()                               # every slot written
    per_chunk = pt.reshape(B, groups, -1, 2).sum(axis=2)
    np.testing.assert_allclose(per_chunk[..., 0], yd.sum(-1), rtol=1e-9)
    np.testing.assert_allclose(per_chunk[..., 1], (yd * yd).sum(-1), rtol=1e-9)


def test_winograd_image_in_batch_equals_image_alone_and_repeats_bit_identically():
    from masklab_hip import _lib, ops
    x = rnd(4, 24, 40, 128)
    _, _, p = _packed(128, 128)
    dc = ops.DeviceConv(p, "cuda")
    xb = dev(x)
    runs = [ops.conv2d(xb, dc, act=_lib.ACT_RELU) for _ in range(5)]
    torch.cuda.synchronize()
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    alone = ops.conv2d(dev(x[2:3]), dc, act=_lib.ACT_RELU)
    assert torch.equal(alone[0], runs[0][2])


def test_winograd_is_not_taken_outside_its_rule():
    """f32x3 math, a strided conv and a 'valid' conv stay on the direct kernel."""
    from masklab_hip import ops
    x = dev(rnd(1, 16, 16, 128))
    _, _, p = _packed(128, 128)
    dc = ops.DeviceConv(p, "cuda")
    _, names = _logged(lambda: (ops.conv2d(x, dc, stride=2), ops.conv2d(x, dc, padding="valid")))
    assert not any(n.startswith("conv_wino") for n in names)
    ops.set_conv_math("f32x3")
    try:
        _, names = _logged(lambda: ops.conv2d(x, dc))
    finally:
        ops.set_conv_math("f32")
    assert not any(n.startswith("conv_wino") for n in names)
