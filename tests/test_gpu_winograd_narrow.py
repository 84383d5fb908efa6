"""GPU tests of narrow convs (cout <= 96 in their automatic 32 / 64 / 96-row packing, and 97..127) on the Winograd kernel
(conv_wino.hip): the launch covers ceil(cout / 64) blocks of 64 channels, and a 32-channel half of a block that lies wholly
past cout stages its share of the patches, keeps every wait and barrier of the K loop and issues no LDS read, no transform,
no MFMA and no store.  The classes: cout <= 32 (one block, dead half), 33..64 (one block), 65..96 (two blocks, the second
with a dead half), 97..127 (two blocks; packed 128 wide, so the eligibility rule itself takes them).  Every case is checked
against fp64 oracle.tfops.conv2d and against the direct kernel (tile = 1 packing of the same weights) within the dense conv
tests' 2e-5 abs on O(1) data (weights scaled 1 / sqrt(9 cin)).  Shapes: a few hundred tiles at most; 4, 12 and 20 chunks of 8
channels (short loops, both parities of the iteration count of a ring with one barrier per two K steps); blocks shared by
two images and tiles past the end."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O
from oracle import tfops as T

RNG = np.random.default_rng(97)
ATOL = 2e-5
CANARY = -7.25
COUTS = [3, 32, 33, 60, 64, 65, 75, 96, 97, 127]
ACT = {None: lambda v: v, "relu": T.relu, "sigmoid": T.sigmoid}


def routed(cout):
    """The couts the narrow predicate (ml_conv2d_wino_narrow) and the eligibility rule send to the Winograd kernel: every
    class was faster there than on the direct kernel (profiles/r14_wino_narrow.md); cout = 32 and 64 alone stay on the
    direct kernel, beside the `live` launches of these widths (tests/test_gpu_live_slots.py holds those to the bits and K
    slices of the launch without `live`)."""
    return cout not in (32, 64)


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


def _dc(w, b, tile=0):
    from masklab_hip import ops, packing
    return ops.DeviceConv(packing.pack_dense(w, b, tile=tile), "cuda")


def _names(fn):
    from masklab_hip import ops
    ops.PROFILE = []
    try:
        r = fn()
        torch.cuda.synchronize()
        return r, [rec["kernel"] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _assert_kernel(names, cout):
    if routed(cout):
        assert names == ["conv_wino_f32"], (cout, names)
    else:
        assert len(names) == 1 and names[0].startswith("conv_mfma"), (cout, names)


def _direct(x, w, b, act):
    """The same conv on the direct 128 x 128 kernel (tile code 1)."""
    from masklab_hip import _lib, ops
    got, names = _names(lambda: ops.conv2d(x, _dc(w, b, tile=1), act=_lib.ACT_BY_NAME[act]))
    assert names[0].startswith("conv_mfma"), names
    return host(got)


@pytest.mark.parametrize("cout", COUTS)
def test_channel_classes_into_a_wider_buffer(cout):
    """Automatic packing, B = 2, 5 x 7 (12 tiles per image: one block holds both images and 40 tiles past the end) and
    13 x 17 (63 tiles per image: the first block holds image 0 and one tile of image 1, the second ends 2 tiles early),
    4 / 12 / 20 chunks, no activation / relu / sigmoid.  The destination is NaN where the conv must write and a canary in
    its four spare channels: a channel < cout that is never stored shows, and so does a store past cout."""
    from masklab_hip import _lib, ops
    worst = 0.0
    for hw in ((5, 7), (13, 17)):
        for cin in (32, 96, 160):
            x = rnd(2, hw[0], hw[1], cin)
            xd = dev(x)
            w, b = _weights(cin, cout)
            dc = _dc(w, b)
            lin = T.conv2d(x.astype(np.float64), w, b)
            for act in (None, "relu", "sigmoid"):
                out = torch.full((2, hw[0], hw[1], cout + 4), float("nan"), device="cuda")
                out[..., cout:] = CANARY
                _, names = _names(lambda: ops.conv2d(xd, dc, act=_lib.ACT_BY_NAME[act], out=out))
                _assert_kernel(names, cout)
                got = host(out)
                assert (got[..., cout:] == CANARY).all(), (hw, cin, act)
                ref = ACT[act](lin)
                direct = _direct(xd, w, b, act)
                worst = max(worst, float(np.abs(got[..., :cout] - ref).max()))
                np.testing.assert_allclose(got[..., :cout], ref, rtol=0, atol=ATOL, err_msg=str((hw, cin, act)))
                np.testing.assert_allclose(got[..., :cout], direct, rtol=0, atol=ATOL, err_msg=str((hw, cin, act)))
    print(f"\nnarrow cout={cout}: max abs vs fp64 {worst:.3e}")


@pytest.mark.parametrize("cout,d", [(3, 3), (60, 4), (75, 5), (96, 4)])
def test_out_view_rows_before_and_after_keep_their_canary(cout, d):
    """The destination as BoxRegressionSubNet.call builds it: image b's level at pred[b, 3 : 3 + H W priors], a row pitch of
    cout floats.  Rows before and after keep a canary; the level's rows start as NaN."""
    from masklab_hip import ops
    B, h, w_, cin = 2, 10, 6, 96
    npri = cout // d
    x = rnd(B, h, w_, cin)
    w, b = _weights(cin, cout)
    rows = h * w_ * npri
    pred = torch.full((B, rows + 3 * npri + 7, d), CANARY, device="cuda")
    pred[:, 3 * npri:3 * npri + rows] = float("nan")
    _, names = _names(lambda: ops.conv2d(dev(x), _dc(w, b), out_view=(pred, 3 * npri * d, cout, pred.shape[1] * d)))
    _assert_kernel(names, cout)
    got = host(pred)
    ref = T.conv2d(x.astype(np.float64), w, b).reshape(B, -1, d)
    np.testing.assert_allclose(got[:, 3 * npri:3 * npri + rows], ref, rtol=0, atol=ATOL)
    assert (got[:, :3 * npri] == CANARY).all() and (got[:, 3 * npri + rows:] == CANARY).all()


@pytest.mark.parametrize("cout,d,act", [(75, 5, "sigmoid"), (60, 4, None)])
def test_five_level_launch_into_one_prediction(cout, d, act):
    """The towers' output launch: five levels 16^2 .. 1^2 of one image, distinct weights per level, each written into its
    rows of one [B, A, d] prediction."""
    from masklab_hip import _lib, ops
    B, cin, npri = 1, 128, cout // d
    levels = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    xs = [rnd(B, h, w_, cin) for h, w_ in levels]
    ws = [_weights(cin, cout) for _ in levels]
    total = sum(h * w_ for h, w_ in levels) * npri
    pred = torch.full((B, total, d), float("nan"), device="cuda")
    problems, off = [], 0
    for x, (w, b), (h, w_) in zip(xs, ws, levels):
        problems.append(dict(x=dev(x), dc=_dc(w, b), act=_lib.ACT_BY_NAME[act], out_view=(pred, off * d, npri * d, total * d)))
        off += h * w_ * npri
    _, names = _names(lambda: ops.conv2d_multi(problems))
    _assert_kernel(names, cout)
    got, off = host(pred), 0
    for x, (w, b), (h, w_) in zip(xs, ws, levels):
        ref = ACT[act](T.conv2d(x.astype(np.float64), w, b)).reshape(B, -1, d)
        np.testing.assert_allclose(got[:, off:off + h * w_ * npri], ref, rtol=0, atol=ATOL, err_msg=str((h, w_)))
        off += h * w_ * npri


@pytest.mark.parametrize("cout", [20, 60, 75])
def test_after_a_full_width_launch_on_large_values(cout):
    """A cout = 128 launch on values of 1e4 immediately before the narrow launch on the same stream: whatever it left in
    the LDS rings and in registers is neither read nor published by the dead half (or by anything else)."""
    from masklab_hip import ops
    cin = 64
    big = dev(rnd(3, 8, 8, cin) * 1e4)
    wb, bb = _weights(cin, 128)
    dcb = _dc(wb * 1e2, bb)
    x = rnd(3, 8, 8, cin)
    w, b = _weights(cin, cout)
    dc, xd = _dc(w, b), dev(x)
    out = torch.full((3, 8, 8, cout + 4), float("nan"), device="cuda")
    out[..., cout:] = CANARY

    def both():
        ops.conv2d(big, dcb)
        ops.conv2d(xd, dc, out=out)
    _, names = _names(both)
    assert names[0] == "conv_wino_f32"
    _assert_kernel(names[1:], cout)
    got = host(out)
    assert (got[..., cout:] == CANARY).all()
    np.testing.assert_allclose(got[..., :cout], T.conv2d(x.astype(np.float64), w, b), rtol=0, atol=ATOL)


@pytest.mark.parametrize("cout", [75, 60])
def test_repeats_are_bit_identical_and_an_image_does_not_depend_on_its_batch(cout):
    """6 x 10 = 15 tiles per image: in a batch of 5, image 2 shares its block with four others."""
    from masklab_hip import _lib, ops
    x = rnd(5, 6, 10, 64)
    w, b = _weights(64, cout)
    dc, xb = _dc(w, b), dev(x)
    runs, names = _names(lambda: [ops.conv2d(xb, dc, act=_lib.ACT_SIGMOID) for _ in range(5)])
    _assert_kernel(names[:1], cout)
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    alone = ops.conv2d(dev(x[2:3]), dc, act=_lib.ACT_SIGMOID)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], runs[0][2])
    np.testing.assert_allclose(host(runs[0]), T.sigmoid(T.conv2d(x.astype(np.float64), w, b)), rtol=0, atol=ATOL)


# ------------------------------------------------------------------ the layers
LAYER_TOL = {"f32": 1e-4, "f32x3": 1e-4, "f16s": 3e-2}     # test_gpu_layers.py TOL; test_gpu_f16_heads.py F16_MODEL_TOL


@pytest.mark.parametrize("math", ["f32", "f32x3", "f16s"])
def test_tower_layers_end_on_the_winograd_kernel_under_f32_only(math):
    """ClassificationSubNet (15 priors x 5 classes = 75, sigmoid) and BoxRegressionSubNet (15 x 4 = 60) on two levels of
    8 x 8 and 4 x 4: under "f32" the last launch of each is the Winograd kernel, under "f32x3" and "f16s" (which read
    the direct-path weights) it is not.  Outputs against the oracle at the layer tests' tolerance of the mode."""
    from masklab_hip import keras_like as K
    from masklab_hip import ops
    from masklab_hip.layers import BoxRegressionSubNet, ClassificationSubNet
    K.clear_session()
    shapes = [(None, 8, 8, 128), (None, 4, 4, 128)]
    half = math == "f16s"
    xs = [rnd(2, *s[1:]) for s in shapes]
    if half:
        xs = [x.astype(np.float16) for x in xs]
    ops.set_conv_math(math)
    try:
        for layer, oracle in ((ClassificationSubNet(2, 5, num_depth=1, num_features=128, num_priors=15, groups=16),
                               lambda f, w: O.classification_subnet(f, w, 5, 1, 16)),
                              (BoxRegressionSubNet(2, num_depth=1, num_features=128, num_priors=15, groups=16),
                               lambda f, w: O.box_regression_subnet(f, w, 1, 16))):
            layer.build(shapes)
            w = K.init_weights(layer.weight_specs(), 11)
            layer.load_weights(w, torch.device("cuda:0"))
            got, names = _names(lambda: host(layer([dev(x) for x in xs])))
            assert (names[-1] == "conv_wino_f32") == (math == "f32"), (math, names)
            want = oracle([x.astype(np.float64) for x in xs], w)
            assert got.shape == want.shape and got.dtype == np.float32
            err = float(np.abs(got - want).max())
            print(f"\n{type(layer).__name__} [{math}]: last launch {names[-1]}, max abs {err:.3e}")
            assert err <= LAYER_TOL[math], (math, type(layer).__name__, err)
    finally:
        ops.set_conv_math("f32")
