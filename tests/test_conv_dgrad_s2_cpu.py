"""CPU tests of the stride-2 data gradient's host side: the class decomposition ml_conv2d_dgrad_s2_classes /
ops.conv2d_dgrad_s2_classes against a NumPy restatement of the parity rule, the refusals by name of the library and of the
op, and the refusals the stride-1 path and the layers keep."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_dgrad_s2_cases as S


def _packed(name):
    from masklab_hip import packing
    g, w, _ = S.inputs(name)
    return g, packing.pack_dense(w)


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_classes_are_the_parity_rule(name):
    from masklab_hip import ops
    g, p = _packed(name)
    got = ops.conv2d_dgrad_s2_classes(p, g["x_shape"], g["padding"], g["dilation"])
    want = S.parity_classes(g)
    assert got == want
    B, H, W, _ = g["x_shape"]
    assert sum(pixels for pixels, _ in got) == B * H * W
    assert S.live_pairs_of_classes(g, got) == S.live_pairs_of_forward(g)
    assert sum(len(taps) for _, taps in got) == g["k"] ** 2          # every tap lives in exactly one class
    for _, taps in got:
        assert taps == sorted(taps)                                   # ascending: the summation order


def test_the_shapes_of_the_decomposition():
    from masklab_hip import ops
    g, p = _packed("same_even")
    assert sorted(len(t) for _, t in ops.conv2d_dgrad_s2_classes(p, g["x_shape"])) == [1, 2, 2, 4]
    g, p = _packed("k1_even")
    assert sorted(len(t) for _, t in ops.conv2d_dgrad_s2_classes(p, g["x_shape"])) == [0, 0, 0, 1]
    g, p = _packed("dil2")
    assert sorted(len(t) for _, t in ops.conv2d_dgrad_s2_classes(p, g["x_shape"], "same", 2)) == [0, 0, 0, 9]
    # (H, W) alone is one image
    assert [n for n, _ in ops.conv2d_dgrad_s2_classes(p, (9, 9), "same", 2)] == [25, 20, 20, 16]


def _desc(**over):
    from masklab_hip import _lib
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Ho, d.Wo = 2, 8, 8, 4, 4
    d.span, d.span_pad, d.cpp_shift, d.in_cstride = 32, 32, 30, 32
    d.KH, d.KW, d.stride, d.dil, d.pad_t, d.pad_l = 3, 3, 2, 1, 0, 0
    d.cout, d.n_pad, d.out_cstride = 32, 32, 32
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over,message", [
    (dict(math=2), "half tensors are refused"),
    (dict(out_f16=1), "half tensors are refused"),
    (dict(group_cin_step=32), "grouped / depthwise problems are refused"),
    (dict(cpp_shift=2), "row-span"),
    (dict(shuffle2x2=1), "shuffle2x2"),
    (dict(stride=1), "stride 1: stride 2 only"),
    (dict(stride=3), "stride 3: stride 2 only"),
    (dict(span=30), "cin (30) must be a multiple of 4"),
    (dict(cout=30), "cout (30) must be a multiple of 4"),
    (dict(KH=7), "at most 5 x 5"),
    (dict(KW=6), "at most 5 x 5"),
    (dict(Ho=0), "does not fit the map"),
    (dict(Wo=6), "does not fit the map"),
])
def test_the_library_refuses_by_name(over, message):
    from masklab_hip import _lib
    lib = _lib.load()
    d = _desc(**over)
    pixels, ntaps, taps = (C.c_int64 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 400)()
    assert lib.ml_conv2d_dgrad_s2_classes(C.byref(d), pixels, ntaps, taps) == -1
    assert message in lib.ml_last_error().decode()
    # the launch entry makes the same checks before it touches a pointer or the device
    assert lib.ml_conv2d_dgrad_s2_f32(C.byref(d), None, None, None) == -1
    assert message in lib.ml_last_error().decode()


def test_the_launch_refuses_a_view_and_aliasing_by_name():
    from masklab_hip import _lib
    lib = _lib.load()
    buf = (C.c_float * 16)()
    base = (C.addressof(buf) + 15) & ~15
    d = _desc(out_cstride=64)
    d.out, d.wgt = base, base
    assert lib.ml_conv2d_dgrad_s2_f32(C.byref(d), C.c_void_p(1 << 20), None, None) == -1
    assert "not a view" in lib.ml_last_error().decode()
    d = _desc()
    d.out, d.wgt = 1 << 30, 1 << 28
    assert lib.ml_conv2d_dgrad_s2_f32(C.byref(d), C.c_void_p((1 << 30) + 64), None, None) == -1
    assert "dx may not overlap dy" in lib.ml_last_error().decode()
    assert lib.ml_conv2d_dgrad_s2_f32(C.byref(d), C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 16), None) == -1
    assert "dx may be add itself" in lib.ml_last_error().decode()
    assert lib.ml_conv2d_dgrad_s2_f32(C.byref(d), C.c_void_p((1 << 20) + 4), None, None) == -1
    assert "16-byte aligned" in lib.ml_last_error().decode()


class _Dc:                                              # what the op reads of a DeviceConv before any launch
    def __init__(self, p):
        self.p = p


def test_the_op_refuses_before_it_needs_a_device():
    from masklab_hip import ops, packing
    r = np.random.default_rng(4)
    dense = packing.pack_dense(r.normal(0, 1, (3, 3, 32, 32)).astype(np.float32))
    dy = torch.zeros((2, 4, 4, 32))
    with pytest.raises(TypeError, match="float32 only"):
        ops.conv2d_dgrad_s2(dy.half(), _Dc(dense), (8, 8))
    grouped = packing.pack_grouped(r.normal(0, 1, (3, 3, 64, 8)).astype(np.float32), 8)
    rowspan = packing.pack_rowspan(r.normal(0, 1, (7, 7, 3, 64)).astype(np.float32))
    shuffle = packing.pack_transpose2x2(r.normal(0, 1, (2, 2, 8, 32)).astype(np.float32))
    for p, message in ((grouped, "grouped / depthwise"), (rowspan, "row-span"), (shuffle, "shuffle2x2")):
        with pytest.raises(ValueError, match=message):
            ops.conv2d_dgrad_s2(dy, _Dc(p), (8, 8))
        with pytest.raises(ValueError, match=message):
            ops.conv2d_dgrad_s2_classes(p, (8, 8))
    with pytest.raises(ValueError, match=r"`dy` is \(2, 4, 4, 32\), expected \(2, 3, 3, 32\)"):
        ops.conv2d_dgrad_s2(dy, _Dc(dense), (8, 8), padding="valid")
    with pytest.raises(ValueError, match="does not fit the 2 x 2 input"):
        ops.conv2d_dgrad_s2(dy, _Dc(dense), (2, 2), padding="valid")
    odd = packing.pack_dense(r.normal(0, 1, (3, 3, 32, 30)).astype(np.float32))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.conv2d_dgrad_s2(torch.zeros((2, 4, 4, 30)), _Dc(odd), (8, 8))
    big = packing.pack_dense(r.normal(0, 1, (7, 7, 4, 4)).astype(np.float32))
    with pytest.raises(RuntimeError, match="at most 5 x 5"):
        ops.conv2d_dgrad_s2_classes(big, (16, 16))
    with pytest.raises(ValueError, match=r"`add` is .* expected \(2, 8, 8, 32\)"):
        ops.conv2d_dgrad_s2(dy, _Dc(dense), (8, 8), add=torch.zeros((2, 8, 8, 16)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv2d_dgrad_s2(dy, _Dc(dense), (8, 8))


def test_the_pinned_refusals_still_raise():
    """What the stride-1 path and the layers refused before the stride-2 kernel existed, they still refuse: the new kernel is
    reached only by its own names (ops.conv2d_dgrad_s2, Conv2D.backward(strided_dx=True))."""
    from masklab_hip import keras_like as K, ops, packing
    dense = packing.pack_dense(np.random.default_rng(4).normal(0, 1, (3, 3, 32, 32)).astype(np.float32))
    with pytest.raises(NotImplementedError, match="stride 2"):
        ops.conv2d_dgrad(torch.zeros((2, 4, 4, 32)), _Dc(dense), (8, 8), stride=2)
    with pytest.raises(NotImplementedError, match="GroupedConv2D.backward"):
        K.GroupedConv2D(64, 8, name="g_s2").backward(None, None, strided_dx=True)
    with pytest.raises(NotImplementedError, match="DepthwiseConv2D.backward"):
        K.DepthwiseConv2D(name="d_s2").backward(None, None)
    with pytest.raises(NotImplementedError, match="Conv2DTranspose.backward"):
        K.Conv2DTranspose(8, name="t_s2").backward(None, None)
    with pytest.raises(NotImplementedError, match="fold_bn"):
        K.Conv2D(8, (3, 3), strides=(2, 2), fold_bn=("bn", 1e-5, True), name="c_bn_s2").backward(None, None, strided_dx=True)
