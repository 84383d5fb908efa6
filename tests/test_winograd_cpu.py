"""CPU tests of the Winograd F(2x2,3x3) path (ml_conv2d_desc.tile = 6): the fp64 weight transform and its packed layout,
a NumPy emulation of the kernel's tile decomposition against a direct fp64 conv, and the library's eligibility rule."""
import ctypes as C
import os

import numpy as np
import pytest

from masklab_hip import packing

RNG = np.random.default_rng(23)


def _direct(x, g):
    """Direct 'same' 3x3 stride-1 correlation in fp64: x [H, W, Cin], g [3, 3, Cin, Cout] -> [H, W, Cout]."""
    H, W, _ = x.shape
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    out = np.zeros((H, W, g.shape[3]))
    for dy in range(3):
        for dx in range(3):
            out += xp[dy:dy + H, dx:dx + W] @ g[dy, dx]
    return out


def _wino(x, g):
    """The kernel's decomposition: 2x2 output tiles over 4x4 patches (zeros outside the image), V = B^T d B, U = G g G^T,
    M = sum_c U .* V per position, Y = A^T M A; outputs past the image edge dropped."""
    H, W, cin = x.shape
    TH, TW = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((2 * TH + 2, 2 * TW + 2, cin))
    xp[1:H + 1, 1:W + 1] = x
    U = packing.winograd_transform(np.transpose(g, (3, 2, 0, 1)))             # [cout][cin][4][4]
    out = np.zeros((2 * TH, 2 * TW, g.shape[3]))
    BT, AT = packing.WINO_BT, packing.WINO_AT
    for ty in range(TH):
        for tx in range(TW):
            d = np.transpose(xp[2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4], (2, 0, 1))   # [cin][4][4]
            V = np.einsum("ai,cij,bj->cab", BT, d, BT)
            M = np.einsum("ocab,cab->oab", U, V)
            out[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = np.transpose(np.einsum("ia,oab,jb->oij", AT, M, AT), (1, 2, 0))
    return out[:H, :W]


def test_weight_transform_matches_numpy_restatement():
    g = RNG.normal(size=(5, 7, 3, 3))
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
    ref = np.stack([np.stack([G @ g[i, j] @ G.T for j in range(7)]) for i in range(5)])
    np.testing.assert_allclose(packing.winograd_transform(g), ref, rtol=1e-15, atol=1e-15)


def test_packed_winograd_layout():
    cin, cout = 64, 96
    w = RNG.normal(size=(3, 3, cin, cout)).astype(np.float32)
    p = packing.pack_dense(w, None, tile=0)
    p.n_pad = 128
    p.wgt = np.pad(p.wgt, ((0, 128 - p.wgt.shape[0]), (0, 0)))
    u = packing.pack_winograd(p)
    assert u.dtype == np.float32 and u.shape == (4, cin // 8, 8, 32, 16)
    U = packing.winograd_transform(np.transpose(w.astype(np.float64), (3, 2, 0, 1)))   # [cout][cin][4][4], fp64
    for n in (0, 33, 95, 127):
        for c in (0, 9, 63):
            got = u[n // 32, c // 8, c % 8, n % 32]
            want = U[n, c].reshape(16).astype(np.float32) if n < cout else np.zeros(16, np.float32)
            np.testing.assert_array_equal(got, want)          # rounded once from fp64


@pytest.mark.parametrize("hw", [(13, 17), (14, 14), (8, 8), (1, 1), (2, 3), (9, 4)])
def test_tile_decomposition_equals_direct_conv(hw):
    x = RNG.normal(size=(hw[0], hw[1], 5))
    g = RNG.normal(size=(3, 3, 5, 4))
    np.testing.assert_allclose(_wino(x, g), _direct(x, g), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- the library's eligibility rule
def _lib_or_skip():
    from masklab_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib, _lib.load()


def _desc(_lib, B=1, H=32, W=32, cin=128, k=3, stride=1, dil=1, pad=1, n_pad=128, cout=128, math=0, **kw):
    d = _lib.ConvDesc()
    d.B, d.H, d.W = B, H, W
    d.in_cstride, d.in_coff, d.span, d.span_pad, d.cpp_shift = cin, 0, cin, -(-cin // 32) * 32, 30
    Ho = (H + 2 * pad - ((k - 1) * dil + 1)) // stride + 1
    Wo = (W + 2 * pad - ((k - 1) * dil + 1)) // stride + 1
    d.Ho, d.Wo, d.KH, d.KW, d.stride, d.dil, d.pad_t, d.pad_l = Ho, Wo, k, k, stride, dil, pad, pad
    d.cout, d.n_pad, d.out_cstride, d.math = cout, n_pad, cout, math
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def test_eligibility_rule():
    _lib, lib = _lib_or_skip()
    ok = lambda **kw: lib.ml_conv2d_wino_eligible(C.byref(_desc(_lib, **kw)))
    assert ok()
    assert ok(cin=160) and ok(H=13, W=17) and ok(H=1, W=1) and ok(cout=75)
    assert not ok(math=3) and not ok(math=1)                   # f32x3 / fp16 operands
    assert not ok(k=1, pad=0) and not ok(stride=2) and not ok(dil=2, pad=2)
    assert not ok(pad=0)                                       # 'valid'
    assert not ok(cin=144)                                     # span % 32
    assert not ok(n_pad=96, cout=75)
    assert not ok(group_cin_step=32) and not ok(shuffle2x2=1)
    # the batch size never changes the answer
    for B in (1, 2, 8, 32):
        for hw in ((128, 128), (64, 64), (8, 8), (14, 14)):
            assert ok(B=B, H=hw[0], W=hw[1])


def test_launch_splits_of_the_winograd_tile_code():
    _lib, lib = _lib_or_skip()
    levels = [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)]
    arr = (_lib.ConvDesc * 5)()
    for i, (h, w) in enumerate(levels):
        arr[i] = _desc(_lib, B=1, H=h, W=w, tile=6)
    sp = (C.c_int32 * 5)()
    assert lib.ml_conv2d_launch_splits(arr, 5, 512 << 20, sp) == 0
    assert list(sp) == [1] * 5
    # the same levels on the direct kernel are cut along K for one image (the case the Winograd path removes)
    for i in range(5):
        arr[i].tile = 0
    assert lib.ml_conv2d_launch_splits(arr, 5, 512 << 20, sp) == 0
    assert max(sp) > 1
