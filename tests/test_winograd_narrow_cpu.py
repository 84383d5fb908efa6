"""CPU tests of the narrow case of the Winograd path: the padded weight layout of a conv packed fewer than 128 rows wide,
the library's narrow predicate (ml_conv2d_wino_narrow) on every desc field it names, and the eligibility rule, which it
leaves as it was."""
import ctypes as C
import os

import numpy as np
import pytest

from masklab_hip import packing

RNG = np.random.default_rng(59)


@pytest.mark.parametrize("cout,n_pad", [(75, 96), (60, 64), (20, 32), (96, 96)])
def test_padded_winograd_weights_equal_the_128_wide_packing(cout, n_pad):
    cin = 64
    w = RNG.normal(size=(3, 3, cin, cout)).astype(np.float32)
    narrow = packing.pack_dense(w, None, tile=0)
    assert narrow.n_pad == n_pad
    wide = packing.pack_dense(w, None, tile=1)
    assert wide.n_pad == 128
    u = packing.pack_winograd(narrow)
    assert u.dtype == np.float32 and u.shape == (4, cin // 8, 8, 32, 16) and u.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(u, packing.pack_winograd(wide))
    rows = u.transpose(0, 3, 1, 2, 4).reshape(128, -1)          # [output row][chunk, channel, position]
    assert (rows[cout:] == 0).all() and (np.abs(rows[:cout]).max(axis=1) > 0).all()
    assert narrow.wgt.shape[0] == n_pad                          # the direct-path weights are not touched


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


def test_narrow_predicate():
    _lib, lib = _lib_or_skip()
    nar = lambda **kw: lib.ml_conv2d_wino_narrow(C.byref(_desc(_lib, **kw)))
    assert not lib.ml_conv2d_wino_narrow(None)
    # the automatic packings of cout <= 96
    for cout, n_pad in ((1, 32), (3, 32), (31, 32), (33, 64), (60, 64), (63, 64), (65, 96), (75, 96), (96, 96)):
        assert nar(cout=cout, n_pad=n_pad), (cout, n_pad)
        assert nar(cout=cout, n_pad=n_pad, cin=160, H=13, W=17) and nar(cout=cout, n_pad=n_pad, H=1, W=1)
    # n_pad: 128 belongs to the eligibility rule, anything else to nobody; cout must fit its rows
    assert not nar(cout=75, n_pad=128) and not nar(cout=128, n_pad=128)
    assert not nar(cout=75, n_pad=80) and not nar(cout=75, n_pad=160) and not nar(cout=75, n_pad=0)
    assert not nar(cout=75, n_pad=64) and not nar(cout=0, n_pad=32)
    # cout = 32 and 64 stay beside their `live` launches on the direct kernel
    assert not nar(cout=32, n_pad=32) and not nar(cout=64, n_pad=64)
    # everything else the rule asks for
    ok75 = dict(cout=75, n_pad=96)
    assert not nar(math=3, **ok75) and not nar(math=1, **ok75) and not nar(math=2, **ok75)
    assert not nar(k=1, pad=0, **ok75) and not nar(stride=2, **ok75) and not nar(dil=2, pad=2, **ok75)
    assert not nar(pad=0, **ok75) and not nar(cin=144, **ok75)
    assert not nar(group_cin_step=32, **ok75) and not nar(shuffle2x2=1, **ok75) and not nar(out_f16=1, **ok75)
    assert not nar(cpp_shift=2, **ok75)
    res = (C.c_float * 1)()
    assert not nar(residual=C.addressof(res), **ok75)
    # no fixed-capacity batches and no epilogue statistics
    live = (C.c_int32 * 1)(1)
    part = (C.c_double * 8)()
    assert not nar(live=C.addressof(live), live_period=1, **ok75)
    assert not nar(gn_partials=C.addressof(part), **ok75)
    # the batch size never changes the answer
    for B in (1, 2, 8, 32):
        for hw in ((128, 128), (64, 64), (8, 8), (14, 14)):
            assert nar(B=B, H=hw[0], W=hw[1], **ok75) and nar(B=B, H=hw[0], W=hw[1], cout=60, n_pad=64)


def test_eligibility_rule_is_unchanged():
    """Every case of tests/test_winograd_cpu.py::test_eligibility_rule, answered as before."""
    _lib, lib = _lib_or_skip()
    ok = lambda **kw: lib.ml_conv2d_wino_eligible(C.byref(_desc(_lib, **kw)))
    assert ok()
    assert ok(cin=160) and ok(H=13, W=17) and ok(H=1, W=1) and ok(cout=75)
    assert not ok(math=3) and not ok(math=1)
    assert not ok(k=1, pad=0) and not ok(stride=2) and not ok(dil=2, pad=2)
    assert not ok(pad=0)
    assert not ok(cin=144)
    assert not ok(n_pad=96, cout=75) and not ok(n_pad=64, cout=60) and not ok(n_pad=32, cout=20)
    assert not ok(group_cin_step=32) and not ok(shuffle2x2=1)
    for B in (1, 2, 8, 32):
        for hw in ((128, 128), (64, 64), (8, 8), (14, 14)):
            assert ok(B=B, H=hw[0], W=hw[1])


def test_launch_splits_of_a_narrow_problem_handed_to_the_kernel():
    """What ops._wino_select hands over (tile = 6, n_pad = 128, cout = 75): planned as one unsplit Winograd launch."""
    _lib, lib = _lib_or_skip()
    levels = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    arr = (_lib.ConvDesc * 5)()
    for i, (h, w) in enumerate(levels):
        assert lib.ml_conv2d_wino_narrow(C.byref(_desc(_lib, H=h, W=w, cout=75, n_pad=96)))
        arr[i] = _desc(_lib, H=h, W=w, cout=75, n_pad=128, tile=6)
    sp = (C.c_int32 * 5)()
    assert lib.ml_conv2d_launch_splits(arr, 5, 512 << 20, sp) == 0
    assert list(sp) == [1] * 5
