"""Fused SqueezeExcite and half skip-add without a GPU: every bad argument is refused with ML_E_BADARG and a message before
anything is launched, the workspace rule, and which mask heads run at capacity."""
import ctypes as C

import numpy as np
import pytest

ML_E_BADARG = -1
FAKE = 1 << 20          # a non-null, 16-byte aligned address: argument checks run before any device access


def _lib():
    from masklab_hip import _lib
    return _lib, _lib.load()


def _desc(**kw):
    _l, _ = _lib()
    d = _l.SeDesc()
    d.x, d.out, d.w1, d.w2 = FAKE, FAKE, FAKE, FAKE
    d.B, d.HW, d.C, d.Hd = 2, 64, 128, 8
    d.live, d.live_period, d.ws_offset = None, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_a_launch_takes_up_to_eight_problems():
    _l, _ = _lib()
    assert _l.SE_MAX_PROBLEMS == 8


def test_workspace_grows_with_samples_and_chunks():
    _, lib = _lib()
    ws = lib.ml_squeeze_excite_workspace_bytes
    one = ws(1, 256, 128)
    assert one == 128 * 8                                   # one 256-pixel chunk: C doubles
    assert ws(1, 257, 128) == 2 * one and ws(1, 160 * 160, 128) == 100 * one
    assert ws(3, 256, 128) == 3 * one and ws(21, 196, 128) == 21 * one
    assert ws(0, 256, 128) == 0 and ws(1, 0, 128) == 0


@pytest.mark.parametrize("fn", ["ml_squeeze_excite_f32", "ml_squeeze_excite_f16"])
@pytest.mark.parametrize("bad,msg", [
    (dict(x=None), "null"), (dict(out=None), "null"), (dict(w1=None), "null"), (dict(w2=None), "null"),
    (dict(C=0), "C ="), (dict(C=130), "C ="), (dict(C=1032), "C ="), (dict(Hd=0), "Hd"), (dict(Hd=65), "Hd"),
    (dict(B=0), "positive"), (dict(HW=0), "positive"),
    (dict(live=FAKE, live_period=3), "live_period"), (dict(live=FAKE, live_period=0), "live_period"),
    (dict(x=FAKE + 8), "aligned"), (dict(out=FAKE + 4), "aligned"), (dict(w1=FAKE + 2), "weights"),
    (dict(ws_offset=8), "workspace"), (dict(ws_offset=1 << 30), "workspace"),
])
def test_squeeze_excite_rejects_bad_arguments(fn, bad, msg):
    _l, lib = _lib()
    if fn.endswith("f16") and bad.get("C") == 130:
        bad = dict(C=132)                                   # (a multiple of 4 but not of 8)
    arr = (_l.SeDesc * 1)(_desc(**bad))
    st = getattr(lib, fn)(arr, 1, C.c_void_p(FAKE), 1 << 20, None)
    assert st == ML_E_BADARG
    assert msg in lib.ml_last_error().decode()


def test_squeeze_excite_rejects_bad_calls():
    _l, lib = _lib()
    arr = (_l.SeDesc * 9)(*[_desc(ws_offset=4096 * i) for i in range(9)])
    assert lib.ml_squeeze_excite_f32(arr, 0, C.c_void_p(FAKE), 1 << 20, None) == ML_E_BADARG
    assert lib.ml_squeeze_excite_f32(arr, 9, C.c_void_p(FAKE), 1 << 20, None) == ML_E_BADARG      # > ML_SE_MAX_PROBLEMS
    assert "problems" in lib.ml_last_error().decode()
    assert lib.ml_squeeze_excite_f32(arr, 1, None, 1 << 20, None) == ML_E_BADARG
    assert lib.ml_squeeze_excite_f32(arr, 1, C.c_void_p(FAKE + 8), 1 << 20, None) == ML_E_BADARG
    assert lib.ml_squeeze_excite_f32(arr, 1, C.c_void_p(FAKE), 1024, None) == ML_E_BADARG       # slab needs 2 KiB
    two = (_l.SeDesc * 2)(_desc(), _desc(ws_offset=1024))                                      # overlapping slices
    assert lib.ml_squeeze_excite_f32(two, 2, C.c_void_p(FAKE), 1 << 20, None) == ML_E_BADARG
    assert "share workspace" in lib.ml_last_error().decode()


def test_add_f16_rejects_bad_arguments():
    _, lib = _lib()
    for args, msg in (((None, FAKE, 8), "bad arguments"), ((FAKE, None, 8), "bad arguments"), ((FAKE, FAKE, 0), "bad arguments"),
                      ((FAKE + 2, FAKE, 8), "aligned"), ((FAKE, FAKE + 6, 8), "aligned")):
        x, y, n = args
        assert lib.ml_add_f16(C.c_void_p(x), C.c_void_p(y), n, None) == ML_E_BADARG
        assert msg in lib.ml_last_error().decode()


def test_squeeze_excite_ops_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    from masklab_hip import ops
    x = torch.zeros(1, 4, 4, 128)
    with pytest.raises(RuntimeError):
        ops.squeeze_excite_multi([dict(x=x, w1=torch.zeros(128, 8), w2=torch.zeros(8, 128))])      # no CPU fallback
    with pytest.raises(RuntimeError):
        ops.add_(x.half(), x.half())


def _mask_head(se, sep, tables=True):
    pytest.importorskip("torch")
    from masklab_hip import keras_like as K
    from masklab_hip.layers import MaskSubNet
    K.clear_session()
    m = MaskSubNet(3, 4, num_depth=2, num_features=128, use_separable_conv=sep, expand_ratio=1,
                   use_squeeze_excite=se, name="mask_sub_net")
    m.build([(2, 5, 14, 14, 128)] * 3)
    m.load_weights(K.init_weights(m.weight_specs(), 0), "cpu")
    if not tables:
        m._tail_tables = None
    return m


@pytest.mark.parametrize("se,sep", [(False, False), (True, False), (False, True), (True, True)])
def test_capacity_supported_for_squeeze_excite_and_separable_mask_heads(se, sep):
    m = _mask_head(se, sep)
    assert m.capacity_supported((14, 14))
    assert not m.capacity_supported((1, 1))
    assert all(len(m._units(b[:-2])) == 2 for b in m.blocks)
    assert not _mask_head(se, sep, tables=False).capacity_supported((14, 14))


def test_squeeze_excite_packs_its_dense_kernels_once():
    m = _mask_head(True, False)
    se = m.blocks[0][0]
    assert type(se).__name__ == "SqueezeExcite"
    assert tuple(se.w1.shape) == (128, 8) and tuple(se.w2.shape) == (8, 128)
    assert se.w1.dtype == se.w2.dtype and str(se.w1.dtype) == "torch.float32"
    assert not hasattr(se.dense1, "dev")                    # the Dense layers only hold their weight specs
    assert set(se.weight_specs()) == {"mask_sub_net/block0/se0/dense1/kernel", "mask_sub_net/block0/se0/dense2/kernel"}
    assert se.get_config()["ratio"] == 16.0
