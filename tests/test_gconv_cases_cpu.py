"""The case table of the grouped 3x3 (tests/gconv_cases.py) against the library's host-only ml_gconv3x3_launch_plan -- the
plan the launchers themselves take their grid and run from: every row is launched with the tile shape, run and block count it
names, the table names all 14 instantiations and walks every one of the 12 that can, the ReLU / ReLU6 data reaches the
clamps, and the entries refuse what they say they refuse.  No GPU: without a device the library plans for 256 compute units,
the MI355X's."""
import ctypes as C

import numpy as np
import pytest

import gconv_cases as GC


def _probe(dtype, c, stride, B=2, H=9, W=9, Cn=64):
    from masklab_hip import _lib
    out = (C.c_int32 * 6)()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rc = _lib.load().ml_gconv3x3_launch_plan(B, H, W, Cn, c, stride, Ho, Wo, int(dtype == "f16"), out)
    return rc, list(out)


@pytest.mark.parametrize("row", GC.ROWS, ids=lambda r: r.name)
def test_row_plans_onto_the_tiles_run_and_blocks_it_names(row):
    from masklab_hip import _lib
    rc, (th, tw, tiles_x, tiles_y, run, blocks) = GC.plan(row)
    assert rc == 0, _lib.load().ml_last_error()
    assert (th, tw, run, blocks) == row.plan
    assert (th, tw) == GC.tile_of(*row.inst)
    Ho, Wo, _, _ = GC.out_hw(row)
    assert (tiles_x, tiles_y) == (-(-Wo // tw), -(-Ho // th))
    assert blocks == tiles_x * -(-tiles_y // run) * (row.C // 64) * row.shape[0]
    if row.c == 32:
        assert run == tiles_y                         # a c = 32 block takes its whole tile column


def test_the_table_names_every_instantiation():
    """The instantiations as the library reports them: the plan entry probed over dtype x c x stride (a refusal is no
    instantiation); the edge rows name each exactly once, and every kind of row that is per body covers all five bodies."""
    probed = {(d, c, s) for d in ("f32", "f16") for c in (2, 4, 8, 16, 32, 64) for s in (1, 2, 3) if _probe(d, c, s)[0] == 0}
    assert len(probed) == 14 and probed == set(GC.INSTANTIATIONS)
    assert sorted(r.inst for r in GC.ROWS if r.kind == "edge") == sorted(probed)
    assert {r.inst for r in GC.ROWS if r.kind == "run"} == probed
    bodies = set(GC.BODY.values())
    assert len(bodies) == 5
    for tag in ("none_", "relu6_", "nobias_"):
        assert {(r.body, r.stride) for r in GC.ROWS if r.name.startswith(tag)} == {(b, s) for b in bodies for s in (1, 2)}
    for tag in ("pad01_", "pad11even_"):
        assert {r.body for r in GC.ROWS if r.name.startswith(tag)} == bodies
    for tag in ("tiny_1x1_", "tiny_1x9_", "tiny_low_wide_"):
        assert {(r.dtype, r.c) for r in GC.ROWS if r.name.startswith(tag)} == set(GC.BODY)
    assert {r.dtype for r in GC.ROWS if r.kind == "edge" and r.C == 192} == {"f32", "f16"}


def test_edge_rows_have_a_full_tile_two_partial_edges_and_odd_maps():
    for row in (r for r in GC.ROWS if r.kind == "edge"):
        th, tw = GC.tile_of(*row.inst)
        _, H, W = row.shape
        Ho, Wo, pt, pl = GC.out_hw(row)
        assert H % 2 == 1 and W % 2 == 1 and (pt, pl) == (1, 1)
        assert th < Ho < 2 * th and tw < Wo < 2 * tw, row.name
        if row.stride == 2:                           # the last window row / column lies on the zero padding
            assert (Ho - 1) * 2 - pt + 2 == H and (Wo - 1) * 2 - pl + 2 == W, row.name


def test_run_rows_walk_three_tiles_and_end_on_a_shorter_run():
    walking = [r for r in GC.ROWS if r.kind == "run" and r.c != 32]
    assert sorted(r.inst for r in walking) == sorted(GC.WALKING) and len(walking) == 12
    for row in walking:
        rc, (th, tw, tiles_x, tiles_y, run, blocks) = GC.plan(row)
        Ho, _, _, _ = GC.out_hw(row)
        assert rc == 0 and run >= 3 and tiles_y % run != 0 and Ho % th != 0, row.name
        assert blocks >= GC.WANT_BLOCKS
        rc, alone = GC.plan(row, B=1)
        assert rc == 0 and alone[4] == 1 and alone[:4] == [th, tw, tiles_x, tiles_y], row.name
    for row in (r for r in GC.ROWS if r.kind == "run" and r.c == 32):
        rc, (th, _, _, tiles_y, run, _) = GC.plan(row)
        assert rc == 0 and run == tiles_y >= 3 and GC.out_hw(row)[0] % th != 0, row.name


def test_padding_rows_resolve_to_what_they_are_for():
    for row in (r for r in GC.ROWS if r.kind == "padding"):
        _, H, W = row.shape
        Ho, Wo, pt, pl = GC.out_hw(row)
        if row.name.startswith(("pad01_", "same_")) and row.stride == 2:
            assert H % 2 == 0 and W % 2 == 0 and (pt, pl) == (0, 0) and (Ho, Wo) == (H // 2, W // 2), row.name
        elif row.name.startswith("pad11even_"):
            assert H % 2 == 0 and W % 2 == 0 and (pt, pl) == (1, 1) and (Ho, Wo) == (H // 2, W // 2), row.name
        elif row.name.startswith("valid_"):
            assert (pt, pl) == (0, 0) and (Ho, Wo) == (H - 2, W - 2), row.name
        else:
            assert row.padding == "same" and row.stride == 1 and (pt, pl, Ho, Wo) == (1, 1, H, W), row.name


def test_relu_and_relu6_rows_reach_the_clamps():
    """On the fp64 reference alone: at least 5 % of a ReLU6 row's pre-activation above 6 and 5 % below 0; at least 5 % of a
    ReLU row's below 0 (run rows: on the two images that have a reference)."""
    n6 = 0
    for row in (r for r in GC.ROWS if r.act is not None):
        pre, _ = GC.reference(row)
        below, above = float((pre < 0).mean()), float((pre > 6).mean())
        assert below >= 0.05, (row.name, below)
        if row.act == "relu6":
            assert above >= 0.05, (row.name, above)
            n6 += 1
    assert n6 == 10


def test_reference_equals_grouped_conv_fast():
    """The torch float64 reference against oracle.grouped_conv_fast (pad 1 each side), once."""
    from oracle import masklab as O
    row = GC.BY_NAME["edge_f32_c8_s1"]
    k, _ = GC.params(row)
    x = GC.batch(row).astype(np.float64)
    Ho, Wo, pt, pl = GC.out_hw(row)
    got = GC.conv_fp64(x, k, row.c, row.stride, Ho, Wo, pt, pl)
    want = O.grouped_conv_fast(x, k.astype(np.float64), row.C // row.c, row.c, row.stride)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    row = GC.BY_NAME["edge_f16_c16_s2"]
    k, _ = GC.params(row)
    x = GC.batch(row).astype(np.float64)
    Ho, Wo, pt, pl = GC.out_hw(row)
    np.testing.assert_allclose(GC.conv_fp64(x, k, row.c, 2, Ho, Wo, pt, pl),
                               O.grouped_conv_fast(x, k.astype(np.float64), row.C // row.c, row.c, 2), rtol=0, atol=1e-12)


def test_entries_refuse_what_they_cannot_run():
    """ML_E_BADARG (-1) with the reason in ml_last_error, from the plan entry and from both launch entries alike; aligned fake
    addresses, nothing is dereferenced or launched."""
    from masklab_hip import _lib
    lib = _lib.load()
    IN, WGT, OUT = 0x10000, 0x20000, 0x30000

    def launch(fn, B=2, H=9, W=9, Cn=64, c=4, stride=1, in_=IN, wgt=WGT, bias=None, out=OUT):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        return fn(in_, wgt, bias, out, B, H, W, Cn, c, Ho, Wo, stride, 1, 1, _lib.ACT_RELU, None)

    def plan(half, B=2, H=9, W=9, Cn=64, c=4, stride=1):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        return lib.ml_gconv3x3_launch_plan(B, H, W, Cn, c, stride, Ho, Wo, half, (C.c_int32 * 6)())

    shape_refusals = [(dict(c=2), b"channels per group 2"), (dict(c=12), b"channels per group 12"),
                      (dict(c=64, Cn=128), b"channels per group 64"), (dict(Cn=96), b"multiple of 64"),
                      (dict(Cn=0), b"multiple of 64"), (dict(stride=3), b"stride must be 1 or 2"),
                      (dict(B=65536), b"bad dims"), (dict(B=0), b"bad dims"),
                      (dict(B=2048, H=1024, W=1024), b"too many pixels")]
    for half, fn in ((0, lib.ml_gconv3x3_f32), (1, lib.ml_gconv3x3_f16)):
        for kw, msg in shape_refusals:
            assert plan(half, **kw) == -1 and msg in lib.ml_last_error(), (half, kw, lib.ml_last_error())
            assert launch(fn, **kw) == -1 and msg in lib.ml_last_error(), (half, kw, lib.ml_last_error())
        for kw in (dict(in_=IN + 4), dict(wgt=WGT + 8), dict(out=OUT + 2), dict(bias=0x40004)):
            assert launch(fn, **kw) == -1 and b"16-byte aligned" in lib.ml_last_error(), (half, kw)
        assert launch(fn, out=None) == -1 and b"null pointer" in lib.ml_last_error()
        assert plan(half, B=2047, H=1024, W=1024) == 0              # just below 2^31 pixels
    assert lib.ml_gconv3x3_launch_plan(2, 9, 9, 64, 4, 1, 9, 9, 0, None) == -1 and b"null pointer" in lib.ml_last_error()
    # groups of 32: half tensors only
    assert plan(0, c=32) == -1 and b"half tensors: also 32" in lib.ml_last_error()
    assert launch(lib.ml_gconv3x3_f32, c=32) == -1 and b"half tensors: also 32" in lib.ml_last_error()
    assert plan(1, c=32) == 0
    assert plan(1, c=32, Cn=16 * 64 + 32) == -1 and b"multiple of 64" in lib.ml_last_error()


def test_depthwise_cases_are_what_they_are_for():
    """tests/dwconv_cases.py asserts on its float64 reference that ReLU6 data spans both clamps and that dilation 12 on a
    5 x 7 map leaves the centre tap alone: here without a GPU, for the fp32 and the half form of every case."""
    import dwconv_cases as DW
    for name, (_, _, _, Cn, _, act, bias) in DW.CASES.items():
        for half in (False, True):
            x, k, b, pre = DW.case(name, 2 * Cn if half else Cn, half)
            assert x.dtype == (np.float16 if half else np.float32) and (b is None) == (bias is None)
            assert pre.shape[3] == x.shape[3] and np.isfinite(pre).all()
    assert {c[5] for c in DW.CASES.values()} == {None, "relu", "relu6"}
