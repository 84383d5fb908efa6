"""CPU tests of the polygon rasteriser (no GPU): the library's host loops over the kernels' edge, scan and store code
(ml_polygon_reference_host) against the NumPy restatement of the contract in tests/polygon_ref.py.  Everything is exact
equality.  skimage parity is unpinned: the restatement, not a run of skimage, is the contract."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import polygon_cases as CASES
import polygon_ref as REF


def _one_plane(ops, poly, H, W, window=None):
    verts, offsets = CASES.pack([poly])
    windows = np.array([window or CASES.full_window(H, W)], np.int32)
    got = ops.polygon_reference_host("instance", verts, offsets, 1, 1, H, W, windows=windows)
    assert got.dtype == np.int8 and got.shape == (1, 1, H, W)
    np.testing.assert_array_equal(got, REF.instance_planes(verts, offsets, windows, 1, 1, H, W))
    return got[0, 0]


@pytest.mark.parametrize("H,W", CASES.SIZES)
def test_host_entry_equals_the_restatement_on_every_polygon_case(H, W):
    from masklab_hip import ops
    for name, poly in CASES.polygons(H, W).items():
        plane = _one_plane(ops, poly, H, W)
        assert set(np.unique(plane)) <= {0, 1}, name
        if name in CASES.DEGENERATE:
            assert not plane.any(), name
        else:
            assert plane.any() and not plane.all(), name
    # the clipped polygon reaches all four borders; the touching one fills up to, but not including, its last row and column
    clipped = _one_plane(ops, CASES.polygons(H, W)["clipped_on_four_sides"], H, W)
    assert clipped[0].any() and clipped[:, 0].any() and clipped[H - 2].any() and clipped[:, W - 2].any()
    touching = _one_plane(ops, CASES.polygons(H, W)["touches_last_row_and_column"], H, W)
    assert touching[H - 2].any() and touching[:, W - 2].any() and not touching[H - 1].any() and not touching[:, W - 1].any()


def test_the_rule_on_a_hand_written_square():
    """A 6 x 6 axis-aligned square on integer vertices (2, 1) .. (8, 7): rows 1..6 and columns 2..7 are filled -- the top
    and the left edge belong to it, the bottom row 7 and the right column 8 do not (y < yp on rows, x < e on columns)."""
    from masklab_hip import ops
    square = np.array([[2.0, 1.0], [8.0, 1.0], [8.0, 7.0], [2.0, 7.0]])
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.int8)
    verts, offsets = CASES.pack([square])
    got = ops.polygon_reference_host("instance", verts, offsets, 1, 1, 9, 10, windows=np.array([[0, 0, 9, 8]], np.int32))
    np.testing.assert_array_equal(got[0, 0], want)
    np.testing.assert_array_equal(REF.polygon_mask(square, 9, 10).astype(np.int8), want)
    # the same square drawn the other way round, and starting from another vertex
    for other in (square[::-1], np.roll(square, 1, axis=0)):
        v, o = CASES.pack([other])
        np.testing.assert_array_equal(ops.polygon_reference_host("instance", v, o, 1, 1, 9, 10, windows=np.array([[0, 0, 9, 8]], np.int32))[0, 0],
                                      want)


def test_bow_tie_is_even_odd():
    """Both lobes of the self-intersecting bow-tie are inside and the crossing is a single point: under the even-odd rule no
    pixel has a winding number of 2 to lose, so the visible property is that the left and the right lobe are filled and the
    middle column band above and below the crossing is not."""
    from masklab_hip import ops
    H, W = CASES.SIZES[0]
    plane = _one_plane(ops, CASES.polygons(H, W)["bow_tie"], H, W)
    assert plane[H // 2, 8] == 1 and plane[H // 2, W - 10] == 1 and plane[5, W // 2] == 0 and plane[H - 6, W // 2] == 0
    # a figure whose overlap IS covered twice: a pentagram's core is outside under even-odd
    t = (np.arange(5) * 2 % 5) * (2 * np.pi / 5) - np.pi / 2
    star = np.stack([40 + 20 * np.cos(t), 22 + 20 * np.sin(t)], axis=1)
    plane = _one_plane(ops, star, H, W)
    assert plane[22, 40] == 0 and plane[8, 40] == 1


@pytest.mark.parametrize("H,W", CASES.SIZES)
def test_windows_padding_planes_and_a_batch_of_two(H, W):
    from masklab_hip import ops
    verts, offsets, windows, B, n = CASES.instance_batch(H, W)
    got = ops.polygon_reference_host("instance", verts, offsets, B, n, H, W, windows=windows)
    want = REF.instance_planes(verts, offsets, windows, B, n, H, W)
    np.testing.assert_array_equal(got, want)
    assert (got[1, 1:] == -1).all() and (got[0] >= 0).all() and (got[1, 0] >= 0).all()
    # the cut window cuts: the circle reaches beyond it, the plane does not
    x1, y1, x2, y2 = windows[0]
    whole = REF.polygon_mask(verts[offsets[0]:offsets[1]], H, W)
    assert whole.sum() > got[0, 0].sum() > 0 and not got[0, 0, :y1].any() and not got[0, 0, :, x2 + 1:].any()
    # x2 >= W is cut to the last column
    assert windows[1][2] >= W and got[0, 1, :, W - 2].any()


def test_no_planes_is_a_no_op():
    from masklab_hip import ops
    none = ops.polygon_reference_host("instance", np.zeros((0, 2)), np.zeros(1, np.int32), 2, 0, 45, 80, windows=np.zeros((0, 4), np.int32))
    assert none.shape == (2, 0, 45, 80) and none.dtype == np.int8
    assert ops.polygon_reference_host("instance", np.zeros((0, 2)), np.zeros(1, np.int32), 0, 3, 45, 80,
                                      windows=np.zeros((0, 4), np.int32)).shape == (0, 3, 45, 80)
    # all planes padding: no vertex at all
    pad = ops.polygon_reference_host("instance", np.zeros((0, 2)), np.zeros(3, np.int32), 1, 2, 9, 21, windows=np.zeros((2, 4), np.int32))
    assert (pad == -1).all()


def test_a_plane_wider_than_one_column_chunk():
    """2100 columns: the kernels work in chunks of 2048 columns, and a threshold beyond the chunk must carry over."""
    from masklab_hip import ops
    H, W = 5, 2100
    poly = np.array([[10.5, 0.0], [2090.5, 0.5], [2070.0, 4.0], [1000.0, 2.5], [30.0, 4.0]])
    plane = _one_plane(ops, poly, H, W, window=[3, 0, 2080, 4])
    assert plane[1, 2047] == 1 and plane[1, 2048] == 1 and plane[1, 2081] == 0


@pytest.mark.parametrize("H,W", CASES.SIZES)
def test_semantic_union_and_except(H, W):
    from masklab_hip import ops
    verts, poly_offsets, group_offsets, B, S = CASES.semantic_batch(H, W)
    got = ops.polygon_reference_host("semantic", verts, poly_offsets, B, S, H, W, group_offsets=group_offsets)
    assert got.dtype == np.uint8 and got.shape == (B, H, W, S)
    np.testing.assert_array_equal(got, REF.semantic_maps(verts, poly_offsets, group_offsets, B, S, H, W))
    m = [REF.polygon_mask(verts[poly_offsets[i]:poly_offsets[i + 1]], H, W) for i in range(5)]
    a, b, c, exc, bow = m
    assert (a & b & ~exc).any()                                                    # the overlap exists ...
    np.testing.assert_array_equal(got[0, :, :, 0], ((a | b) & ~exc).astype(np.uint8))   # ... and is a union, not an xor
    assert (c & exc).any() and not got[0, :, :, 1][exc].any() and not got[0, :, :, 0][exc].any()   # in a label and excepted -> 0
    assert not got[0, :, :, 2].any()                                               # a label with no polygons
    np.testing.assert_array_equal(got[1, :, :, 2], bow.astype(np.uint8))
    assert not got[1, :, :, :2].any()


def test_argument_errors_from_the_wrappers_and_the_raw_abi():
    from masklab_hip import _lib, ops
    verts, offsets = CASES.pack([CASES.polygons(45, 80)["triangle"]])
    win = np.array([[0, 0, 79, 44]], np.int32)
    host = lambda **kw: ops.polygon_reference_host(**{**dict(kind="instance", verts=verts, offsets=offsets, B=1, n_or_S=1, H=45, W=80,
                                                             windows=win), **kw})
    with pytest.raises(ValueError):
        host(kind="outline")
    with pytest.raises(TypeError):
        host(verts=verts.astype(np.float32))
    with pytest.raises(TypeError):
        host(offsets=offsets.astype(np.int64))
    with pytest.raises(ValueError):
        host(offsets=np.array([2, 0], np.int32))                                   # not monotonic
    with pytest.raises(ValueError):
        host(offsets=np.array([0, 4], np.int32))                                   # past the end
    with pytest.raises(ValueError):
        host(offsets=np.array([0, 1, 3], np.int32))                                # B*n + 1 entries expected
    with pytest.raises(ValueError):
        host(H=0)
    with pytest.raises(ValueError):
        host(H=1 << 16, W=1 << 15)
    with pytest.raises(ValueError):
        host(windows=None)
    with pytest.raises(ValueError):
        host(windows=np.zeros((2, 4), np.int32))
    sv, spo, sgo, B, S = CASES.semantic_batch(45, 80)
    with pytest.raises(ValueError):
        ops.polygon_reference_host("semantic", sv, spo, B, 17, 45, 80, group_offsets=np.zeros(B * 18 + 1, np.int32))
    with pytest.raises(ValueError):
        ops.polygon_reference_host("semantic", sv, spo, B, S, 45, 80, group_offsets=sgo[::-1].copy())
    with pytest.raises(ValueError):
        ops.polygon_reference_host("semantic", sv, spo, B, S, 45, 80)
    # the device wrappers refuse before they touch the device (this machine may have none)
    with pytest.raises(ValueError):
        ops.polygon_instance_masks(verts, offsets, win, 1, 1, 0, 80)
    with pytest.raises(ValueError):
        ops.polygon_semantic_maps(sv, spo, sgo, B, 17, 45, 80)
    with pytest.raises(ValueError):
        ops.polygon_instance_masks(verts, offsets, win, -1, 1, 45, 80)

    lib = _lib.load()
    p = lambda a: C.c_void_p(a.ctypes.data)
    out = np.full(45 * 80, 0x5A, np.uint8)
    bad = np.array([2, 0], np.int32)
    I, Sm = _lib.POLYGON_INSTANCE, _lib.POLYGON_SEMANTIC
    assert lib.ml_polygon_reference_host(I, p(verts), 3, p(bad), 0, None, p(win), 1, 1, 45, 80, p(out)) != 0
    assert b"monotonic" in lib.ml_last_error()
    assert lib.ml_polygon_reference_host(I, p(verts), 3, p(np.array([0, 4], np.int32)), 0, None, p(win), 1, 1, 45, 80, p(out)) != 0
    assert lib.ml_polygon_reference_host(I, None, 3, p(offsets), 0, None, p(win), 1, 1, 45, 80, p(out)) != 0
    assert b"null" in lib.ml_last_error()
    assert lib.ml_polygon_reference_host(I, p(verts), 3, p(offsets), 0, None, None, 1, 1, 45, 80, p(out)) != 0
    assert lib.ml_polygon_reference_host(I, p(verts), 3, p(offsets), 0, None, p(win), 1, 1, 1 << 16, 1 << 15, p(out)) != 0
    assert lib.ml_polygon_reference_host(7, p(verts), 3, p(offsets), 0, None, p(win), 1, 1, 45, 80, p(out)) != 0
    assert lib.ml_polygon_reference_host(Sm, p(sv), len(sv), p(spo), 5, p(sgo), None, B, 17, 45, 80, p(out)) != 0
    assert b"S=17" in lib.ml_last_error()
    assert lib.ml_polygon_reference_host(Sm, p(sv), len(sv), p(spo), 5, p(sgo[::-1].copy()), None, B, S, 45, 80, p(out)) != 0
    assert (out == 0x5A).all()                                                     # nothing was written
    # the device entries refuse before any launch
    assert lib.ml_polygon_instance_masks(None, 3, None, None, 1, 1, 45, 80, None, None) != 0
    assert lib.ml_polygon_instance_masks(None, -1, None, None, 1, 1, 45, 80, None, None) != 0
    assert lib.ml_polygon_instance_masks(None, 3, None, None, 1, 1, 0, 80, None, None) != 0
    assert lib.ml_polygon_semantic_maps(None, 3, None, 1, None, 1, 17, 45, 80, None, None) != 0
    assert lib.ml_polygon_semantic_maps(None, 3, None, 1, None, 1, 3, 45, 80, None, None) != 0
    assert b"polygon_semantic_maps" in lib.ml_last_error()
    assert lib.ml_polygon_instance_masks(None, 0, None, None, 0, 3, 45, 80, None, None) == 0          # B == 0: a no-op
    assert lib.ml_polygon_instance_masks(None, 0, None, None, 2, 0, 45, 80, None, None) == 0          # n == 0: a no-op
