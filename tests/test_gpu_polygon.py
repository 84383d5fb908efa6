"""GPU tests of the polygon rasteriser (csrc/polygon.hip): the two kernels against the NumPy restatement of the contract in
tests/polygon_ref.py and against the library's host loops.  Everything is exact equality; outputs start out as stale bytes.
skimage parity is unpinned: the restatement is the contract.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import dirty_memory as DM
import polygon_cases as CASES
import polygon_ref as REF


@pytest.mark.parametrize("H,W", CASES.SIZES)
def test_every_polygon_case_equals_the_restatement(H, W):
    """All single-polygon cases as the planes of one batch of one image, each with the full window."""
    from masklab_hip import ops
    cases = CASES.polygons(H, W)
    verts, offsets = CASES.pack(list(cases.values()))
    n = len(cases)
    windows = np.array([CASES.full_window(H, W)] * n, np.int32)
    want = REF.instance_planes(verts, offsets, windows, 1, n, H, W)
    with DM.poisoned():
        dirty = DM.snapshot([ops.polygon_instance_masks(verts, offsets, windows, 1, n, H, W) for _ in range(2)])
    with DM.zeroed():
        clean = DM.snapshot(ops.polygon_instance_masks(verts, offsets, windows, 1, n, H, W))
    for got in (*dirty, clean):
        assert got.dtype == np.int8
        for j, name in enumerate(cases):
            np.testing.assert_array_equal(got[0, j], want[0, j], err_msg=name)
    for j, name in enumerate(cases):
        assert want[0, j].any() != (name in CASES.DEGENERATE), name


@pytest.mark.parametrize("H,W", CASES.SIZES)
def test_windows_padding_planes_and_semantic_maps(H, W):
    from masklab_hip import ops
    verts, offsets, windows, B, n = CASES.instance_batch(H, W)
    with DM.poisoned():
        got = host(ops.polygon_instance_masks(verts, offsets, windows, B, n, H, W))
    np.testing.assert_array_equal(got, REF.instance_planes(verts, offsets, windows, B, n, H, W))
    assert (got[1, 1:] == -1).all()
    sv, spo, sgo, B, S = CASES.semantic_batch(H, W)
    with DM.poisoned():
        sem = DM.snapshot([ops.polygon_semantic_maps(sv, spo, sgo, B, S, H, W) for _ in range(2)])
    want = REF.semantic_maps(sv, spo, sgo, B, S, H, W)
    assert sem[0].dtype == np.uint8 and want.any()
    np.testing.assert_array_equal(sem[0], want)
    np.testing.assert_array_equal(sem[1], want)
    np.testing.assert_array_equal(sem[0], ops.polygon_reference_host("semantic", sv, spo, B, S, H, W, group_offsets=sgo))
    # offsets and vertices that are on the device already are taken as they are
    again = ops.polygon_semantic_maps(dev(sv), dev(spo), dev(sgo), B, S, H, W)
    np.testing.assert_array_equal(host(again), want)
    empty = ops.polygon_instance_masks(verts, offsets[:1], windows[:0], 2, 0, H, W)
    assert tuple(empty.shape) == (2, 0, H, W) and empty.dtype == torch.int8 and empty.is_cuda


def test_random_batch_equals_the_host_entry():
    from masklab_hip import ops
    B, n, H, W = 2, 3, 53, 77
    verts, offsets, windows = CASES.random_batch(B, n, H, W, seed=5377)
    want = ops.polygon_reference_host("instance", verts, offsets, B, n, H, W, windows=windows)
    np.testing.assert_array_equal(want, REF.instance_planes(verts, offsets, windows, B, n, H, W))
    assert (want == 1).any() and (want == 0).any() and (want == -1).any()
    with DM.poisoned():
        got = host(ops.polygon_instance_masks(verts, offsets, windows, B, n, H, W))
    np.testing.assert_array_equal(got, want)


def test_a_plane_wider_than_one_column_chunk_and_taller_than_one_block():
    """2100 columns x 19 rows: two column chunks (2048), three row groups (8)."""
    from masklab_hip import ops
    H, W = 19, 2100
    poly = np.array([[10.5, 0.0], [2090.5, 0.5], [2070.0, 18.0], [1000.0, 9.5], [30.0, 17.0]])
    verts, offsets = CASES.pack([poly, CASES.circle(1050.0, 9.0, 8.5, V=700)])
    windows = np.array([[3, 0, 2080, 18], [0, 0, W - 1, H - 1]], np.int32)
    want = REF.instance_planes(verts, offsets, windows, 1, 2, H, W)
    with DM.poisoned():
        got = host(ops.polygon_instance_masks(verts, offsets, windows, 1, 2, H, W))
    np.testing.assert_array_equal(got, want)
    assert want[0, 0, 1, 2047] == 1 and want[0, 0, 1, 2048] == 1 and want[0, 1].any()
    poly_offsets, group_offsets = offsets, np.array([0, 1, 2], np.int32)           # S = 1: the polygon minus the circle
    sem = host(ops.polygon_semantic_maps(verts, poly_offsets, group_offsets, 1, 1, H, W))
    np.testing.assert_array_equal(sem, REF.semantic_maps(verts, poly_offsets, group_offsets, 1, 1, H, W))


@pytest.mark.parametrize("off", [1, 7])
def test_views_off_a_16_byte_boundary_with_guards_on_a_side_stream(off):
    """Outputs sliced from the middle of a larger allocation at an odd byte offset and pre-filled with 0x5A: every byte of
    the view is written, no byte outside it, on a stream that is not the default one."""
    from masklab_hip import ops
    H, W = CASES.SIZES[1]
    verts, offsets, windows, B, n = CASES.instance_batch(H, W)
    sv, spo, sgo, Bs, S = CASES.semantic_batch(H, W)
    want_inst = REF.instance_planes(verts, offsets, windows, B, n, H, W)
    want_sem = REF.semantic_maps(sv, spo, sgo, Bs, S, H, W)
    guard = 0x5A
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    for dtype, want, shape in ((torch.int8, want_inst, (B, n, H, W)), (torch.uint8, want_sem, (Bs, H, W, S))):
        count = int(np.prod(shape))
        buf = DM.fill_bytes(torch.empty(count + 64, dtype=dtype, device="cuda"), guard)
        assert buf.data_ptr() % 16 == 0
        lead = 16 + off
        out = buf[lead:lead + count].view(shape)
        assert out.data_ptr() % 16 == off
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(2):
                if dtype == torch.int8:
                    got = ops.polygon_instance_masks(verts, offsets, windows, B, n, H, W, out=out)
                else:
                    got = ops.polygon_semantic_maps(sv, spo, sgo, Bs, S, H, W, out=out)
                assert got.data_ptr() == out.data_ptr()
        stream.synchronize()
        whole = host(buf)
        np.testing.assert_array_equal(whole[lead:lead + count].reshape(shape), want)
        assert DM.holds(whole[:lead], guard) and DM.holds(whole[lead + count:], guard), "wrote outside the view"


def test_ops_refuse_what_they_cannot_do():
    from masklab_hip import ops
    verts, offsets, windows, B, n = CASES.instance_batch(45, 80)
    with pytest.raises(ValueError):
        ops.polygon_instance_masks(verts, offsets[::-1].copy(), windows, B, n, 45, 80)
    with pytest.raises(ValueError):
        ops.polygon_instance_masks(verts, offsets, windows[:3], B, n, 45, 80)
    with pytest.raises(TypeError):
        ops.polygon_instance_masks(verts.astype(np.float32), offsets, windows, B, n, 45, 80)
    with pytest.raises(ValueError):
        ops.polygon_instance_masks(verts, offsets, windows, B, n, 45, 80, out=torch.empty((B, n, 45, 81), dtype=torch.int8, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.polygon_instance_masks(verts, offsets, windows, B, n, 45, 80, device="cpu")


def test_more_polygons_in_one_image_than_the_kernel_keeps_offsets_for():
    """530 small triangles in image 1 (the semantic kernel keeps 512 polygon offsets of an image in LDS and reads the rest from
    global memory), behind an image 0 with three polygons so that the cached range does not start at 0."""
    from masklab_hip import ops
    H, W = CASES.SIZES[1]
    rng = np.random.default_rng(530)
    few = [CASES.polygons(H, W)[k] for k in ("triangle", "concave", "bow_tie")]
    many = [np.stack([rng.uniform(0, W, 3), rng.uniform(0, H, 3)], axis=1) for _ in range(530)]
    verts, poly_offsets = CASES.pack(few + many)
    group_offsets = np.array([0, 1, 2, 3, 3 + 200, 3 + 525, 3 + 530], np.int32)       # B = 2, S = 2: (1, 1, 1 except) | (200, 325, 5 except)
    want = REF.semantic_maps(verts, poly_offsets, group_offsets, 2, 2, H, W)
    assert want[1, :, :, 1].any() and not want[1, :, :, 1].all()
    with DM.poisoned():
        got = host(ops.polygon_semantic_maps(verts, poly_offsets, group_offsets, 2, 2, H, W))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, ops.polygon_reference_host("semantic", verts, poly_offsets, 2, 2, H, W, group_offsets=group_offsets))
