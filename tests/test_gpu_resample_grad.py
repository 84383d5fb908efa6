"""GPU tests of the resampling backward (csrc/resample_grad.hip): ops.roi_crop_resize_grad, ops.resize_bilinear_ac_grad,
ops.global_mean_grad and the layer methods on top of them against torch autograd over the float64 restatements of
tests/resample_grad_ref.py.  The bar is the project's gradient bar, |got - want| <= 1e-5 * S, S = sum |weight * dy| the
uncancelled magnitude of the element (exact zeros where no sample reaches).  A term is a product of two float32 weights and a
float32 gradient added in float32: a few 1e-7 of S; the 1x1 source sums in float64.  Every op also holds: two launches give the
same bits; the bits do not depend on what outputs and workspace held; the inputs are left unchanged; float16, channel counts
that are no multiple of 4 and mismatched shapes are refused with their message.  -m gpu.

Largest |got - want| / S measured on the MI355X, per case (RoI: over its three levels; the bar is 1e-5):
    RoI     crop14 1.8e-07   crop3x5 1.6e-07   crop1 1.0e-07   crop14_c4 1.4e-07   70 RoIs on one level 7.9e-08
    resize  up2 1.3e-07   odd 1.4e-07   same 0   down 7.5e-08   column 5.7e-08   pooled 1.0e-08   tail 1.4e-07
            pooled_big 4.3e-09   odd slice 1.4e-07   pooled slice 1.2e-08
    layers  top-down 0 / 1.1e-07 / 7.3e-08 (finest first)   global_mean_grad 5.1e-08, 5.6e-08"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import dirty_memory as DM
import resample_grad_ref as R


def _bits(a, b, what):
    DM.assert_same_bits(DM.snapshot(a), DM.snapshot(b), what)


def _kernels(fn):
    """-> (fn(), the launcher names it recorded in ops.PROFILE, in launch order)"""
    from masklab_hip import ops
    ops.PROFILE = []
    try:
        out = fn()
        return out, [r["kernel"] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _everything(run, inputs, what):
    """What every op holds: -> the first launch's snapshot, after two launches gave the same bits, stale and zeroed outputs
    and workspace gave those bits too, and the inputs (device tensor, host array) are what they were"""
    got = DM.snapshot(run())
    _bits(run(), got, f"{what}: two launches")
    with DM.zeroed():
        clean = DM.snapshot(run())
    with DM.poisoned():
        dirty = DM.snapshot(run())
    DM.assert_same_bits(dirty, clean, f"{what}: stale outputs and workspace")
    DM.assert_same_bits(clean, got, f"{what}: zeroed outputs and workspace")
    for t, a in inputs:
        np.testing.assert_array_equal(host(t), a, err_msg=f"{what}: an input changed")
    return got


# ------------------------------------------------------------------ RoI align
@functools.lru_cache(maxsize=None)
def roi_reference(name):
    """-> (case, want per level, S per level): computed once per case, shared and left unchanged"""
    case = R.roi_case(name)
    want, S = R.roi_align_grad(case["dys"], case["rows"], case["shapes"], case["crop"], case["img_hw"])
    return case, want, S


def _roi_tables(case):
    """The forward's tables from the device's own MaskDistribute; they are the restatement's"""
    from masklab_hip import ops
    rows = dev(case["rows"])
    slots, lcounts, lmax, _ = ops.mask_distribute(rows, len(case["shapes"]) - 1, 1.0, has_k=True)
    ref_slots, ref_counts = R.level_slots(case["rows"], len(case["shapes"]))
    np.testing.assert_array_equal(host(slots), ref_slots)
    np.testing.assert_array_equal(host(lcounts), ref_counts)
    np.testing.assert_array_equal(host(lmax), ref_counts.max(axis=0))
    return rows, slots, lcounts


@pytest.mark.parametrize("name", list(R.ROI_CASES))
def test_roi_crop_resize_grad(name):
    from masklab_hip import ops
    case, want, S = roi_reference(name)
    rows, slots, lcounts = _roi_tables(case)
    shapes, crop, img = case["shapes"], case["crop"], case["img_hw"]
    dys = [dev(d) for d in case["dys"]]                         # the capacity form: n_l = cap, 1e30 in the padded slots

    def run(d=dys, **kw):
        return ops.roi_crop_resize_grad(d, shapes, rows, slots, lcounts, crop, img, **kw)

    got = _everything(run, list(zip(dys, case["dys"])) + [(rows, case["rows"])], name)
    for level, (g, w, s) in enumerate(zip(got, want, S)):
        assert g.dtype == np.float32
        R.check(g, w, s, f"{name} level {level}")
    assert not got[0][1].any() and not got[2][1].any()          # an image with no RoI on a level: zeros, written
    # the sized form ([B, max count, ...]) gives the capacity form's bits
    _bits(run([dev(d) for d in R.sized(case)]), got, f"{name}: sized form")
    # add= in place is add + the gradient computed separately: one float32 addition, so the very bits (and so within the bar)
    r = np.random.default_rng(11)
    adds = [r.normal(0, 1, s).astype(np.float32) for s in shapes]
    bufs = [dev(a) for a in adds]
    ret = run(add=bufs, out=bufs)
    assert all(o.data_ptr() == b.data_ptr() for o, b in zip(ret, bufs))
    for level, (o, a, g) in enumerate(zip(ret, adds, got)):
        np.testing.assert_array_equal(host(o), a + g, err_msg=f"{name} level {level}: add in place")
    _bits(run(add=[dev(a) for a in adds]), ret, f"{name}: add out of place")
    # the layer method is the op
    from masklab_hip.layers.instance import PyramidRoiAlign
    layer = PyramidRoiAlign(crop_size=crop, name="pyramid_roi_align")
    _bits(layer.backward(dys, shapes, rows, img, slots, lcounts), got, f"{name}: PyramidRoiAlign.backward")


def test_roi_crop_resize_grad_more_rois_than_one_lds_chunk():
    """70 RoIs of one image on one level: the walk over the RoIs crosses the boundary of the 64 the kernel stages at a time"""
    from masklab_hip import ops
    case = R.many_rois_case()
    assert case["counts"][0, 0] == 70 and R.margin(case["rows"], case["shapes"], case["crop"], case["img_hw"]) >= 1e-3
    want, S = R.roi_align_grad(case["dys"], case["rows"], case["shapes"], case["crop"], case["img_hw"])
    rows, slots, lcounts = _roi_tables(case)
    dys = [dev(d) for d in case["dys"]]
    got = _everything(lambda: ops.roi_crop_resize_grad(dys, case["shapes"], rows, slots, lcounts, case["crop"], case["img_hw"]),
                      [(dys[0], case["dys"][0])], "70 RoIs")
    R.check(got[0], want[0], S[0], "70 RoIs")


def test_roi_crop_resize_grad_refusals():
    from masklab_hip import ops
    case = roi_reference("crop3x5")[0]
    rows, slots, lcounts = _roi_tables(case)
    dys = [dev(d) for d in case["dys"]]
    run = lambda d=dys, shapes=case["shapes"], **kw: ops.roi_crop_resize_grad(d, shapes, rows, slots, lcounts, case["crop"],
                                                                             case["img_hw"], **kw)
    with pytest.raises(TypeError, match="float32 only"):
        run([d.half() for d in dys])
    with pytest.raises(ValueError, match="multiple of 4"):
        run([torch.zeros((2, R.CAP, 3, 5, 6), device="cuda")] * 3, [(2, 16, 16, 6), (2, 8, 8, 6), (2, 4, 4, 6)])
    with pytest.raises(ValueError, match="expected"):
        run([d[:, :, :, :4].contiguous() for d in dys])
    with pytest.raises(ValueError, match=r"`add` is .* expected \(2, 16, 16, 8\)"):
        run(add=[torch.zeros((2, 8, 8, 8), device="cuda")] * 3)
    with pytest.raises(RuntimeError, match="may not overlap dy"):
        flat = torch.zeros(2 * 16 * 16 * 8, device="cuda")
        run([flat[:2 * R.CAP * 3 * 5 * 8].view(2, R.CAP, 3, 5, 8)] + dys[1:], out=[flat.view(2, 16, 16, 8), None, None])


# ------------------------------------------------------------------ resize_bilinear(align_corners=True)
@functools.lru_cache(maxsize=None)
def resize_reference(name, cs=None, coff=0):
    dy, shape = R.resize_case(name, cs, coff)
    want, S = R.resize_grad(dy[..., coff:coff + shape[3]], shape[1], shape[2])
    return dy, shape, want, S


@pytest.mark.parametrize("name", list(R.RESIZE_CASES))
def test_resize_bilinear_ac_grad(name):
    from masklab_hip import ops
    dy_h, (B, H, W, Cc), want, S = resize_reference(name)
    dy = dev(dy_h)
    got = _everything(lambda: ops.resize_bilinear_ac_grad(dy, H, W), [(dy, dy_h)], name)
    assert got.dtype == np.float32 and got.shape == (B, H, W, Cc)
    R.check(got, want, S, name)
    if name == "down":
        assert (S == 0).any() and not got[S == 0].any()          # sources no sample touches: exact zeros
    from masklab_hip.layers.misc import ResizeLike
    _bits(ResizeLike(name="resize_like").backward(dy, (B, H, W, Cc)), got, f"{name}: ResizeLike.backward")


@pytest.mark.parametrize("name", ["odd", "pooled"])
def test_resize_bilinear_ac_grad_reads_a_concat_slice(name):
    """dy = channels 8:16 of a 24-channel tensor: the bits of the gradient of that slice on its own"""
    from masklab_hip import ops
    dy_h, (B, H, W, Cc), want, S = resize_reference(name, 24, 8)
    dy = dev(dy_h)
    got = _everything(lambda: ops.resize_bilinear_ac_grad(dy, H, W, C=Cc, dy_coff=8), [(dy, dy_h)], f"{name} slice")
    R.check(got, want, S, f"{name} slice")
    _bits(ops.resize_bilinear_ac_grad(dev(dy_h[..., 8:8 + Cc]), H, W), got, f"{name}: the slice on its own")
    from masklab_hip.layers.misc import ResizeLike
    _bits(ResizeLike(name="resize_like").backward(dy, (B, H, W, Cc), dy_coff=8), got, f"{name}: ResizeLike.backward")


@pytest.mark.parametrize("name", ["up2", "pooled"])
def test_resize_bilinear_ac_grad_add_in_place(name):
    from masklab_hip import ops
    dy_h, (B, H, W, Cc), want, S = resize_reference(name)
    add_h = np.random.default_rng(13).normal(0, 1, (B, H, W, Cc)).astype(np.float32)
    dy, buf = dev(dy_h), dev(add_h)
    ret = ops.resize_bilinear_ac_grad(dy, H, W, add=buf, out=buf)
    assert ret.data_ptr() == buf.data_ptr()
    # add + the gradient computed separately: one float32 addition, so the very bits (and so within the bar)
    np.testing.assert_array_equal(host(ret), add_h + host(ops.resize_bilinear_ac_grad(dy, H, W)))
    _bits(ops.resize_bilinear_ac_grad(dy, H, W, add=dev(add_h)), ret, f"{name}: add out of place")


def test_resize_bilinear_ac_grad_refusals():
    from masklab_hip import ops
    dy = torch.zeros((1, 8, 8, 8), device="cuda")
    with pytest.raises(TypeError, match="float32 only"):
        ops.resize_bilinear_ac_grad(dy.half(), 4, 4)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.resize_bilinear_ac_grad(torch.zeros((1, 8, 8, 6), device="cuda"), 4, 4)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.resize_bilinear_ac_grad(dy, 4, 4, C=2, dy_coff=4)
    with pytest.raises(ValueError, match="no slice of dy"):
        ops.resize_bilinear_ac_grad(dy, 4, 4, C=8, dy_coff=4)
    with pytest.raises(ValueError, match=r"`out` is \(1, 4, 4, 4\), expected \(1, 4, 4, 8\)"):
        ops.resize_bilinear_ac_grad(dy, 4, 4, out=torch.zeros((1, 4, 4, 4), device="cuda"))
    with pytest.raises(RuntimeError, match="may not overlap dy"):
        ops.resize_bilinear_ac_grad(dy, 8, 8, out=dy)


# ------------------------------------------------------------------ layers
def test_feature_pyramid_backward_top_down():
    """Three levels, finest first: d_merged[l+1] += resize^T(d_merged[l]) in place, against autograd through the restated
    forward chain merged[l] = lateral[l] + resize(merged[l+1])"""
    from masklab_hip.layers.detection import FeaturePyramid
    sizes = [(13, 9), (7, 5), (4, 3)]
    r = np.random.default_rng(17)
    d_h = [r.normal(0, 1, (2,) + s + (8,)).astype(np.float32) for s in sizes]
    lateral = [torch.zeros(d.shape, dtype=torch.float64, requires_grad=True) for d in d_h]
    merged = lateral[-1]
    total = (merged * torch.from_numpy(d_h[-1].astype(np.float64))).sum()
    for l in (1, 0):
        merged = lateral[l] + R.resize(merged, *sizes[l])
        total = total + (merged * torch.from_numpy(d_h[l].astype(np.float64))).sum()
    total.backward()
    # S of a level: its own gradient plus the transposed resize of the finer level's S
    S = [np.abs(d_h[0]).astype(np.float64)]
    for l in (1, 2):
        My, Mx = R.resize_axis_matrix(sizes[l][0], sizes[l - 1][0]), R.resize_axis_matrix(sizes[l][1], sizes[l - 1][1])
        S.append(np.abs(d_h[l]) + R._apply_t(np.abs(My), np.abs(Mx), torch.from_numpy(S[-1])).numpy())
    fpn = FeaturePyramid([8, 16, 32], num_features=8, name="fpn")
    d = [dev(a) for a in d_h]
    got = fpn.backward_top_down(d)
    assert [g.data_ptr() for g in got] == [t.data_ptr() for t in d]
    for l, (g, lat, s) in enumerate(zip(got, lateral, S)):
        R.check(host(g), lat.grad.numpy(), s, f"top-down level {l}")
    np.testing.assert_array_equal(host(got[0]), d_h[0])            # the finest level's gradient is its own
    _bits(fpn.backward_top_down([dev(a) for a in d_h]), got, "top-down: two runs")


@pytest.mark.parametrize("shape", [(2, 5, 7, 8), (1, 33, 17, 12)])
def test_global_mean_grad(shape):
    from masklab_hip import ops
    B, H, W, Cc = shape
    r = np.random.default_rng(19)
    dpool_h = r.normal(0, 1, (B, 1, 1, Cc)).astype(np.float32)
    add_h = r.normal(0, 1, shape).astype(np.float32)
    dpool = dev(dpool_h)
    got = _everything(lambda: ops.global_mean_grad(dpool, H, W), [(dpool, dpool_h)], f"global_mean_grad {shape}")
    want, S = R.global_mean_grad(dpool_h, H, W)
    np.testing.assert_allclose(want, np.broadcast_to(dpool_h.astype(np.float64) / (H * W), shape), rtol=1e-15)   # the closed form
    R.check(got, want, S, f"global_mean_grad {shape}")
    buf = dev(add_h)
    ret = ops.global_mean_grad(dpool, H, W, add=buf, out=buf)
    assert ret.data_ptr() == buf.data_ptr()
    np.testing.assert_array_equal(host(ret), add_h + got)           # add + the gradient computed separately: the very bits
    with pytest.raises(TypeError, match="float32 only"):
        ops.global_mean_grad(dpool.half(), H, W)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.global_mean_grad(torch.zeros((1, 1, 1, 6), device="cuda"), H, W)
    with pytest.raises(ValueError, match="expected"):
        ops.global_mean_grad(dpool, H, W, add=torch.zeros((B, H, W + 1, Cc), device="cuda"))
