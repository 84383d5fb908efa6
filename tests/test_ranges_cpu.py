"""CPU tests of the launchers' memory-range checks (csrc/ranges.h) at their boundaries.  Every pointer here is made up, so every
case ends in a host-side refusal and none reaches a launch: a REFUSED range is shown by its own message, an ACCEPTED one by the
refusal that follows it in the same entry point (`workspace_bytes=0` giving "workspace is too small", a later problem with a bad
pointer, ...).  Where no host check follows the range test only the refusing side can be shown here.

"Abutting" means as tight as the entry point's alignment checks allow: one byte for the uint8 entry points, one float (4 bytes)
or one 16-byte row where a pointer must be aligned so.  No GPU."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

MB = 1 << 20


def _lib_and_err():
    from masklab_hip import _lib
    lib = _lib.load()
    return _lib, lib, lambda: lib.ml_last_error().decode()


# ------------------------------------------------------------------ conv_grad.hip: a dy view's exact extent
def _wgrad_view(B, bstride):
    """One 1x1 problem: 2 x 2 output pixels, cout 4 read at channel stride 8, d.out the view's first element (channel 4 of a
    buffer at 2 MB) -> (descriptor, the view's first byte, bytes to one past its last element)"""
    from masklab_hip import ops, packing
    g = ops.conv2d_wgrad_geometry((B, 2, 2, 4), packing.pack_dense(np.zeros((1, 1, 4, 4), np.float32)), dy_cstride=8,
                                  dy_bstride=bstride)
    first = 2 * MB + 16
    g.conv.in_, g.conv.out = MB, first
    bs = bstride if bstride else 4 * 8
    return g, first, ((B - 1) * bs + 3 * 8 + 4) * 4


@pytest.mark.parametrize("B,bstride", [(1, 0), (2, 40)])
@pytest.mark.parametrize("which", ["dkernel", "dbias"])
def test_wgrad_accepts_an_output_at_the_views_real_end_and_refuses_one_float_earlier(B, bstride, which):
    _lib, lib, err = _lib_and_err()
    g, first, nbytes = _wgrad_view(B, bstride)
    assert nbytes == (112 if B == 1 else 272)
    message = {"dkernel": "dkernel may not overlap x or dy", "dbias": "dbias may not overlap x, dy or dkernel"}[which]

    def launch(at):
        g.dkernel, g.dbias = (at, None) if which == "dkernel" else (8 * MB, at)
        arr = (_lib.ConvWgradDesc * 1)(g)
        assert lib.ml_conv2d_wgrad_multi_f32(arr, 1, C.c_void_p(256), 0, None) == -1
        return err()

    assert "workspace is too small" in launch(first + nbytes)          # the first byte after the view's last element
    assert message in launch(first + nbytes - 4)
    assert message in launch(first)
    out_bytes = 4 * 4 * 4 if which == "dkernel" else 4 * 4
    assert message in launch(first - out_bytes + 4)                     # its last float is the view's first
    assert "workspace is too small" in launch(first - out_bytes)


@pytest.mark.parametrize("B,bstride,nbytes", [(1, 0, 112), (2, 40, 272)])
def test_gather_refuses_an_out_inside_the_views_last_pixel(B, bstride, nbytes):
    """No host check follows the gather's range test: the accepting side is a GPU test (tests/test_gpu_ranges.py)"""
    _lib, lib, err = _lib_and_err()
    dy = 2 * MB + 16
    out_bytes = B * 4 * 4 * 4
    for out in (dy + nbytes - 4, dy, dy - out_bytes + 4):
        assert lib.ml_conv2d_grad_gather_dy_f32(dy, out, B, 4, 4, 8, bstride, None) == -1
        assert "out may not overlap dy" in err()


# ------------------------------------------------------------------ visualize.hip
def test_serving_visualize_ranges_at_one_byte():
    _lib, lib, err = _lib_and_err()
    cols = (C.c_float * 48)()
    B, n, mh, mw, H, W, Ks = 1, 2, 3, 3, 4, 4, 3
    px = B * H * W
    images, det, ins, seg, far = MB, 2 * MB, 3 * MB, 4 * MB, 6 * MB
    sizes = {det: B * n * 24, ins: B * n * mh * mw * 4, seg: px * Ks * 4}

    def call(out, thr):
        assert lib.ml_serving_visualize_u8(images, det, ins, seg, out, thr, cols, 5, 0.3, cols, Ks, 0.3, B, n, mh, mw, H, W, None) == -1
        return err()

    out_msg, thr_msg = "out overlaps an input or the threshold workspace", "threshold_ws overlaps an input"
    for other, nbytes in sizes.items():
        assert out_msg in call(other - px * 3 + 1, 5 * MB)              # out's last byte is the other's first
        assert out_msg in call(other + nbytes - 1, 5 * MB)              # out's first byte is the other's last
        # one byte apart: accepted, shown by the next refusal (the threshold workspace inside the frames)
        assert thr_msg in call(other - px * 3, images + 8)
        assert thr_msg in call(other + nbytes, images + 8)
    # out against the threshold workspace, which hangs 3 bytes out of det (behind it, in front of it) so that the next
    # refusal still comes where out is accepted
    thr = det + sizes[det] - 1
    assert out_msg in call(thr + 3, thr)
    assert thr_msg in call(thr + 4, thr)
    thr = det - 3
    assert out_msg in call(thr - px * 3 + 1, thr)
    assert thr_msg in call(thr - px * 3, thr)
    # the threshold workspace against each input: nothing follows that test, the refusing side only
    for other, nbytes in list(sizes.items()) + [(images, px * 3)]:
        assert thr_msg in call(far, other - 3)
        assert thr_msg in call(far, other + nbytes - 1)


def test_draw_instance_refuses_an_out_that_shares_one_byte():
    _lib, lib, err = _lib_and_err()
    cols = (C.c_float * 48)()
    B, n, H, W = 1, 2, 4, 4
    px = B * H * W
    images, det, masks = MB, 2 * MB, 3 * MB
    for other, nbytes in ((det, B * n * 24), (masks, px * n * 4)):
        for out in (other - px * 3 + 1, other + nbytes - 1):
            assert lib.ml_draw_instance_u8(images, det, masks, out, cols, 5, 0.3, B, n, H, W, None) == -1
            assert "draw_instance: out overlaps det or masks" in err()


# ------------------------------------------------------------------ jpeg.hip
def test_jpeg_encode_refuses_lengths_that_share_one_byte():
    _lib, lib, err = _lib_and_err()
    H, W = 32, 48
    cap, ws_bytes = lib.ml_jpeg_encode_capacity(H, W), lib.ml_jpeg_encode_workspace_bytes(1, H, W)
    img, out, ws = MB, 2 * MB, 4 * MB
    for other, nbytes in ((img, H * W * 3), (out, cap), (ws, ws_bytes)):
        for lengths in (other - 3, other + nbytes - 1):                 # B = 1: lengths is one int32
            assert lib.ml_jpeg_encode_u8(img, 1, H, W, 95, out, cap, lengths, ws, None) == -1
            assert "jpeg_encode: workspace or lengths overlaps another buffer" in err()


# ------------------------------------------------------------------ deconv_out.hip: the tapes
def test_tape_launch_ranges_at_one_row():
    _lib, lib, err = _lib_and_err()
    K, c_mid, M = 32, 128, 294
    x_bytes, t_bytes = M * K * 4, M * 4 * c_mid * 4

    def prob(x):
        d = _lib.DeconvOutProblem()
        d.x, d.wd, d.wo_table, d.out = x, 40 * MB, 41 * MB, 42 * MB
        d.M, d.hw, d.w, d.rois_per_image = M, 49, 7, 3
        return d

    def call(xs, tapes):
        arr = (_lib.DeconvOutProblem * len(xs))(*[prob(x) for x in xs])
        assert lib.ml_deconv2x2_out1x1_tape_f32(arr, (C.c_void_p * len(tapes))(*tapes), len(xs), K, c_mid, 3, 4, 1, 4, None) == -1
        return err()

    x0, x1 = MB, 2 * MB
    # the tape against x, from both sides; accepted: problem 1's misaligned tape is the next refusal
    assert "problem 0: the tape overlaps x" in call([x0, x1], [x0 + x_bytes - 16, 8 * MB])
    assert "problem 0: the tape overlaps x" in call([x0, x1], [x0 - t_bytes + 16, 8 * MB])
    assert "problem 1: the tape must be a 16-byte aligned" in call([x0, x1], [x0 + x_bytes, 20 * MB + 4])
    assert "problem 1: the tape must be a 16-byte aligned" in call([x0 + t_bytes, x1 + t_bytes], [x0, 20 * MB + 4])
    # a tape against an earlier tape; accepted: problem 1's tape on its own x is the next refusal
    t0 = 8 * MB
    assert "problems 0 and 1 write the same tape" in call([x0, x1], [t0, t0 + t_bytes - 16])
    assert "problems 0 and 1 write the same tape" in call([x0, x1], [t0, t0 - t_bytes + 16])
    assert "problem 1: the tape overlaps x" in call([x0, t0 + t_bytes], [t0, t0 + t_bytes])
    assert "problem 1: the tape overlaps x" in call([x0, t0 - t_bytes], [t0, t0 - t_bytes])


# ------------------------------------------------------------------ dwconv_grad.hip
def test_dwconv_wgrad_ranges_at_one_float():
    from masklab_hip import ops
    _lib, lib, err = _lib_and_err()
    C_ = 32
    x, dy = MB, 2 * MB
    x_bytes = dy_bytes = 2 * 8 * 8 * C_ * 4
    dk_bytes, db_bytes = 9 * C_ * 4, C_ * 4
    message = "the outputs may not overlap x, dy or each other"

    def launch(dkernel, dbias):
        d = ops.dwconv3x3_wgrad_geometry((2, 8, 8, C_))
        d.x, d.dy, d.dkernel, d.dbias = x, dy, dkernel, dbias
        arr = (_lib.DwGradDesc * 1)(d)
        assert lib.ml_dwconv3x3_wgrad_multi_f32(arr, 1, C.c_void_p(256), 0, None) == -1
        return err()

    far_k, far_b = 8 * MB, 9 * MB
    for other, nbytes in ((x, x_bytes), (dy, dy_bytes)):
        assert message in launch(other - dk_bytes + 4, far_b)
        assert message in launch(other + nbytes - 4, far_b)
        assert message in launch(far_k, other - db_bytes + 4)
        assert message in launch(far_k, other + nbytes - 4)
        assert "workspace is too small" in launch(other - dk_bytes, far_b)
        assert "workspace is too small" in launch(other + nbytes, far_b)
        assert "workspace is too small" in launch(far_k, other - db_bytes)
        assert "workspace is too small" in launch(far_k, other + nbytes)
    assert message in launch(far_k, far_k - db_bytes + 4)
    assert message in launch(far_k, far_k + dk_bytes - 4)
    assert "workspace is too small" in launch(far_k, far_k - db_bytes)
    assert "workspace is too small" in launch(far_k, far_k + dk_bytes)


def test_dwconv_dgrad_ranges_at_one_row():
    from masklab_hip import ops
    _lib, lib, err = _lib_and_err()
    C_ = 32
    dx_bytes = dy_bytes = 2 * 8 * 8 * C_ * 4
    w_bytes = 9 * C_ * 4

    def prob(i, dx):
        d = ops.dwconv3x3_wgrad_geometry((2, 8, 8, C_))
        base = 16 * MB * (i + 1)
        d.dy, d.wgt, d.dx = base, base + MB, dx
        return d

    def launch(*dxs):
        arr = (_lib.DwGradDesc * len(dxs))(*[prob(i, dx) for i, dx in enumerate(dxs)])
        assert lib.ml_dwconv3x3_dgrad_multi_f32(arr, len(dxs), None) == -1
        return err()

    dy0, w0 = 16 * MB, 17 * MB
    message = "problem 0: dx may not overlap dy or the kernel"
    for other, nbytes in ((dy0, dy_bytes), (w0, w_bytes)):
        assert message in launch(other - dx_bytes + 16, 2 * MB)
        assert message in launch(other + nbytes - 16, 2 * MB)
        # accepted: problem 1 without a dx is the next refusal
        assert "problem 1: null pointer" in launch(other - dx_bytes, None)
        assert "problem 1: null pointer" in launch(other + nbytes, None)
    # dx against another problem's dx
    assert "problems 0 and 1 write the same dx" in launch(2 * MB, 2 * MB + dx_bytes - 16)
    assert "problems 0 and 1 write the same dx" in launch(2 * MB, 2 * MB - dx_bytes + 16)
    assert "problem 2: null pointer" in launch(2 * MB, 2 * MB + dx_bytes, None)
    assert "problem 2: null pointer" in launch(2 * MB, 2 * MB - dx_bytes, None)


# ------------------------------------------------------------------ resample_grad.hip
def test_resample_grad_ranges_at_one_row():
    _lib, lib, err = _lib_and_err()
    B, Cc, Ho, Wo = 2, 8, 6, 6
    dy = MB
    # the 1x1 source: accepted ranges go on to the workspace it needs
    dx_bytes, dy_bytes = B * Cc * 4, B * Ho * Wo * Cc * 4

    def bilinear(dx):
        assert lib.ml_resize_bilinear_ac_grad_f32(dy, None, dx, B, 1, 1, Cc, Ho, Wo, Cc, 0, None, 0, None) == -1
        return err()

    assert "dx may not overlap dy" in bilinear(dy + dy_bytes - 16)
    assert "dx may not overlap dy" in bilinear(dy - dx_bytes + 16)
    assert "needs a workspace" in bilinear(dy + dy_bytes)
    assert "needs a workspace" in bilinear(dy - dx_bytes)

    # the global mean: accepted ranges go on to a shifted `add`
    HW = 9
    dpool, pool_bytes, mean_bytes = MB, B * Cc * 4, B * HW * Cc * 4

    def mean(dx):
        assert lib.ml_global_mean_grad_f32(dpool, dx + 16, dx, B, HW, Cc, None) == -1
        return err()

    assert "dx may not overlap dpool" in mean(dpool + pool_bytes - 16)
    assert "dx may not overlap dpool" in mean(dpool - mean_bytes + 16)
    assert "not a shifted view" in mean(dpool + pool_bytes)
    assert "not a shifted view" in mean(dpool - mean_bytes)

    # the RoI crops: levels are checked from the last one down, so level 0 (n_l > cap) is the refusal after level 1's ranges
    cap, ch, cw, Hf, Wf, n_l = 3, 2, 2, 4, 4, 2
    lv_dy, lvdx_bytes, lvdy_bytes = 4 * MB, B * Hf * Wf * Cc * 4, B * n_l * ch * cw * Cc * 4

    def crops(dx):
        level = (_lib.RoiGradLevel * 2)()
        level[0].dy, level[0].dx, level[0].Hf, level[0].Wf, level[0].n_l = 8 * MB, 9 * MB, Hf, Wf, cap + 1
        level[1].dy, level[1].dx, level[1].Hf, level[1].Wf, level[1].n_l = lv_dy, dx, Hf, Wf, n_l
        args = (C.c_void_p(4096), 7, 1, C.c_void_p(8192), C.c_void_p(12288), B)
        assert lib.ml_roi_crop_resize_grad_f32(level, 2, *args, Cc, cap, 2, ch, cw, 64.0, 64.0, None) == -1
        return err()

    assert "level 1: dx may not overlap dy" in crops(lv_dy + lvdy_bytes - 16)
    assert "level 1: dx may not overlap dy" in crops(lv_dy - lvdx_bytes + 16)
    assert "level 0: bad dims" in crops(lv_dy + lvdy_bytes)
    assert "level 0: bad dims" in crops(lv_dy - lvdx_bytes)
