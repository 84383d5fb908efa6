"""NumPy restatements for the generator tests (test infrastructure, not collected: no `test_` prefix).

  * `cv2_resize`: cv2.resize(src, (ow, oh)) with the default INTER_LINEAR for uint8 and float64 images, restated from
    OpenCV's plain C++ path as include/masklab_hip.h ("Generator resizes") states it, the switch to INTER_AREA at exactly
    2x on both axes included.  OpenCV parity is unpinned: cv2 is not available where the tests run, so this text is the
    contract the kernels are held to.
  * `getitem`: MaskLabGenerator.__getitem__ as the reference writes it -- one cv2.resize per image, per float64 copy of a
    semantic map and per live mask, np.round, the boxes scaled in place.
"""
import numpy as np

F32 = np.float32


def axis_taps(dst, src):
    """One axis: -> (s0, s1 int64 [dst], w0, w1 float32 [dst])."""
    scale = 1.0 / (np.float64(dst) / np.float64(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    assert f.dtype == F32
    low, high = s < 0, s >= src - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = src - 1, 0
    return s, np.minimum(s + 1, src - 1), F32(1) - f, f


def is_area(H, W, oh, ow):
    return H == 2 * oh and W == 2 * ow


def _taps(src, oh, ow):
    """-> the four gathered neighbours [oh,ow,C] and the weights shaped to broadcast over them."""
    y0, y1, wy0, wy1 = axis_taps(oh, src.shape[0])
    x0, x1, wx0, wx1 = axis_taps(ow, src.shape[1])
    rows0, rows1 = src[y0], src[y1]
    col = lambda w: w[None, :, None]
    row = lambda w: w[:, None, None]
    return (rows0[:, x0], rows0[:, x1], rows1[:, x0], rows1[:, x1]), (col(wx0), col(wx1)), (row(wy0), row(wy1))


def _quad(src):
    return src[0::2, 0::2], src[0::2, 1::2], src[1::2, 0::2], src[1::2, 1::2]


def linear_u8(src, oh, ow):
    """The fixed-point INTER_LINEAR path on a uint8 [H,W,C] image, whatever the ratio."""
    (s00, s01, s10, s11), wx, wy = _taps(src.astype(np.int32), oh, ow)
    coef = lambda w: np.rint(w * F32(2048)).astype(np.int16).astype(np.int32)
    a0, a1, b0, b1 = coef(wx[0]), coef(wx[1]), coef(wy[0]), coef(wy[1])
    r0, r1 = s00 * a0 + s01 * a1, s10 * a0 + s11 * a1
    out = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def linear_f64(src, oh, ow):
    """The float64 INTER_LINEAR path on a [H,W,C] image, whatever the ratio (not rounded)."""
    (s00, s01, s10, s11), wx, wy = _taps(src.astype(np.float64), oh, ow)
    wx0, wx1, wy0, wy1 = (w.astype(np.float64) for w in (*wx, *wy))
    h0 = s00 * wx0 + s01 * wx1
    h1 = s10 * wx0 + s11 * wx1
    return h0 * wy0 + h1 * wy1


def resize_u8(src, oh, ow):
    """cv2.resize(src, (ow, oh)) of a uint8 [H,W,C] image."""
    if is_area(src.shape[0], src.shape[1], oh, ow):
        s00, s01, s10, s11 = (q.astype(np.int32) for q in _quad(src))
        return ((s00 + s01 + s10 + s11 + 2) >> 2).astype(np.uint8)
    return linear_u8(src, oh, ow)


def resize_f64(src, oh, ow):
    """cv2.resize(src, (ow, oh)) of a float64 [H,W,C] image (not rounded)."""
    if is_area(src.shape[0], src.shape[1], oh, ow):
        s00, s01, s10, s11 = (q.astype(np.float64) for q in _quad(src))
        return (s00 + s01 + s10 + s11) * 0.25
    return linear_f64(src, oh, ow)


def cv2_resize(src, dsize):
    """cv2.resize(src, dsize) with dsize = (width, height), as the reference calls it: [H,W] or [H,W,C], uint8 or float64."""
    ow, oh = dsize
    img = src if src.ndim == 3 else src[..., None]
    if src.dtype == np.uint8:
        out = resize_u8(img, oh, ow)
    elif src.dtype == np.float64:
        out = resize_f64(img, oh, ow)
    else:
        raise TypeError(src.dtype)
    return out if src.ndim == 3 else out[..., 0]


def getitem(dataset, index, batch_size, scale_ratio, rng=None):
    """The reference generator's __getitem__ -> (X,).  The dataset's 'detection' array is scaled in place, as there."""
    data = dataset[batch_size * index:batch_size * (index + 1)]
    images = data['images']
    gt_seg = data['semantic'].astype(np.float64)
    gt_seg_exist = data['semantic_exist'].astype(np.float64)
    gt_boxes = data['detection']
    gt_masks = data['instance']
    gt_boxes_exist = data['instance_exist'].astype(np.float64)
    if isinstance(scale_ratio, (tuple, list)):
        scale_ratio = (rng if rng is not None else np.random).uniform(*scale_ratio)
    height, width = images.shape[1:3]
    target_h = int(height * scale_ratio) // 32 * 32
    target_w = int(width * scale_ratio) // 32 * 32

    batch_images = np.stack([cv2_resize(image, (target_w, target_h)) for image in images])
    batch_seg = np.round(np.stack([cv2_resize(seg, (target_w, target_h)) for seg in gt_seg]))

    batch_masks = np.full(gt_masks.shape[:2] + (target_h, target_w), -1, np.int8)
    for i, masks in enumerate(gt_masks):
        for j, mask in enumerate(masks):
            if mask[0, 0] != -1.:
                batch_masks[i, j] = cv2_resize(mask.astype(np.uint8), (target_w, target_h))

    for column, ratio in enumerate((target_w / width, target_h / height, target_w / width, target_h / height)):
        gt_boxes[gt_boxes[..., 5] > 0, column] *= ratio
    return ({"images": batch_images, "gt_seg": batch_seg, "gt_seg_exist": gt_seg_exist, "gt_boxes": gt_boxes,
             "gt_boxes_exist": gt_boxes_exist, "gt_masks": batch_masks},)
