"""NumPy restatement of the reference's evaluation loop (road_project/train.py:94-212) and of its metric layers
(engine/metrics.py) -- test infrastructure, not collected.  The loop is written as the reference writes it: one full H x W
canvas per detection, logical_and / logical_or over whole canvases; cv2.resize(INTER_LINEAR) of a float64 image is
restated per axis from OpenCV's resize (PARITY UNPINNED: cv2 is not installed where the tests run, this text is the
contract).  Deviations, the ones masklab_hip/evaluate.py documents: an empty box gives an empty mask, an empty union IoU 0,
canvases are addressed by detection row, rows with conf < 0 / label < 0 never pair."""
import numpy as np

F32 = np.float32


# ----------------------------------------------------------------------------- cv2.resize(src, (bw, bh)), float64 image
def _axis(dst, src):
    scale = 1.0 / (dst / src)                                     # double scale_x = 1. / inv_scale_x
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    assert f.dtype == F32
    low = s < 0
    s[low], f[low] = 0, 0
    high = s >= src - 1
    s[high], f[high] = src - 1, 0
    return s, np.minimum(s + 1, src - 1), (F32(1) - f).astype(np.float64), f.astype(np.float64)


def resize_linear(image, bw, bh):
    image = np.asarray(image, np.float64)
    y0, y1, wy0, wy1 = _axis(bh, image.shape[0])
    x0, x1, wx0, wx1 = _axis(bw, image.shape[1])
    rows0 = image[y0][:, x0] * wx0 + image[y0][:, x1] * wx1      # the horizontal pass of the two source rows
    rows1 = image[y1][:, x0] * wx0 + image[y1][:, x1] * wx1
    return rows0 * wy0[:, None] + rows1 * wy1[:, None]


def clipped_box(row, image_h, image_w):
    """train.py:128-136: a detection row (cx, cy, w, h, ...) -> integer (x0, y0, x1, y1); float64 corners clipped to the
    image, then truncated the way an int32 array truncates them."""
    cx, cy, w, h = (np.float64(v) for v in row[:4])
    corners = [np.clip(cx - w / 2, 0, image_w), np.clip(cy - h / 2, 0, image_h),
               np.clip(cx + w / 2, 0, image_w), np.clip(cy + h / 2, 0, image_h)]
    return tuple(int(v) for v in np.array(corners, dtype=np.int32))


def pasted_mask(row, mask, image_h, image_w):
    """train.py:137-141 for one detection row -> the int8 canvas [image_h, image_w]: the mask, negatives clamped to 0,
    resized to the clipped box, thresholded at 0.5 and surrounded by zeros.  An empty box leaves the canvas empty."""
    canvas = np.zeros((image_h, image_w), np.int8)
    x0, y0, x1, y1 = clipped_box(row, image_h, image_w)
    if x1 > x0 and y1 > y0:
        canvas[y0:y1, x0:x1] = resize_linear(np.maximum(np.asarray(mask, np.float64), 0.0), x1 - x0, y1 - y0) > 0.5
    return canvas


# ----------------------------------------------------------------------------- what the three kernels compute
def mask_areas(gt):
    return (np.asarray(gt) != 0).sum(axis=(2, 3)).astype(np.int64)


def pair_stats(det, ins, gt, pairs):
    B, n = det.shape[:2]
    G, H, W = gt.shape[1:]
    out = np.zeros((len(pairs), 2), np.int64)
    for k, (b, i, g) in enumerate(pairs):
        if not (0 <= b < B and 0 <= i < n and 0 <= g < G):
            out[k] = -1
            continue
        canvas = pasted_mask(det[b, i], ins[b, i], H, W)
        out[k] = np.sum(np.logical_and(canvas, gt[b, g])), np.sum(np.logical_or(canvas, gt[b, g]))
    return out


def semantic_counts(pr, gt):
    both = np.logical_and(gt > 0.5, pr > 0.5).sum(axis=(1, 2))
    either = np.logical_or(gt > 0.5, pr > 0.5).sum(axis=(1, 2))
    return np.stack([both, either], axis=-1).astype(np.int64)


# ----------------------------------------------------------------------------- the loop
def _extent(boxes, axis):
    """(low, high) of (cx, cy, w, h) boxes along x (axis 0) or y (axis 1)"""
    half = boxes[:, 2 + axis] / 2
    return boxes[:, axis] - half, boxes[:, axis] + half


def match(pr_detection, gt_detection):
    """train.py:144-182 in float64 -> the (pr_i, gt_i) pairs with box IoU x (labels equal) > 0.5, in np.where's row-major
    order over the [prediction, ground truth] matrix.  0 / 0 is NaN and compares false."""
    pr = np.asarray(pr_detection, np.float64)
    gt = np.asarray(gt_detection, np.float64)
    overlap = np.ones((len(pr), len(gt)))
    for axis in (0, 1):
        p_lo, p_hi = _extent(pr, axis)
        g_lo, g_hi = _extent(gt, axis)
        shared = np.minimum(g_hi[None, :], p_hi[:, None]) - np.maximum(g_lo[None, :], p_lo[:, None])
        overlap = overlap * np.maximum(0.0, shared)
    both = (gt[:, 2] * gt[:, 3])[None, :] + (pr[:, 2] * pr[:, 3])[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        score = overlap / (both - overlap) * (gt[None, :, 4] == pr[:, None, 4])
        paired = score > 0.5
    paired[pr[:, 5] < 0, :] = False                       # a padded prediction
    paired[:, gt[:, 4] < 0] = False                       # a padded ground-truth slot
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(paired))]


def evaluate_ref(instance_labels, semantic_labels, batches):
    """batches: iterable of (pr_detections, pr_instances, pr_semantics, gt_detections, gt_instances, gt_semantics) NumPy
    arrays -> {label: {"iou", "counts", "miou"}}, instance labels first (train.py:98-209)."""
    table = {name: {"iou": 0.0, "counts": 0.0} for name in list(instance_labels) + list(semantic_labels)}

    def add(name, value):
        table[name]["iou"] += value
        table[name]["counts"] += 1

    for pr_dets, pr_inss, pr_sems, gt_dets, gt_inss, gt_sems in batches:
        for det, ins, sem, gt_det, gt_ins, gt_sem in zip(pr_dets, pr_inss, pr_sems, gt_dets, gt_inss, gt_sems):
            height, width = sem.shape[:2]
            canvases = {}                                             # one full canvas per paired detection row
            for i, g in match(det, gt_det):
                if i not in canvases:
                    canvases[i] = pasted_mask(det[i], ins[i], height, width)
                either = np.logical_or(canvases[i], gt_ins[g]).sum()
                both = np.logical_and(canvases[i], gt_ins[g]).sum()
                add(instance_labels[int(det[i, 4])], both / either if either else 0.0)
            truth, pred = gt_sem > 0.5, sem > 0.5
            per_class = (truth & pred).sum(axis=(0, 1)) / ((truth | pred).sum(axis=(0, 1)) + 1e-7)
            has_instances = bool(np.any(gt_ins[..., -1] != -1))        # train.py:206: gates the third ('crack') row
            for c, value in enumerate(per_class):
                if c != 2 or has_instances:
                    add(semantic_labels[c], value)
    for row in table.values():
        row["miou"] = row["iou"] / (row["counts"] + 1e-7)
    return table


# ----------------------------------------------------------------------------- the metric layers, float32
def class_binary_iou(seg_true, seg_pred, threshold=0.5):
    """engine/metrics.py:83-99 -> a list of C float32 [B] arrays."""
    thr = np.float64(F32(threshold))
    t = (np.asarray(seg_true).astype(np.float64) > thr).astype(F32)
    p = (np.asarray(seg_pred).astype(np.float64) > thr).astype(F32)
    intersection = np.sum(t * p, axis=(1, 2), dtype=np.float64).astype(F32)   # counts below 2^24: exact in float32
    area_true = np.sum(t, axis=(1, 2), dtype=np.float64).astype(F32)
    area_pred = np.sum(p, axis=(1, 2), dtype=np.float64).astype(F32)
    union = area_true + area_pred - intersection
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, intersection / union, F32(1)).astype(F32)
    return [iou[:, c] for c in range(iou.shape[1])]


def confusion_matrix_metric(cls_true, cls_pred, mask, threshold=0.3):
    """engine/metrics.py:16-60 -> (precision, recall, accuracy, fmeasure) float32 and the counts (tp, fp, fn, tn).  Class C
    stands for 'background': the truth of an anchor whose mask is not 0, the prediction of a row whose maximum is not
    above the threshold.  np.argmax, like tf.argmax, takes the first maximum.  Anchors with mask == -1 are dropped."""
    C = cls_pred.shape[2]
    truth_rows = np.asarray(cls_true, F32).reshape(-1, C)
    pred_rows = np.asarray(cls_pred, F32).reshape(-1, C)
    flags = np.asarray(mask, F32).reshape(-1)
    truth = np.where(flags == 0, truth_rows.argmax(axis=1), C)
    pred = np.where(pred_rows.max(axis=1) > F32(threshold), pred_rows.argmax(axis=1), C)
    kept, agree, object_ = flags != -1, truth == pred, pred < C
    counts = [int(np.sum(kept & a & b)) for a, b in ((agree, object_), (~agree, object_), (~agree, ~object_), (agree, ~object_))]
    tp, fp, fn, tn = (F32(v) for v in counts)
    eps = F32(1e-7)                                                    # K.epsilon()
    precision, recall = tp / (tp + fp + eps), tp / (tp + fn + eps)
    accuracy = (tp + tn) / (tp + tn + fp + fn + eps)
    return (precision, recall, accuracy, F32(2) * (precision * recall) / (precision + recall + eps)), counts
