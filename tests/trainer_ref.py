"""NumPy restatement of the trainer network's forward tail (test infrastructure, not collected): the reference's
AssignBoxes (engine/layers/detection.py:589-697), AssignMasks (instance.py:296-386), AssignSeg (semantic.py:304-311) and
the four loss layers of engine/losses.py, written from the reference text.  Element arithmetic is float32, operation by
operation as TensorFlow evaluates the graph; reductions run in float64 and are rounded to float32 once.  The assignments are
written the LITERAL way -- the full [B,G,A] IoU matrix through oracle.metrics.calculate_iou, np.argwhere index lists in
tf.where's row-major order, a sequential update and np.add.at scatters -- so that the per-anchor rule the kernels follow is
checked against it rather than assumed."""
import numpy as np

from oracle import tfops
from oracle.metrics import calculate_iou, detection_iou_metric

F32 = np.float32
F64 = np.float64
EPS = F32(1e-7)                     # K.epsilon()


# ----------------------------------------------------------------------------- AssignBoxes
def iou_matrix(gt_boxes, pr_boxes):
    """detection.py:624-628 -> float32 [B,G,A]: CalculateIOU([gt rows, pr_boxes[0]]) times (gt cx != -1)."""
    gt = np.asarray(gt_boxes, F32)
    B, G, _ = gt.shape
    iou = calculate_iou(gt.reshape(-1, 6)[:, :4], np.asarray(pr_boxes, F32)).reshape(B, G, -1)
    return iou * (gt[..., 0] != -1).astype(F32)[..., None]


def match_indices(gt_boxes, iou):
    """detection.py:630-639 -> (best [B,G], match rows (b, g, a)): tf.where(iou >= 0.5) in row-major order, then the best
    prior of every ground truth with conf > 0, in (b, g) order."""
    gt = np.asarray(gt_boxes, F32)
    B, G, A = iou.shape
    match = np.argwhere(iou >= F32(0.5))
    best = iou.reshape(-1, A).argmax(axis=1)                        # the first maximum, as tf.argmax
    bs, gs = np.meshgrid(np.arange(B), np.arange(G), indexing="ij")
    best_rows = np.stack([bs.ravel(), gs.ravel(), best], axis=1)
    not_matched = np.flatnonzero(gt[..., 5].ravel() > 0)
    return best.reshape(B, G), np.concatenate([match, best_rows[not_matched]], axis=0)


def assign_boxes(gt_boxes, pr_boxes, num_classes):
    """AssignBoxes.call -> (best int64 [B,G], cls_true [B,A,C], loc_true [B,A,4], assign_mask [B,A,1])."""
    gt, pr = np.asarray(gt_boxes, F32), np.asarray(pr_boxes, F32)
    iou = iou_matrix(gt, pr)
    B, G, A = iou.shape
    best, match = match_indices(gt, iou)
    b_i, g_i, p_i = match[:, 0], match[:, 1], match[:, 2]
    cls = np.full((B, A), -1, F32)
    for k in range(len(match)):                                     # tensor_scatter_nd_update in index order: the last wins
        cls[b_i[k], p_i[k]] = gt[b_i[k], g_i[k], 4]
    cls = np.where(cls != -1, cls, F32(num_classes))
    one_hot = (cls.astype(np.int32)[..., None] == np.arange(num_classes + 1)).astype(F32)
    assign_mask = one_hot[..., -1].copy()
    ignore = np.argwhere((iou < F32(0.5)) & (iou >= F32(0.4)))
    ignore_mask = np.zeros((B, A), np.int64)
    np.add.at(ignore_mask, (ignore[:, 0], ignore[:, 2]), 1)
    assign_mask = np.where(ignore_mask > 0, F32(-1), assign_mask)
    p, g = pr[p_i], gt[b_i, g_i, :4]
    hats = [(g[:, 0] - p[:, 0]) / p[:, 2], (g[:, 1] - p[:, 1]) / p[:, 3], np.log(g[:, 2] / p[:, 2]), np.log(g[:, 3] / p[:, 3])]
    loc = np.zeros((4, B, A), F32)
    for q in range(4):                                              # tf.scatter_nd ADDS duplicates, in index order
        np.add.at(loc[q], (b_i, p_i), hats[q].astype(F32))
    return best, one_hot[..., :num_classes], np.ascontiguousarray(loc.transpose(1, 2, 0)), assign_mask[..., None]


# ----------------------------------------------------------------------------- ClassLoss, BoxLoss
def split_masks(mask):
    m = np.asarray(mask, F32).reshape(mask.shape[0], -1)
    return (m == 1).astype(F32), (m == 0).astype(F32), (m != -1).astype(F32)          # neg, pos, not ignored


def focal_loss(y_true, y_pred, gamma, alpha):
    y_pred = np.clip(y_pred, EPS, F32(1) - EPS)
    pt = np.where(y_true == 1, y_pred, F32(1) - y_pred)
    return F32(alpha) * (-np.power(F32(1) - pt, F32(gamma)) * np.log(pt))


def class_loss(cls_true, cls_pred, mask, cls_exists, weight=1., alpha=.25, gamma=2.):
    """ClassLoss.call -> float32 [B]."""
    neg, pos, keep = split_masks(mask)
    t = (np.asarray(cls_true, F32) != 0).astype(F32)
    loss = focal_loss(t, np.asarray(cls_pred, F32), gamma, alpha) * np.asarray(cls_exists, F32)[:, None, :]
    loss = keep[..., None] * loss
    num_tot = (pos + neg).sum(axis=1, dtype=F64)
    return F32(weight) * (loss.sum(axis=(1, 2), dtype=F64) / (num_tot + F64(EPS))).astype(F32)


class BoxLoss:
    """BoxLoss with its two moving vectors; every call updates them when use_adjust."""

    def __init__(self, weight=1., momentum=0.9, beta=.11, use_adjust=False):
        self.weight, self.momentum, self.beta, self.use_adjust = weight, momentum, beta, use_adjust
        self.moving_mean = np.full(4, beta, F32)
        self.moving_var = np.zeros(4, F32)

    def __call__(self, loc_true, loc_pred, mask):
        loc_true, loc_pred = np.asarray(loc_true, F32), np.asarray(loc_pred, F32)
        _, pos, _ = split_masks(mask)
        if self.use_adjust:
            n = F64(pos.size)
            offsets = np.abs(loc_true - loc_pred) * pos[..., None]
            mean = (offsets.sum(axis=(0, 1), dtype=F64) / n).astype(F32)
            dev = offsets - mean
            var = ((dev * dev).sum(axis=(0, 1), dtype=F64) / n).astype(F32)
            self.moving_mean = self.moving_mean * F32(self.momentum) + mean * F32(1 - self.momentum)
            self.moving_var = self.moving_var * F32(self.momentum) + var * F32(1 - self.momentum)
            beta = np.clip(self.moving_mean - self.moving_var, F32(1e-3), F32(self.beta))
        else:
            beta = F32(self.beta)
        d = loc_true - loc_pred
        l1 = np.abs(d) - F32(0.5) * beta
        l2 = F32(0.5) * (d * d) / beta
        loss = np.where(l1 < beta, l2, l1)                           # the comparison as written
        loss = (((loss[..., 0] + loss[..., 1]) + loss[..., 2]) + loss[..., 3]) / F32(4)
        num_pos = pos.sum(axis=1, dtype=F64)
        return F32(self.weight) * ((pos * loss).sum(axis=1, dtype=F64) / (num_pos + F64(EPS))).astype(F32)


# ----------------------------------------------------------------------------- AssignMasks, MaskLoss
def normalize_boxes(boxes, H, W):
    cx, cy, w, h = (np.asarray(boxes, F32)[:, k] for k in range(4))
    return np.stack([(cy - h / F32(2)) / F32(H), (cx - w / F32(2)) / F32(W), (cy + h / F32(2)) / F32(H),
                     (cx + w / F32(2)) / F32(W)], axis=1)


def match_rois(roi_boxes, gt_boxes, threshold=0.5):
    """instance.py:343-362 for one image -> (matched bool [R], gt index [R])."""
    roi, gt = np.asarray(roi_boxes, F32), np.asarray(gt_boxes, F32)
    iou = calculate_iou(gt[:, :4], roi[:, :4])
    live = ((gt[:, None, 5] != -1) & (roi[None, :, 5] != -1)).astype(F32)
    same = (gt[:, None, 4] == roi[None, :, 4]).astype(F32)
    iou = iou * live * same
    return iou.max(axis=0) >= F32(threshold), iou.argmax(axis=0)


def assign_masks(roi_boxes, gt_boxes, gt_masks, crop_hw, num_classes, threshold=0.5, dtype=F32):
    """AssignMasks.call -> (int32 [B,R,h,w], the crop samples [B,R,h,w] in `dtype`, matched bool [B,R])."""
    B, R = roi_boxes.shape[:2]
    H, W = gt_masks.shape[2:]
    out = np.empty((B, R) + tuple(crop_hw), np.int32)
    samples = np.empty((B, R) + tuple(crop_hw), dtype)
    matched = np.empty((B, R), bool)
    for b in range(B):
        matched[b], gi = match_rois(roi_boxes[b], gt_boxes[b], threshold)
        cls = np.where(matched[b], np.asarray(gt_boxes[b], F32)[gi, 4], F32(num_classes))
        samples[b] = tfops.crop_and_resize(gt_masks[b].astype(dtype)[..., None], normalize_boxes(roi_boxes[b], H, W), gi,
                                           tuple(crop_hw))[..., 0]
        out[b] = np.where(samples[b] > 0.5, cls[:, None, None], F32(num_classes)).astype(np.int32)
    return out, samples, matched


def binary_cross_entropy(y_true, y_pred, label_smoothing):
    y_true = F32(1 - label_smoothing) * y_true + F32(label_smoothing / 2.)
    return -(y_true * np.log(y_pred + EPS) + (F32(1) - y_true) * np.log(F32(1) - y_pred + EPS))


def mask_loss(mask_true, mask_pred, weight=1., label_smoothing=0.):
    """MaskLoss.call -> float32 [B]."""
    mask_pred = np.asarray(mask_pred, F32)
    B, R, h, w, C = mask_pred.shape
    classes = mask_true.min(axis=(2, 3))
    out = np.zeros(B, F32)
    for b in range(B):
        losses = []
        for r in np.flatnonzero(classes[b] < C):
            c = classes[b, r]
            loss = binary_cross_entropy((mask_true[b, r] == c).astype(F32), mask_pred[b, r, :, :, c], label_smoothing)
            losses.append(F32(loss.sum(dtype=F64) / (h * w)))
        losses = np.asarray(losses, F32)
        out[b] = F32(weight) * F32(losses.sum(dtype=F64) / (np.count_nonzero(losses) + 1))
    return out


# ----------------------------------------------------------------------------- AssignSeg, SegLoss
def assign_seg(gt_seg, out_hw, dtype=F32):
    """AssignSeg.call -> (rounded half to even [B,oh,ow,C], the resized samples before rounding)."""
    resized = tfops.resize_bilinear_align_corners(np.asarray(gt_seg).astype(dtype), int(out_hw[0]), int(out_hw[1]))
    return np.rint(resized), resized


def seg_loss(seg_true, seg_pred, seg_exist, weight=1., label_smoothing=0.):
    """SegLoss.call -> float32 [B]."""
    seg_true, seg_pred = np.asarray(seg_true, F32), np.asarray(seg_pred, F32)
    B, H, W, C = seg_pred.shape
    loss = binary_cross_entropy(seg_true, seg_pred, label_smoothing)
    loss = (loss.sum(axis=(1, 2), dtype=F64) / (H * W)).astype(F32)
    loss = np.asarray(seg_exist).astype(F32) * loss
    return F32(weight) * (loss.sum(axis=1, dtype=F64) / C).astype(F32)


# ----------------------------------------------------------------------------- the model's tail
def trainer_tail(cfg, inputs, fw, box_loss):
    """The trainer network from the predictions on: `fw` holds cls_pred, loc_pred, pr_boxes [A,4], proposed, roi_boxes,
    roi_masks and seg_pred (NumPy), `box_loss` a BoxLoss above in the state the device layer was in before the call.
    -> {output name: float32 [B]} plus the intermediate targets."""
    import evaluate_ref
    c = cfg.loss
    C = len(cfg.dataset.instance_labels)
    gt_boxes = np.asarray(inputs["gt_boxes"], F32)
    best, cls_true, loc_true, assign_mask = assign_boxes(gt_boxes, fw["pr_boxes"], C)
    out = {"class_loss": class_loss(cls_true, fw["cls_pred"], assign_mask, inputs["gt_boxes_exist"], c.cls_loss_weight, c.cls_loss_alpha,
                                    c.cls_loss_gamma),
           "box_loss": box_loss(loc_true, fw["loc_pred"], assign_mask)}
    names = ("detection_precision_metric", "detection_recall_metric", "detection_fmeasure_metric")
    out.update(zip(names, detection_iou_metric(fw["proposed"], gt_boxes)))
    match, _, _ = assign_masks(fw["roi_boxes"], gt_boxes, inputs["gt_masks"], fw["roi_masks"].shape[2:4], C)
    out["mask_loss"] = mask_loss(match, fw["roi_masks"], c.mask_loss_weight, c.mask_loss_label_smoothing)
    seg_assigned, _ = assign_seg(inputs["gt_seg"], fw["seg_pred"].shape[1:3])
    out["seg_loss"] = seg_loss(seg_assigned, fw["seg_pred"], inputs["gt_seg_exist"], c.seg_loss_weight, c.seg_loss_label_smoothing)
    out.update(zip(("other_road_iou_metric", "my_road_metric", "crack_iou_metric"),
                   evaluate_ref.class_binary_iou(seg_assigned, fw["seg_pred"])))
    targets = dict(best_prior=best, cls_true=cls_true, loc_true=loc_true, assign_mask=assign_mask, match_gt_masks=match,
                   seg_assigned=seg_assigned)
    return out, targets
