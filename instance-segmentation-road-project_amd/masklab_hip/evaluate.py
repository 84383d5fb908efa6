"""The reference's evaluation loop (road_project/train.py:94-212) on the deploy model's outputs: mean mask IoU per instance
label over the matched (prediction, ground truth) pairs and mean IoU per semantic label, the table the reference logs when
a checkpoint is trained.  Needs neither pandas nor cv2.

The predictions stay on the device.  Box matching (at most ~100 x G boxes per image) runs on the host in float64 as the
reference writes it; all pixel work -- ground-truth mask areas, the (intersection, union) of every matched pair, the
semantic counts -- runs in the integer counting kernels of csrc/evaluate.hip, which never build the reference's [n,H,W]
canvases.  The arithmetic contract is stated in include/masklab_hip.h ("Evaluation"); tests/evaluate_ref.py restates the
loop in NumPy and the results agree exactly.  Where the loop here differs from the reference on purpose:

  * a predicted box clipped to zero width or height is an EMPTY mask (the reference raises inside cv2.resize);
  * a matched pair whose union is empty adds IoU 0 (the reference adds NaN);
  * predicted masks are addressed by their detection row (the reference numbers only rows with conf >= 0, the same thing
    whenever padded rows come last, as TrimInstances leaves them);
  * OpenCV parity is unpinned: the resize is cv2.resize(INTER_LINEAR) restated from its source, not checked against a run.
"""
import numpy as np
import torch

CRACK_CLASS = 2          # train.py:206-208: the third semantic row is counted only for images that have instance labels


def match_boxes(pr_detection, gt_detection):
    """train.py:144-182 in float64: pr_detection [n,6], gt_detection [G,6] rows (cx, cy, w, h, label, conf) -> the
    (pr_i, gt_i) index arrays of np.where(iou * (labels equal) > 0.5), row-major.  NaN compares false; a predicted row with
    conf < 0 and a ground-truth row with label < 0 never pair."""
    pr = np.asarray(pr_detection, dtype=np.float64)
    gt = np.asarray(gt_detection, dtype=np.float64)
    gt_area = gt[:, 2] * gt[:, 3]
    pr_area = pr[:, 2] * pr[:, 3]
    areas = gt_area[None, :] + pr_area[:, None]
    gx1, gx2 = (gt[:, 0] - gt[:, 2] / 2)[None, :], (gt[:, 0] + gt[:, 2] / 2)[None, :]
    gy1, gy2 = (gt[:, 1] - gt[:, 3] / 2)[None, :], (gt[:, 1] + gt[:, 3] / 2)[None, :]
    px1, px2 = (pr[:, 0] - pr[:, 2] / 2)[:, None], (pr[:, 0] + pr[:, 2] / 2)[:, None]
    py1, py2 = (pr[:, 1] - pr[:, 3] / 2)[:, None], (pr[:, 1] + pr[:, 3] / 2)[:, None]
    in_width = np.maximum(0., np.minimum(gx2, px2) - np.maximum(gx1, px1))
    in_height = np.maximum(0., np.minimum(gy2, py2) - np.maximum(gy1, py1))
    intersection = in_width * in_height
    union = areas - intersection
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = intersection / union
        iou = iou * np.equal(gt[None, :, -2], pr[:, None, -2])
        hit = iou > 0.5
    hit &= (pr[:, -1] >= 0)[:, None] & (gt[:, -2] >= 0)[None, :]
    return np.where(hit)


class Evaluator:
    """Accumulates the reference's result table over batches.

    `instance_labels[k]` names detection class k, `semantic_labels[c]` channel c of the semantic map (the reference's
    config.dataset.instance_labels / semantic_labels)."""

    def __init__(self, instance_labels, semantic_labels, device="cuda"):
        self.instance_labels = list(instance_labels)
        self.semantic_labels = list(semantic_labels)
        names = self.instance_labels + self.semantic_labels
        if len(set(names)) != len(names):
            raise ValueError("Evaluator: every label needs a row of its own, got duplicates in " + repr(names))
        self.device = torch.device(device)
        self.table = {name: [0.0, 0.0] for name in names}          # label -> [iou, counts], float64 like the DataFrame

    def _device(self, a, dtypes, name):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype not in dtypes:
            raise TypeError(f"Evaluator.update: `{name}` must be one of {dtypes}, got {t.dtype}")
        t = t.to(self.device).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()           # a slice of a batch: the kernels load 16 bytes at a time

    @staticmethod
    def _pairs(det_host, gt_detection):
        """int32 [P,3] rows (b, pr_i, gt_i): every image's matches in order."""
        rows = [np.zeros((0, 3), np.int64)]
        for b in range(len(det_host)):
            p, g = match_boxes(det_host[b], gt_detection[b])
            rows.append(np.stack([np.full(len(p), b), p, g], axis=1))
        return np.concatenate(rows).astype(np.int32)

    def _counts(self, pr_detection, pr_instance, pr_semantic, gt_detection, gt_instance, gt_semantic):
        """-> host arrays: detections [B,n,6], pairs int32 [P,3], their (intersection, union) int64 [P,2], semantic counts
        int64 [B,C,2].  Three launch groups; the mask areas run while the host matches the boxes."""
        from . import ops
        det = self._device(pr_detection, (torch.int32,), "pr_detection")
        ins = self._device(pr_instance, (torch.int32,), "pr_instance")
        sem = self._device(pr_semantic, (torch.int32,), "pr_semantic")
        gt_sem = self._device(gt_semantic, (torch.uint8,), "gt_semantic")
        sem_counts = ops.eval_semantic_counts(sem, gt_sem)
        pairs, pair_counts = np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int64)
        det_host = det.cpu().numpy()
        if gt_instance.shape[1] > 0 and det.shape[1] > 0:
            gt_ins = self._device(gt_instance, (torch.int8, torch.uint8), "gt_instance")
            gt_area = ops.eval_mask_area(gt_ins)
            pairs = self._pairs(det_host, gt_detection)
            if len(pairs):
                pair_counts = ops.eval_mask_pairs(det, ins, gt_ins, gt_area, torch.from_numpy(pairs).to(self.device)).cpu().numpy()
        return det_host, pairs, pair_counts, sem_counts.cpu().numpy()

    def update(self, pr_detection, pr_instance, pr_semantic, gt_detection, gt_instance, gt_semantic):
        """One batch.  Predictions: the deploy model's outputs, device tensors or arrays -- [B,n,6] int32, [B,n,h,w] int32,
        [B,H,W,C] int32.  Ground truth in the reference dataset's layout: [B,G,6] float, [B,G,H,W] int8 or uint8,
        [B,H,W,C] uint8; masks and maps that are device tensors already (a MaskLabDataset batch) are not copied to the host."""
        on_device = isinstance(gt_instance, torch.Tensor) and gt_instance.is_cuda    # a MaskLabDataset batch: the masks stay there
        if not on_device:
            gt_instance = np.asarray(gt_instance)
        B = gt_instance.shape[0]
        if len(pr_detection) != B or len(pr_instance) != B or len(pr_semantic) != B or len(gt_detection) != B or len(gt_semantic) != B:
            raise ValueError("Evaluator.update: the batch sizes differ")
        if pr_semantic.shape[-1] > len(self.semantic_labels):
            raise ValueError(f"Evaluator.update: {pr_semantic.shape[-1]} semantic classes, {len(self.semantic_labels)} labels")
        # train.py:206, on the host array as stored (an int8 mask holds -1 where a 0 / 255 mask was set)
        if on_device:                                                                # the last column alone, B flags read back
            has_instances = (gt_instance[..., -1] != -1).reshape(B, -1).any(dim=1).cpu().tolist()
        else:
            has_instances = [bool(np.any(gt_instance[b][..., -1] != -1)) for b in range(B)]
        det_host, pairs, pair_counts, sem_counts = self._counts(pr_detection, pr_instance, pr_semantic, gt_detection, gt_instance,
                                                                gt_semantic)
        at = 0
        for b in range(B):
            while at < len(pairs) and pairs[at, 0] == b:
                inter, union = (int(v) for v in pair_counts[at])
                row = self.table[self.instance_labels[int(det_host[b, pairs[at, 1], -2])]]
                row[0] += inter / union if union > 0 else 0.0
                row[1] += 1
                at += 1
            for c in range(sem_counts.shape[1]):
                if c == CRACK_CLASS and not has_instances[b]:
                    continue
                row = self.table[self.semantic_labels[c]]
                row[0] += float(sem_counts[b, c, 0]) / (float(sem_counts[b, c, 1]) + 1e-7)
                row[1] += 1

    def result(self):
        """{label: {"iou", "counts", "miou" = iou / (counts + 1e-7)}}, the instance labels first."""
        return {name: {"iou": iou, "counts": counts, "miou": iou / (counts + 1e-7)} for name, (iou, counts) in self.table.items()}


def evaluate(model, dataset, batch_size=1):
    """The loop of train.py:101-209.  `model`: a DeployModel; `dataset`: anything with len() and slice indexing that returns
    the reference's dict with 'images', 'detection', 'semantic' and 'instance'.  The labels are
    model.configuration.dataset's, like the reference's.  -> Evaluator.result()."""
    labels = model.configuration.dataset
    ev = Evaluator(labels.instance_labels, labels.semantic_labels, device=model.model.device)
    for idx in range(len(dataset) // batch_size):
        targets = dataset[idx * batch_size:(idx + 1) * batch_size]
        pr_detections, pr_instances, pr_semantics = model(targets['images'])
        ev.update(pr_detections, pr_instances, pr_semantics, targets['detection'], targets['instance'], targets['semantic'])
    return ev.result()


def validate(trainer, generator, steps=None):
    """What `fit_generator(validation_data=generator)` reports for a trainer network (road_project/train.py:98-101: every
    output is a metric with aggregation 'mean', every output whose name contains 'loss' is also a loss by its mean).
    `trainer`: a TrainerModel (anything callable on the generator's dict that returns one [B] tensor per name of its
    `output_names`); `generator`: a MaskLabGenerator; `steps`: batches to run, None = len(generator).
    -> {"val_<name>": mean over all samples of all batches} plus "val_loss", the sum of the loss means.  The batches are
    equal-sized (the generator drops the remainder).  The sums accumulate in float64 on the device and are read once at the
    end; Keras keeps float32 running totals."""
    steps = len(generator) if steps is None else int(steps)
    if steps < 1 or steps > len(generator):
        raise ValueError(f"validate: {steps} steps asked of a generator of {len(generator)} batches")
    names = list(trainer.output_names)
    total, samples = None, 0
    for i in range(steps):
        outs = trainer(generator[i][0])
        if len(outs) != len(names):
            raise ValueError(f"validate: the trainer returned {len(outs)} outputs for {len(names)} names")
        batch = torch.stack([o.reshape(-1) for o in outs]).to(torch.float64)        # [names, B]
        total = batch.sum(dim=1) if total is None else total + batch.sum(dim=1)
        samples += batch.shape[1]
    means = (total / samples).cpu().numpy()
    result = {"val_" + n: float(m) for n, m in zip(names, means)}
    result["val_loss"] = float(sum(m for n, m in zip(names, means) if "loss" in n))
    return result
