"""The inputs the evaluation tests share (test infrastructure, not collected): one 97 x 131 batch whose boxes take every
path of the pasted-mask arithmetic, its ground truth, the box-matching cases and a two-image toy dataset."""
import numpy as np

from masklab_hip.evaluate import Evaluator

H, W = 97, 131
INSTANCE_LABELS = ['car', 'bump', 'manhole', 'steel', 'pothole']
SEMANTIC_LABELS = ['other_road', 'my_road', 'crack']

# (cx, cy, w, h, label, conf): what each row is there for
BOXES = [
    (60, 40, 30, 20, 0, 90),       # inside the image
    (5, 50, 30, 24, 1, 80),        # clipped at the left border
    (125, 50, 30, 24, 1, 80),      # ... right
    (60, 4, 26, 20, 2, 70),        # ... top
    (60, 92, 26, 21, 2, 70),       # ... bottom
    (65, 48, 200, 200, 3, 60),     # covers the whole image
    (40, 30, 9, 5, 4, 60),         # smaller than the mask
    (50, 60, 14, 14, 0, 50),       # exactly 14 x 14: from a 28 x 28 mask every sample is a mean of 2 x 2 entries
    (70, 50, 56, 56, 0, 50),       # 56 x 56
    (30, 30, 0, 10, 1, 40),        # w = 0: an empty mask
    (20, 70, 1, 1, 1, 40),         # a single pixel
    (-1, -1, -1, -1, -1, -1),      # a padded row
]
HALF_ROW = 7                       # its 28 x 28 mask is striped: every 2 x 2 mean is exactly 0.5 and must not count


def predictions(size, seed=0):
    """-> det int32 [2,12,6], ins int32 [2,12,size,size]: image 0 holds BOXES, image 1 no detection at all."""
    rng = np.random.default_rng(seed + size)
    det = np.full((2, len(BOXES), 6), -1, np.int32)
    det[0] = np.asarray(BOXES, np.int32)
    coarse = rng.integers(0, 2, (2, len(BOXES), size // 7, size // 7))
    ins = np.kron(coarse, np.ones((7, 7), np.int64)).astype(np.int32)          # blobs, so that resizes keep something
    ins ^= (rng.random(ins.shape) < 0.1).astype(np.int32)                       # and single-pixel noise
    ins[0, 0, :2] = -1                                                          # negatives are clamped to 0
    ins[0, HALF_ROW] = np.arange(size)[None, :] % 2                             # vertical stripes
    ins[0, 10] = 1
    return det, ins


def ground_truth(seed=1):
    """-> gt_det float64 [2,3,6], gt_ins int8 [2,3,H,W], gt_sem uint8 [2,H,W,3].  Slot 0: a 0 / 255 uint8 mask cast to
    int8 (set pixels are -1); slot 1: empty; slot 2: the padding slot, filled with -1.  Image 1: only padding slots."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    blob = (((yy - 45) / 30.0) ** 2 + ((xx - 62) / 50.0) ** 2 < 1).astype(np.uint8) * 255
    gt_ins = np.full((2, 3, H, W), -1, np.int8)
    gt_ins[0, 0] = blob.astype(np.int8)
    gt_ins[0, 1] = 0
    gt_det = np.full((2, 3, 6), -1.0)
    gt_det[0, 0] = (66, 48, 70, 60, 0, 1)
    gt_det[0, 1] = (60, 5, 26, 20, 2, 1)
    gt_sem = (rng.random((2, H, W, 3)) < 0.4).astype(np.uint8) * np.array([1, 255, 1], np.uint8)
    return gt_det, gt_ins, gt_sem


def semantic_prediction(shape, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < 0.5).astype(np.int32)


def all_pairs(B, n, G):
    """every (b, pr_i, gt_i) and five rows with one index out of range"""
    inside = [(b, i, g) for b in range(B) for i in range(n) for g in range(G)]
    return np.asarray(inside + [(B, 0, 0), (0, n, 0), (0, 0, G), (-1, 0, 0), (0, -1, 0)], np.int32)


# ----------------------------------------------------------------------------- box matching: (pr rows, gt rows, pairs)
MATCHING = {
    "same box, same label": ([(50, 50, 20, 20, 1, 90)], [(50, 50, 20, 20, 1, 1)], [(0, 0)]),
    "class mismatch": ([(50, 50, 20, 20, 1, 90)], [(50, 50, 20, 20, 2, 1)], []),
    "IoU exactly 0.5": ([(10, 10, 20, 10, 1, 90)], [(10, 10, 10, 10, 1, 1)], []),
    "IoU just above 0.5": ([(10, 10, 19, 10, 1, 90)], [(10, 10, 10, 10, 1, 1)], [(0, 0)]),
    "padded predicted row": ([(50, 50, 20, 20, 1, 90), (-1,) * 6], [(50, 50, 20, 20, 1, 1), (-1,) * 6], [(0, 0)]),
    "padded row with a real box": ([(50, 50, 20, 20, 1, -1)], [(50, 50, 20, 20, 1, 1)], []),
    "ground truth without a label": ([(50, 50, 20, 20, -1, 90)], [(50, 50, 20, 20, -1, 1)], []),
    "zero detections": ([(-1,) * 6], [(50, 50, 20, 20, 1, 1)], []),
    "NaN: two empty boxes": ([(50, 50, 0, 0, 1, 90), (30, 30, 10, 10, 0, 90)], [(50, 50, 0, 0, 1, 1), (30, 30, 10, 10, 0, 1)], [(1, 1)]),
    "row-major order": ([(30, 30, 10, 10, 0, 90), (30, 30, 10, 10, 0, 80)], [(30, 31, 10, 10, 0, 1), (30, 30, 10, 10, 0, 1)],
                        [(0, 0), (0, 1), (1, 0), (1, 1)]),
}


class ToyDataset:
    """The slice protocol of the reference's dataset over NumPy arrays."""

    def __init__(self, images, detection, instance, semantic):
        self.arrays = {"images": images, "detection": detection, "instance": instance, "semantic": semantic}

    def __len__(self):
        return len(self.arrays["images"])

    def __getitem__(self, item):
        return {k: v[item] for k, v in self.arrays.items()}


class HostReferenceEvaluator(Evaluator):
    """The product's table with the counts from ml_eval_reference_host -- the kernels' per-thread code in CPU loops over
    NumPy arrays -- in place of the launches: what the CPU tests can run."""

    def _counts(self, pr_detection, pr_instance, pr_semantic, gt_detection, gt_instance, gt_semantic):
        from masklab_hip import ops
        det_host = np.asarray(pr_detection)
        pairs, pair_counts = np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int64)
        if gt_instance.shape[1] > 0 and det_host.shape[1] > 0:
            pairs = self._pairs(det_host, gt_detection)
            if len(pairs):
                pair_counts = ops.eval_reference_host(det=det_host, ins=pr_instance, gt=gt_instance, pairs=pairs)[1]
        return det_host, pairs, pair_counts, ops.eval_reference_host(pr_sem=pr_semantic, gt_sem=gt_semantic)[2]
