"""Fixtures of the generator tests (test infrastructure, not collected), shared by the CPU and the GPU tests: the resize
shapes the issue names and a tiny in-memory dataset in the reference dataset's layout."""
import numpy as np

# (H, W) -> (oh, ow): down, exactly 2x on both axes (INTER_AREA), 2x on one axis only (linear), up, the identity, one
# source pixel, one destination pixel, odd sizes
RESIZE_SHAPES = [((45, 80), (32, 32)), ((64, 128), (32, 64)), ((64, 100), (32, 64)), ((5, 7), (13, 9)), ((9, 9), (9, 9)),
                 ((1, 1), (4, 4)), ((7, 5), (1, 1)), ((37, 53), (16, 24))]
AREA_SHAPE = ((64, 128), (32, 64))
CHANNELS = (1, 3, 4)


def random_bytes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


class TinyDataset:
    """`num` samples of H x W in the reference dataset's layout: full-range random bytes for the images and the first
    semantic channel, a 0 / 1 and a 0 / 255 semantic channel; instance masks int8 [num,n,H,W] -- per sample a 0 / 1 mask, a
    0 / 255 mask (0 / -1 as int8) whose first pixel is clear, a full-range one, and -1 planes as padding from `live[i]` on.
    Slicing returns COPIES (the reference generator scales the boxes it is handed in place)."""

    def __init__(self, num, H, W, n=4, live=(3, 1, 0, 4), seed=0, num_classes=5):
        rng = np.random.default_rng(seed)
        self.images = rng.integers(0, 256, (num, H, W, 3), dtype=np.uint8)
        self.semantic = np.stack([rng.integers(0, 256, (num, H, W), dtype=np.uint8),
                                  (rng.random((num, H, W)) < 0.5).astype(np.uint8),
                                  (rng.random((num, H, W)) < 0.5).astype(np.uint8) * 255], axis=-1)
        self.semantic_exist = rng.integers(0, 2, (num, 3)).astype(bool)
        self.instance_exist = rng.integers(0, 2, (num, num_classes)).astype(bool)
        self.instance = np.full((num, n, H, W), -1, np.int8)
        self.detection = np.full((num, n, 6), -1.0)
        for i in range(num):
            for j in range(min(n, live[i % len(live)])):
                kind = j % 3
                if kind == 0:
                    mask = (rng.random((H, W)) < 0.5).astype(np.uint8)
                elif kind == 1:
                    mask = (rng.random((H, W)) < 0.5).astype(np.uint8) * 255
                    mask[0, 0] = 0
                else:
                    mask = rng.integers(0, 255, (H, W), dtype=np.uint8)          # never 255 at [0, 0]: a live plane
                self.instance[i, j] = mask.view(np.int8)
                self.detection[i, j] = (rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1, W), rng.uniform(1, H),
                                        rng.integers(0, num_classes), 1.0)
        self.order = np.arange(num)
        self.rng = np.random.default_rng(seed + 1)

    def __len__(self):
        return len(self.order)

    def __getitem__(self, sl):
        idx = self.order[sl]
        return {"images": self.images[idx], "semantic": self.semantic[idx], "semantic_exist": self.semantic_exist[idx],
                "detection": self.detection[idx], "instance": self.instance[idx], "instance_exist": self.instance_exist[idx]}

    def shuffle(self):
        self.rng.shuffle(self.order)
