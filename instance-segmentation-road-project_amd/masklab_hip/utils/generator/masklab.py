"""The reference's `MaskLabGenerator` (engine/utils/generator/masklab.py): one scale per batch, every image, semantic map
and instance mask through `cv2.resize(x, (target_w, target_h))`, the boxes scaled -> the dict of six arrays the trainer
network takes.  The three resizes run on the device, one launch per kind per batch (csrc/cv_resize.hip); neither cv2 nor a
float64 copy of the semantic maps is needed.

OpenCV parity is unpinned: the kernels restate cv2.resize from OpenCV's source (include/masklab_hip.h, "Generator resizes")
and are held to the NumPy restatement in tests/generator_ref.py, not to a run of OpenCV.  Where the generator differs from
the reference on purpose:

  * `images`, `gt_seg` and `gt_masks` are torch tensors on `device`; `gt_seg` is float32 (or uint8 with
    `seg_dtype=torch.uint8`) where the reference returns float64 -- the values are integers in 0..255 either way;
  * the boxes are scaled on a float64 COPY; the reference scales the dataset's own array in place;
  * a dict for `dataset` (from which the reference builds its MaskLabDataset) raises NotImplementedError: build the
    `masklab_hip.utils.MaskLabDataset` yourself and pass the object; a target size of zero raises ValueError (the
    reference fails inside cv2.resize);
  * `rng` (a np.random.Generator) draws the scale; None is the global np.random, as in the reference;
  * `device="cpu"` runs the library's host reference loops: slow, for machines without a GPU.
"""
import numpy as np
import torch


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class MaskLabGenerator:
    """`engine.utils.MaskLabGenerator(dataset, scale_ratio, batch_size, shuffle)` plus `device`, `rng` and `seg_dtype`.

    `dataset`: anything with len(), slice indexing that returns the reference dataset's dict ('images' uint8 [B,H,W,3],
    'semantic' uint8 [B,H,W,S], 'semantic_exist' [B,S], 'detection' [B,n,6], 'instance' int8 [B,n,H,W] with -1 planes as
    padding, 'instance_exist' [B,K]) and shuffle().  The arrays may be NumPy arrays or torch tensors already on the device."""

    def __init__(self, dataset, scale_ratio=(0.4, 0.6), batch_size=8, shuffle=True, device="cuda", rng=None,
                 seg_dtype=torch.float32):
        if isinstance(dataset, dict):
            raise NotImplementedError("MaskLabGenerator: building a MaskLabDataset from a dict needs the reference's file reading "
                                      "(cv2, pandas), which is out of scope: pass a dataset object")
        if not (hasattr(dataset, "__len__") and hasattr(dataset, "__getitem__") and hasattr(dataset, "shuffle")):
            raise ValueError("MaskLabGenerator: `dataset` must be a dataset object with len(), slice indexing and shuffle()")
        if seg_dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"MaskLabGenerator: seg_dtype must be torch.float32 or torch.uint8, got {seg_dtype}")
        self.dataset = dataset
        self.scale_ratio = scale_ratio
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.device = torch.device(device)
        self.rng = rng
        self.seg_dtype = seg_dtype
        self.on_epoch_end()

    def __len__(self):
        return len(self.dataset) // self.batch_size

    def on_epoch_end(self):
        if self.shuffle:
            self.dataset.shuffle()

    # ---- the three resizes
    def _bytes(self, a, dtype, name):
        """-> `a` as a contiguous tensor on self.device, or (host path) as a contiguous array, of torch dtype `dtype`."""
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if a.dtype != dtype or a.dim() != 4:
            raise TypeError(f"MaskLabGenerator: `{name}` must be a 4-d {dtype} array, got {a.dtype} {tuple(a.shape)}")
        return a.cpu().contiguous().numpy() if self.device.type == "cpu" else a.to(self.device).contiguous()

    def _resize(self, images, semantic, masks, th, tw):
        from ... import ops
        if self.device.type == "cpu":
            seg_mode = "round_f32" if self.seg_dtype == torch.float32 else "round_u8"
            out = (ops.cv_resize_reference_host(images, th, tw), ops.cv_resize_reference_host(semantic, th, tw, mode=seg_mode),
                   ops.cv_resize_reference_host(masks, th, tw, skip_minus_one=True))
            return tuple(torch.from_numpy(a) for a in out)
        return (ops.cv_resize_linear(images, th, tw), ops.cv_resize_linear_round(semantic, th, tw, dtype=self.seg_dtype),
                ops.cv_resize_linear(masks, th, tw, skip_minus_one=True))

    def __getitem__(self, index):
        data = self.dataset[self.batch_size * index:self.batch_size * (index + 1)]
        images = self._bytes(data['images'], torch.uint8, 'images')
        semantic = self._bytes(data['semantic'], torch.uint8, 'semantic')
        masks = self._bytes(data['instance'], torch.int8, 'instance')
        gt_seg_exist = _host(data['semantic_exist']).astype(np.float64)
        gt_boxes_exist = _host(data['instance_exist']).astype(np.float64)
        gt_boxes = np.array(_host(data['detection']), dtype=np.float64)          # a copy: the dataset's rows stay as they are

        if isinstance(self.scale_ratio, (tuple, list)):
            scale_ratio = (self.rng if self.rng is not None else np.random).uniform(*self.scale_ratio)
        else:
            scale_ratio = self.scale_ratio
        height, width = (int(v) for v in images.shape[1:3])
        if tuple(semantic.shape[:3]) != tuple(images.shape[:3]) or masks.shape[0] != images.shape[0] \
                or tuple(masks.shape[2:]) != (height, width):
            raise ValueError(f"MaskLabGenerator: images {tuple(images.shape)}, semantic {tuple(semantic.shape)} and instance "
                             f"{tuple(masks.shape)} do not fit")
        target_h = int(height * scale_ratio) // 32 * 32
        target_w = int(width * scale_ratio) // 32 * 32
        if target_h <= 0 or target_w <= 0:
            raise ValueError(f"MaskLabGenerator: scale {scale_ratio} of {height} x {width} gives the target size {target_h} x "
                             f"{target_w} (sizes are cut to multiples of 32)")

        batch_images, batch_seg, batch_masks = self._resize(images, semantic, masks, target_h, target_w)

        live = gt_boxes[..., 5] > 0                                              # padding rows keep their -1
        gt_boxes[live, :4] *= np.array([target_w / width, target_h / height, target_w / width, target_h / height])
        return ({"images": batch_images, "gt_seg": batch_seg, "gt_seg_exist": gt_seg_exist, "gt_boxes": gt_boxes,
                 "gt_boxes_exist": gt_boxes_exist, "gt_masks": batch_masks},)
