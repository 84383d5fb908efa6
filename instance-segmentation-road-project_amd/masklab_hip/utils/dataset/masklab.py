"""The reference's `MaskLabDataset` (engine/utils/dataset/masklab.py) fed from the `images/` and `labels/` folders alone:
the polygon labels are drawn per batch straight into device tensors (csrc/polygon.hip: one launch for the instance planes,
one for the semantic maps), where the reference draws every polygon once with skimage.draw.polygon into a `processed/`
tree of PNGs (road_project/setup/process.py) and reads them back with cv2 and pandas.  No cv2, skimage or pandas and no
`processed/` tree is needed.

skimage parity is unpinned: the polygon rule is the one of include/masklab_hip.h ("Dataset polygons"), held to its NumPy
restatement in tests/polygon_ref.py and not to a run of skimage.  What is kept from the reference, and where this differs:

  * the batch dict of a slice: `images` uint8 [B,H,W,3] RGB, `semantic` uint8 [B,H,W,S] of 0 / 1 and `instance` int8
    [B,n,H,W] (padding planes -1) are torch tensors on `device`; `detection` float64 [B,n,6] (rows cx, cy, w, h, label
    index, 1.0; padding -1), `semantic_exist` [B,S] and `instance_exist` [B,K] float64 are NumPy.  n is the largest
    instance count of the batch and may be 0 (the reference fails on a batch without instances).
  * instances are the annotations whose label is in `instance_labels` with w * h > min_area, in the fixed order of
    load_labels (folders, files, file order: the reference's order depends on os.listdir and an unstable sort).
  * an instance plane is its polygon inside the reference's window: int() truncation of (cx - w/2, cy - h/2, cx + w/2,
    cy + h/2), then max(., 0).  The reference crops that window into a PNG and pastes it back through cv2.resize to the
    shape of the very slice it was cut from: the resize is always the identity.
  * a semantic channel is the union of its label's polygons (w * h > 0; min_area plays no part) minus the union of the
    polygons of `except_semantic_labels`.
  * an image the label table does not know gets zero exist flags ([S] / [K] zeros; the reference returns a single 0. for
    a single sample); a label without a folder counts as never listed.
  * an int or str index returns one sample: `instance` uint8 [k,H,W] without padding, `detection` [k,6].
  * a baseline JPEG is decoded on the device (ops.decode_jpeg, libjpeg's bytes); anything else, and everything with
    device="cpu", goes through Pillow.  Images of different sizes in one batch raise ValueError (the reference resizes the
    images and then fails in its instance paste).  An instance polygon without vertices raises ValueError.
  * device="cpu" draws with the library's host loops and returns CPU tensors: slow, for machines without a GPU.
  * `rng` (a np.random.Generator) shuffles the cases; None is the global np.random, as in the reference."""
import glob
import os

import numpy as np
import torch

from .dataset import Dataset
from .labels import load_labels

_INT32 = 2 ** 31 - 1


class MaskLabDataset(Dataset):
    def __init__(self, cases=None, instance_labels=('car', 'bump', 'manhole', 'steel', 'pothole'),
                 semantic_labels=('other_road', 'my_road', 'crack'), data_dir="./datasets/", min_area=1000.,
                 except_semantic_labels=('car',), device="cuda", rng=None, **kwargs):
        super().__init__()
        self.data_dir = data_dir
        self.image_dir = os.path.join(data_dir, "images/")
        self.label_dir = os.path.join(data_dir, "labels/")
        self.cases = np.array(sorted(get_image_cases(self.image_dir)) if cases is None else cases)
        self.instance_labels = instance_labels
        self.semantic_labels = semantic_labels
        self.except_semantic_labels = except_semantic_labels
        self.min_area = min_area
        self.device = torch.device(device)
        self.rng = rng
        from ... import _lib
        if len(semantic_labels) > _lib.EVAL_MAX_CLASSES:
            raise ValueError(f"MaskLabDataset: {len(semantic_labels)} semantic labels, at most {_lib.EVAL_MAX_CLASSES}")

        self.label_exists, self.annotations = load_labels(self.label_dir)
        # per image: its instances (cx, cy, w, h, label index, polygon) and its polygons per semantic group (S labels + except)
        self._instances, self._groups = {}, {}
        S = len(semantic_labels)
        for a in self.annotations:
            name, label = a["file_name"], a["label"]
            if label in instance_labels and a["w"] * a["h"] > min_area:
                self._instances.setdefault(name, []).append(
                    (a["cx"], a["cy"], a["w"], a["h"], float(list(instance_labels).index(label)), a["annotation"]))
            groups = [s for s, l in enumerate(semantic_labels) if l == label] + ([S] if label in except_semantic_labels else [])
            for g in groups:
                self._groups.setdefault(name, [[] for _ in range(S + 1)])[g].append(a["annotation"])
        self.config = {"cases": list(self.cases), "instance_labels": instance_labels, "semantic_labels": semantic_labels,
                       "data_dir": data_dir, "min_area": min_area}
        self.config.update(kwargs)

    def __len__(self):
        return len(self.cases)

    def shuffle(self):
        (self.rng if self.rng is not None else np.random).shuffle(self.cases)

    def get_config(self):
        return self.config

    # ---- the tables
    def _exist(self, case_name, labels):
        row = self.label_exists["files"].get(case_name)
        return np.array([0.0 if row is None else row.get(label, 0.0) for label in labels], np.float64)

    def get_semantic_exist(self, case_name):
        return self._exist(case_name, self.semantic_labels)

    def get_instance_exist(self, case_name):
        return self._exist(case_name, self.instance_labels)

    def get_detection(self, case_name):
        rows = [inst[:5] + (1.0,) for inst in self._instances.get(case_name, [])]
        return np.array(rows, np.float64).reshape(len(rows), 6)

    # ---- the images
    def _read_images(self, cases):
        """-> uint8 [B,H,W,3] RGB on self.device."""
        paths = [os.path.join(self.image_dir, str(c)) for c in cases]
        frames, by_mode = [None] * len(paths), {}
        if self.device.type == "cuda":
            from ... import ops
            for i, path in enumerate(paths):
                if os.path.splitext(path)[1].lower() not in (".jpg", ".jpeg"):
                    continue
                with open(path, "rb") as f:
                    content = f.read()
                try:
                    info = ops.jpeg_info(content)
                except ops.UnsupportedJpeg:
                    continue                                                    # progressive, 4:2:2, ...: Pillow
                by_mode.setdefault(info[:3], []).append((i, content))
            for items in by_mode.values():
                for at in range(0, len(items), 32):
                    chunk = items[at:at + 32]
                    decoded = ops.decode_jpeg([c for _, c in chunk], self.device)
                    for (i, _), frame in zip(chunk, decoded):
                        frames[i] = frame
        for i, path in enumerate(paths):
            if frames[i] is None:
                frames[i] = torch.from_numpy(_read_with_pillow(path)).to(self.device)
        sizes = {tuple(f.shape) for f in frames}
        if len(sizes) > 1:
            raise ValueError(f"MaskLabDataset: the images of one batch must have one size, got {sorted(sizes)} for {list(cases)}")
        return torch.stack(frames)

    # ---- the masks
    def _windows(self, instances):
        out = []
        for cx, cy, w, h, _, _ in instances:
            box = (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)
            out.append([min(max(int(v), 0), _INT32) for v in box])
        return out

    def _draw(self, cases, H, W, n):
        """-> (instance int8 [B,n,H,W], semantic uint8 [B,H,W,S]) on self.device."""
        from ... import ops
        B, S = len(cases), len(self.semantic_labels)
        planes, windows = [], []
        for case in cases:
            instances = self._instances.get(str(case), [])
            for inst in instances:
                if len(inst[5]) == 0:
                    raise ValueError(f"MaskLabDataset: an instance of {case} has a polygon without vertices")
            planes += [inst[5] for inst in instances] + [np.zeros((0, 2))] * (n - len(instances))
            windows += self._windows(instances) + [[0, 0, 0, 0]] * (n - len(instances))
        verts, plane_offsets = _pack(planes)
        windows = np.array(windows, np.int32).reshape(B * n, 4)
        polys, group_offsets = [], [0]
        for case in cases:
            for group in self._groups.get(str(case), [[]] * (S + 1)):
                polys += group
                group_offsets.append(len(polys))
        sem_verts, poly_offsets = _pack(polys)
        group_offsets = np.array(group_offsets, np.int32)
        if self.device.type == "cpu":
            instance = ops.polygon_reference_host("instance", verts, plane_offsets, B, n, H, W, windows=windows)
            semantic = ops.polygon_reference_host("semantic", sem_verts, poly_offsets, B, S, H, W, group_offsets=group_offsets)
            return torch.from_numpy(instance), torch.from_numpy(semantic)
        return (ops.polygon_instance_masks(verts, plane_offsets, windows, B, n, H, W, device=self.device),
                ops.polygon_semantic_maps(sem_verts, poly_offsets, group_offsets, B, S, H, W, device=self.device))

    def __getitem__(self, index):
        if isinstance(index, (int, np.integer, str)):
            case_name = str(self.cases[index]) if not isinstance(index, str) else index
            images = self._read_images([case_name])
            H, W = (int(v) for v in images.shape[1:3])
            detection = self.get_detection(case_name)
            instance, semantic = self._draw([case_name], H, W, len(detection))
            return {"images": images[0], "semantic": semantic[0], "semantic_exist": self.get_semantic_exist(case_name),
                    "detection": detection, "instance": instance[0].view(torch.uint8),
                    "instance_exist": self.get_instance_exist(case_name)}
        cases = [str(c) for c in np.atleast_1d(self.cases[index])]
        if not cases:
            raise ValueError(f"MaskLabDataset: the index {index} selects no case")
        images = self._read_images(cases)
        H, W = (int(v) for v in images.shape[1:3])
        detections = [self.get_detection(c) for c in cases]
        n = max(len(d) for d in detections)
        detection = np.full((len(cases), n, 6), -1.0)
        for i, d in enumerate(detections):
            detection[i, :len(d)] = d
        instance, semantic = self._draw(cases, H, W, n)
        return {"images": images, "semantic": semantic,
                "semantic_exist": np.stack([self.get_semantic_exist(c) for c in cases]).reshape(len(cases), len(self.semantic_labels)),
                "detection": detection, "instance": instance,
                "instance_exist": np.stack([self.get_instance_exist(c) for c in cases]).reshape(len(cases), len(self.instance_labels))}


def _pack(polys):
    """A list of float64 [V,2] -> (verts [total,2], offsets int32 [len + 1])."""
    offsets = np.zeros(len(polys) + 1, np.int64)
    if polys:
        offsets[1:] = np.cumsum([len(p) for p in polys])
    if offsets[-1] > _INT32:
        raise ValueError(f"MaskLabDataset: {offsets[-1]} vertices in one batch")
    verts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in polys]) if polys else np.zeros((0, 2))
    return np.ascontiguousarray(verts, np.float64), offsets.astype(np.int32)


def _read_with_pillow(path):
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError(f"MaskLabDataset: reading {path} on the host needs Pillow (only baseline JPEGs are decoded on the "
                          f"device)") from e
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), np.uint8)                      # a writable copy


def get_image_cases(image_dir):
    """The file names (without their folders) of every .jpg / .jpeg / .png under `image_dir`, in glob's order."""
    file_paths = glob.glob(os.path.join(image_dir, "**/*"), recursive=True)
    image_formats = (".jpg", ".jpeg", ".png")
    return [os.path.split(p)[1] for p in file_paths if os.path.splitext(p)[1].lower() in image_formats]
