"""A tiny data directory in the reference's layout (test infrastructure, not collected), shared by the CPU and the GPU dataset
tests: four 64 x 96 JPEGs under images/, imglab / COCO files under labels/<label>/, and the batch the reference's
MaskLabDataset.__getitem__ would return for it, restated on tests/polygon_ref.py (no PNG tree: the crop, write, read and
cv2.resize back into the slice it was cut from is the identity)."""
import json
import os

import numpy as np

import polygon_ref as REF

H, W = 64, 96
CASES = ["a.jpg", "b.jpg", "c.jpg", "d.jpg"]
INSTANCE_LABELS = ("car", "bump")
SEMANTIC_LABELS = ("other_road", "my_road")
EXCEPT_LABELS = ("car",)
MIN_AREA = 100.0

# label -> file -> (listed images, [(image, [cx, cy, w, h], segmentation)]): hand-written
CAR_A = [[30.5, 20.25, 70.0, 22.5, 66.25, 50.0, 28.0, 47.5]]                       # w * h = 42 * 29.75
BUMP_A_SMALL = [[5.0, 5.0, 12.0, 5.5, 11.0, 12.0]]                                 # 7 * 7 = 49: below MIN_AREA
BUMP_A_FLAT = [[40.0, 40.0, 50.0, 40.0, 60.0, 40.0]]                               # h = 0: dropped by load_labels
BUMP_B_1 = [[10.0, 8.0, 40.0, 9.0], [38.0, 30.0, 12.0, 28.0]]                      # two parts: one polygon of 4 vertices
BUMP_B_2 = [[50.5, 30.5, 90.0, 33.0, 93.5, 60.0, 70.0, 45.0, 52.0, 62.0]]
CAR_B = [[-6.0, 40.0, 30.0, 42.0, 28.0, 70.0, -3.0, 66.0]]                         # leaves the image: clipped; the window starts at 0
ROAD_A = [[2.0, 30.0, 94.0, 28.0, 95.0, 63.0, 1.0, 62.0]]
OTHER_A_1 = [[3.0, 2.0, 50.0, 3.0, 48.0, 26.0, 4.0, 25.0]]
OTHER_A_2 = [[30.0, 10.0, 80.0, 12.0, 78.0, 34.0, 32.0, 30.0]]                     # overlaps OTHER_A_1 and CAR_A
OTHER_D = [[10.0, 10.0, 85.0, 15.0, 60.0, 55.0]]


def _bbox(seg):
    flat = np.array([v for part in seg for v in part], np.float64).reshape(-1, 2)
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    return [float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), float(hi[0] - lo[0]), float(hi[1] - lo[1])]


SPEC = {
    "car": {"cars.json": (["a.jpg", "b.jpg", "d.jpg"], [("a.jpg", CAR_A), ("b.jpg", CAR_B)])},          # d.jpg: listed, no annotation
    "bump": {"one.json": (["b.jpg"], [("b.jpg", BUMP_B_1)]),
             "two.json": (["a.jpg", "b.jpg"], [("a.jpg", BUMP_A_SMALL), ("b.jpg", BUMP_B_2), ("a.jpg", BUMP_A_FLAT)])},
    "my_road": {"road.json": (["a.jpg", "b.jpg"], [("a.jpg", ROAD_A)])},                                  # b.jpg: listed, no annotation
    "other_road": {"other.json": (["a.jpg", "d.jpg"], [("a.jpg", OTHER_A_1), ("a.jpg", OTHER_A_2), ("d.jpg", OTHER_D)]),
                   "notes.txt": None},                                                                  # not a .json: ignored
}

# what load_labels must return, hand-written: folders sorted, files sorted, file order; BUMP_A_FLAT dropped
ANNOTATIONS = [("b.jpg", "bump", BUMP_B_1), ("a.jpg", "bump", BUMP_A_SMALL), ("b.jpg", "bump", BUMP_B_2), ("a.jpg", "car", CAR_A),
               ("b.jpg", "car", CAR_B), ("a.jpg", "my_road", ROAD_A), ("a.jpg", "other_road", OTHER_A_1),
               ("a.jpg", "other_road", OTHER_A_2), ("d.jpg", "other_road", OTHER_D)]
LABELS = ["bump", "car", "my_road", "other_road"]
# c.jpg is in no file: no row.  d.jpg is listed under car without an annotation there.
EXISTS = {"a.jpg": {"bump": 1.0, "car": 1.0, "my_road": 1.0, "other_road": 1.0},
          "b.jpg": {"bump": 1.0, "car": 1.0, "my_road": 1.0, "other_road": 0.0},
          "d.jpg": {"bump": 0.0, "car": 1.0, "my_road": 0.0, "other_road": 1.0}}
# instances per image in the dataset's order (bump before car: folders sorted), label index in INSTANCE_LABELS
INSTANCES = {"a.jpg": [("car", CAR_A)], "b.jpg": [("bump", BUMP_B_1), ("bump", BUMP_B_2), ("car", CAR_B)], "c.jpg": [], "d.jpg": []}


def write_data_dir(root, sizes=None):
    """Writes images/ and labels/ under `root` (Pillow).  sizes: {case: (H, W)} for images that are not 64 x 96."""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"))
    rng = np.random.default_rng(64)
    for case in CASES:
        h, w = (sizes or {}).get(case, (H, W))
        smooth = np.kron(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3)), np.ones((8, 8, 1)))[:h, :w]
        Image.fromarray(smooth.astype(np.uint8)).save(os.path.join(root, "images", case), quality=90)
    for label, files in SPEC.items():
        os.makedirs(os.path.join(root, "labels", label))
        for file_name, content in files.items():
            path = os.path.join(root, "labels", label, file_name)
            if content is None:
                open(path, "w").write("not a label file\n")
                continue
            listed, annotations = content
            ids = {name: 10 + i for i, name in enumerate(listed)}
            coco = {"images": [{"file_name": name, "id": ids[name], "width": W, "height": H} for name in listed],
                    "categories": [{"name": "anything", "id": 1, "supercategory": "none"}],   # the folder names the label
                    "annotations": [{"id": k + 1, "image_id": ids[name], "category_id": 1, "bbox": _bbox(seg), "segmentation": seg,
                                     "ignore": 0, "iscrowd": 0} for k, (name, seg) in enumerate(annotations)],
                    "type": "instances"}
            json.dump(coco, open(path, "w"))
    open(os.path.join(root, "labels", "README"), "w").write("a file, not a label folder\n")
    return root


def _poly(seg):
    return np.array([v for part in seg for v in part], np.float64).reshape(-1, 2)


def _window(seg):
    cx, cy, w, h = _bbox(seg)
    return [max(int(v), 0) for v in (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)]


def expected_sample(case, images):
    """The reference's single-sample dict for `case`; images: {case: uint8 [H,W,3]}."""
    insts = INSTANCES[case]
    detection = np.array([_bbox(seg) + [float(INSTANCE_LABELS.index(label)), 1.0] for label, seg in insts], np.float64).reshape(-1, 6)
    instance = np.zeros((len(insts), H, W), np.uint8)
    for k, (_, seg) in enumerate(insts):
        x1, y1, x2, y2 = _window(seg)
        instance[k, y1:y2 + 1, x1:x2 + 1] = REF.polygon_mask(_poly(seg), H, W)[y1:y2 + 1, x1:x2 + 1]
    semantic = np.zeros((H, W, len(SEMANTIC_LABELS)), np.uint8)
    mine = [(label, seg) for name, label, seg in ANNOTATIONS if name == case]
    excepted = np.zeros((H, W), bool)
    for label, seg in mine:
        if label in EXCEPT_LABELS:
            excepted |= REF.polygon_mask(_poly(seg), H, W)
    for s, wanted in enumerate(SEMANTIC_LABELS):
        mask = np.zeros((H, W), bool)
        for label, seg in mine:
            if label == wanted:
                mask |= REF.polygon_mask(_poly(seg), H, W)
        semantic[..., s] = mask & ~excepted
    row = EXISTS.get(case)
    exist = lambda labels: np.array([row[l] if row else 0.0 for l in labels], np.float64)
    return {"images": images[case], "semantic": semantic, "semantic_exist": exist(SEMANTIC_LABELS), "detection": detection,
            "instance": instance, "instance_exist": exist(INSTANCE_LABELS)}


def expected_batch(cases, images):
    """The reference's slice dict for `cases`, n = the largest instance count (0 allowed)."""
    samples = [expected_sample(c, images) for c in cases]
    n = max(len(s["detection"]) for s in samples)
    detection = np.full((len(cases), n, 6), -1.0)
    instance = np.full((len(cases), n, H, W), -1, np.int8)
    for i, s in enumerate(samples):
        detection[i, :len(s["detection"])] = s["detection"]
        instance[i, :len(s["instance"])] = s["instance"]
    stack = lambda key: np.stack([s[key] for s in samples])
    return {"images": stack("images"), "semantic": stack("semantic"), "semantic_exist": stack("semantic_exist"), "detection": detection,
            "instance": instance, "instance_exist": stack("instance_exist")}


def read_images(root):
    from PIL import Image
    return {c: np.asarray(Image.open(os.path.join(root, "images", c)).convert("RGB"), np.uint8) for c in CASES}


class InMemory:
    """The in-memory twin of the dataset, in the layout MaskLabGenerator takes (tests/generator_cases.py: TinyDataset)."""

    def __init__(self, root):
        self.images = read_images(root)

    def __len__(self):
        return len(CASES)

    def __getitem__(self, sl):
        return expected_batch(CASES[sl], self.images)

    def shuffle(self):
        pass
