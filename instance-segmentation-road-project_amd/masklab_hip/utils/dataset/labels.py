"""The reference's label tables (road_project/setup/process.py: load_label_dataframes_from_imglab_files, with
road_project/setup/imglab.py: imglabformat_to_dataframe) restated with `json` alone: no pandas.

Every sub-folder of `labels/` is a label; every `*.json` in it is an imglab / COCO file with `images[{file_name, id}]`,
`annotations[{image_id, category_id, bbox: [cx, cy, w, h], segmentation}]` and `categories[{name, id}]`.  Kept from the
reference:

  * an annotation's label is the FOLDER name; the category name is ignored (the reference overwrites the column), but an
    annotation whose category_id or image_id the file does not list is dropped, as the reference's inner joins drop it;
  * `segmentation` is flattened and reshaped to (-1, 2): several parts become one polygon;
  * annotations with w * h <= 0 are dropped;
  * the "label exists" table has a row for every image with at least one annotation (under any label, w * h <= 0 ones
    included); its flag for a label is 1.0 when the image is LISTED in the `images` of any of that label's files, whether or
    not it has annotations there.  An image the table does not know gets zeros from the dataset.

Where the reference's order depends on os.listdir and an unstable sort, this order is fixed: folders sorted by name, files
sorted by name, annotations in file order -- so an image's annotations, and with them its instances, come in that order."""
import json
import os

import numpy as np


def load_labels(label_dir):
    """-> (label_exists, annotations).  label_exists: {"labels": [label, ...], "files": {file_name: {label: 0.0 / 1.0}}};
    annotations: a list of {"file_name", "cx", "cy", "w", "h", "label", "annotation": float64 [V,2]} in the fixed order."""
    labels, listed, annotations, annotated = [], {}, [], set()
    for label in sorted(os.listdir(label_dir)):
        folder = os.path.join(label_dir, label)
        if not os.path.isdir(folder):
            continue
        labels.append(label)
        listed[label] = set()
        for file_name in sorted(os.listdir(folder)):
            if os.path.splitext(file_name)[1].lower() != ".json":
                continue
            with open(os.path.join(folder, file_name), "r") as f:
                coco = json.load(f)
            names = {}
            for image in coco["images"]:
                names.setdefault(image["id"], image["file_name"])
                listed[label].add(image["file_name"])
            categories = {c["id"] for c in coco["categories"]}
            for a in coco["annotations"]:
                if a["category_id"] not in categories or a["image_id"] not in names:
                    continue
                image = names[a["image_id"]]
                annotated.add(image)
                cx, cy, w, h = (float(v) for v in a["bbox"][:4])
                if not w * h > 0:
                    continue
                flat = np.asarray(_flatten(a["segmentation"]), np.float64)
                if flat.size % 2:
                    raise ValueError(f"load_labels: {os.path.join(folder, file_name)}: a segmentation of {image} has "
                                     f"{flat.size} coordinates, not pairs")
                annotations.append({"file_name": image, "cx": cx, "cy": cy, "w": w, "h": h, "label": label,
                                    "annotation": flat.reshape(-1, 2)})
    files = {name: {label: float(name in listed[label]) for label in labels} for name in sorted(annotated)}
    return {"labels": labels, "files": files}, annotations


def _flatten(seg):
    out = []
    for part in seg:
        if isinstance(part, (list, tuple)):
            out.extend(_flatten(part))
        else:
            out.append(part)
    return out
