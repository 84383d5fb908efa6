#!/usr/bin/env python3
"""Writes tests/golden/jpeg/: the frames of the JPEG encoder tests, libjpeg's own streams for the frames whose
dimensions are multiples of 16 (written by Pillow, which links libjpeg-turbo), and manifest.json with libjpeg's distance
from the fp64 oracle of tests/jpeg_ref.py on each of them: the share of quantised coefficients that differ from the
oracle's rounding and the largest difference.  That share is the yardstick the device encoder is held to.

Frames whose dimensions are not multiples of 16 have no libjpeg figures: libjpeg fills the blocks beyond the image
with "dummy" blocks (the neighbour's DC, zero AC), the device encoder encodes the replicated samples.

Needs Pillow.  The photo frames are crops of the reference project's test/test_input.jpg (image data); without
--photo the crops already in frames.npz are kept.

Usage:  python tests/golden/make_jpeg_golden.py [--photo /path/to/test_input.jpg]"""
import argparse
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as J  # noqa: E402

OUT = os.path.join(HERE, "jpeg")
QUALITIES = {"noise_64x80": (95, 50, 100), "photo_160x240": (95, 50, 100), "smooth_96x128": (95,)}


def smooth(H, W, seed):
    """A few seeded low-frequency waves per channel plus a little noise: mostly small AC coefficients."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.01, 0.12), rng.uniform(0.01, 0.12), rng.uniform(0, 6.28)
            out[..., c] += rng.uniform(20, 45) * np.sin(fy * y + fx * x + ph)
    out += 128 + rng.normal(0, 1.5, out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def frames(photo_path):
    rng = np.random.default_rng(20240607)
    f = {"noise_64x80": rng.integers(0, 256, (64, 80, 3), dtype=np.uint8),
         "smooth_96x128": smooth(96, 128, 5),
         "noise_37x53": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
         "smooth_48x70": smooth(48, 70, 6)}
    if photo_path:
        from PIL import Image
        photo = np.asarray(Image.open(photo_path).convert("RGB"))
        f["photo_160x240"] = np.ascontiguousarray(photo[0:160, 1080:1320])
        f["photo_150x203"] = np.ascontiguousarray(photo[80:230, 1100:1303])
    else:
        with np.load(os.path.join(OUT, "frames.npz")) as z:
            f["photo_160x240"], f["photo_150x203"] = z["photo_160x240"], z["photo_150x203"]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photo", default=None)
    args = ap.parse_args()
    import PIL
    from PIL import Image
    os.makedirs(OUT, exist_ok=True)
    arrays = frames(args.photo)
    from PIL import features
    turbo = " (libjpeg-turbo)" if features.check_feature("libjpeg_turbo") else ""
    manifest = {"writer": f"Pillow {PIL.__version__}, libjpeg {features.version('jpg')}{turbo}", "frames": {}}
    streams = {}
    for name, frame in sorted(arrays.items()):
        H, W = frame.shape[:2]
        entry = {"height": H, "width": W, "multiple_of_16": H % 16 == 0 and W % 16 == 0, "libjpeg": {}}
        for q in QUALITIES.get(name, ()):
            buf = io.BytesIO()
            Image.fromarray(frame).save(buf, "JPEG", quality=q)
            data = buf.getvalue()
            dec = J.decode(data, (H, W))
            share, largest = J.compare(dec["coefficients"], frame, q)
            key = f"{name}_q{q}_libjpeg"
            streams[key] = np.frombuffer(data, np.uint8)
            entry["libjpeg"][str(q)] = {"stream": key, "bytes": len(data), "share_differing": share, "max_difference": largest,
                                        "luminance_table": dec["qtables"][0].tolist(),
                                        "chrominance_table": dec["qtables"][1].tolist()}
        manifest["frames"][name] = entry
    manifest["largest_libjpeg_share"] = {
        str(q): max(e["libjpeg"][str(q)]["share_differing"] for e in manifest["frames"].values() if str(q) in e["libjpeg"])
        for q in (95, 50, 100)}
    np.savez_compressed(os.path.join(OUT, "frames.npz"), **arrays, **streams)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for name, e in manifest["frames"].items():
        print(name, {q: (round(v["share_differing"], 5), v["max_difference"]) for q, v in e["libjpeg"].items()})


if __name__ == "__main__":
    main()
