#!/usr/bin/env python3
"""Writes tests/golden/jpeg_decode/: JPEG streams written by Pillow (libjpeg-turbo) and the pixels Pillow decodes from
them -- the bytes the device decoder (csrc/jpeg_decode.hip) has to reproduce.  The frames are those of
tests/golden/jpeg/frames.npz; its committed libjpeg streams are decoded too (their streams stay where they are).

  streams.npz    the new streams, uint8
  pixels.npz     Pillow's decode of every supported case: uint8 [H,W,3] ([H,W] for grayscale: the three channels agree)
  manifest.json  case -> {stream: "<file>:<key>", pixels: key or null, mode, supported, what}

Cases that differ only in how the same coefficients are coded (restart intervals, optimised Huffman tables) share one
pixel array; the generator checks that Pillow decodes them alike.

Needs Pillow.  Usage:  python tests/golden/make_jpeg_decode_golden.py"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_jpeg_golden import smooth  # noqa: E402

OUT = os.path.join(HERE, "jpeg_decode")


def pillow_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(bytes(data))) as im:
        mode = im.mode
        rgb = np.array(im.convert("RGB"), dtype=np.uint8)
    if mode == "L":
        assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 0] == rgb[..., 2]).all()
        return rgb[..., 0].copy()
    return rgb


def pillow_encode(frame, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", **kw)
    return buf.getvalue()


def main():
    import PIL
    from PIL import features
    os.makedirs(OUT, exist_ok=True)
    with np.load(os.path.join(HERE, "jpeg", "frames.npz")) as z:
        frames = {k: z[k] for k in z.files}
    with open(os.path.join(HERE, "jpeg", "manifest.json")) as fh:
        committed = json.load(fh)
    turbo = " (libjpeg-turbo)" if features.check_feature("libjpeg_turbo") else ""
    manifest = {"writer": f"Pillow {PIL.__version__}, libjpeg {features.version('jpg')}{turbo}", "cases": {}}
    streams, pixels = {}, {}

    def case(name, data, mode, what, source=None, supported=True, pixels_key=None):
        entry = {"stream": source or f"jpeg_decode/streams.npz:{name}", "mode": mode, "supported": supported, "what": what,
                 "pixels": None, "bytes": len(data)}
        if source is None:
            streams[name] = np.frombuffer(data, np.uint8)
        if supported:
            got = pillow_decode(data)
            key = pixels_key or name
            if key in pixels:
                assert np.array_equal(pixels[key], got), (name, "does not decode to the pixels of", key)
            else:
                pixels[key] = got
            entry["pixels"] = key
        manifest["cases"][name] = entry

    # the committed libjpeg streams: 64x80, 96x128, 160x240 at quality 50, 95, 100
    for fname, e in sorted(committed["frames"].items()):
        for q, rec in sorted(e["libjpeg"].items()):
            case(rec["stream"], bytes(frames[rec["stream"]]), "420", f"{fname} at quality {q}: whole MCUs",
                 source=f"jpeg/frames.npz:{rec['stream']}")
    photo = frames["photo_150x203"]
    for fname in ("noise_37x53", "smooth_48x70", "photo_150x203"):
        case(f"{fname}_q95", pillow_encode(frames[fname], quality=95), "420", "odd sizes: ceil chroma, right and bottom crop")
    for h, w in ((1, 1), (8, 9), (17, 33)):
        case(f"crop_{h}x{w}_q95", pillow_encode(np.ascontiguousarray(photo[:h, :w]), quality=95), "420",
             "a single MCU / a one-column chroma plane where both edge rules meet")
    case("smooth_40x1048_q75", pillow_encode(smooth(40, 1048, 7), quality=75), "420",
         "66 MCUs a row (more than a wave), W no multiple of 16")
    case("photo_150x203_444", pillow_encode(photo, quality=95, subsampling=0), "444", "no upsampling step")
    gray = np.ascontiguousarray((photo.astype(np.int64) @ np.array([299, 587, 114]) // 1000).astype(np.uint8))
    case("photo_150x203_gray", pillow_encode(gray, quality=95), "gray", "one component, a non-interleaved scan")
    same = "photo_150x203_q95"
    case("photo_150x203_restart_blocks5", pillow_encode(photo, quality=95, restart_marker_blocks=5), "420",
         "DRI: a restart marker every 5 MCUs", pixels_key=same)
    case("photo_150x203_restart_rows1", pillow_encode(photo, quality=95, restart_marker_rows=1), "420",
         "DRI: a restart marker every MCU row", pixels_key=same)
    case("photo_150x203_optimize", pillow_encode(photo, quality=95, optimize=True), "420", "optimised Huffman tables",
         pixels_key=same)
    case("photo_150x203_progressive", pillow_encode(photo, quality=95, progressive=True), "progressive",
         "unsupported: SOF2", supported=False)
    case("photo_150x203_422", pillow_encode(photo, quality=95, subsampling=1), "422", "unsupported: 2x1 sampling",
         supported=False)

    np.savez_compressed(os.path.join(OUT, "streams.npz"), **streams)
    np.savez_compressed(os.path.join(OUT, "pixels.npz"), **pixels)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
