#!/usr/bin/env python3
"""Entropy decoding of the serving model's JPEG request on the device (the jpeg_entropy_* kernels of
csrc/jpeg_decode.hip) against the host's Huffman decoder: wall-clock ms, a device synchronise closing every timing, the
two paths alternated in one process after a warm-up --

  host     ops.decode_jpeg(entropy="host"): ml_jpeg_decode_entropy into pinned memory, the upload of the packed
           coefficients, the two launches (what the parent commit does);
  device   ops.decode_jpeg(entropy="device"): the upload of the file and its plan, the six entropy launches, the same
           two launches, the read of the status word,

on the two 1 x 1080 x 1920 requests of scripts/jpeg_decode_timing.py (quality 75 and 95), the results compared byte for
byte.  Then `ContentServingModel.predict` both ways on the shipped SE-ResNet-34 head configuration (f32).  One JSON line
per leg: median, min, max and the inter-quartile range as the spread; a leg is a gain only if the device's median plus
its spread is below the host's median minus its spread.  Each request's status words are printed (status, block, most
rounds a workgroup needed, last launch in which a state crossed a workgroup boundary), and with --fixtures the status
of every committed fixture stream.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/jpeg_entropy_timing.py --skip-model` run.

Usage (GPU box):  timeout 600 python scripts/jpeg_entropy_timing.py [--steps 30] [--warmup 5] [--skip-model] [--fixtures]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts"),
                os.path.join(ROOT, "tests")]

from jpeg_decode_timing import tiled_photo  # noqa: E402
from jpeg_encode_timing import alternate, stats  # noqa: E402


def report(leg, times, extra):
    d, h = stats(times["device"]), stats(times["host"])
    line = {"leg": leg, "shape": "1x1080x1920", "entropy_device": d, "entropy_host": h,
            "host_minus_device_ms": round(h["ms_median"] - d["ms_median"], 3),
            "gain": bool(d["ms_median"] + d["ms_iqr"] < h["ms_median"] - h["ms_iqr"]), **extra}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--fixtures", action="store_true")
    ap.add_argument("--quality", type=int, nargs="*", default=[75, 95])
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ops, serving
    from masklab_hip import retinamasklab as R
    H, W = 1080, 1920
    frame = torch.from_numpy(tiled_photo(H, W)[None]).cuda()
    requests = {}
    for q in args.quality:
        request = ops.jpeg_contents(*ops.encode_jpeg(frame, q))[0]
        requests[q] = request
        kept = {}

        def device():
            kept["device"] = ops.decode_jpeg(request, "cuda:0", entropy="device")

        def host():
            kept["host"] = ops.decode_jpeg(request, "cuda:0", entropy="host")

        t = alternate({"device": device, "host": host}, args.steps, args.warmup)
        _, _, status = ops.jpeg_entropy_device(request, "cuda:0")
        bits, per_wg = ops.jpeg_entropy_geometry()
        report("ops.decode_jpeg", t, {"quality": q, "file_bytes": len(request), "same_bytes": bool(torch.equal(kept["device"], kept["host"])),
                                      "status_block_rounds_launch": status[0].tolist(),
                                      "subsequences": -(-len(request) * 8 // bits), "subsequence_bits": bits,
                                      "subsequences_per_workgroup": per_wg})
    if args.fixtures:
        import jpeg_decode_ref as D
        cases = D.load_cases(os.path.join(ROOT, "tests", "golden"))
        names = [k for k in sorted(cases) if cases[k]["supported"]]
        _, _, status = ops.jpeg_entropy_device([cases[k]["stream"] for k in names], "cuda:0")
        print(json.dumps({"fixtures": {k: status[b].tolist() for b, k in enumerate(names)},
                          "not_synced": int((status[:, 0] == 11).sum()), "status_0": int((status[:, 0] == 0).sum())}), flush=True)
    if args.skip_model:
        return
    from se_heads_timing import shipped_head_config
    cfg = shipped_head_config("seresnet34")
    ops.set_conv_math("f32")
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)                    # some anchors pass min_confidence
    model.load_weights(w, "cuda:0")
    deploy = R.construct_deploy_network(cfg, model)
    served = {e: serving.ContentServingModel(cfg, deploy, device="cuda:0", entropy=e) for e in ("device", "host")}
    for q, request in requests.items():
        answers = {}

        def run(e):
            answers[e] = served[e].predict(request)

        t = alternate({"device": lambda: run("device"), "host": lambda: run("host")}, args.steps, args.warmup)
        same = answers["device"][0][0] == answers["host"][0][0] and bool(np.array_equal(answers["device"][1], answers["host"][1]))
        report("ContentServingModel.predict -> [content, summary]", t, {"quality": q, "file_bytes": len(request), "same_answer": same,
                                                                        "backbone": "seresnet34", "math": "f32"})


if __name__ == "__main__":
    main()
