#!/usr/bin/env python3
"""The serving model's 'visualize' output (csrc/visualize.hip): ms of the fused render (ml_serving_visualize_u8) at
1 x 1080 x 1920 and 8 x 1080 x 1920 with 100 detections per image, of the literal chain (CropAndPadMask's canvases +
DrawBoxes + DrawInstance + DrawSegmentation) at 1 x 1080 x 1920, and of the serving step with and without `visualize` on
the shipped SE-ResNet-34 head configuration in the "f32" conv math at 1 x 1080 x 1920.  Seeded scenes, a warm-up, device
events around every step; the fused render's achieved bytes/s (18 B per pixel algorithmically: frame, 3-class seg, out)
against the sustained copy bandwidth in profiles/r03_peaks.json.  One JSON line per leg.

Usage (GPU box):  python scripts/serving_visualize_timing.py [--steps 20] [--warmup 3] [--skip-model]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]


def _timed(fn, steps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def scene(B, H, W, n, seed, mh=28, mw=28):
    """n detections per image, boxes up to a sixth of the frame, five classes, conf above the 50 cut; 0/1 masks and a
    3-class 0/1 semantic map."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    det = np.zeros((B, n, 6), np.int32)
    det[..., 0] = rng.integers(0, W, (B, n))
    det[..., 1] = rng.integers(0, H, (B, n))
    det[..., 2] = rng.integers(8, W // 6, (B, n))
    det[..., 3] = rng.integers(8, H // 6, (B, n))
    det[..., 4] = rng.integers(0, 5, (B, n))
    det[..., 5] = rng.integers(51, 100, (B, n))
    ins = (rng.random((B, n, mh, mw)) > 0.4).astype(np.int32)
    seg = (rng.random((B, H, W, 3)) > 0.6).astype(np.int32)
    images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return [torch.from_numpy(a).cuda() for a in (images, det, ins, seg)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ModelConfiguration, ops
    from masklab_hip import retinamasklab as R

    post = ModelConfiguration().postprocess
    pal = (post.instance_colors, post.instance_alpha, post.semantic_colors, post.semantic_alpha)
    peaks = os.path.join(ROOT, "profiles", "r03_peaks.json")
    copy_gbs = json.load(open(peaks))["copy_global_x4"]["read_plus_write_GBs"] if os.path.exists(peaks) else None
    for B in (1, 8):
        images, det, ins, seg = scene(B, 1080, 1920, 100, seed=B)
        med, lo, hi = _timed(lambda: ops.serving_visualize(images, det, ins, seg, *pal), args.steps, args.warmup)
        nbytes = 18 * B * 1080 * 1920
        gbs = nbytes / (med * 1e-3) / 1e9
        print(json.dumps({"leg": "fused render", "shape": f"{B}x1080x1920", "detections_per_image": 100,
                          "bytes_moved_MB": round(nbytes / 1e6, 1), "us_median": round(med * 1e3, 1),
                          "us_min": round(lo * 1e3, 1), "us_max": round(hi * 1e3, 1), "GB_s": round(gbs, 1),
                          "of_copy_peak": round(gbs / copy_gbs, 3) if copy_gbs else None}), flush=True)
        if B == 1:
            def literal():
                cpm = ops.crop_pad_mask(det, ins, 1080, 1920)
                v = ops.draw_boxes(images, det)
                v = ops.draw_instance(v, det, cpm, post.instance_colors, post.instance_alpha)
                return ops.draw_segmentation(v, seg, post.semantic_colors, post.semantic_alpha)
            med, lo, hi = _timed(literal, args.steps, args.warmup)
            print(json.dumps({"leg": "literal chain", "shape": "1x1080x1920", "detections_per_image": 100,
                              "canvas_MB": round(4 * 100 * 1080 * 1920 / 1e6, 1), "us_median": round(med * 1e3, 1),
                              "us_min": round(lo * 1e3, 1)}), flush=True)
        del images, det, ins, seg
        torch.cuda.empty_cache()
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
    images = torch.from_numpy(np.random.default_rng(1080).integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)).cuda()
    res = {}
    for vis in (False, True, False, True):                            # interleaved: drift shows as a spread, not a bias
        serving = R.construct_serving_network(cfg, deploy, visualize=vis)
        med, lo, hi = _timed(lambda: serving(images), args.steps, args.warmup)
        res.setdefault(vis, []).append(med)
        print(json.dumps({"leg": "serving step", "backbone": "seresnet34", "shape": "1x1080x1920", "math": "f32",
                          "visualize": vis, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}),
              flush=True)
    base, with_vis = min(res[False]), min(res[True])
    print(json.dumps({"leg": "serving step cost of visualize", "ms_without": round(base, 3), "ms_with": round(with_vis, 3),
                      "pct": round(100 * (with_vis - base) / base, 2)}), flush=True)


if __name__ == "__main__":
    main()
