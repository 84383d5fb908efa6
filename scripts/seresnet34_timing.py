#!/usr/bin/env python3
"""SE-ResNet-34 -- the reference project's own backbone (road_project/train.py:36-58) -- under its shipped head
configuration: ms per forward at 8 x 1024^2 and at the serving shape 1 x 540 x 960, in the "f32" conv math, eager and
with enable_graphs(); and the SE block tail kernel (csrc/se_residual.hip) alone on the stage-1 shape of the 1024^2 batch
(8 x 256^2 x 64 fp32, 134 MB per tensor) and on the stage-4 shape, its achieved bytes/s against the sustained copy
bandwidth in profiles/r03_peaks.json.  Device events around every step, after a warm-up.  One JSON line per leg.

Usage (GPU box):  python scripts/seresnet34_timing.py [--steps 10] [--warmup 3] [--shapes 8x1024x1024,1x540x960]"""
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


def tail_legs(steps, warmup, copy_gbs):
    import torch
    from masklab_hip import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for (B, H, W, C) in ((8, 256, 256, 64), (8, 32, 32, 512)):
        Hd = C // 16
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        x, sc = r(B, H, W, C), r(B, H, W, C)
        w1, b1, w2, b2 = r(C, Hd) * 0.1, r(Hd) * 0.1, r(Hd, C) * 0.1, r(C) * 0.1
        s, t = r(C).abs() + 0.5, r(C) * 0.1
        n = x.numel() * 4
        legs = [("se_residual", lambda: ops.se_residual(x, sc, w1, b1, w2, b2, s, t), 4 * n),
                ("se_residual +y", lambda: ops.se_residual(x, sc, w1, b1, w2, b2, s, t, want_y=True), 5 * n),
                ("bn_relu", lambda: ops.bn_relu(x, s, t), 2 * n)]
        for name, fn, nbytes in legs:
            med, lo, hi = _timed(fn, steps * 5, warmup)
            gbs = nbytes / (med * 1e-3) / 1e9
            print(json.dumps({"leg": name, "shape": f"{B}x{H}x{W}x{C}", "MB_per_tensor": round(n / 1e6, 1),
                              "bytes_moved_MB": round(nbytes / 1e6, 1), "ms_median": round(med, 4),
                              "ms_min": round(lo, 4), "GB_s": round(gbs, 1),
                              "of_copy_peak": round(gbs / copy_gbs, 3) if copy_gbs else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="8x1024x1024,1x540x960")
    ap.add_argument("--graphs", default="0,1", help="0: eager, 1: enable_graphs()")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ops, retinamasklab as R
    from se_heads_timing import shipped_head_config

    peaks = os.path.join(ROOT, "profiles", "r03_peaks.json")
    copy_gbs = json.load(open(peaks))["copy_global_x4"]["read_plus_write_GBs"] if os.path.exists(peaks) else None
    tail_legs(args.steps, args.warmup, copy_gbs)
    if args.skip_model:
        return
    cfg = shipped_head_config("seresnet34")
    _, model = R.construct_masklab_networks(cfg)
    model.load_weights(model.init_weights(5), "cuda:0")
    ops.set_conv_math("f32")
    rng = np.random.default_rng(0)
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        images = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
        for graphs in (bool(int(v)) for v in args.graphs.split(",")):
            model.enable_graphs(graphs)
            med, lo, hi = _timed(lambda: model(images), args.steps, args.warmup)
            print(json.dumps({"leg": "forward", "backbone": "seresnet34", "shape": shape, "math": "f32", "graphs": graphs,
                              "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                              "img_s": round(B / (med * 1e-3), 1), "steps": args.steps}), flush=True)
            model.enable_graphs(False)
        # the backbone alone (to C5 + P6): its share of the forward
        bb = model.backbone_network
        med, lo, hi = _timed(lambda: bb(images), args.steps, args.warmup)
        print(json.dumps({"leg": "backbone only", "shape": shape, "math": "f32", "ms_median": round(med, 3),
                          "ms_min": round(lo, 3)}), flush=True)


if __name__ == "__main__":
    main()
