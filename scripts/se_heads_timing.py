#!/usr/bin/env python3
"""ms per forward of the reference project's shipped head configuration (SqueezeExcite in every head, four pyramid levels,
128 features; road_project/train.py:36-58 of the reference) on ResNeXt-50, at 8 x 1024^2 and at the reference's serving
shape 1 x 540 x 960 (engine/config.py:13,167), in the "f32" and "f16s" conv maths, eager and with enable_graphs().
Device events around every step, after a warm-up of every leg.  One JSON line per leg.

Usage (GPU box):  python scripts/se_heads_timing.py [--tree DIR] [--steps 10] [--warmup 3] [--label NAME]
--tree: the repository root whose package is imported (default: this one), so that two builds -- e.g. a parent commit
unpacked with `git archive` and built beside this tree -- can be timed by alternating processes."""
import argparse
import json
import os
import sys


def shipped_head_config(bt):
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
    cfg.backbone.backbone_outputs = ('C3', 'C4', 'C5', 'P6')
    cfg.detection.num_features = 128
    cfg.detection.num_depth = 3
    cfg.detection.use_squeeze_excite = True
    cfg.detection.pr_scales = [2 ** 0, 2 ** (1 / 3), 2 ** (2 / 3)]
    cfg.detection.pr_ratios = [1 / 2, 1, 2, 5, 8]
    cfg.instance.crop_size = (14, 14)
    cfg.instance.max_k = 2
    cfg.instance.num_features = 128
    cfg.instance.num_depth = 4
    cfg.instance.use_squeeze_excite = True
    cfg.semantic.num_features = 128
    cfg.semantic.num_depth = 3
    cfg.semantic.use_squeeze_excite = True
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--shapes", default="8x1024x1024,1x540x960")
    ap.add_argument("--maths", default="f32,f16s")
    ap.add_argument("--graphs", default="0,1", help="0: eager, 1: enable_graphs()")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "instance-segmentation-road-project_amd")]
    import numpy as np
    import torch
    from masklab_hip import ops, retinamasklab as R

    cfg = shipped_head_config("resnext50")
    _, model = R.construct_masklab_networks(cfg)
    model.load_weights(model.init_weights(5), "cuda:0")
    rng = np.random.default_rng(0)
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        images = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
        for math in args.maths.split(","):
            for graphs in (bool(int(g)) for g in args.graphs.split(",")):
                rec = {"label": args.label, "shape": shape, "math": math, "graphs": graphs}
                ops.set_conv_math(math)
                model.enable_graphs(graphs)
                try:
                    for _ in range(args.warmup):
                        model(images)
                    torch.cuda.synchronize()
                    times = []
                    for _ in range(args.steps):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        model(images)
                        b.record()
                        torch.cuda.synchronize()
                        times.append(a.elapsed_time(b))
                    rec.update(ms_median=round(float(np.median(times)), 3), ms_min=round(float(min(times)), 3),
                               ms_max=round(float(max(times)), 3), steps=args.steps,
                               whole_graph=bool(graphs and model._graphs and next(iter(model._graphs))[3]))
                except NotImplementedError as e:          # (a build without the fp16-storage SqueezeExcite)
                    rec["error"] = f"{type(e).__name__}: {e}"[:200]
                finally:
                    model.enable_graphs(False)
                    ops.set_conv_math("f32")
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
