#!/usr/bin/env python3
"""SE-ResNeXt-50 and SE-ResNet-50 (vendored thirdparty senet.py, offered by the reference's load_backbone): the fused SE
bottleneck tail (csrc/se_bottleneck.hip) alone on the four stage shapes of the 8 x 1024^2 batch, fp32 and half, its
algorithmic bytes/s (c3 read twice, residual once, out written once) against a device copy timed in the same process;
then the backbone alone (to C5 + P6 / P7, the default outputs) and the whole forward (default heads) of both models at
8 x 1024^2 in "f32" and "f16s" and at 1 x 540 x 960 eager and with enable_graphs().  Device events around every step,
after a warm-up.  One JSON line per leg.  The share of the three kernels inside a tail (pool, gate, stream) comes from
a kernel trace of `--tail-only` (rocprofv3 --kernel-trace --stats).

Usage (GPU box):  python scripts/senet_timing.py [--steps 10] [--warmup 3] [--tail-only]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

TAIL_SHAPES = ((8, 256, 256, 256), (8, 128, 128, 512), (8, 64, 64, 1024), (8, 32, 32, 2048))


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


def copy_leg(steps, warmup):
    """Read + write rate of a device copy of one 537 MB fp32 tensor (8 x 256^2 x 256)."""
    import torch
    src = torch.randn(8 * 256 * 256 * 256, device="cuda")
    dst = torch.empty_like(src)
    med, lo, _ = _timed(lambda: dst.copy_(src), steps * 3, warmup)
    gbs = 2 * src.numel() * 4 / (med * 1e-3) / 1e9
    print(json.dumps({"leg": "copy", "MB": round(src.numel() * 4 / 1e6, 1), "ms_median": round(med, 4),
                      "ms_min": round(lo, 4), "rw_GB_s": round(gbs, 1)}), flush=True)
    return gbs


def tail_legs(steps, warmup, copy_gbs):
    import torch
    from masklab_hip import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for dtype in (torch.float32, torch.float16):
        for (B, H, W, C) in TAIL_SHAPES:
            Hd = C // 16
            r = lambda *s: torch.randn(*s, device="cuda", generator=g)
            c3, res = r(B, H, W, C).to(dtype), r(B, H, W, C).to(dtype)
            w1, b1, w2, b2 = r(C, Hd) * 0.05, r(Hd) * 0.1, r(Hd, C) * 0.1, r(C) * 0.1
            nbytes = 4 * c3.numel() * c3.element_size()
            med, lo, _ = _timed(lambda: ops.se_bottleneck(c3, res, w1, b1, w2, b2, out=c3), steps * 5, warmup)
            gbs = nbytes / (med * 1e-3) / 1e9
            print(json.dumps({"leg": "se_bottleneck", "dtype": str(dtype).split(".")[-1], "shape": f"{B}x{H}x{W}x{C}",
                              "MB_per_tensor": round(c3.numel() * c3.element_size() / 1e6, 1),
                              "bytes_moved_MB": round(nbytes / 1e6, 1), "us_median": round(med * 1e3, 1),
                              "us_min": round(lo * 1e3, 1), "TB_s": round(gbs / 1e3, 3),
                              "of_copy": round(gbs / copy_gbs, 3)}), flush=True)


def model_legs(steps, warmup):
    import numpy as np
    import torch
    from masklab_hip import ModelConfiguration, ops, retinamasklab as R
    rng = np.random.default_rng(0)
    for bt in ("seresnext50", "seresnet50"):
        cfg = ModelConfiguration()
        cfg.backbone.backbone_type = bt
        _, model = R.construct_masklab_networks(cfg)
        model.load_weights(model.init_weights(5), "cuda:0")
        bb = model.backbone_network
        for shape, maths, graph_modes in (("8x1024x1024", ("f32", "f16s"), (False,)), ("1x540x960", ("f32",), (False, True))):
            B, H, W = (int(v) for v in shape.split("x"))
            images = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
            for math in maths:
                ops.set_conv_math(math)
                med, lo, _ = _timed(lambda: bb(images), steps, warmup)
                print(json.dumps({"leg": "backbone", "backbone": bt, "shape": shape, "math": math,
                                  "ms_median": round(med, 3), "ms_min": round(lo, 3)}), flush=True)
                for graphs in graph_modes:
                    model.enable_graphs(graphs)
                    med, lo, hi = _timed(lambda: model(images), steps, warmup)
                    print(json.dumps({"leg": "forward", "backbone": bt, "shape": shape, "math": math, "graphs": graphs,
                                      "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                                      "img_s": round(B / (med * 1e-3), 1)}), flush=True)
                    model.enable_graphs(False)
                ops.set_conv_math("f32")
        del model, bb
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tail-only", action="store_true")
    args = ap.parse_args()
    copy_gbs = copy_leg(args.steps, args.warmup)
    tail_legs(args.steps, args.warmup, copy_gbs)
    if not args.tail_only:
        model_legs(args.steps, args.warmup)


if __name__ == "__main__":
    main()
