#!/usr/bin/env python3
"""ResNet-50's projection unit as one GEMM (csrc/conv1x1_dual.hip, ops.set_projection_fusion("on")) against the two
launches it replaces (the shortcut conv, then the 2c conv with the shortcut as residual -- kernels this project had
before and that the fusion does not touch): wall-clock ms, a device synchronise closing every timing, the two paths
alternated in one process after a warm-up --

  unit      the four projection units of the 8 x 1024^2 batch alone, fp32 and half tensors, on random data; the two
            results are compared (they differ by rounding only);
  backbone  the ResNet-50 backbone (to C5 + P6 / P7, the default outputs) at 8 x 1024^2 in "f32" and "f16s";
  forward   the whole forward of the default ModelConfiguration() at 8 x 1024^2 in "f32" and "f16s".

One JSON line per leg: median, min, max and the inter-quartile range as the spread; a leg counts as a gain only if the
fused median plus its spread is below the two-launch median minus its spread.  The fused path is the default only if the
whole-forward leg is a gain.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/resnet50_timing.py --units-only --steps 5` run.

Usage (GPU box):  timeout 900 python scripts/resnet50_timing.py [--steps 30] [--warmup 5] [--units-only] [--skip-forward]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from jpeg_encode_timing import alternate, stats  # noqa: E402

# (B, H, W of the block input x, Ka, Kx, N, stride): stages 2..5 of 8 x 1024^2
UNITS = ((8, 256, 256, 64, 64, 256, 1), (8, 256, 256, 128, 256, 512, 2), (8, 128, 128, 256, 512, 1024, 2),
         (8, 64, 64, 512, 1024, 2048, 2))


def report(leg, times, extra):
    fused, two = stats(times["fused"]), stats(times["two_launches"])
    line = {"leg": leg, **extra, "fused": fused, "two_launches": two,
            "two_minus_fused_ms": round(two["ms_median"] - fused["ms_median"], 3),
            "gain": bool(fused["ms_median"] + fused["ms_iqr"] < two["ms_median"] - two["ms_iqr"])}
    print(json.dumps(line), flush=True)
    return line["gain"]


def unit_legs(steps, warmup):
    import numpy as np
    import torch
    from masklab_hip import _lib, ops
    rng = np.random.default_rng(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for dtype in (torch.float32, torch.float16):
        for (B, H, W, Ka, Kx, N, s) in UNITS:
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            f = lambda *sh, sd=1.0: (rng.standard_normal(sh) * sd).astype(np.float32)
            d = ops.DeviceDualConv(f(1, 1, Ka, N, sd=Ka ** -0.5), f(N), f(1, 1, Kx, N, sd=Kx ** -0.5), f(N), "cuda")
            a = torch.randn(B, Ho, Wo, Ka, device="cuda", generator=g).to(dtype)
            x = torch.randn(B, H, W, Kx, device="cuda", generator=g).to(dtype)
            kept = {}

            def fused():
                kept["fused"] = ops.conv1x1_dual(a, x, d, s)

            def two():
                sc = ops.conv2d(x, d.dc_x, stride=s, padding="valid")
                kept["two"] = ops.conv2d(a, d.dc_a, padding="valid", act=_lib.ACT_RELU, residual=sc)

            t = alternate({"fused": fused, "two_launches": two}, steps, warmup)
            diff = float((kept["fused"].float() - kept["two"].float()).abs().max())
            M, es = B * Ho * Wo, a.element_size()
            fused_bytes = es * (a.numel() + B * Ho * Wo * Kx + M * N)          # inputs sampled once, output once
            med = float(np.median(t["fused"])) * 1e-3
            report("unit", t, {"dtype": str(dtype).split(".")[-1], "x": f"{B}x{H}x{W}x{Kx}", "a": f"{B}x{Ho}x{Wo}x{Ka}",
                               "N": N, "stride": s, "max_abs_diff_between_paths": diff,
                               "fused_TFLOP_s": round(2.0 * M * N * (Ka + Kx) / med / 1e12, 1),
                               "fused_algorithmic_TB_s": round(fused_bytes / med / 1e12, 3),
                               "shortcut_tensor_MB_not_written": round(es * M * N / 1e6, 1)})
            del a, x, d, kept
            torch.cuda.empty_cache()


def model_legs(steps, warmup, forward):
    import numpy as np
    import torch
    from masklab_hip import ModelConfiguration, ops, retinamasklab as R
    cfg = ModelConfiguration()
    assert cfg.backbone.backbone_type == "resnet50"
    _, model = R.construct_masklab_networks(cfg)
    model.load_weights(model.init_weights(5), "cuda:0")
    bb = model.backbone_network
    images = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (8, 1024, 1024, 3), dtype=np.uint8)).cuda()
    gains, before = {}, ops.PROJECTION_FUSION

    def path(mode, fn):
        def run():
            ops.set_projection_fusion(mode)
            fn()
        return run

    for math in ("f32", "f16s"):
        ops.set_conv_math(math)
        for leg, fn in (("backbone", lambda: bb(images)), ("forward", lambda: model(images))):
            if leg == "forward" and not forward:
                continue
            t = alternate({"fused": path("on", fn), "two_launches": path("off", fn)}, steps, warmup)
            med = float(np.median(t["fused"]))
            gains[(leg, math)] = report(leg, t, {"shape": "8x1024x1024", "math": math,
                                                 "fused_img_s": round(8 / (med * 1e-3), 1)})
        ops.set_conv_math("f32")
    ops.set_projection_fusion(before)
    return gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--units-only", action="store_true")
    ap.add_argument("--skip-forward", action="store_true")
    args = ap.parse_args()
    unit_legs(args.steps, args.warmup)
    if not args.units_only:
        model_legs(args.steps, args.warmup, not args.skip_forward)


if __name__ == "__main__":
    main()
