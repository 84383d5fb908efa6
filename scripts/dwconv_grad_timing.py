#!/usr/bin/env python3
"""The depthwise 3x3 convolution's backward (csrc/dwconv_grad.hip) at the shape the default configuration's 8 x 1024 x 1024
batch meets in the ASPP on ResNet-50: C5 = [8, 32, 32, 2048] at dilations 6, 12 and 18, and the whole semantic head's backward.

  d6 / d12 / d18   one dilation: ops.dwconv3x3_wgrad (dw + db) and ops.dwconv3x3_dgrad (dx), each alone;
  multi            the three dilations as ONE ops.dwconv3x3_wgrad_multi launch pair on their shared input, and ONE
                   ops.dwconv3x3_dgrad_multi launch into three dx tensors;
  head             ASPPNetwork + SegmentationSubNet at the default configuration (128 features, 16 groups, rates (6, 12, 18),
                   skip C3 = [8, 128, 128, 512] -> 32 features, depth 4, 3 classes): call_with_tape, and backward of both.

Per leg and direction:

  fused      the HIP launches of the op;
  torch      aten.convolution_backward (what autograd calls) with groups = C on the same tensors in channels-last form, the
             weight + bias gradient or the input gradient alone.  Not a product path: a yardstick only;
  floor_ms   each operand read once (dw + db: x and dy; dx: dy, plus the write of dx) at 4 856 GB/s, the copy rate DESIGN.md
             uses (profiles/r03_peaks.json copy_global_x4).  In `multi` the weight gradient's x is ONE tensor read by three
             problems: the floor counts it once.

Each number is the HIP-event time of `--inner` back-to-back calls divided by their number, `--steps` such windows after a
warm-up; median, min, max.  The calls of a window rotate through enough copies of the operands that their footprint exceeds
`--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold an operand from one call to the next.  One JSON line
per leg and direction; the fused gradients must agree with torch's to 1e-3 of the largest gradient, nothing else is asserted.

Usage (GPU box):  timeout 900 python scripts/dwconv_grad_timing.py [--steps 7] [--inner 10] [--warmup 2] [--legs d6,multi,head]
                  [--no-torch]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from generator_timing import time_launch  # noqa: E402

B, HW, C = 8, 32, 2048
RATES = (6, 12, 18)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--legs", default="d6,d12,d18,multi,head")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import keras_like, ops, packing
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_grad_timing: no GPU -- nothing is measured without one")
    with open(os.path.join(ROOT, "profiles", "r03_peaks.json")) as f:
        copy_rate = json.load(f)["copy_global_x4"]["read_plus_write_GBs"]
    gen = torch.Generator(device="cuda").manual_seed(23)
    randn = lambda *shape: torch.randn(shape, device="cuda", generator=gen)
    rng = np.random.default_rng(23)

    def stats(ms, enq):
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "enqueue_ms": round(float(np.median(enq)), 4)}

    def agree(got, want):
        return bool((got - want).abs().max() <= 1e-3 * want.abs().max().clamp(min=1e-30))

    def leg(name, rates):
        n = len(rates)
        ws = [rng.normal(0, 0.3, (3, 3, C, 1)).astype(np.float32) for _ in rates]
        wd = [torch.from_numpy(packing.pack_depthwise(w)).cuda() for w in ws]
        wt = [torch.from_numpy(np.ascontiguousarray(w.transpose(2, 3, 0, 1))).cuda() for w in ws]          # [C,1,3,3]
        act = B * HW * HW * C * 4
        per_copy = act * (1 + n)
        copies = min(64, max(2, math.ceil(args.footprint_mb * 2 ** 20 / per_copy)))
        sets = [(randn(B, HW, HW, C), [randn(B, HW, HW, C) for _ in rates]) for _ in range(copies)]
        dxs = [[torch.empty((B, HW, HW, C), device="cuda") for _ in rates] for _ in range(2)]               # written, never read
        kept = {}

        def wgrad(k):
            x, dys = sets[k]
            kept["wgrad"] = ops.dwconv3x3_wgrad_multi([dict(x=x, dy=dy, dilation=r) for dy, r in zip(dys, rates)])

        def dgrad(k):
            _, dys = sets[k]
            kept["dgrad"] = ops.dwconv3x3_dgrad_multi([dict(dy=dy, wgt=w, in_hw=(HW, HW), dilation=r, out=o)
                                                       for dy, w, r, o in zip(dys, wd, rates, dxs[k % 2])])

        def torch_back(k, mask):
            x, dys = sets[k]
            kept["torch"] = [torch.ops.aten.convolution_backward(dy.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), w, [C], [1, 1], [r, r],
                                                                 [r, r], False, [0, 0], C, mask) for dy, w, r in zip(dys, wt, rates)]

        for direction, fn, mask, nbytes in (("wgrad", wgrad, [False, True, True], act * (1 + n)),
                                            ("dgrad", dgrad, [True, False, False], act * 2 * n)):
            ms, enq = time_launch(fn, copies, args.steps, args.inner, args.warmup)
            line = dict(leg=name, direction=direction, x=[B, HW, HW, C], dilations=list(rates), copies_rotated=copies,
                        fused=stats(ms, enq))
            if not args.no_torch:
                ms_t, enq_t = time_launch(lambda k: torch_back(k, mask), copies, args.steps, args.inner, args.warmup)
                line["torch"] = stats(ms_t, enq_t)
                fn(0)
                torch_back(0, mask)
                torch.cuda.synchronize()
                if direction == "wgrad":
                    ok = all(agree(dk, t[1].permute(2, 3, 0, 1)) and agree(db, t[2]) for (dk, db), t in zip(kept["wgrad"], kept["torch"]))
                else:
                    ok = all(agree(dx, t[0].permute(0, 2, 3, 1)) for dx, t in zip(kept["dgrad"], kept["torch"]))
                line["gradients_agree"] = ok
                line["fused_faster_than_torch"] = bool(line["fused"]["ms_median"] < line["torch"]["ms_median"])
            floor_ms = nbytes / (copy_rate * 1e9) * 1e3
            line.update(bytes=nbytes, copy_rate_GBs=copy_rate, floor_ms=round(floor_ms, 4),
                        fused_over_floor=round(line["fused"]["ms_median"] / floor_ms, 2),
                        fused_GBs=round(nbytes / line["fused"]["ms_median"] / 1e6, 1))
            if direction == "wgrad":
                line["slices"] = list(ops.dwconv3x3_wgrad_plan((B, HW, HW, C), dilation=rates[0]))
            print(json.dumps(line), flush=True)
            if not args.no_torch:
                assert line["gradients_agree"], f"{name} {direction}: the fused gradient differs from torch's"
        del sets, kept, dxs
        torch.cuda.empty_cache()

    def head():
        from masklab_hip.layers.semantic import ASPPNetwork, SegmentationSubNet
        aspp = ASPPNetwork(num_features=128, atrous_rate=RATES, groups=16, name="aspp")
        seg = SegmentationSubNet(num_depth=4, num_features=128, num_skip_features=32, num_classes=3, groups=16, name="seg")
        c5, c3 = (B, HW, HW, C), (B, 128, 128, 512)
        seg.build([aspp.build(c5), c3])
        specs = dict(aspp.weight_specs())
        specs.update(seg.weight_specs())
        weights = keras_like.init_weights(specs, 0)
        for k in weights:                                   # the towers' init (stddev 0.01) starves a random backward of signal
            if k.endswith("/kernel"):
                weights[k] = rng.normal(0, 0.05, weights[k].shape).astype(np.float32)
        aspp.load_weights(weights, torch.device("cuda:0"))
        seg.load_weights(weights, torch.device("cuda:0"))
        x, skip, d_seg = randn(*c5), randn(*c3), randn(B, 128, 128, 3)
        state = {}

        def forward(k):
            a, ta = aspp.call_with_tape(x)
            _, ts = seg.call_with_tape([a, skip])
            state["tapes"] = (ta, ts)

        def backward(k):
            ta, ts = state["tapes"]
            (d_aspp, _), g = seg.backward(ts, d_seg, need_dx=(True, False))
            state["out"] = aspp.backward(ta, d_aspp, need_dx=False), g

        def both(k):
            forward(k)
            backward(k)

        for what, fn in (("call_with_tape", forward), ("call_with_tape + backward (head tune: no input gradients)", both)):
            ms, enq = time_launch(fn, 1, args.steps, max(1, args.inner // 2), 1)
            print(json.dumps(dict(leg="head", what=what, c5=list(c5), c3=list(c3), fused=stats(ms, enq))), flush=True)
        ops.PROFILE = []
        both(0)
        torch.cuda.synchronize()
        per = {}
        for rec in ops.PROFILE:
            per[rec["kernel"]] = per.get(rec["kernel"], 0.0) + rec["start"].elapsed_time(rec["end"])
        ops.PROFILE = None
        print(json.dumps(dict(leg="head", what="ms per op of one call_with_tape + backward (event pairs around each launcher)",
                              ms={k: round(v, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])})), flush=True)

    legs = args.legs.split(",")
    for r in RATES:
        if f"d{r}" in legs:
            leg(f"d{r}", (r,))
    if "multi" in legs:
        leg("multi", RATES)
    if "head" in legs:
        head()


if __name__ == "__main__":
    main()
