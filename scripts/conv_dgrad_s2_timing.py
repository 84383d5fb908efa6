#!/usr/bin/env python3
"""The stride-2 data gradient (csrc/conv_grad.hip, ops.conv2d_dgrad_s2) at three shapes, dx at

  [8,16,16,256]    from P7_conv on an 8 x 1024 x 1024 batch (3x3, 256 -> 256)
  [8,256,256,64]   a 3x3 stride-2 conv 64 -> 128 (SE-ResNet-34's stage transitions)
  [8,256,256,256]  a 1x1 stride-2 conv 256 -> 512 (ResNet-50's stage transitions)

Per shape, padding ((1, 1), (1, 1)) for the 3x3 convs and none for the 1x1 so that all three routes compute one function:

  s2           ops.conv2d_dgrad_s2;
  torch        aten.convolution_backward's input gradient alone (output_mask = [True, False, False]) on channels-last views of
               the same NHWC memory;
  zero_insert  what the project could run before the kernel existed: dy scattered into a zeroed stride-1 gradient
               [B,H,W,cout] (a fill and a strided copy, both timed), then ops.conv2d_dgrad -- four times the MACs;
  floor        the forward's MACs (B Ho Wo kh kw cin cout) at the measured fp32 MFMA rate, or dy, the kernel and dx once at
               the sustained copy rate, whichever is larger (profiles/r03_peaks.json).

Each number is the HIP-event time of `--inner` back-to-back calls divided by their number, `--steps` such windows after a
warm-up; the median of the windows.  The calls of a window rotate through enough copies of the operands that their footprint
exceeds `--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold an operand from one call to the next.  The
whole table is measured `--runs` times (default 3) in this one process on one device; a cell shows the median run and the
spread (min - max) over the runs.  One JSON line per shape and run, then the table.  The three routes must agree to 1e-3 of
the largest value; nothing else is asserted.

Usage (GPU box):  timeout 900 python scripts/conv_dgrad_s2_timing.py [--runs 3] [--steps 5] [--inner 10] [--warmup 2]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from generator_timing import time_launch  # noqa: E402

# (dx shape [B,H,W,cin], cout, kernel)
SHAPES = [((8, 16, 16, 256), 256, 3), ((8, 256, 256, 64), 128, 3), ((8, 256, 256, 256), 512, 1)]
LEGS = ("s2", "torch", "zero_insert")


def measure(shape, cout, k, args, peaks, gen):
    import numpy as np
    import torch
    from masklab_hip import ops, packing
    B, H, W, cin = shape
    pad = (k - 1) // 2
    padding = ((pad, pad), (pad, pad))
    Ho, Wo, _, _ = packing.resolve_padding(H, W, k, k, 2, 1, padding)
    w = torch.randn((k, k, cin, cout), device="cuda", generator=gen) * 0.05
    dc = ops.DeviceConv(packing.pack_dense(w.cpu().numpy()), torch.device("cuda"))
    w_t = w.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)        # [cout,cin,kh,kw], NHWC memory
    per_copy = 4 * (B * Ho * Wo * cout + B * H * W * cin)
    copies = min(64, max(2, math.ceil(args.footprint_mb * 2 ** 20 / per_copy)))
    dys = [torch.randn((B, Ho, Wo, cout), device="cuda", generator=gen) for _ in range(copies)]
    dxs = [torch.empty(shape, device="cuda") for _ in range(copies)]
    dzs = [torch.empty((B, H, W, cout), device="cuda") for _ in range(copies)]
    x_like = torch.empty(shape, device="cuda").permute(0, 3, 1, 2)                    # only its sizes and strides are read
    kept = {}

    def s2(i):
        kept["s2"] = ops.conv2d_dgrad_s2(dys[i], dc, shape, padding=padding, out=dxs[i])

    def torch_leg(i):
        kept["torch"] = torch.ops.aten.convolution_backward(dys[i].permute(0, 3, 1, 2), x_like, w_t, None, [2, 2], [pad, pad],
                                                            [1, 1], False, [0, 0], 1, [True, False, False])[0]

    def zero_insert(i):
        dz = dzs[i]
        dz.zero_()
        dz[:, ::2, ::2].copy_(dys[i])
        kept["zero_insert"] = ops.conv2d_dgrad(dz, dc, shape, stride=1, padding=padding, out=dxs[i])

    fns = {"s2": s2, "torch": torch_leg, "zero_insert": zero_insert}
    macs = B * Ho * Wo * k * k * cin * cout
    nbytes = 4 * (B * Ho * Wo * cout + w.numel() + B * H * W * cin)
    floor_ms = max(2.0 * macs / (peaks["TFLOPs"] * 1e12), nbytes / (peaks["GBs"] * 1e9)) * 1e3
    line = {"dx": list(shape), "cout": cout, "k": k, "copies_rotated": copies, "macs": macs, "bytes": nbytes,
            "floor_ms": round(floor_ms, 4)}
    for leg in LEGS:
        ms, enq = time_launch(fns[leg], copies, args.steps, args.inner, args.warmup)
        line[leg] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "enqueue_ms": round(float(np.median(enq)), 4)}
    got = {}
    for leg in LEGS:
        fns[leg](0)
        torch.cuda.synchronize()
        t = kept[leg]
        got[leg] = (t.permute(0, 2, 3, 1) if leg == "torch" else t).clone()
    top = got["s2"].abs().max()
    line["agree"] = all(bool((got[leg] - got["s2"]).abs().max() <= 1e-3 * top) for leg in ("torch", "zero_insert"))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv_dgrad_s2_timing: no GPU -- nothing is measured without one")
    with open(os.path.join(ROOT, "profiles", "r03_peaks.json")) as f:
        p = json.load(f)
    peaks = {"TFLOPs": p["mfma_f32_32x32x2_f32"]["TFLOPs"], "GBs": p["copy_global_x4"]["read_plus_write_GBs"]}
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")]
    lines = {s[0]: [] for s in shapes}
    for run in range(args.runs):
        gen = torch.Generator(device="cuda").manual_seed(run)
        for shape, cout, k in shapes:
            line = measure(shape, cout, k, args, peaks, gen)
            line["run"] = run
            print(json.dumps(line), flush=True)
            assert line["agree"], f"{shape}: the three routes differ"
            lines[shape].append(line)
            torch.cuda.empty_cache()
    print()
    print(f"ms per call: median run (min - max over {args.runs} runs); floor at {peaks['TFLOPs']} TF fp32 MFMA / {peaks['GBs']:.0f} GB/s")
    print("| dx | conv | " + " | ".join(LEGS) + " | floor |")
    print("|---|---|" + "---|" * (len(LEGS) + 1))
    for shape, cout, k in shapes:
        cells = []
        for leg in LEGS:
            ms = sorted(l[leg]["ms_median"] for l in lines[shape])
            cells.append(f"{float(np.median(ms)):.3f} ({ms[0]:.3f} - {ms[-1]:.3f})")
        print(f"| {list(shape)} | {k}x{k} {shape[3]}->{cout} | " + " | ".join(cells) + f" | {lines[shape][0]['floor_ms']:.3f} |")
    for shape, cout, k in shapes:
        med = lambda leg: float(np.median([l[leg]["ms_median"] for l in lines[shape]]))
        for other in ("torch", "zero_insert"):
            verdict = "faster than" if med("s2") < med(other) else "SLOWER than"
            print(f"{list(shape)}: s2 {med('s2'):.3f} ms is {verdict} {other} {med(other):.3f} ms")


if __name__ == "__main__":
    main()
