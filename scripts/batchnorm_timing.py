#!/usr/bin/env python3
"""BatchNormalization's training forward and backward (csrc/batchnorm.hip) at ResNet-50's BatchNormalization shapes on an
8 x 1024 x 1024 batch (134 217 728 elements the first two, then half as many from one to the next):

  [8,512,512,64]  [8,256,256,256]  [8,128,128,512]  [8,64,64,1024]  [8,32,32,2048]

Per shape:

  train / train_relu      ops.batchnorm_train (statistics, finish with the moving update, apply), without and with the fused ReLU;
  grad / grad_relu        ops.batchnorm_grad (reduce, finish, apply): dx, dgamma, dbeta; with relu the mask is read from y;
  torch_train             torch.nn.functional.batch_norm(training=True) on a channels-last view of the same NHWC memory, the
                          running statistics updated;
  torch_backward          its autograd backward alone (torch.autograd.grad on a graph built beforehand, not timed);
  floor                   the bytes the passes must move over the sustained copy rate of profiles/r03_peaks.json -- forward: x
                          read twice and y written, 12 B per element; backward: x and dy read twice and dx written, 20 B per
                          element, and y read twice more with a fused ReLU, 28 B.

Each number is the HIP-event time of `--inner` back-to-back calls divided by their number, `--steps` such windows after a
warm-up; the median of the windows.  The calls of a window rotate through enough copies of the operands that their footprint
exceeds `--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold an operand from one call to the next.  The
whole table is measured `--runs` times (default 3) in this one process on one device; a cell shows the median run and the
spread (min - max) over the runs.  One JSON line per shape and run, then the table.  y and dx of both sides must agree to
1e-3 of the largest value, nothing else is asserted.

Usage (GPU box):  timeout 900 python scripts/batchnorm_timing.py [--runs 3] [--steps 5] [--inner 10] [--warmup 2]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from generator_timing import time_launch  # noqa: E402

EPS, MOMENTUM = 1e-3, 0.99
SHAPES = [(8, 512, 512, 64), (8, 256, 256, 256), (8, 128, 128, 512), (8, 64, 64, 1024), (8, 32, 32, 2048)]
LEGS = ("train", "train_relu", "torch_train", "grad", "grad_relu", "torch_backward")
FLOOR_BYTES = {"train": 12, "train_relu": 12, "torch_train": 12, "grad": 20, "grad_relu": 28, "torch_backward": 20}


def measure(shape, args, rate, gen):
    import numpy as np
    import torch
    from masklab_hip import ops
    F = torch.nn.functional
    C = shape[-1]
    gamma = torch.rand(C, device="cuda", generator=gen) + 0.5
    beta = torch.randn(C, device="cuda", generator=gen) * 0.1
    mm, mv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    first = (torch.randn(shape, device="cuda", generator=gen) + 0.3, torch.randn(shape, device="cuda", generator=gen))
    per_copy = sum(t.numel() * t.element_size() for t in first)
    copies = min(64, max(2, math.ceil(args.footprint_mb * 2 ** 20 / per_copy)))
    sets = [first] + [tuple(t.clone() for t in first) for _ in range(copies - 1)]
    # what the backward legs read, made beforehand: the forward's y and saved statistics, torch's graph
    fwd = {relu: [ops.batchnorm_train(x, gamma, beta, mm, mv, MOMENTUM, EPS, relu=relu) for x, _ in sets] for relu in (False, True)}
    tg, tb = gamma.detach().requires_grad_(True), beta.detach().requires_grad_(True)
    leaves = [x.permute(0, 3, 1, 2).detach().requires_grad_(True) for x, _ in sets]
    graphs = [F.batch_norm(l, None, None, tg, tb, True, 1.0 - MOMENTUM, EPS) for l in leaves]
    kept = {}

    def train(k, relu=False):
        kept["train"] = ops.batchnorm_train(sets[k][0], gamma, beta, mm, mv, MOMENTUM, EPS, relu=relu)

    def grad(k, relu=False):
        y, saved = fwd[relu][k][:2]
        kept["grad"] = ops.batchnorm_grad(sets[k][0], sets[k][1], saved, gamma, y=y if relu else None, relu=relu)

    def torch_train(k):
        with torch.no_grad():
            kept["torch_train"] = F.batch_norm(sets[k][0].permute(0, 3, 1, 2), mm, mv, gamma, beta, True, 1.0 - MOMENTUM, EPS)

    def torch_backward(k):
        kept["torch_backward"] = torch.autograd.grad(graphs[k], (leaves[k], tg, tb), sets[k][1].permute(0, 3, 1, 2), retain_graph=True)

    fns = {"train": train, "train_relu": lambda k: train(k, True), "torch_train": torch_train, "grad": grad,
           "grad_relu": lambda k: grad(k, True), "torch_backward": torch_backward}
    line = {"x": list(shape), "copies_rotated": copies, "copy_rate_GBs": rate}
    for leg in LEGS:
        ms, enq = time_launch(fns[leg], copies, args.steps, args.inner, args.warmup)
        floor_ms = FLOOR_BYTES[leg] * first[0].numel() / (rate * 1e9) * 1e3
        line[leg] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "enqueue_ms": round(float(np.median(enq)), 4), "floor_ms": round(floor_ms, 4)}
    train(0), grad(0), torch_train(0), torch_backward(0)
    torch.cuda.synchronize()
    pairs = ((kept["train"][0], kept["torch_train"].permute(0, 2, 3, 1)), (kept["grad"][0], kept["torch_backward"][0].permute(0, 2, 3, 1)),
             (kept["grad"][2], kept["torch_backward"][1]), (kept["grad"][3], kept["torch_backward"][2]))
    line["agree"] = all(bool((got - want).abs().max() <= 1e-3 * want.abs().max()) for got, want in pairs)
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
        raise SystemExit("batchnorm_timing: no GPU -- nothing is measured without one")
    with open(os.path.join(ROOT, "profiles", "r03_peaks.json")) as f:
        rate = json.load(f)["copy_global_x4"]["read_plus_write_GBs"]
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")]
    lines = {shape: [] for shape in shapes}
    for run in range(args.runs):
        gen = torch.Generator(device="cuda").manual_seed(run)
        for shape in shapes:
            line = measure(shape, args, rate, gen)
            line["run"] = run
            print(json.dumps(line), flush=True)
            assert line["agree"], f"{shape}: the kernels' results differ from torch's"
            lines[shape].append(line)
            torch.cuda.empty_cache()
    print()
    print(f"ms per call: median run (min - max over {args.runs} runs); floor at {rate:.0f} GB/s")
    print("| x | " + " | ".join(LEGS) + " | floor fwd / bwd / bwd relu |")
    print("|---|" + "---|" * (len(LEGS) + 1))
    for shape in shapes:
        cells = []
        for leg in LEGS:
            ms = sorted(l[leg]["ms_median"] for l in lines[shape])
            cells.append(f"{float(np.median(ms)):.3f} ({ms[0]:.3f} - {ms[-1]:.3f})")
        fl = lines[shape][0]
        floors = " / ".join(f"{fl[leg]['floor_ms']:.3f}" for leg in ("train", "grad", "grad_relu"))
        print(f"| {list(shape)} | " + " | ".join(cells) + f" | {floors} |")
    for shape in shapes:
        med = lambda leg: float(np.median([l[leg]["ms_median"] for l in lines[shape]]))
        for ours, theirs in (("train", "torch_train"), ("grad", "torch_backward")):
            verdict = "faster than" if med(ours) < med(theirs) else "SLOWER than"
            print(f"{list(shape)}: {ours} {med(ours):.3f} ms is {verdict} {theirs} {med(theirs):.3f} ms")


if __name__ == "__main__":
    main()
