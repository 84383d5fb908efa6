#!/usr/bin/env python3
"""One Winograd launch (conv_wino_f32) of a chosen head shape, N times -- the program scripts/kernel_pmc.sh runs under
rocprofv3 --pmc, and the A/B timer of two library builds.  GPU box:
    python3 scripts/wino_single.py [--shape all|NAME[,NAME...]] [--reps N] [--lib PATH] [--save DIR] [--time]
Shapes (8 x 1024^2 ResNeXt-50 bench step):
  tower   : the P3-P7 tower launch, `multi x5`: 8 images at 128^2, 64^2, 32^2, 16^2, 8^2, 128 -> 128, relu
  decoder : the 128^2 semantic / decoder conv, 8 images, 160 -> 128, relu
  mask    : the 14 x 14 mask-head launch, `multi x3`: 800 RoIs (100 per image) over three levels (400 / 250 / 150), 128 -> 128
  level128: the decoder's grid at 128 -> 128: with `decoder` (the same 1024 blocks, 8 K steps more) the time per K step
  cls_out : the class tower's output launch, `multi x5` like `tower`, 128 -> 75, sigmoid (two channel blocks, the second half dead)
  box_out : the box tower's output launch, 128 -> 60, no activation (one channel block)
  out32 / out96: the same launch at 128 -> 32 (one block, dead half) and 128 -> 96 (the widest of the 65..96 class)
--direct packs with the explicit tile code of the automatic choice (same packing, same direct kernel as without the Winograd
path), so a narrow shape can be timed on both kernels from one build;
--lib loads another build of the library (the product path has no override), so the parent's build and this one can be
timed in alternating processes; --save writes the sha256 of each output tensor's bytes to DIR/<shape>.sha256 (compare two builds
bit for bit); --time prints
the per-launch HIP-event time (median of 3 runs of N back-to-back launches) and the executed TF (2 x tiles x 16 positions x Cin x Cout per problem)."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd")]
import numpy as np
import torch

from masklab_hip import _lib, ops, packing

SHAPES = {
    "tower": (128, 128, [(8, 128), (8, 64), (8, 32), (8, 16), (8, 8)]),
    "decoder": (160, 128, [(8, 128)]),
    "mask": (128, 128, [(400, 14), (250, 14), (150, 14)]),
    "level128": (128, 128, [(8, 128)]),
    "cls_out": (128, 75, [(8, 128), (8, 64), (8, 32), (8, 16), (8, 8)]),
    "box_out": (128, 60, [(8, 128), (8, 64), (8, 32), (8, 16), (8, 8)]),
    "out32": (128, 32, [(8, 128), (8, 64), (8, 32), (8, 16), (8, 8)]),
    "out96": (128, 96, [(8, 128), (8, 64), (8, 32), (8, 16), (8, 8)]),
}
ACTS = {"cls_out": _lib.ACT_SIGMOID, "box_out": _lib.ACT_NONE}


def setup(name, seed=0, direct=False):
    cin, cout, levels = SHAPES[name]
    rng = np.random.default_rng(seed)
    w = (rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.normal(size=cout).astype(np.float32)
    tile = {128: 1, 64: 2, 32: 3}[packing.ntile_for(cout)] if direct else 0
    dc = ops.DeviceConv(packing.pack_dense(w, b, tile=tile), "cuda")
    probs, flops = [], 0.0
    for B, hw in levels:
        x = torch.from_numpy(rng.normal(size=(B, hw, hw, cin)).astype(np.float32)).cuda()
        out = torch.empty((B, hw, hw, cout), device="cuda")
        probs.append(dict(x=x, dc=dc, padding="same", act=ACTS.get(name, _lib.ACT_RELU), out=out))
        flops += 2.0 * B * ((hw + 1) // 2) ** 2 * 16 * cin * cout
    return probs, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="all (the three shipped shapes) or a comma-separated list of " + ", ".join(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lib", default=None, help="an experiment build of the library")
    ap.add_argument("--save", default=None, metavar="DIR", help="write the sha256 of each output to DIR/<shape>.sha256")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--direct", action="store_true", help="the direct kernel: pack with the automatic choice's explicit tile code")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    ops.set_conv_math("f32")
    names = ("tower", "decoder", "mask") if args.shape == "all" else tuple(args.shape.split(","))
    if any(n not in SHAPES for n in names):
        ap.error("--shape: all or names out of " + ", ".join(SHAPES))
    for name in names:
        probs, flops = setup(name, direct=args.direct)
        ops.PROFILE = []
        ops.conv2d_multi(probs)
        torch.cuda.synchronize()
        kernels = {rec["kernel"] for rec in ops.PROFILE}
        ops.PROFILE = None
        assert (kernels == {"conv_wino_f32"}) != args.direct, (name, kernels)
        times = []
        for _ in range(3):                          # back-to-back launches between two events: the per-launch mean
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                ops.conv2d_multi(probs)
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e) / args.reps)
        if args.save:
            os.makedirs(args.save, exist_ok=True)
            with open(os.path.join(args.save, "%s.sha256" % name), "w") as f:
                for i, pr in enumerate(probs):
                    f.write("%d %s\n" % (i, hashlib.sha256(pr["out"].cpu().numpy().tobytes()).hexdigest()))
        if args.time:
            ms = float(np.median(times))
            print(f"{name:8s} {1e3 * ms:8.1f} us  {flops / ms / 1e9:6.1f} TF executed  (median of 3 x {args.reps} launches)  {'/'.join(sorted(kernels))}", flush=True)
    print("done")


if __name__ == "__main__":
    main()
