#!/usr/bin/env python3
"""One whole TrainerModel.train_on_batch of the reference's default configuration (ResNet-50, plain heads four units deep)
at the training batch of 8 images of 1024 x 1024, split per op group: what share of a step the re-pack takes.

Every launcher of masklab_hip.ops records a HIP-event pair around its launches when ops.PROFILE is a list; the records of
`--steps` steps after `--warmup` are summed per launcher name and the names are folded into groups (forward convolutions,
GroupNorm, the weight gradients, losses, the optimizer, the re-pack, ...; the data gradients run the forward conv
kernels on transposed weights and are recorded under the convolutions).  `step_ms` is the event time of a whole
step without the profile's events, median of the steps; the groups' share is of the sum of the recorded launches (what is
between launches -- host work, torch ops -- is `step_ms` minus that sum).  One JSON line per group and one for the step.

Usage (GPU box):  timeout 600 python scripts/train_step_timing.py [--steps 5] [--warmup 2] [--batch 8] [--size 1024]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd")]

GROUPS = (("repack", ("repack_weights",)), ("optimizer", ("optimizer_step",)),
          ("weight gradients", ("wgrad", "out1x1_grad", "grad_relayout")),
          ("GroupNorm backward", ("groupnorm_chunk_grad", "groupnorm_grad")), ("other backward", ("_grad", "gather")),
          ("losses and targets", ("loss", "assign", "iou", "best_prior")), ("GroupNorm forward", ("groupnorm",)),
          ("convolutions: forward and data gradients", ("conv", "deconv", "stem", "wino")))


def group_of(kernel):
    for name, keys in GROUPS:
        if any(k in kernel for k in keys):
            return name
    return "other forward (resize, RoI align, detection, pooling)"


def build(B, S):
    """-> (the default configuration's trainer with init_weights(seed=2) loaded, a batch of B images of S x S on the device)"""
    import numpy as np
    import torch
    from masklab_hip import ModelConfiguration, retinamasklab as R
    trainer, _ = R.construct_masklab_networks(ModelConfiguration(), with_trainer=True)
    trainer.load_weights(trainer.init_weights(seed=2), "cuda:0")
    rng = np.random.default_rng(3)
    G = 6
    gt_boxes = np.full((B, G, 6), -1, np.float32)
    gt_masks = np.full((B, G, S, S), -1, np.int8)
    for b in range(B):
        for g in range(G - 1):
            cx, cy = rng.uniform(0.2 * S, 0.8 * S, 2)
            w, h = rng.uniform(0.05 * S, 0.3 * S, 2)
            gt_boxes[b, g] = (cx, cy, w, h, rng.integers(0, 5), 1)
            gt_masks[b, g] = 0
            gt_masks[b, g, int(max(cy - h / 2, 0)):int(cy + h / 2), int(max(cx - w / 2, 0)):int(cx + w / 2)] = 1
    batch = dict(images=rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8), gt_boxes=gt_boxes,
                 gt_boxes_exist=np.ones((B, 5), np.float32), gt_masks=gt_masks,
                 gt_seg=(rng.random((B, S, S, 3)) < 0.5).astype(np.uint8), gt_seg_exist=np.ones((B, 3), np.float32))
    batch = {k: torch.as_tensor(v).to("cuda:0") for k, v in batch.items()}      # on the device once: a generator's job
    return trainer, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ops
    from masklab_hip.optimizers import RectifiedAdam
    if not torch.cuda.is_available():
        raise SystemExit("train_step_timing: no GPU -- nothing is measured without one")
    trainer, batch = build(args.batch, args.size)
    opt = RectifiedAdam(1e-4)
    for _ in range(args.warmup):
        trainer.train_on_batch(batch, opt)
    torch.cuda.synchronize()
    whole = []
    for _ in range(args.steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        trainer.train_on_batch(batch, opt)
        e.record()
        e.synchronize()
        whole.append(s.elapsed_time(e))
    sums, launches = {}, {}
    for _ in range(args.steps):
        ops.PROFILE = []
        trainer.train_on_batch(batch, opt)
        torch.cuda.synchronize()
        for r in ops.PROFILE:
            g = group_of(r["kernel"])
            sums[g] = sums.get(g, 0.0) + r["start"].elapsed_time(r["end"])
            launches[g] = launches.get(g, 0) + 1
        ops.PROFILE = None
    total = sum(sums.values()) / args.steps
    for g, ms in sorted(sums.items(), key=lambda kv: -kv[1]):
        print(json.dumps({"group": g, "ms_per_step": round(ms / args.steps, 4), "launchers_per_step": launches[g] // args.steps,
                          "share_of_launches": round(ms / args.steps / total, 4)}))
    print(json.dumps({"step_ms_median": round(float(np.median(whole)), 3), "step_ms_min": round(min(whole), 3),
                      "step_ms_max": round(max(whole), 3), "recorded_launch_ms": round(total, 3), "batch": args.batch, "size": args.size,
                      "head_weights": len(trainer.device_params())}))


if __name__ == "__main__":
    main()
