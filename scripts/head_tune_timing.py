#!/usr/bin/env python3
"""One "heads" step and one "head_tune" step of TrainerModel.train_on_batch on the reference's default configuration at the
training batch of 8 images of 1024 x 1024 (scripts/train_step_timing.py's model and batch), measured in one job, and where
the difference goes.

`heads_ms` / `head_tune_ms`: the HIP-event time of a whole step, the two stages alternated step by step, the median of
`--steps` steps each after `--warmup`; the whole alternation `--runs` times (default 3) in this one process, median run and
spread over the runs.  Then, over `--steps` profiled head_tune steps (ops.PROFILE records an event pair around every
launcher): the stride-2 data-gradient kernel's launches ("conv_dgrad_s2"), the RoI align's backward
("roi_crop_resize_grad"), and an event pair around FeaturePyramid.backward as a whole -- each as milliseconds per step and as
a share of head_tune_ms - heads_ms.  (What the shares leave: MaskSubNet's input gradient, the towers' sums, the extra levels'
other launches, the larger optimizer and re-pack launches, host work.)  One JSON line.

Usage (GPU box):  timeout 900 python scripts/head_tune_timing.py [--runs 3] [--steps 5] [--warmup 2] [--batch 8] [--size 1024]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from train_step_timing import build  # noqa: E402

PARENT_HEADS_MS = 33.7                # profiles/r25_train_step.txt: the "heads" step before this stage existed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
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
        raise SystemExit("head_tune_timing: no GPU -- nothing is measured without one")
    trainer, batch = build(args.batch, args.size)
    opts = {"heads": RectifiedAdam(1e-4), "head_tune": RectifiedAdam(1e-4)}

    def step(stage):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        trainer.train_on_batch(batch, opts[stage], trainable=stage)
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for _ in range(args.warmup):
        for stage in opts:
            step(stage)
    runs = {stage: [] for stage in opts}
    for _ in range(args.runs):
        ms = {stage: [] for stage in opts}
        for _ in range(args.steps):
            for stage in opts:
                ms[stage].append(step(stage))
        for stage in opts:
            runs[stage].append(float(np.median(ms[stage])))
    # where the difference goes: profiled head_tune steps
    fpn = trainer.detection_networks[1]
    real_backward, fpn_events = fpn.backward, []

    def timed_backward(*a, **kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = real_backward(*a, **kw)
        e.record()
        fpn_events.append((s, e))
        return out

    parts = {"conv_dgrad_s2": 0.0, "roi_crop_resize_grad": 0.0}
    fpn.backward = timed_backward
    try:
        for _ in range(args.steps):
            ops.PROFILE = []
            trainer.train_on_batch(batch, opts["head_tune"], trainable="head_tune")
            torch.cuda.synchronize()
            for r in ops.PROFILE:
                if r["kernel"] in parts:
                    parts[r["kernel"]] += r["start"].elapsed_time(r["end"])
            ops.PROFILE = None
    finally:
        ops.PROFILE = None
        del fpn.backward
    parts["FeaturePyramid.backward"] = sum(s.elapsed_time(e) for s, e in fpn_events)
    med = {stage: float(np.median(v)) for stage, v in runs.items()}
    diff = med["head_tune"] - med["heads"]
    line = {"batch": args.batch, "size": args.size, "runs": args.runs, "steps": args.steps, "parent_heads_ms": PARENT_HEADS_MS}
    for stage, v in runs.items():
        line[f"{stage}_ms"] = {"median": round(med[stage], 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    line["difference_ms"] = round(diff, 3)
    for name, ms in parts.items():
        line[name] = {"ms_per_step": round(ms / args.steps, 4), "share_of_difference": round(ms / args.steps / diff, 4)}
    line["weights"] = {"heads": len(trainer.device_params()), "head_tune": len(trainer.device_params(stage="head_tune"))}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
