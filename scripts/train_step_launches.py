#!/usr/bin/env python3
"""The launches of one TrainerModel.call and one TrainerModel.train_on_batch at the configuration of the training-step tests
(tests/train_step_cases.py: the default heads one unit deep, 2 x 64 x 96), as text: for each of the two, every launcher
record of ops.PROFILE as `kernel | shape label` in launch order, then every entry of ops.LAUNCH_LOG (the dense convs' shape
labels and K slices).  Two trees that launch the same work write the same file, so a change that must add, drop, reorder or
rename no launch is checked by running this on both and diffing the two files.

Usage (GPU box):  timeout 300 python scripts/train_step_launches.py OUT.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "tests")]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    import torch
    import train_step_cases as TC
    from masklab_hip import ops
    from masklab_hip.optimizers import AdamW
    if not torch.cuda.is_available():
        raise SystemExit("train_step_launches: no GPU -- nothing is launched without one")
    trainer, _ = TC.build()
    trainer.load_weights(trainer.init_weights(seed=2), "cuda:0")
    batch = TC.inputs()
    lines = []
    for what, run in (("call", lambda: trainer(batch)), ("train_on_batch", lambda: trainer.train_on_batch(batch, AdamW(1e-3)))):
        ops.PROFILE, ops.LAUNCH_LOG = [], []
        try:
            run()
            torch.cuda.synchronize()
            lines.append(f"== {what}: {len(ops.PROFILE)} launcher records")
            lines += [f"{r['kernel']} | {r.get('shape', '')}" for r in ops.PROFILE]
            lines.append(f"== {what}: {len(ops.LAUNCH_LOG)} dense-conv launches")
            lines += [f"{label} | {' '.join(str(k) for k in splits)}" for label, splits in ops.LAUNCH_LOG]
        finally:
            ops.PROFILE = ops.LAUNCH_LOG = None
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"train_step_launches: {len(lines)} lines -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
