#!/usr/bin/env python3
"""The generator's three resize launches (csrc/cv_resize.hip) at the sizes a validation run meets, each beside its byte
floor.

  linear  8 x 1080 x 1920 at scale 0.5 -> 512 x 960 (INTER_LINEAR, ratio 2.11 x 2.0)
  area    8 x 2048 x 2048 at scale 0.5 -> 1024 x 1024 (exactly 2x on both axes: the INTER_AREA path)

each with 3 image channels, 3 semantic channels and 16 instance planes per image, half of them -1 padding.  Per launch:
HIP-event time of `--inner` back-to-back launches divided by their number, `--steps` such windows after `--warmup`, the
median with min / max.  The launches of a window rotate through enough copies of source and
destination that their footprint exceeds `--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold a
source from one launch to the next, so the times are HBM times.

The launches are enqueued from Python (ctypes, argument checks), so an event time per launch is an UPPER bound of the
kernel's time: `enqueue_ms` is the host's wall-clock time per launch for enqueueing a window, and where it is not well
below the event time the launch is host-bound and the kernel is faster than the line says (`host_bound`).  Kernel times
proper come from running this script under `rocprofv3 --kernel-trace --stats` (a run of its own; kernel names
`resize_kernel<0, uint8>` = fixed point, `<1, float>` / `<1, uint8>` = float64 + round).

floor_ms = (source bytes the taps touch + destination bytes) / the measured copy rate `copy_global_x4` of
profiles/r03_peaks.json.  The source bytes are counted from the resize's own taps: the distinct source rows x distinct
source columns x C of every live plane, one byte of every skipped plane.  One JSON line per launch; nothing is asserted.

Usage (GPU box):  timeout 600 python scripts/generator_timing.py [--steps 9] [--inner 300] [--warmup 1]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

B, SEM, PLANES = 8, 3, 16
LEGS = [("linear", 1080, 1920), ("area", 2048, 2048)]


def touched(src, dst):
    """Distinct source indices one axis of the resize reads (include/masklab_hip.h, "Generator resizes": the axis rule)."""
    import numpy as np
    if src == 2 * dst:
        return src
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * (1.0 / (dst / src)) - 0.5).astype(np.float32)
    s0 = np.clip(np.floor(f).astype(np.int64), 0, src - 1)
    return len(np.union1d(s0, np.minimum(s0 + 1, src - 1)))


def time_launch(fn, copies, steps, inner, warmup):
    """fn(k) launches on copy k.  -> (event ms per launch, host enqueue ms per launch), one value each per window."""
    import time
    import torch
    for k in range(max(warmup * inner, copies)):
        fn(k % copies)
    torch.cuda.synchronize()
    out, enq, k = [], [], 0
    for _ in range(steps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        for _ in range(inner):
            fn(k % copies)
            k += 1
        end.record()
        enq.append((time.perf_counter() - t0) * 1e3 / inner)
        end.synchronize()
        out.append(start.elapsed_time(end) / inner)
    return out, enq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--footprint-mb", type=int, default=768)
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ops
    if not torch.cuda.is_available():
        sys.exit("generator_timing: needs the GPU (no fallback: a CPU time says nothing about the kernels)")
    peaks = json.load(open(os.path.join(ROOT, "profiles", "r03_peaks.json")))
    rate = peaks["copy_global_x4"]["read_plus_write_GBs"] * 1e9
    gen = torch.Generator(device="cuda").manual_seed(1080)
    for leg, H, W in LEGS:
        th, tw = int(H * 0.5) // 32 * 32, int(W * 0.5) // 32 * 32
        pix_needed = touched(H, th) * touched(W, tw)
        masks = torch.randint(0, 2, (B, PLANES, H, W), dtype=torch.int8, device="cuda", generator=gen)
        masks[:, PLANES // 2:] = -1
        launches = {
            "images": (torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen),
                       lambda x, out: ops.cv_resize_linear(x, th, tw, out=out), torch.uint8, B * pix_needed * 3),
            "semantic": (torch.randint(0, 2, (B, H, W, SEM), dtype=torch.uint8, device="cuda", generator=gen),
                         lambda x, out: ops.cv_resize_linear_round(x, th, tw, out=out), torch.float32, B * pix_needed * SEM),
            "masks": (masks, lambda x, out: ops.cv_resize_linear(x, th, tw, skip_minus_one=True, out=out), torch.int8,
                      B * (PLANES // 2) * pix_needed + B * (PLANES // 2)),
        }
        for name, (x, op, out_dtype, src_bytes) in launches.items():
            first = op(x, None)
            dst_bytes = first.numel() * first.element_size()
            copies = max(1, math.ceil(args.footprint_mb * 2 ** 20 / (x.numel() + dst_bytes)))
            xs = [x] + [x.clone() for _ in range(copies - 1)]
            outs = [first] + [torch.empty_like(first) for _ in range(copies - 1)]
            ms, enq = time_launch(lambda k: op(xs[k], outs[k]), copies, args.steps, args.inner, args.warmup)
            med, enq_med = float(np.median(ms)), float(np.median(enq))
            floor_ms = (src_bytes + dst_bytes) / rate * 1e3
            print(json.dumps({"leg": leg, "launch": name, "kernel": "direct byte gathers", "shape": f"{tuple(x.shape)} -> {tuple(first.shape)}",
                              "out_dtype": str(out_dtype).replace("torch.", ""), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                              "ms_max": round(max(ms), 4), "enqueue_ms": round(enq_med, 4), "host_bound": bool(enq_med > 0.8 * med),
                              "window_ms": round(med * args.inner, 1), "source_bytes_needed": int(src_bytes),
                              "source_bytes_whole": int(x.numel()), "destination_bytes": int(dst_bytes),
                              "floor_ms": round(floor_ms, 4), "time_over_floor": round(med / floor_ms, 2),
                              "achieved_GBs_of_needed_bytes": round((src_bytes + dst_bytes) / med / 1e6, 1),
                              "copies_rotated": copies, "copy_rate_GBs": peaks["copy_global_x4"]["read_plus_write_GBs"]}), flush=True)
            del xs, outs, first
        del launches, masks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
