#!/usr/bin/env python3
"""The dataset's two polygon launches (csrc/polygon.hip) at the serving size, each beside the byte floor of its output
writes and beside the library's host loops.

  8 x 1080 x 1920, 16 instance planes per image (12 polygons of 24..96 vertices inside their bounding-box windows, 4 padding
  planes of -1), S = 3 semantic labels: per image 2 + 1 + 10 label polygons and 4 polygons in the except group.

Per launch: HIP-event time of `--inner` back-to-back launches divided by their number, `--steps` such windows after
`--warmup`, the median with min / max.  The launches of a window rotate through enough output tensors that their footprint
exceeds `--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold an output from one launch to the next, so
the times are HBM times.  Vertices, offsets and windows are uploaded once, before the clock starts (a few hundred KB; in
MaskLabDataset they go up with every batch).

The launches are enqueued from Python (ctypes, argument checks), so an event time per launch is an UPPER bound of the
kernel's time: `enqueue_ms` is the host's wall-clock time per launch for enqueueing a window, and where it is not well
below the event time the launch is host-bound (`host_bound`).

floor_ms = output bytes (B*n*H*W for the planes, B*H*W*S for the maps; the vertices are noise beside them) / the measured
copy rate `copy_global_x4` of profiles/r03_peaks.json, which counts bytes read plus bytes written: a kernel that only
writes moves half the bytes of a copy of the same size, so the floor is the time of a copy of HALF the output.
host_ms: ml_polygon_reference_host on `--threads` (16) host threads, one task per plane / per image (the semantic maps
have only 8 images to hand out), wall clock, best of 2.  One JSON line per launch; nothing is asserted.

Usage (GPU box):  timeout 600 python scripts/dataset_timing.py [--steps 9] [--inner 100] [--warmup 1]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

B, H, W, N, S = 8, 1080, 1920, 16, 3
LIVE = 12


def blob(rng, cx, cy, r, V):
    import numpy as np
    t = np.sort(rng.uniform(0, 2 * np.pi, V))
    rad = r * rng.uniform(0.6, 1.0, V)
    return np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], axis=1)


def pack(polys):
    import numpy as np
    offsets = np.zeros(len(polys) + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in polys])
    return np.ascontiguousarray(np.concatenate(polys + [np.zeros((0, 2))]), np.float64), offsets


def workload(seed=1080):
    import numpy as np
    rng = np.random.default_rng(seed)
    planes, windows, polys, group_offsets = [], [], [], [0]
    for _ in range(B):
        for k in range(N):
            if k >= LIVE:
                planes.append(np.zeros((0, 2)))
                windows.append([0, 0, 0, 0])
                continue
            p = blob(rng, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(40, 300), int(rng.integers(24, 97)))
            lo, hi = p.min(axis=0), p.max(axis=0)
            planes.append(p)
            windows.append([max(int(lo[0]), 0), max(int(lo[1]), 0), max(int(hi[0]), 0), max(int(hi[1]), 0)])
        groups = [[blob(rng, rng.uniform(0, W), rng.uniform(0, H), 500, 48) for _ in range(2)],
                  [blob(rng, W / 2, H * 0.7, 900, 200)],
                  [blob(rng, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(10, 60), 16) for _ in range(10)],
                  [blob(rng, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(80, 250), 40) for _ in range(4)]]
        for g in groups:
            polys += g
            group_offsets.append(len(polys))
    verts, plane_offsets = pack(planes)
    sem_verts, poly_offsets = pack(polys)
    return (verts, plane_offsets, np.array(windows, np.int32)), (sem_verts, poly_offsets, np.array(group_offsets, np.int32))


def time_launch(fn, copies, steps, inner, warmup):
    """fn(k) launches on output k.  -> (event ms per launch, host enqueue ms per launch), one value each per window."""
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


def host_loops(inst, sem, threads):
    """-> (instance ms, semantic ms, instance planes, semantic maps): wall clock of the host entry on `threads` threads."""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from masklab_hip import ops
    verts, plane_offsets, windows = inst
    sem_verts, poly_offsets, group_offsets = sem

    def plane(p):
        b, e = int(plane_offsets[p]), int(plane_offsets[p + 1])
        return ops.polygon_reference_host("instance", verts[b:e], np.array([0, e - b], np.int32), 1, 1, H, W, windows=windows[p:p + 1])

    def image(b):
        g = group_offsets[b * (S + 1):(b + 1) * (S + 1) + 1]
        po = poly_offsets[g[0]:g[-1] + 1]
        return ops.polygon_reference_host("semantic", sem_verts[po[0]:po[-1]], (po - po[0]).astype(np.int32), 1, S, H, W,
                                          group_offsets=(g - g[0]).astype(np.int32))
    best = [math.inf, math.inf]
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(2):
            t0 = time.perf_counter()
            planes = list(pool.map(plane, range(B * N)))
            t1 = time.perf_counter()
            maps = list(pool.map(image, range(B)))
            t2 = time.perf_counter()
            best = [min(best[0], (t1 - t0) * 1e3), min(best[1], (t2 - t1) * 1e3)]
    return best[0], best[1], np.concatenate(planes).reshape(B, N, H, W), np.concatenate(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ops
    if not torch.cuda.is_available():
        sys.exit("dataset_timing: needs the GPU (no fallback: a CPU time says nothing about the kernels)")
    peaks = json.load(open(os.path.join(ROOT, "profiles", "r03_peaks.json")))
    rate = peaks["copy_global_x4"]["read_plus_write_GBs"] * 1e9
    inst, sem = workload()
    host_inst_ms, host_sem_ms, host_planes, host_maps = host_loops(inst, sem, args.threads)
    dev = lambda a: torch.from_numpy(a).cuda()
    d_inst, d_sem = [dev(a) for a in inst], [dev(a) for a in sem]
    launches = {
        "instance": (lambda out: ops.polygon_instance_masks(*d_inst, B, N, H, W, out=out), (B, N, H, W), torch.int8, host_inst_ms,
                     host_planes, int(inst[1][-1]), B * LIVE),
        "semantic": (lambda out: ops.polygon_semantic_maps(*d_sem, B, S, H, W, out=out), (B, H, W, S), torch.uint8, host_sem_ms,
                     host_maps, int(sem[1][-1]), len(sem[1]) - 1),
    }
    for name, (op, shape, dtype, host_ms, host_out, vertices, polygons) in launches.items():
        nbytes = int(np.prod(shape))
        copies = max(1, math.ceil(args.footprint_mb * 2 ** 20 / nbytes))
        outs = [torch.empty(shape, dtype=dtype, device="cuda") for _ in range(copies)]
        op(outs[0])
        torch.cuda.synchronize()
        same = bool(np.array_equal(outs[0].cpu().numpy(), host_out))
        ms, enq = time_launch(lambda k: op(outs[k]), copies, args.steps, args.inner, args.warmup)
        med, enq_med = float(np.median(ms)), float(np.median(enq))
        floor_ms = nbytes / rate * 1e3
        print(json.dumps({"launch": name, "shape": str(shape), "vertices": vertices, "polygons": polygons, "set_fraction": round(float((host_out == 1).mean()), 4),
                          "device_equals_host": same, "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "enqueue_ms": round(enq_med, 4), "host_bound": bool(enq_med > 0.8 * med), "window_ms": round(med * args.inner, 1),
                          "output_bytes": nbytes, "floor_ms": round(floor_ms, 4), "time_over_floor": round(med / floor_ms, 2),
                          "time_over_floor_min_max": [round(min(ms) / floor_ms, 2), round(max(ms) / floor_ms, 2)],
                          "written_GBs": round(nbytes / med / 1e6, 1), "copies_rotated": copies,
                          "copy_rate_GBs": peaks["copy_global_x4"]["read_plus_write_GBs"], "host_threads": args.threads,
                          "host_ms": round(host_ms, 1), "host_over_device": round(host_ms / med, 1)}), flush=True)
        del outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
