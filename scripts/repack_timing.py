#!/usr/bin/env python3
"""The re-pack of stepped weights (csrc/repack.hip, ops.repack_weights) over the head convolutions of the default
configuration: every plain Conv2D and Conv2DTranspose under the class, box, mask, ASPP and segmentation sub-networks, each
with the forms a float32 training step touches -- the dense packing and bias, the Winograd form of the stride-1 3x3 convs,
the data gradient's transposed packing (`dgrad`) and its Winograd form, the transposed conv's 1x1 twin.  (Not in the set:
the ASPP's concat slices and the mask tail's tables, which the layers bind themselves once they have `repack()`.)

  repack     one ops.repack_weights call over all of them with a kept job list and table (one launch; the table is uploaded
             once and skips its host checks while it is handed the same job dicts with their tensors where they were);
  launch     ml_repack_f32 alone on the table that call left on the device;
  floor      masters read once + every form written once = `bytes`; a plain device copy that moves as many bytes
             (bytes / 2 read, bytes / 2 written) measured here gives floor_ms;
  host       the route it replaces: the stepped masters copied to the host, `load_weights` of the same layers, the same
             lazy forms touched again (wall clock, device synchronised).

Each device number is the HIP-event time of `--inner` back-to-back calls divided by their number, `--steps` such windows
after a warm-up; median, min, max.  The calls rotate through enough copies of every tensor that their footprint exceeds
`--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold a tensor from one call to the next.  One JSON line per
leg; the ratio to the floor is reported, nothing is asserted.

Usage (GPU box):  timeout 600 python scripts/repack_timing.py [--steps 7] [--inner 10] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from generator_timing import time_launch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--footprint-mb", type=int, default=768)
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import ModelConfiguration, _lib, keras_like as K, ops, retinamasklab as R
    if not torch.cuda.is_available():
        raise SystemExit("repack_timing: no GPU -- nothing is measured without one")
    device = torch.device("cuda:0")
    cfg = ModelConfiguration()
    _, model = R.construct_masklab_networks(cfg)
    weights = model.init_weights(seed=1)
    model.load_weights(weights, device)
    heads = [model.detection_networks[2], model.detection_networks[3], model.instance_networks[3]] + list(model.semantic_networks)

    def walk(layer):
        yield layer
        for ch in layer.children():
            yield from walk(ch)

    layers = [l for h in heads for l in walk(h)
              if (type(l) is K.Conv2D and not l.fold_bn and not l.image_input) or type(l) is K.Conv2DTranspose]

    def touch(l):
        """The forms a float32 training step reads.  -> the layer's DeviceConvs"""
        if type(l) is K.Conv2DTranspose:
            l.dev1x1.dgrad
            return [(l.dev, "deconv", 1), (l.dev1x1, "deconv", 4)]
        dc = l.dev
        wino = dc.p.KH == 3 and dc.p.KW == 3 and dc.p.n_pad <= 128
        if l.strides[0] == 1:
            dc.dgrad
            if wino:
                dc.wgt_wino
            if wino and dc.dgrad.p.n_pad <= 128:
                dc.dgrad.wgt_wino
        return [(dc, "conv", 1)]

    def stats(ms):
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    jobs = []
    for l in layers:
        mk = torch.from_numpy(weights[f"{l.name}/kernel"]).to(device)
        mb = torch.from_numpy(weights[f"{l.name}/bias"]).to(device) if f"{l.name}/bias" in weights else None
        for dc, layout, reps in touch(l):
            dc.bind_master(mk, mb if dc.bias is not None else None, layout=layout, bias_reps=reps)
            jobs += dc.repack_jobs()
    table = ops.RepackTable()
    ops.repack_weights(jobs, table)
    nbytes, units = table.nbytes, table.units
    master_bytes = sum(4 * j["N"] * j["C"] * j["KH"] * j["KW"] for j in jobs)

    def clone(job):
        c = lambda t: None if t is None else t.clone()
        side = lambda d: None if d is None else {k: (c(v) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        return dict(job, src=c(job["src"]), src_bias=c(job["src_bias"]), bias=c(job["bias"]), fwd=side(job["fwd"]), tr=side(job["tr"]))

    copies = max(2, -(-args.footprint_mb * (1 << 20) // nbytes))
    sets = [(jobs, table)] + [([clone(j) for j in jobs], ops.RepackTable()) for _ in range(copies - 1)]
    ms, enq = time_launch(lambda k: ops.repack_weights(*sets[k]), copies, args.steps, args.inner, args.warmup)
    lib = _lib.load()

    def launch(k):                                          # the launch alone, its table as the call above left it
        t = sets[k][1]
        lib.ml_repack_f32(ops._ptr_as(t.table, _lib.RepackJob), t.n, t.units, ops._stream())

    lms, lenq = time_launch(launch, copies, args.steps, args.inner, args.warmup)
    half = nbytes // 2 // 16 * 16
    bufs = [(torch.empty(half, dtype=torch.uint8, device=device), torch.empty(half, dtype=torch.uint8, device=device))
            for _ in range(copies)]
    cms, _ = time_launch(lambda k: bufs[k][1].copy_(bufs[k][0]), copies, args.steps, args.inner, args.warmup)
    floor = float(np.median(cms))
    print(json.dumps({"leg": "repack", "layers": len(layers), "jobs": len(jobs), "units": units, "bytes": nbytes,
                      "master_bytes": master_bytes, "copies": copies, **stats(ms), "enqueue_ms": round(float(np.median(enq)), 4),
                      "GBs": round(nbytes / np.median(ms) / 1e6, 1)}))
    print(json.dumps({"leg": "launch", **stats(lms), "enqueue_ms": round(float(np.median(lenq)), 4),
                      "GBs": round(nbytes / np.median(lms) / 1e6, 1)}))
    print(json.dumps({"leg": "floor", "copy_bytes_each_way": half, **stats(cms), "GBs": round(2 * half / floor / 1e6, 1),
                      "repack_over_floor": round(float(np.median(ms)) / floor, 2),
                      "launch_over_floor": round(float(np.median(lms)) / floor, 2)}))

    # the host route: device -> host, numpy, host -> device
    masters = {}
    for l in layers:
        masters[f"{l.name}/kernel"] = torch.from_numpy(weights[f"{l.name}/kernel"]).to(device)
        if f"{l.name}/bias" in weights:
            masters[f"{l.name}/bias"] = torch.from_numpy(weights[f"{l.name}/bias"]).to(device)
    host_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stepped = {k: v.cpu().numpy() for k, v in masters.items()}
        for l in layers:
            l._load_own(stepped, device)
            touch(l)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"leg": "host", **stats(host_ms), "over_repack": round(float(np.median(host_ms) / np.median(ms)), 1)}))


if __name__ == "__main__":
    main()
