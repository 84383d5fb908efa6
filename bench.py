#!/usr/bin/env python3
"""bench.py -- images/sec of the MaskLab inference hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

N > 1: the driver launches this file under `python -m torch.distributed.run --nproc-per-node N ...` (one rank per
GPU, RCCL).  Started BARE with --gpus N > 1 (no WORLD_SIZE in the environment) it launches those N ranks itself --
before the parent touches the GPU -- relays rank 0's JSON line and exits with the launcher's code; when fewer than
N GPUs are visible it exits non-zero instead of silently measuring one GPU.

A "step" = one complete hot-path forward (preprocess, backbone, P6/P7, FPN, cls/box
towers, box decode, DetectionProposal, RoI crop, mask head, ASPP + decoder) over one batch of synthetic 1024x1024
RGB images already resident in HBM, plus -- for N>1 -- the RCCL all-gather of the fixed-capacity per-GPU detections,
issued on its own HIP stream so that it overlaps the next step's backbone.  Default workload = BASELINE.json
configs[2] (ResNeXt-50 full MaskLab, 8 images per GPU; N GPUs process 8*N images = configs[3] at N=8, weak scaling).
Weights are random-init of that architecture (no network for checkpoints), with the class logits widened x8 for the
TIMED batch so that the NMS and mask head carry their full load (100 RoIs / image).

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the K steps,
writes the last timed step's outputs if --dump-outputs DIR is given, and prints the line; `value` / `ms_per_step` are
that timing.  With --full it measures and checks everything else too, and the line carries these extra objects (each
can still be switched off by its --no-* option; without --full they are null):
  roofline     -- the dominant kernel (MFMA implicit-GEMM conv, 128x128 tile): algorithmic FLOP of all its launches
                  in one step / their summed duration, timed with HIP events on the launch stream in an instrumented
                  step; peak = 157.3 TFLOP/s (fp32 MFMA).  `traffic` comes from a committed PMC pass only when that
                  pass was taken on the kernel sources this library was built from (hash check), else null.
  cpu_baseline -- the oracle forward (a CPU restatement of the reference, "port": not TF-Keras) on the host cores, two ways:
                  pure NumPy / BLAS, and with its convolutions run by torch-CPU / oneDNN on all threads (what a competent
                  CPU forward costs); CPU model, thread counts, 1x1024^2 and 1x512^2 samples (warm-up + median), SURVEY
                  8(d); `value` = the fastest full-size setting, `cores` = its thread count.
  parity       -- image 0 of ONE full-batch GPU forward (the launch shapes that are timed) vs the oracle at full size on an
                  UN-saturated score fixture (oracle/fixtures.py): float outputs within 1e-3, (anchor, class) rows and
                  their ORDER exact.  The oracle is parity-UNPINNED against TensorFlow.
  f32x3        -- the same workload timed once more under the split-operand conv math (one GPU, fp32 workloads).
  other_configs -- short timings of the other BASELINE configs' shapes (default workload, one GPU).
  kernels      -- per-kernel time, FLOP and bytes of the instrumented step (with `roofline`).

--dump-outputs DIR: after the timed steps, rank 0 writes the output list of its LAST timed step (what a caller of the
forward receives; with N>1 also the merged detections) as DIR/<name>.npy, float32 (float64 for integer outputs), at
most DUMP_BUDGET_BYTES in all: an output that does not fit its share is replaced by a fixed, seeded sample of its
elements.  Inputs and weights are seeded, so two builds run with the same arguments can be compared output by output.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "instance-segmentation-road-project_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# `peak` of the roofline object = the guide's figures (/opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters):
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense fp16/bf16 MFMA peak, never the 2:1-sparsity figure
PEAK_HBM_GBS = 8000.0
# ... and beside them what an MI355X box of this pool SUSTAINS ("overwrite with a measured peak on the box"):
# profiles/*_peaks.json = scripts/calibrate/calib.hip -- back-to-back MFMA issue on non-zero register operands, and a
# 1 GiB copy (read + write) -- reported as `peak_measured` / `frac_of_measured`, never instead of `peak`.


def measured_peaks():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_peaks.json")))
    if not files:
        return None
    try:
        d = json.load(open(files[-1]))
        copies = [v["read_plus_write_GBs"] for k, v in d.items() if isinstance(v, dict) and "read_plus_write_GBs" in v]
        return {"source": os.path.relpath(files[-1], ROOT), "hbm_GBs": max(copies),
                "mfma_f32_TFLOPs": d["mfma_f32_32x32x2_f32"]["TFLOPs"],
                "mfma_f16_TFLOPs": max(d["mfma_f32_32x32x16_f16"]["TFLOPs"], d["mfma_f32_16x16x32_f16"]["TFLOPs"])}
    except Exception:
        return None

WORKLOADS = {
    # name: (backbone, per-GPU batch, H, W)
    "resnext50_full_b8_1024": ("resnext50", 8, 1024, 1024),      # BASELINE configs[2]/[3]
    "mobilenet_fpn_aspp_b1_1024": ("mobilenet", 1, 1024, 1024),  # BASELINE configs[1] (heads on device too)
    "mobilenet_full_b1_512": ("mobilenet", 1, 512, 512),         # BASELINE configs[0] shape
    "resnext50_full_b2_256": ("resnext50", 2, 256, 256),         # quick functional check
    "resnext101_full_b16_1280_f32": ("resnext101", 16, 1280, 1280),  # BASELINE configs[4] shape, fp32 path
    "resnext101_full_b16_1280_f16": ("resnext101", 16, 1280, 1280),  # BASELINE configs[4]: fp16 MFMA path, fp16 storage
    "resnext50_full_b8_1024_f16": ("resnext50", 8, 1024, 1024),      # configs[2] shape on the fp16 path
    "resnext50_full_b8_1024_x3": ("resnext50", 8, 1024, 1024),       # configs[2], fp32 tensors, split-operand products (f32x3)
    "resnext101_full_b16_1280_x3": ("resnext101", 16, 1280, 1280),   # configs[4] shape, fp32 tensors, f32x3
}
# which roofline binds each kernel class
HBM_BOUND = ("groupnorm", "gconv3x3", "dwconv3x3", "maxpool", "stem7x7s2_pool_h", "resize", "preprocess", "detection", "cast", "trim",
             "semantic_smoothing", "crop_pad", "instance_summary")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="resnext50_full_b8_1024", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: roofline / per-kernel step, f32x3 leg, cpu_baseline + parity, "
                         "other configs (the --no-* options below switch single parts off)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64, sampled to fit "
                         "DUMP_BUDGET_BYTES)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--quick-cpu-baseline", action="store_true",
                    help="one oracle forward only (parity + a single timing), no repeats / 1-thread / 512^2 legs")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-f32x3", action="store_true", help="skip the extra timed leg under the split-operand conv math")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short timings of the other BASELINE configs' shapes (default workload, one GPU)")
    ap.add_argument("--dump-launches", default=None,
                    help="write one line per profiled launch to this file (the roofline step: needs --full)")
    ap.add_argument("--host-inputs", action="store_true",
                    help="every step starts from pinned HOST uint8 images (PCIe-inclusive rate; not the headline)")
    ap.add_argument("--graph", action="store_true",
                    help="replay stage 1 of the forward from a hipGraph (launch-bound small batches)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_launches and not (args.full and not args.no_roofline):
        ap.error("--dump-launches writes the launches of the roofline step: it needs --full (and no --no-roofline)")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks here.  Nothing in this process has touched
    the GPU (torch.cuda.device_count() does not initialise it), and the ranks are CHILD processes -- never an exec
    of a process that holds the device."""
    import socket
    import torch
    rehearsal = os.environ.get("MASKLAB_BENCH_REHEARSAL") == "1"
    visible = torch.cuda.device_count()
    if visible < args.gpus and not rehearsal:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but only {visible} GPU(s) are visible: refusing to report a "
                         f"{args.gpus}-GPU number from fewer devices")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=dict(os.environ))     # (each rank sets HSA_ENABLE_IPC_MODE_LEGACY itself, see main)
    raise SystemExit(proc.returncode)


def csrc_hash():
    """sha256 over the kernel sources the shared library is built from (what a PMC pass must match)."""
    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    h.update(open(os.path.join(ROOT, "include", "masklab_hip.h"), "rb").read())
    return h.hexdigest()


DUMP_BUDGET_BYTES = 60 << 20          # --dump-outputs: all arrays together (under 64 MB with the .npy headers)


def dump_outputs(named, out_dir, budget=DUMP_BUDGET_BYTES):
    """[(name, tensor)] -> out_dir/<name>.npy.  Floating outputs are written as float32 (float64 stays float64), integer
    and bool outputs as float64, which holds them exactly.  Smallest first, every output gets an equal share of what the
    budget has left; one larger than its share is written as a fixed sample instead: `share` distinct flat indices,
    sorted, drawn by a generator seeded with the output's element count -- the same elements on every run and build.
    -> {name: {"shape": [...], "sampled": number of elements written or None when whole}}"""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)

    def np_dtype(t):
        return np.float32 if t.is_floating_point() and t.dtype != torch.float64 else np.float64

    _TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64}

    items = sorted(named, key=lambda nt: nt[1].numel() * np.dtype(np_dtype(nt[1])).itemsize)
    left, info = budget, {}
    for i, (name, t) in enumerate(items):
        t = t.detach()
        dt = np_dtype(t)
        share = left // (len(items) - i)
        n = t.numel()
        if n * np.dtype(dt).itemsize <= share:
            a = t.to(_TORCH_OF[dt]).cpu().numpy()
            sampled = None
        else:
            k = share // np.dtype(dt).itemsize
            idx = np.sort(np.random.default_rng(n).choice(n, size=k, replace=False, shuffle=False))
            a = t.reshape(-1)[torch.from_numpy(idx).to(t.device)].to(_TORCH_OF[dt]).cpu().numpy()
            sampled = int(k)
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        left -= a.nbytes
        info[name] = {"shape": list(t.shape), "sampled": sampled}
    return info


# bench.py kernel label -> substring of the demangled kernel name in a rocprofv3 pass (a label covers every instantiation
# of that tile shape: the plain kernel and the one that also writes the GroupNorm partial sums -- their launches are
# averaged together, weighted by dispatches)
_TRAFFIC_KERNELS = {
    "conv_mfma_128x128": ("conv_mfma_kernel<2, 2, 2, 2, 0,",), "conv_mfma_128x64": ("conv_mfma_kernel<2, 2, 2, 1, 0,",),
    "conv_mfma_128x32": ("conv_mfma_kernel<4, 1, 1, 1, 0,",),
    "conv_mfma_256x128_x3": ("conv_mfma_kernel<8, 1, 1, 4, 3,",), "conv_mfma_128x128_x3": ("conv_mfma_kernel<4, 1, 1, 4, 3,",),
    "conv_mfma_128x64_x3": ("conv_mfma_kernel<4, 1, 1, 2, 3,",),
    "conv_mfma_128x128_h": ("conv_mfma_kernel<2, 2, 2, 2, 2,",),
    "conv1x1_h256_h": ("conv1x1_h256_kernel", "conv1x1_h8_kernel"), "conv1x1_pipe_h": ("conv1x1_pipe_kernel<_Float16",),
    "conv1x1_pipe": ("conv1x1_pipe_kernel<float",), "conv1x1_pipe_x3": ("f32x3_t",), "gconv3x3_mfma4_h": ("gconv_mfma4h_kernel", "gconv16h_kernel"),
}


def measured_traffic(kernel_label, workload="resnext50_full_b8_1024"):
    """HBM bytes per launch of the dominant kernel from the newest committed PMC pass of THIS workload
    (profiles/*traffic.json, scripts/pmc_traffic.py: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same
    command, FETCH x2 gfx950 correction) -- ONLY if that pass recorded the hash of the current kernel sources; a stale
    pass gives None."""
    import glob
    want = _TRAFFIC_KERNELS.get(kernel_label)
    if want is None:
        return None
    try:
        h = csrc_hash()
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*traffic.json")), reverse=True):
            doc = json.load(open(f))
            if doc.get("workload", "resnext50_full_b8_1024") != workload or doc.get("source_sha256") != h:
                continue
            tot = n = 0
            for k, v in doc["kernels"].items():
                if any(w in k for w in want):
                    tot += v["hbm_bytes_per_launch"] * v["dispatches"]
                    n += v["dispatches"]
            if n:
                return round(tot / n)
    except Exception:
        pass
    return None


def build_model(backbone, device, seed=0, cls_scale=8.0):
    import numpy as np
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = backbone
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(seed)
    hot = dict(w)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            hot[k] = (w[k] * cls_scale).astype(np.float32)
    model.load_weights(hot, device)
    return cfg, model, w, hot


def _time_config(workload, device, math, graph, rank, steps=20, warmup=3):
    """One more model of WORKLOADS[workload], built, warmed and timed like the main loop (`steps` forwards between two
    synchronisations, inputs resident in HBM), under conv math `math`; released afterwards."""
    import numpy as np
    import torch
    from masklab_hip import ops
    backbone, B, H, W = WORKLOADS[workload]
    ops.set_conv_math(math)
    model = None
    try:
        cfg, model, _w, _hot = build_model(backbone, device)
        images = torch.from_numpy(np.random.default_rng(1234 + rank).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(device)
        if graph:
            model.enable_graphs(True)

        def run(defer):
            """`steps` forwards between two synchronisations.  defer=False: every forward hands over the model's real
            output list (under hipGraph: the ONE host read of the RoI level maxima + the two molding copies per
            forward, the MoldBatch equivalent); defer=True: replays enqueued back to back, nothing read or molded."""
            def one():
                o = model(images, defer=defer)
                return o
            one()
            torch.cuda.synchronize(device)
            for _ in range(warmup):
                one()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                one()
            torch.cuda.synchronize(device)
            return time.perf_counter() - t0

        dt = run(False)
        out = {"value": round(B * steps / dt, 3), "unit": "images/sec", "ms_per_step": round(1e3 * dt / steps, 3),
               "steps": steps, "warmup": warmup, "per_gpu_batch": B, "height": H, "width": W, "hipgraph": bool(graph),
               "dtype": ops.dtype_label()}
        if graph:
            # beside it: replays only (outputs deferred) -- the GPU-side cost of a forward when a serving loop overlaps the
            # read of forward i with forward i + 1; NOT a complete forward (no molded roi_boxes / roi_masks are produced)
            dte = run(True)
            out["ms_per_step_replay_only"] = round(1e3 * dte / steps, 3)
            out["note"] = ("ms_per_step / value: every forward returns the molded output list (host read of L ints + mold "
                           "copies included); ms_per_step_replay_only: graph replays back to back, outputs never molded")
        return out
    finally:
        ops.set_conv_math("f32")
        del model
        torch.cuda.empty_cache()


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _time_oracle(fn, repeats, max_seconds, min_repeats=1):
    """median wall time of up to `repeats` calls; stops early once max_seconds have been spent, but never before
    `min_repeats` calls."""
    times, t_all = [], time.perf_counter()
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
        if len(times) >= min_repeats and time.perf_counter() - t_all > max_seconds:
            break
    times.sort()
    return times[len(times) // 2], len(times)


class _TorchCpuConvs:
    """cpu_baseline ONLY (never the parity checker): for its duration the oracle's convolutions -- Conv2D, DepthwiseConv2D,
    the ResNeXt grouped 3x3, Conv2DTranspose 2x2 s2 and max-pool, i.e. every op that is a loop of NumPy GEMMs / einsums in
    oracle/tfops.py -- run through torch-CPU (oneDNN, channels-last, all threads) on the same weights and in the same
    graph; GroupNorm, resize, crop_and_resize, box decode and NMS stay the oracle's NumPy.  This is what a competent CPU
    forward of this network costs; kind: "port (torch-CPU convs)".  Exits restore the NumPy functions."""

    def __enter__(self):
        import numpy as np
        import torch
        import torch.nn.functional as F
        from oracle import masklab as O
        from oracle import tfops as T
        self._saved = {(m, n): getattr(m, n) for m, n in ((T, "conv2d"), (T, "depthwise_conv2d"), (T, "max_pool"),
                                                          (T, "conv2d_transpose_2x2_s2"), (O, "grouped_conv_fast"))}
        wcache = {}

        def nchw(x):                       # NHWC numpy -> NCHW view in channels-last memory (no copy)
            return torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)

        def nhwc(t):
            return t.permute(0, 2, 3, 1).contiguous().numpy()

        def weight(w, perm, groups_shape=None):
            key = (id(w), perm)
            if key not in wcache:
                t = torch.from_numpy(np.ascontiguousarray(np.transpose(w, perm)).astype(np.float32))
                if groups_shape is not None:
                    t = t.reshape(groups_shape)
                wcache[key] = (w, t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t)
            return wcache[key][1]

        def padded(x, kh, kw, stride, dilation, padding):
            _, _, pt, pb, pl, pr = T._resolve_padding(x, kh, kw, stride, dilation, padding)
            t = nchw(x.astype(np.float32, copy=False))
            return F.pad(t, (pl, pr, pt, pb)) if (pt or pb or pl or pr) else t

        def conv2d(x, w, b=None, stride=1, padding="same", dilation=1):
            kh, kw, _, _ = w.shape
            y = F.conv2d(padded(x, kh, kw, stride, dilation, padding), weight(w, (3, 2, 0, 1)),
                         None if b is None else torch.from_numpy(np.asarray(b, np.float32)), stride=stride, dilation=dilation)
            return nhwc(y)

        def depthwise_conv2d(x, w, stride=1, padding="same", dilation=1):
            kh, kw, cin, mult = w.shape
            wt = weight(w, (2, 3, 0, 1), (cin * mult, 1, kh, kw))          # out channel = cin_idx * mult + m
            return nhwc(F.conv2d(padded(x, kh, kw, stride, dilation, padding), wt, None, stride=stride, dilation=dilation,
                                 groups=cin))

        def grouped_conv_fast(x, dw_kernel, groups, c, stride):
            # out[g*c+m] = sum_i conv(x[g*c+i], K[.., g*c+i, m]) = conv2d(groups) with weight[g*c+m, i] = K[.., g*c+i, m]
            k = np.asarray(dw_kernel).reshape(3, 3, groups, c, c)           # [kh, kw, g, i, m]
            wt = weight(dw_kernel, (0, 1, 2, 3))                            # (cache key only)
            key = ("g", id(dw_kernel))
            if key not in wcache:
                wcache[key] = (dw_kernel, torch.from_numpy(np.ascontiguousarray(np.transpose(k, (2, 4, 3, 0, 1)))
                                                           .reshape(groups * c, c, 3, 3).astype(np.float32))
                               .contiguous(memory_format=torch.channels_last))
            del wt
            t = F.pad(nchw(x.astype(np.float32, copy=False)), (1, 1, 1, 1))
            return nhwc(F.conv2d(t, wcache[key][1], None, stride=stride, groups=groups))

        def conv2d_transpose_2x2_s2(x, w, b=None):
            wt = weight(w, (3, 2, 0, 1))                                     # [cin, cout, 2, 2]
            return nhwc(F.conv_transpose2d(nchw(x.astype(np.float32, copy=False)), wt,
                                           None if b is None else torch.from_numpy(np.asarray(b, np.float32)), stride=2))

        def max_pool(x, k=3, stride=2):
            return nhwc(F.max_pool2d(nchw(x.astype(np.float32, copy=False)), k, stride))

        T.conv2d, T.depthwise_conv2d, T.max_pool, T.conv2d_transpose_2x2_s2 = conv2d, depthwise_conv2d, max_pool, conv2d_transpose_2x2_s2
        O.grouped_conv_fast = grouped_conv_fast
        return self

    def __exit__(self, *exc):
        for (m, n), f in self._saved.items():
            setattr(m, n, f)
        return False


def cpu_baseline_and_parity(cfg, model, weights, hot_weights, backbone, batch, device, f16, quick, extra_modes=()):
    """The oracle (the CPU restatement of the reference forward) as checker and as the timed CPU baseline.
    batch: the bench batch, uint8 [B,H,W,3] on the device; the oracle runs its image 0, the GPU side of the parity check
    runs the WHOLE batch in one forward (the launches bench.py times) and image 0 of that forward is compared.
    -> (cpu_baseline, parity of the current conv math, {mode: parity} for `extra_modes` -- the same oracle outputs, the
    GPU forward repeated under that mode)."""
    import numpy as np
    import torch
    from threadpoolctl import threadpool_info, threadpool_limits
    from oracle import fixtures as FX
    from oracle import masklab as O
    from oracle import metrics as OM
    img = batch[:1].cpu().numpy()
    H, W = img.shape[1:3]
    cores = os.cpu_count() or 1
    torch.set_num_threads(cores)
    blas = [int(i.get("num_threads", 0)) for i in threadpool_info() if i.get("user_api") == "blas"]
    blas_threads = max(blas) if blas else cores

    # ---- fixture: un-saturated scores (distinct fp32 values), threshold in a score gap, order stability checked
    scale = FX.KNOWN_SCALE.get((backbone, H)) if H == W else None
    notes = {}
    if scale is None:                       # small workloads: one extra detection-only oracle pass picks the scale
        c1, l1 = O.inference_forward(cfg, weights, img, literal_groups=False, with_instance=False, with_semantic=False)
        scale, _ = FX.choose_logit_scale(cfg, c1, l1, H, W)
        notes["scale_chosen_by"] = "choose_logit_scale (extra detection-only oracle pass)"
        if scale is None:
            scale, notes["scale_chosen_by"] = 8.0, "no order-stable scale found: x8 (order not required)"
    w_fix = FX.scale_cls_logits(weights, scale)

    def oracle_forward(image=img):
        return O.inference_forward(cfg, w_fix, image, literal_groups=False, return_internals=True,
                                   min_confidence=lambda c: FX.gap_threshold(c)[0])

    t0 = time.perf_counter()
    want, internals = oracle_forward()       # warm-up of the timing AND the parity reference
    first_dt = time.perf_counter() - t0
    thr = internals["min_confidence"]

    # ---- timings: all BLAS threads, 8 threads and 1 thread at full size; all / 1 thread at 512^2.
    # `value` is the FASTEST full-size figure (the oracle's many small GEMMs do not scale over 64+ BLAS threads: on the
    # EPYC 9575F box one thread beats all of them), `cores` the thread count it was measured with.
    samples, threads_of = {}, {}
    full = f"1x{H}x{W}"
    if quick:
        samples[f"{full} all threads"] = (first_dt, 1)
        threads_of[f"{full} all threads"] = blas_threads
    else:
        # median of up to 5 after the warm-up, at least 3 for EVERY thread setting, each leg capped in
        # wall time so that the default run stays within minutes (`repeats` reports the n each median is over)
        reps = lambda n_min, budget: _time_oracle(oracle_forward, 5, budget, n_min)
        samples[f"{full} all threads"] = reps(3, 45.0)
        threads_of[f"{full} all threads"] = blas_threads
        if blas_threads > 8:
            with threadpool_limits(limits=8):
                samples[f"{full} 8 threads"] = reps(3, 30.0)
            threads_of[f"{full} 8 threads"] = 8
        with threadpool_limits(limits=1):
            samples[f"{full} 1 thread"] = reps(3, 30.0)
        threads_of[f"{full} 1 thread"] = 1
        if min(H, W) > 512:
            small = np.ascontiguousarray(img[:, :512, :512])
            oracle_forward(small)
            samples["1x512x512 all threads"] = _time_oracle(lambda: oracle_forward(small), 5, 12.0, 3)
            with threadpool_limits(limits=1):
                samples["1x512x512 1 thread"] = _time_oracle(lambda: oracle_forward(small), 5, 12.0, 3)
    # ---- the same forward with its convolutions on torch-CPU (oneDNN): what a competent CPU implementation costs.  The
    # patch lives in THIS leg only; the parity reference above came from the unpatched NumPy oracle.
    torch_tag = "torch-CPU convs"
    # Thread counts: 16 (or every core of a smaller host), then 32 where the host has them, then 1.  NOT "all threads" on a
    # big host: with 64 intra-op threads the many small convs of the towers thrash (round 4 box: 54 s per forward against
    # 1.3 s with 16 threads) -- a data point that only costs minutes.
    t_main = min(16, cores)
    legs = [t_main] + ([] if quick else ([32] if cores >= 32 else []) + ([1] if t_main > 1 else []))
    with _TorchCpuConvs():
        for li, nt in enumerate(legs):
            torch.set_num_threads(nt)
            try:
                with threadpool_limits(limits=nt):
                    if li == 0:
                        oracle_forward()                         # warm-up (oneDNN primitive caches, weight re-layouts)
                    k_nt = f"{full} {torch_tag}, {nt} thread{'s' if nt > 1 else ''}"
                    samples[k_nt] = (_time_oracle(oracle_forward, 1, 0.0) if quick else
                                     _time_oracle(oracle_forward, 5 if li == 0 else 3, 25.0, 3 if li == 0 else 2))
                    threads_of[k_nt] = nt
            finally:
                torch.set_num_threads(cores)
    best = min((k for k in samples if k.startswith(full)), key=lambda k: samples[k][0])
    dt, n_rep = samples[best]
    on_torch = torch_tag in best
    cpu = {"value": round(1.0 / dt, 4), "unit": "images/sec", "cores": threads_of[best],
           "kind": "port (torch-CPU convs)" if on_torch else "port",
           "sample": f"1 image {H}x{W}, full hot-path forward of the oracle (CPU restatement, not TF-Keras) "
                     f"{'with its convolutions on torch-CPU / oneDNN' if on_torch else 'in NumPy / BLAS'}: fastest setting "
                     f"({best.split(' ', 1)[1]}), median of {n_rep} after 1 warm-up, {dt:.2f}s each; the NumPy-only figures "
                     f"are beside it in images_per_sec",
           "cpu_model": _cpu_model(), "host_cores": cores, "blas_threads": blas_threads,
           "images_per_sec": {k: round(1.0 / v[0], 4) for k, v in samples.items()},
           "seconds": {k: round(v[0], 2) for k, v in samples.items()},
           "repeats": {k: v[1] for k, v in samples.items()}}
    if f16:                                  # the fp16 mode has its own (looser) bar: tests/test_gpu_f16.py
        return cpu, None, {}
    names = ["cls_pred", "loc_pred", "roi_boxes", "roi_masks", "seg_pred"]
    ref = dict(zip(names, want))
    # stability of the fixture itself: the oracle's kept list under +-3e-5 score noise (GPU deviation ~1e-5)
    boxes = FX.boxes_from(cfg, ref["loc_pred"], H, W)
    _, stable = FX.order_stability(cfg, ref["cls_pred"], boxes, thr, trials=8)
    _, gap = FX.gap_threshold(ref["cls_pred"])

    def gpu_parity():
        return _gpu_parity(cfg, model, w_fix, hot_weights, batch, device, thr, ref, internals, stable, gap, scale, notes)

    parity = gpu_parity()
    extra = {}
    from masklab_hip import ops
    base_mode = ops.CONV_MATH
    for mode in extra_modes:
        ops.set_conv_math(mode)
        try:
            extra[mode] = gpu_parity()
        finally:
            ops.set_conv_math(base_mode)
    return cpu, parity, extra


def _gpu_parity(cfg, model, w_fix, hot_weights, batch, device, thr, ref, internals, stable, gap, scale, notes):
    """GPU side of the parity check under the current conv math: the WHOLE bench batch in one forward -- the same launch
    shapes as the timed steps -- with the fixture's class-output kernels and threshold; image 0 of that forward is what
    is compared with the oracle.  (The timed steps run with x8 class logits so that NMS and the mask head carry their
    full load; only the class towers' output convs differ, so `timed_forward` additionally checks that loc_pred and
    seg_pred of the x8-logit forward are BIT-identical to the checked forward's.)"""
    import numpy as np
    import torch
    from oracle import fixtures as FX
    from oracle import metrics as OM
    names = ["cls_pred", "loc_pred", "roi_boxes", "roi_masks", "seg_pred"]
    hot = dict(zip(names, model(batch)))                   # the timed configuration, as timed
    hot_loc, hot_seg = hot["loc_pred"].clone(), hot["seg_pred"].clone()
    del hot
    model.reload_class_outputs(w_fix)
    old_thr = model.detection_proposal.min_confidence
    model.detection_proposal.min_confidence = thr
    try:
        outs = model(batch, want_kept=True)
        det0 = model.last_detections
        timed_equal = bool(torch.equal(outs[1], hot_loc) and torch.equal(outs[4], hot_seg))
        lcounts = det0["level_counts"].cpu().numpy()
        gpu_kept = det0["kept"][0, :int(det0["counts"][0])].cpu().numpy()
        # image 0 of the batch, molded as the model molds it when it is run alone (reference misc.py:231-286)
        # (only image 0 of the per-anchor / per-pixel tensors crosses PCIe; the RoI tensors are re-molded from the batch's)
        got = FX.image_of_batch(names, [(o[:1] if n in ("cls_pred", "loc_pred", "seg_pred") else o).cpu().numpy()
                                        for n, o in zip(names, outs)], lcounts, 0)
    finally:
        model.detection_proposal.min_confidence = old_thr
        model.reload_class_outputs(hot_weights)          # back to the timed configuration
    got = dict(zip(names, got))
    diffs = {}
    for n in ("cls_pred", "loc_pred", "seg_pred", "roi_masks"):
        diffs[n] = float(np.abs(got[n].astype(np.float64) - ref[n]).max()) if got[n].shape == ref[n].shape else None
    ref_kept = internals["kept"][:, 1:]                          # (anchor, class) of the image, oracle order
    order_exact = bool(gpu_kept.shape == ref_kept.shape and np.array_equal(gpu_kept, ref_kept))
    rows_exact = bool(got["roi_boxes"].shape == ref["roi_boxes"].shape and
                      np.array_equal(got["roi_boxes"][..., 4], ref["roi_boxes"][..., 4]) and
                      np.array_equal(got["roi_boxes"] == -1, ref["roi_boxes"] == -1))
    if rows_exact:
        diffs["roi_boxes.score"] = float(np.abs(got["roi_boxes"][..., 5] - ref["roi_boxes"][..., 5]).max())
        diffs["roi_boxes.xywh(rel)"] = float((np.abs(got["roi_boxes"][..., :4] - ref["roi_boxes"][..., :4]) /
                                              np.maximum(np.abs(ref["roi_boxes"][..., :4]), 1.0)).max())
    # precision / recall / F at IoU 0.5 (reference engine/metrics.py:109-165) of the GPU detections
    # against the oracle's -- the stand-in for "box AP vs Keras ref", 1.0 = same detections
    pr, rc, fm = OM.detection_iou_metric(got["roi_boxes"], ref["roi_boxes"])
    # an unstable fixture is a FAILED parity leg, not a waiver of the order requirement
    ok = bool(all(v is not None and v <= 1e-3 for v in diffs.values()) and rows_exact and
              float(fm[0]) >= 0.999 and order_exact and stable == 8)
    ok = ok and timed_equal
    parity = {"image": f"rank 0, image 0 of ONE {int(batch.shape[0])}-image forward (the timed launch shapes)", "tolerance": 1e-3,
              "timed_forward": {"loc_pred_and_seg_pred_bit_identical_to_the_checked_forward": timed_equal,
                                "note": "the timed steps differ from the checked forward only in the class towers' output "
                                        "kernels (x8 logits: full NMS / mask-head load)"},
              "fixture": dict({"cls_logit_scale": scale, "min_confidence": thr, "threshold_gap": float(f"{gap:.3e}"),
                               "candidates": int((ref["cls_pred"] >= thr).sum()),
                               "max_score": round(float(ref["cls_pred"].max()), 4),
                               "oracle_order_stable_under_3e-5_noise": f"{stable}/8"}, **notes),
              "max_abs_diff": {k: (None if v is None else float(f"{v:.3e}")) for k, v in diffs.items()},
              "detections": int(len(ref_kept)), "order_exact": order_exact, "rows_exact": rows_exact,
              "detection_precision": round(float(pr[0]), 6), "detection_recall": round(float(rc[0]), 6),
              "detection_fmeasure": round(float(fm[0]), 6), "ok": ok}
    return parity


def main():
    args = parse_args()
    # The host driver of this pool supports dmabuf IPC only: without this RCCL's (and torch's) cross-process buffer
    # sharing fails with `hipIpcGetMemHandle: invalid argument`.  Set in EVERY rank before torch initialises -- the
    # driver's launch (`torch.distributed.run ... bench.py`) and the self-spawned one reach this line alike.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    world_env = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and world_env is None:
        spawn_ranks(args)                      # does not return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(world_env or "1")
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} != WORLD_SIZE {world}")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    # MASKLAB_BENCH_REHEARSAL=1: rehearse the N>1 code path on a ONE-GPU box -- every rank on cuda:0, gloo
    # instead of RCCL.  The numbers of such a run mean nothing; the driver's real runs never set it.
    rehearsal = os.environ.get("MASKLAB_BENCH_REHEARSAL") == "1"
    if rehearsal:
        import faulthandler
        faulthandler.enable()
    if not rehearsal and local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} has no GPU (LOCAL_RANK {local_rank}, "
                         f"{torch.cuda.device_count()} visible): one process per GPU")
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    from masklab_hip import _lib, ops, parallel
    _lib.check(_lib.load().ml_device_check(), "ml_device_check")
    backbone, B, H, W = WORKLOADS[args.workload]
    f16 = args.workload.endswith("_f16")
    if f16:
        ops.set_conv_math("f16s")      # BASELINE config 5: fp16 MFMA, fp16 tensors in the backbone body, fp32 heads
    if args.workload.endswith("_x3"):
        ops.set_conv_math("f32x3")     # fp32 tensors; every product = 3 f16 MFMAs on operands split into two halves
    cfg, model, weights, hot_weights = build_model(backbone, device)
    images = torch.from_numpy(np.random.default_rng(1234 + rank).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(device)
    if args.graph:
        model.enable_graphs(True)
    if os.environ.get("MASKLAB_SIDE_STREAM") == "0":       # A/B knob; the model's default is on
        model.use_side_stream = False

    def mark(msg):
        if rehearsal:
            print(f"[rehearsal rank {rank}] {msg}", file=sys.stderr, flush=True)

    mark("model built")
    host_images = images.cpu().pin_memory() if args.host_inputs else None
    gather = parallel.AsyncDetectionGather(device) if world > 1 else None
    cap = cfg.detection.nms_max_output_size
    pending = []                               # all-gathers in flight (consumed one step later)

    def step(collective=True):
        # (under --graph the whole forward is one replay; the model then reads the L per-level RoI maxima and molds
        # roi_boxes / roi_masks -- the MoldBatch equivalent -- so every timed step yields the model's real output list)
        outs = model(host_images.to(device, non_blocking=True) if args.host_inputs else images)
        mark("forward enqueued")
        if gather is not None and collective:
            if pending:                        # the previous batch's merged detections: make them visible to this stream
                gather.wait(pending.pop())
            pending.append(gather.launch(model.last_detections["payload"], cap, snapshot=args.graph))
            mark("detections gather issued")
        return outs

    def drain():
        merged = None
        while pending:
            merged = gather.wait(pending.pop())
        return merged

    step()                                 # untimed priming step, whatever --warmup is: module load, kernel attributes,
    drain()                                # scratch buffers, allocator pools and the RCCL communicator are one-time costs
    torch.cuda.synchronize(device)
    for _ in range(args.warmup):
        step()
    drain()
    torch.cuda.synchronize(device)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        outs = step()
    merged = drain()                       # the last all-gather is inside the timed region too
    torch.cuda.synchronize(device)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if rehearsal else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    gathered_images = int(merged[0].shape[0]) if merged is not None else B
    if merged is not None:
        # the merge must be the reference's Concatenate(axis=0) (engine/parallel.py:92-107): B x world images, rank r's
        # rows at offset r.  Checked on the LAST timed step, outside the timed region; a mismatch is a failed run.
        own_p, own_c = parallel.unpack_payload(model.last_detections["payload"], cap)
        err = parallel.check_merged(merged[0], merged[1], own_p, own_c, rank, world)
        if err:
            raise SystemExit(f"bench.py: rank {rank}: merged detections are wrong: {err}")

    # how loaded NMS / mask head were: read from the LAST timed step (same batch, same weights as every timed step),
    # before anything below runs another forward and overwrites what it returned
    n_det = n_cand = []
    dumped = None
    if rank == 0:
        det = model.last_detections
        n_det = det["counts"].cpu().tolist() if det else []
        n_cand = (outs[0] >= cfg.detection.min_confidence).sum(dim=(1, 2)).cpu().tolist() if det else []
        if args.dump_outputs:
            named = list(zip(model.output_names, outs))
            if merged is not None:
                named += [("gathered_proposals", merged[0]), ("gathered_counts", merged[1])]
            dumped = dump_outputs(named, args.dump_outputs)

    roofline = None
    per_kernel = None
    if rank == 0 and args.full and not args.no_roofline:
        ops.PROFILE = []
        step(collective=False)          # rank 0 only: the other ranks are not in this step, so no collective
        torch.cuda.synchronize(device)
        recs, ops.PROFILE = ops.PROFILE, None
        if args.dump_launches:
            with open(args.dump_launches, "w") as f:
                for r in recs:
                    ms = r["start"].elapsed_time(r["end"])
                    f.write(f"{r['kernel']:28s} {r.get('shape', ''):60s} {1e3 * ms:9.1f} us "
                            f"{r['flops'] / 1e9 / max(ms, 1e-9):8.2f} TF/s {r['bytes'] / 1e6 / max(ms, 1e-9):9.1f} GB/s\n")
        agg = {}
        for r in recs:
            a = agg.setdefault(r["kernel"], {"launches": 0, "ms": 0.0, "gflop": 0.0, "mbytes": 0.0, "staged_mb": 0.0})
            a["staged_mb"] += r.get("staged_bytes", 0.0) / 1e6
            a["launches"] += 1
            a["ms"] += r["start"].elapsed_time(r["end"])
            a["gflop"] += r["flops"] / 1e9
            a["mbytes"] += r["bytes"] / 1e6
        per_kernel = {}
        for k, v in agg.items():
            e = {"launches": v["launches"], "ms": round(v["ms"], 3), "gflop": round(v["gflop"], 2),
                 "mbytes": round(v["mbytes"], 1), "tflops": round(v["gflop"] / max(v["ms"], 1e-9), 2),
                 "gbs": round(v["mbytes"] / max(v["ms"], 1e-9), 1)}
            if k.startswith(HBM_BOUND) or k.endswith("_h"):
                e["bound"], e["hbm_frac"] = "hbm", round(e["gbs"] / PEAK_HBM_GBS, 4)
            elif k.startswith(("conv_mfma", "conv1x1", "deconv2x2", "stem7x7s2_pool")):     # (the fp32 fused stem is MFMA-bound)
                # the dense MFMA peak of the type the kernel multiplies in: "_f16" / "_h" launches run fp16 MFMAs
                peak = PEAK_F16_MFMA_TFLOPS if (k.endswith(("_f16", "_h")) or f16) else PEAK_F32_MFMA_TFLOPS
                if k.endswith("_x3"):          # three f16 MFMA flops per algorithmic flop
                    peak = round(PEAK_F16_MFMA_TFLOPS / 3.0, 1)
                e["bound"], e["mfma_frac"], e["mfma_peak"] = "mfma", round(e["tflops"] / peak, 4), peak
                e["hbm_frac"] = round(e["gbs"] / PEAK_HBM_GBS, 4)
                if e["hbm_frac"] > e["mfma_frac"]:
                    e["bound"] = "hbm"
            per_kernel[k] = e
        dom = max(agg, key=lambda k: agg[k]["ms"])
        d = agg[dom]
        traffic = measured_traffic(dom, args.workload)      # None unless a PMC pass of THIS workload on THESE sources is committed
        common = {"timing": "HIP events per launch, auxiliary streams off: each kernel alone on the chip",
                  "launches_per_step": d["launches"], "avg_launch_us": round(1e3 * d["ms"] / d["launches"], 2),
                  "algorithmic_bytes_per_launch": round(1e6 * d["mbytes"] / d["launches"]),
                  "algorithmic_gflop_per_step": round(d["gflop"], 2)}
        mp = measured_peaks()
        if dom.startswith("conv_mfma") and not (f16 or dom.endswith("_h")):
            ach = d["gflop"] / d["ms"]          # GFLOP/ms = TFLOP/s
            # f32x3: `achieved` counts ALGORITHMIC flops; the matrix pipe issues three f16 MFMA flops for each
            x3 = dom.endswith("_x3")
            peak = round(PEAK_F16_MFMA_TFLOPS / 3.0, 1) if x3 else PEAK_F32_MFMA_TFLOPS
            roofline = dict({"kernel": dom, "bound": "mfma", "achieved": round(ach, 2), "peak": peak,
                             "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic}, **common)
            if x3:
                roofline["peak_note"] = "dense f16 MFMA peak / 3 (three f16 MFMAs per fp32-grade product)"
            if mp:
                pm = round(mp["mfma_f16_TFLOPs"] / 3.0, 1) if x3 else mp["mfma_f32_TFLOPs"]
                roofline.update(peak_measured=pm, frac_of_measured=round(ach / pm, 4), peak_measured_source=mp["source"])
        else:
            # HBM-bound kernels -- including the dense conv on the fp16 path: at fp16 the ridge is ~300 flop/B,
            # far above the 1x1 convs' arithmetic intensity, so moving the operands binds, not the matrix cores
            ach = d["mbytes"] / d["ms"]         # MB/ms = GB/s
            roofline = dict({"kernel": dom, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS,
                             "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": traffic}, **common)
            if mp:
                roofline.update(peak_measured=mp["hbm_GBs"], frac_of_measured=round(ach / mp["hbm_GBs"], 4),
                                peak_measured_source=mp["source"])
            if dom.startswith(("conv_mfma", "conv1x1")):
                roofline["mfma_tflops"] = round(d["gflop"] / d["ms"], 2)
                roofline["mfma_peak"] = PEAK_F16_MFMA_TFLOPS
                if mp:
                    roofline["mfma_peak_measured"] = mp["mfma_f16_TFLOPs"]
            if dom == "conv1x1_h256_h" and d["staged_mb"] > 0:
                # The half 256 x 256-tile kernel is bound by neither HBM nor the matrix pipe but by the per-CU L1 -> LDS request
                # path its operands are staged through (rocprofv3 --pmc: TA busy 50-62 %, MFMA busy 32-45 %, request
                # latencies short -- profiles/r04_h256_pmc.md).  `achieved` = bytes STAGED per launch (every 256-row tile: its
                # 256 x K activations + 256 x K weights) / launch time.  The HBM and MFMA figures of the same launches stay
                # beside it.
                # peak: what LDS-direct loads deliver into LDS from L2 with every CU streaming and nothing else going on --
                # 66-73 GB/s per CU, 16.8-18.8 TB/s chip-wide (MI355X_MICROARCH.md, "Indexed rows: gather into LDS", rows
                # served from the XCD's L2); the L1's nominal fill width (64 B/clk/CU) is twice that and never observed
                l1_peak = 18800.0
                ach_l1 = d["staged_mb"] / d["ms"]
                roofline.update(hbm={"achieved": roofline["achieved"], "peak": PEAK_HBM_GBS, "frac": roofline["frac"]},
                                bound="l2_lds", achieved=round(ach_l1, 1), peak=round(l1_peak, 1), frac=round(ach_l1 / l1_peak, 4),
                                bound_note="L2 -> LDS staging path: peak = 18.8 TB/s, the guide's measured chip-wide rate of LDS-direct "
                                           "loads served from L2; rocprofv3 --pmc on this kernel: TA busy 50-62 %, matrix pipe busy "
                                           "32-45 %, the two barely overlapping (profiles/r04_h256_pmc.md)",
                                staged_bytes_per_launch=round(1e6 * d["staged_mb"] / d["launches"]))
                roofline.pop("peak_measured", None)
                roofline.pop("frac_of_measured", None)

    # ---- the same workload once more under "f32x3" (fp32 tensors; every product of the dense convs = three f16 MFMAs
    # on operands split into two halves, fp32 accumulation -- tests/test_gpu_f32x3.py holds it to the fp32 bars and shows
    # its error against fp64 is not above the fp32 MFMA path's).  Reported BESIDE `value`, never as `value`: the headline
    # stays the exact-product fp32 path.  One GPU, the fp32 workloads only.
    alt = None
    want_alt = args.full and world == 1 and not f16 and not args.workload.endswith("_x3") and not args.no_f32x3
    if want_alt:
        ops.set_conv_math("f32x3")
        try:
            step()
            torch.cuda.synchronize(device)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize(device)
            ta = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize(device)
            dta = time.perf_counter() - ta
            alt = {"value": round(B * args.steps / dta, 3), "unit": "images/sec", "ms_per_step": round(1e3 * dta / args.steps, 3),
                   "steps": args.steps, "warmup": args.warmup, "dtype": ops.dtype_label(),
                   "note": "same workload, same timing protocol as `value`; fp32 tensors in HBM, fp32 accumulation; "
                           "operands carry 22 bits (2^-22 relative for 2^-14 <= |x| < 65520)"}
        finally:
            ops.set_conv_math("f32")

    cpu = parity = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu, parity, extra = cpu_baseline_and_parity(cfg, model, weights, hot_weights, backbone, images,
                                                     device, f16, args.quick_cpu_baseline,
                                                     extra_modes=("f32x3",) if alt is not None else ())
        if alt is not None:
            alt["parity"] = extra.get("f32x3")

    # ---- the other BASELINE configurations' per-GPU shapes, timed briefly in the same run so that the driver's record
    # holds a number for them too (the default workload on one GPU only; never part of `value`; a failure here is recorded,
    # not raised): configs[4]'s shard (ResNeXt-101, 16 x 1280^2, fp16 MFMA path with fp16 storage) and configs[0]
    # (MobileNet, 1 x 512^2; whole-forward hipGraph), the latter under both fp32-tensor conv maths.
    others = None
    if rank == 0 and world == 1 and args.workload == "resnext50_full_b8_1024" and args.full and not args.no_other_configs:
        others = {}
        for key, wl, math, graph in (("resnext101_full_b16_1280_f16", "resnext101_full_b16_1280_f16", "f16s", False),
                                     ("mobilenet_full_b1_512_graph", "mobilenet_full_b1_512", "f32", True),
                                     ("mobilenet_full_b1_512_graph_f32x3", "mobilenet_full_b1_512", "f32x3", True)):
            try:
                others[key] = _time_config(wl, device, math, graph, rank)
            except Exception as e:                       # noqa: BLE001 -- reported in the line
                others[key] = {"error": f"{type(e).__name__}: {e}"[:300]}

    if rank == 0:
        total_images = B * world * args.steps
        line = {
            "metric": "images/sec at 1024x1024 (MaskLab inference hot path, full forward)",
            "value": round(total_images / dt, 3),
            "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ops.dtype_label(), "data": "synthetic",
            "config": {"workload": args.workload, "per_gpu_batch": B, "global_batch": B * world,
                       "height": H, "width": W, "parallelism": f"dp{world}", "hipgraph": bool(args.graph),
                       "inputs": "pinned host memory, copied every step" if args.host_inputs else "resident in HBM",
                       "weights": "random init (cls logits x8 so NMS / mask head run at full load)",
                       "collective": (f"1 all-gather of [{B},{cap}*6+1] f32 per step on a side stream "
                                      f"({'gloo rehearsal' if rehearsal else 'RCCL'}), merged batch {gathered_images}")
                       if world > 1 else None,
                       "detections_per_image_rank0": n_det, "nms_candidates_per_image_rank0": n_cand},
            "full": bool(args.full),
            "roofline": roofline, "cpu_baseline": cpu, "parity": parity, "f32x3": alt, "other_configs": others,
            "kernels": per_kernel,
            "dumped_outputs": None if dumped is None else {"dir": args.dump_outputs, "arrays": dumped},
            # the ONE native library the product path loaded (masklab_hip/_lib.py: no override), and its sources' hash
            "library": {"path": os.path.relpath(_lib.LIB_PATH, ROOT), "abi_version": int(_lib.load().ml_version()),
                        "kernel_sources_sha256": csrc_hash()},
        }
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
