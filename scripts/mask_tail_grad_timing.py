#!/usr/bin/env python3
"""The mask head's tail backward (csrc/deconv_out_grad.hip) and the forward's tape launch (csrc/deconv_out.hip) at the serving
shape of the tail: 800 RoIs (8 images x 100), 14 x 14 crops, 256 channels in, C_mid = 256, 3 classes -- M = 156 800 input
pixels, T = [M, 4, 256] float32 = 642 MB.

  tail       ops.deconv2x2_out1x1_grad (dT + dWo + dbo in one pass over T) on a dense dy, on a dy with mask_loss's sparsity
             (one class channel of about half the RoIs), and in place (out=T);
             floor_ms      T read once + dT written once + dy read once at the copy rate of profiles/r03_peaks.json;
             composition   the existing ops it replaces: dy brought to GEMM order (a pixel un-shuffle, torch), ops.conv2d_wgrad
                           (dWo, dbo; x = T), ops.conv2d_dgrad through the dy gather (dy Wo^T), ops.relu_grad (the mask);
  full       the whole backward of the tail -- tail + the transposed conv's weight and data gradients on its 1x1 view + the
             re-layout -- against torch autograd's backward of conv_transpose2d + relu + 1x1 conv (channels-last tensors;
             a yardstick only, not a product path);
  tape       the forward launch with and without the tape store;
  plain      the plain forward launch alone (with --lib: on another build of the library, e.g. the parent commit's, in a
             process of its own -- the job alternates the two builds);
  head       MaskSubNet at the default configuration (depth 4, 256 features, 16 groups, 3 classes) on three levels of
             8 x (50, 30, 20) RoIs: call_with_tape, and call_with_tape + backward.

Each number is the HIP-event time of `--inner` back-to-back calls divided by their number, `--steps` such windows after a
warm-up; median, min, max.  The calls of a window rotate through enough copies of the operands that their footprint exceeds
`--footprint-mb` (default 768): the 256 MiB last-level cache cannot hold an operand from one call to the next.  One JSON line
per leg; the fused gradients must agree with the composition's / torch's to 1e-3 of the largest gradient (torch's with the
ReLU's mask taken from the device's T: two float32 evaluations of T differ on the side of 0 a few elements fall on), nothing
else is asserted.

Usage (GPU box):  timeout 900 python scripts/mask_tail_grad_timing.py [--steps 7] [--inner 10] [--warmup 2]
                  [--legs tail,full,tape,plain,head] [--lib PATH]"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instance-segmentation-road-project_amd"), os.path.join(ROOT, "scripts")]

from generator_timing import time_launch  # noqa: E402

B, NL, H, W, CIN, CMID, NCLS = 8, 100, 14, 14, 256, 256, 3
R = B * NL
M = R * H * W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--footprint-mb", type=int, default=768)
    ap.add_argument("--legs", default="tail,full,tape,head")
    ap.add_argument("--lib", default=None, help="another build of the library (the `plain` leg only)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from masklab_hip import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        have = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:      # an older build: bind what it has
            del _lib.SIGNATURES[name]
    from masklab_hip import keras_like, ops, packing
    if not torch.cuda.is_available():
        raise SystemExit("mask_tail_grad_timing: no GPU -- nothing is measured without one")
    with open(os.path.join(ROOT, "profiles", "r03_peaks.json")) as f:
        copy_rate = json.load(f)["copy_global_x4"]["read_plus_write_GBs"]
    gen = torch.Generator(device="cuda").manual_seed(29)
    randn = lambda *shape: torch.randn(shape, device="cuda", generator=gen)
    rng = np.random.default_rng(29)
    device = torch.device("cuda:0")
    relu, sig = _lib.ACT_BY_NAME["relu"], _lib.ACT_BY_NAME["sigmoid"]

    def stats(ms, enq):
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "enqueue_ms": round(float(np.median(enq)), 4)}

    def off(got, want):
        """the largest difference relative to the largest gradient"""
        return float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))

    def agree(got, want):
        return off(got, want) <= 1e-3

    wd = rng.normal(0, 0.05, (2, 2, CMID, CIN)).astype(np.float32)
    bd = rng.normal(0, 0.1, CMID).astype(np.float32)
    wo = rng.normal(0, 0.1, (1, 1, CMID, NCLS)).astype(np.float32)
    bo = rng.normal(0, 0.1, NCLS).astype(np.float32)
    wo_d = torch.from_numpy(wo).cuda()
    t_bytes = M * 4 * CMID * 4
    copies = max(2, math.ceil(args.footprint_mb * 2 ** 20 / t_bytes))

    def make_dy(sparse):
        dy = randn(B, NL, 2 * H, 2 * W, NCLS)
        if sparse:
            keep = (torch.rand((B, NL, 1, 1, 1), device="cuda", generator=gen) < 0.5).float()
            cls = torch.nn.functional.one_hot(torch.randint(0, NCLS, (B, NL), device="cuda", generator=gen), NCLS).float()
            dy = dy * keep * cls[:, :, None, None, :]
        return dy.contiguous()

    def forward_problem(x, out):
        table, bo_p, _ = packing.pack_out1x1_table(wo, bo)
        if "dc" not in forward_problem.__dict__:
            forward_problem.dc = ops.DeviceConv(packing.pack_transpose2x2(wd, bd), device)
            forward_problem.table, forward_problem.bo = torch.from_numpy(table).cuda(), torch.from_numpy(bo_p).cuda()
        return dict(x=x, dc=forward_problem.dc, wo_table=forward_problem.table, bo=forward_problem.bo, out=out, out_base=0,
                    rois_per_image=NL)

    def tail_leg():
        Ts = [torch.relu(randn(M, 4, CMID)) for _ in range(copies)]
        outs = [torch.empty((M, 4, CMID), device="cuda") for _ in range(2)]
        kept = {}
        dc_out = ops.DeviceConv(packing.pack_dense(wo, bo), device)
        for label, sparse in (("dense dy", False), ("mask_loss's sparsity", True)):
            dy = make_dy(sparse)

            def fused(k, dy=dy):
                kept["fused"] = ops.deconv2x2_out1x1_grad(dy, Ts[k], wo_d, (H, W), NL, out=outs[k % 2])

            def composed(k, dy=dy):
                T = Ts[k]
                dyg = dy.view(R, H, 2, W, 2, NCLS).permute(0, 1, 3, 2, 4, 5).reshape(R, H * W * 4, 1, NCLS).contiguous()
                xv = T.view(R, H * W * 4, 1, CMID)
                dk, db = ops.conv2d_wgrad(xv, dyg, dc_out, padding="valid")
                d = ops.conv2d_dgrad(dyg, dc_out, (H * W * 4, 1), padding="valid", out=outs[k % 2].view(R, H * W * 4, 1, CMID))
                ops.relu_grad(T.view(-1), d.view(-1), out=d.view(-1))
                kept["composed"] = (d.view(M, 4, CMID), dk, db)

            ms, enq = time_launch(fused, copies, args.steps, args.inner, args.warmup)
            ms_c, enq_c = time_launch(composed, copies, args.steps, args.inner, args.warmup)
            fused(0)
            f = [t.clone() for t in kept["fused"]]
            composed(0)
            torch.cuda.synchronize()
            ok = all(agree(a, b) for a, b in zip(f, kept["composed"]))
            nbytes = 2 * t_bytes + dy.numel() * 4
            floor_ms = nbytes / (copy_rate * 1e9) * 1e3
            line = dict(leg="tail", dy=label, T=[M, 4, CMID], ncls=NCLS, copies_rotated=copies, fused=stats(ms, enq),
                        composition=stats(ms_c, enq_c), gradients_agree=ok, bytes=nbytes, copy_rate_GBs=copy_rate,
                        floor_ms=round(floor_ms, 4), fused_over_floor=round(float(np.median(ms)) / floor_ms, 2),
                        fused_GBs=round(nbytes / float(np.median(ms)) / 1e6, 1),
                        composition_over_fused=round(float(np.median(ms_c)) / float(np.median(ms)), 2),
                        slices=list(ops.deconv2x2_out1x1_grad_plan(M, H * W, W, NL, CMID, NCLS)))
            print(json.dumps(line), flush=True)
            assert ok, "the fused gradients differ from the composition's"
        dy = make_dy(False)
        ms, enq = time_launch(lambda k: ops.deconv2x2_out1x1_grad(dy, Ts[k], wo_d, (H, W), NL, out=Ts[k]), copies, args.steps,
                              args.inner, args.warmup)
        print(json.dumps(dict(leg="tail", dy="dense dy, in place (out=T)", fused=stats(ms, enq))), flush=True)

    def full_leg():
        xs = [randn(R, H, W, CIN) for _ in range(2)]
        dy = make_dy(False)
        dc1 = ops.DeviceConv(packing.pack_dense(packing.transpose2x2_as_1x1(wd), np.tile(bd, 4)), device)
        masks = torch.empty((B, NL, 2 * H, 2 * W, NCLS), device="cuda")
        tapes = []
        for x in xs:
            ops.deconv2x2_out1x1_multi([forward_problem(x, masks)], NCLS, relu, sig, tape=tapes)
        kept = {}

        def fused(k):
            x, T = xs[k % 2], tapes[k % 2]
            dT, dk, db = ops.deconv2x2_out1x1_grad(dy, T, wo_d, (H, W), NL)
            dyv = dT.view(R, H, W, 4 * CMID)
            dk1, db4 = ops.conv2d_wgrad(x, dyv, dc1)
            kept["fused"] = (ops.conv2d_dgrad(dyv, dc1, (H, W)),) + ops.deconv2x2_grad_relayout(dk1, db4) + (dk, db)

        leaves = [torch.from_numpy(np.ascontiguousarray(wd.transpose(3, 2, 0, 1))).cuda().requires_grad_(True),
                  torch.from_numpy(bd).cuda().requires_grad_(True),
                  torch.from_numpy(np.ascontiguousarray(wo[0, 0].T)[:, :, None, None]).cuda().requires_grad_(True),
                  torch.from_numpy(bo).cuda().requires_grad_(True)]
        F = torch.nn.functional
        graphs = []
        for x in xs:
            xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)                   # channels-last memory, NCHW view
            z = F.conv2d(torch.relu(F.conv_transpose2d(xt, leaves[0], leaves[1], stride=2)), leaves[2], leaves[3])
            graphs.append((xt, z))
        dz = dy.view(R, 2 * H, 2 * W, NCLS).permute(0, 3, 1, 2)

        def torch_back(k):
            xt, z = graphs[k % 2]
            kept["torch"] = torch.autograd.grad(z, [xt] + leaves, dz, retain_graph=True)

        ms, enq = time_launch(fused, 2, args.steps, args.inner, args.warmup)
        ms_t, enq_t = time_launch(torch_back, 2, args.steps, args.inner, args.warmup)
        fused(0)
        torch_back(0)
        torch.cuda.synchronize()
        dx, dkd, dbd, dko, dbo = kept["fused"]
        tx, twd, tbd, two, tbo = kept["torch"]
        # T comes from two float32 evaluations: where its pre-activation is within rounding of 0 they fall on different sides
        # of the ReLU's kink, and every gradient behind that element differs by a whole term.  So the differences to autograd
        # are reported, and agreement is asserted against torch matmuls that take the mask from the device's own T
        txp = tx.permute(0, 2, 3, 1)
        to_autograd = dict(dx=off(dx, txp), dkd=off(dkd, twd.permute(2, 3, 1, 0)), dbd=off(dbd, tbd),
                           dko=off(dko[0, 0], two[:, :, 0, 0].T), dbo=off(dbo, tbo))
        T, x = tapes[0], xs[0]
        dyg = dy.view(R, H, 2, W, 2, NCLS).permute(0, 1, 3, 2, 4, 5).reshape(M, 4, NCLS)
        d2 = ((T > 0) * (dyg @ wo_d[0, 0].T)).view(M, 4 * CMID)
        k1 = torch.from_numpy(packing.transpose2x2_as_1x1(wd)).cuda()[0, 0]
        same_mask = dict(dx=off(dx.view(M, CIN), d2 @ k1.T),
                         dkd=off(dkd, (x.view(M, CIN).T @ d2).view(CIN, 4, CMID).permute(1, 2, 0).reshape(2, 2, CMID, CIN)),
                         dbd=off(dbd, d2.view(M, 4, CMID).sum(dim=(0, 1))),
                         dko=off(dko[0, 0], torch.einsum("mqc,mqk->ck", T, dyg)), dbo=off(dbo, dyg.sum(dim=(0, 1))))
        ok = all(v <= 1e-3 for v in same_mask.values())
        fmt = lambda d: {k: float("%.3g" % v) for k, v in d.items()}
        print(json.dumps(dict(leg="full", what="tail + 1x1-view wgrad / dgrad + re-layout against torch autograd's backward of "
                              "conv_transpose2d + relu + conv2d 1x1", x=[R, H, W, CIN], fused=stats(ms, enq), torch=stats(ms_t, enq_t),
                              largest_difference_to_autograd=fmt(to_autograd), largest_difference_same_mask=fmt(same_mask),
                              gradients_agree=ok, torch_over_fused=round(float(np.median(ms_t)) / float(np.median(ms)), 2))), flush=True)
        assert ok, "the fused gradients differ from torch's on the same ReLU mask"

    def forward_leg(with_tape):
        x_bytes = R * H * W * CIN * 4
        n = max(2, math.ceil(args.footprint_mb * 2 ** 20 / x_bytes))
        xs = [randn(R, H, W, CIN) for _ in range(n)]
        masks = torch.empty((B, NL, 2 * H, 2 * W, NCLS), device="cuda")
        ms, enq = time_launch(lambda k: ops.deconv2x2_out1x1_multi([forward_problem(xs[k], masks)], NCLS, relu, sig), n, args.steps,
                              args.inner, args.warmup)
        line = dict(leg="tape" if with_tape else "plain", library=_lib.LIB_PATH, x=[R, H, W, CIN], copies_rotated=n,
                    plain=stats(ms, enq))
        if with_tape:
            tape_out = [torch.empty((M, 4, CMID), device="cuda") for _ in range(2)]

            def taped(k):
                ops.deconv2x2_out1x1_multi([dict(forward_problem(xs[k], masks), tape_out=tape_out[k % 2])], NCLS, relu, sig, tape=[])

            ms_t, enq_t = time_launch(taped, n, args.steps, args.inner, args.warmup)
            extra = float(np.median(ms_t)) - float(np.median(ms))
            line.update(tape=stats(ms_t, enq_t), tape_bytes=t_bytes, store_ms=round(extra, 4),
                        store_floor_ms=round(t_bytes / (copy_rate * 1e9) * 1e3 * 2, 4),       # a write alone: half of a copy's traffic
                        tape_over_plain=round(float(np.median(ms_t)) / float(np.median(ms)), 2))
        print(json.dumps(line), flush=True)

    def head_leg():
        from masklab_hip.layers.instance import MaskSubNet
        n_l = (50, 30, 20)
        net = MaskSubNet(num_blocks=3, num_classes=NCLS, name="mask")
        shapes = [(B, n, H, W, 256) for n in n_l]
        net.build(shapes)
        weights = keras_like.init_weights(net.weight_specs(), 0)
        for k in weights:                                   # the init (stddev 0.01) starves a random backward of signal
            if k.endswith("/kernel"):
                weights[k] = rng.normal(0, 0.05, weights[k].shape).astype(np.float32)
        net.load_weights(weights, device)
        xs = [randn(*s) for s in shapes]
        d = make_dy(True)
        state = {}

        def forward(k):
            state["tape"] = net.call_with_tape(xs)[1]

        def both(k):
            forward(k)
            state["out"] = net.backward(state["tape"], d, consume_tape=True)

        for what, fn in (("call", lambda k: net.call(xs)), ("call_with_tape", forward), ("call_with_tape + backward", both)):
            ms, enq = time_launch(fn, 1, args.steps, max(1, args.inner // 2), 1)
            print(json.dumps(dict(leg="head", what=what, rois=[B, list(n_l)], fused=stats(ms, enq))), flush=True)
        ops.PROFILE = []
        both(0)
        torch.cuda.synchronize()
        per = {}
        for rec in ops.PROFILE:
            per[rec["kernel"]] = per.get(rec["kernel"], 0.0) + rec["start"].elapsed_time(rec["end"])
        ops.PROFILE = None
        print(json.dumps(dict(leg="head", what="ms per op of one call_with_tape + backward (event pairs around each launcher)",
                              ms={k: round(v, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])})), flush=True)

    legs = args.legs.split(",")
    if "plain" in legs:
        forward_leg(False)
    if "tape" in legs:
        forward_leg(True)
    if "tail" in legs:
        tail_leg()
    if "full" in legs:
        full_leg()
    if "head" in legs:
        head_leg()


if __name__ == "__main__":
    main()
