"""No result may depend on what a workspace or a fresh output tensor held before the launch.

Every op of masklab_hip/ops.py works in a grow-only scratch buffer (`ops.workspace(nbytes, device, tag)`) that is shared by
all launches of its tag and re-carved from each launch's shape, and returns `torch.empty` tensors.  Here every family is
launched on stale memory (tests/dirty_memory.py: 0xFF bytes -- NaN, -1, the largest key -- in every workspace and every
fresh tensor) and with a launch of another shape in between (X, Y, X).  For every case of `CASES`:

  (a) the result on poisoned memory equals the result on zeroed memory bit for bit,
  (b) no 0xFF element is left where the op promises a value (`never_poison`: outputs in which NaN / -1 is no legal value),
  (c) what the op promises not to touch still holds the fill exactly (result keys that start with "untouched:"),
  (d) the second X of X, Y, X equals the first bit for bit,
  (e) the result meets the bar of the op's own test (same reference, same tolerance).

Then the whole forwards, the serving chain and the evaluation loop on poisoned memory against their clean runs, and captured
graphs with an eager forward of another shape between two replays.  tests/test_dirty_memory_cpu.py holds every workspace tag
of ops.py to a case of `CASES`.  -m gpu."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import dirty_memory as DM
from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
    """One row of the table: `tags` = the ops.workspace tags its launches use; build() (GPU needed) -> dict(run_x, run_y,
    check): run_x / run_y launch and return {name: tensor or array}, check(result of X) holds it to the op's own bar."""

    def __init__(self, name, tags, build, never_poison=()):
        self.name, self.tags, self.build, self.never_poison = name, frozenset(tags), build, tuple(never_poison)

    def __repr__(self):
        return self.name


def _normal(rng, *shape, scale=1.0, dtype=np.float32):
    return (rng.standard_normal(shape) * scale).astype(np.float32).astype(dtype)


# ------------------------------------------------------------------ conv: split-K slabs
def _conv_split_k(math):
    def build():
        from masklab_hip import _lib, ops, packing
        from oracle import tfops as T
        rng = np.random.default_rng(31)
        f16 = math == "f16s"          # fp32 tensors in this mode run on fp16 MFMA operands (a half output takes no residual)
        h = (lambda a: a.astype(np.float16).astype(np.float64)) if f16 else (lambda a: a.astype(np.float64))

        def problem(k, cin, cout, hw, res):
            x = _normal(rng, 2, hw, hw, cin)
            w, b = _normal(rng, k, k, cin, cout, scale=1.0 / np.sqrt(k * k * cin)), _normal(rng, cout)
            r = _normal(rng, 2, hw, hw, cout) if res else None
            return dict(x=x, w=w, b=b, r=r, xd=dev(x), rd=None if r is None else dev(r),
                        dc=ops.DeviceConv(packing.pack_dense(w, b), "cuda"))

        X, Y = problem(3, 256, 75, 4, True), problem(1, 2048, 128, 1, False)

        def run(p, must_split):
            ops.set_conv_math(math)
            ops.LAUNCH_LOG = []
            try:
                out = ops.conv2d(p["xd"], p["dc"], padding="same", act=_lib.ACT_RELU, residual=p["rd"])
                log = ops.LAUNCH_LOG
            finally:
                ops.LAUNCH_LOG = None
                ops.set_conv_math("f32")
            assert len(log) == 1 and (not must_split or min(log[0][1]) > 1), f"not cut along K: {log}"
            return {"out": out}

        def check(got):
            ref = T.relu(T.conv2d(h(X["x"]), h(X["w"]), X["b"].astype(np.float64), 1, "same") + X["r"].astype(np.float64))
            # test_conv2d_split_k_small_m; fp16 operands: test_conv2d_f16_split_k_and_multi_problem (the same rounded operands)
            np.testing.assert_allclose(got["out"], ref, atol=5e-5 if f16 else 3e-5)

        return dict(run_x=lambda: run(X, True), run_y=lambda: run(Y, False), check=check)
    return Case(f"conv_split_k[{math}]", ["conv"], build, never_poison=["out"])


def _conv_multi():
    """The 5-level launch of test_conv2d_multi_problem_launch: per-problem slab offsets, and the strided-view destination."""
    def build():
        from masklab_hip import _lib, ops, packing
        from oracle import tfops as T
        rng = np.random.default_rng(32)
        nc, pri = 5, 15

        def levels(B, sizes):
            xs = [_normal(rng, B, h, w_, 128) for h, w_ in sizes]
            ws = [(_normal(rng, 3, 3, 128, 128, scale=0.03), _normal(rng, 128)) for _ in sizes]
            wo = [(_normal(rng, 3, 3, 128, pri * nc, scale=0.03), _normal(rng, pri * nc)) for _ in sizes]
            return dict(B=B, sizes=sizes, xs=xs, ws=ws, wo=wo, xd=[dev(x) for x in xs],
                        dcs=[ops.DeviceConv(packing.pack_dense(w, b), "cuda") for w, b in ws],
                        dco=[ops.DeviceConv(packing.pack_dense(w, b), "cuda") for w, b in wo])

        X = levels(2, [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)])
        Y = levels(3, [(8, 8), (4, 4), (2, 2)])

        def run(p):
            outs = ops.conv2d_multi([dict(x=x, dc=dc, act=_lib.ACT_RELU) for x, dc in zip(p["xd"], p["dcs"])])
            total = sum(h * w_ * pri for h, w_ in p["sizes"])
            pred = torch.empty((p["B"], total, nc), dtype=torch.float32, device="cuda")
            probs, off = [], 0
            for x, dc, (h, w_) in zip(p["xd"], p["dco"], p["sizes"]):
                probs.append(dict(x=x, dc=dc, act=_lib.ACT_SIGMOID, out_view=(pred, off * nc, pri * nc, total * nc)))
                off += h * w_ * pri
            ops.conv2d_multi(probs)
            return {"levels": list(outs), "pred": pred}

        def check(got):
            refs = []
            for x, (w, b), (wo, bo), o in zip(X["xs"], X["ws"], X["wo"], got["levels"]):
                np.testing.assert_allclose(o, T.relu(T.conv2d(x.astype(np.float64), w, b)), atol=2e-5)
                refs.append(T.sigmoid(T.conv2d(x.astype(np.float64), wo, bo)).reshape(X["B"], -1, nc))
            np.testing.assert_allclose(got["pred"], np.concatenate(refs, 1), atol=2e-5)

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("conv_multi_problem", ["conv"], build, never_poison=["levels", "pred"])


# ------------------------------------------------------------------ GroupNormalization
def _gn():
    def build():
        from masklab_hip import ops
        from oracle import tfops as T
        rng = np.random.default_rng(33)

        def problem(shape, G):
            x = _normal(rng, *shape) * 3 + 1.5
            g, b = rng.uniform(0.5, 1.5, shape[-1]).astype(np.float32), _normal(rng, shape[-1])
            return dict(x=x, g=g, b=b, G=G, xd=dev(x), gd=dev(g), bd=dev(b))

        X, Y = problem((2, 16, 16, 128), 16), problem((4, 1, 1, 128), 32)

        def run(p):
            dense = ops.groupnorm_chunk(p["xd"], p["gd"], p["bd"], p["G"])
            B, H, W, C = p["x"].shape
            buf = torch.empty((B, H, W, C + 32), dtype=torch.float32, device="cuda")
            ops.groupnorm_chunk(p["xd"], p["gd"], p["bd"], p["G"], relu=True, out=buf, out_coff=32)
            sl = host(buf)
            return {"dense": dense, "slice": sl[..., 32:], "untouched:slice": sl[..., :32]}

        def check(got):
            ref = T.group_norm(X["x"].astype(np.float64), X["g"], X["b"], X["G"])
            np.testing.assert_allclose(got["dense"], ref, atol=2e-5)              # test_groupnorm_chunk
            np.testing.assert_allclose(got["slice"], T.relu(ref), atol=2e-5)

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("gn", ["gn"], build, never_poison=["dense", "slice"])


def _gn_multi():
    def build():
        from masklab_hip import _lib, ops, packing
        from oracle import tfops as T
        rng = np.random.default_rng(34)
        shapes = [(2, 64, 64, 128, 16), (2, 32, 32, 128, 16), (2, 16, 16, 128, 16), (2, 8, 8, 128, 16), (2, 4, 4, 128, 16),
                  (9, 14, 14, 128, 16), (2, 16, 16, 128, 32)]       # test_groupnorm_multi_equals_single_launches
        xs = [_normal(rng, *s[:4]) + 0.5 for s in shapes]
        gb = [(rng.uniform(0.5, 1.5, s[3]).astype(np.float32), _normal(rng, s[3])) for s in shapes]
        probs = [dict(x=dev(x), gamma=dev(g), beta=dev(b), groups=s[4]) for x, (g, b), s in zip(xs, gb, shapes)]
        # the statistics-from-the-conv-epilogue form (test_groupnorm_statistics_from_the_conv_epilogue): 3 x 128 x 128
        B, H, W = 3, 128, 128
        cx, (cw, cb) = dev(_normal(rng, B, H, W, 128)), (_normal(rng, 3, 3, 128, 128, scale=0.03), _normal(rng, 128))
        dc = ops.DeviceConv(packing.pack_dense(cw, cb), "cuda")
        cg, cbeta = dev(rng.uniform(0.5, 1.5, 128).astype(np.float32)), dev(_normal(rng, 128))
        two_pass = host(ops.groupnorm_chunk(ops.conv2d(cx, dc, act=_lib.ACT_RELU), cg, cbeta, 16))

        def run_x():
            outs = ops.groupnorm_chunk_multi([dict(p) for p in probs[:5]])
            part = torch.empty((B * H * W // 128, 4, 2), dtype=torch.float64, device="cuda")
            y = ops.conv2d(cx, dc, act=_lib.ACT_RELU, gn_partials=part)
            (fused,) = ops.groupnorm_chunk_multi([dict(x=y, gamma=cg, beta=cbeta, groups=16, out=y, partials=(part, 32))])
            return {"levels": list(outs), "partials": part, "fused": fused}

        def check(got):
            for x, (g, b), s, o in zip(xs, gb, shapes, got["levels"]):
                np.testing.assert_allclose(o, T.group_norm(x.astype(np.float64), g, b, s[4]), atol=2e-5)
            np.testing.assert_allclose(got["fused"], two_pass, rtol=0, atol=2e-6)

        return dict(run_x=run_x, run_y=lambda: {"levels": ops.groupnorm_chunk_multi([dict(p) for p in probs[5:]])}, check=check)
    return Case("gn_multi", ["gn_multi", "conv"], build, never_poison=["levels", "partials", "fused"])


# ------------------------------------------------------------------ squeeze-excite
def _se(shape, other, half):
    def build():
        from masklab_hip import ops
        import test_gpu_squeeze_excite as SE
        dt, tdt = (np.float16, torch.float16) if half else (np.float32, torch.float32)

        def problem(B, H, W, C, Hd):
            rng = np.random.default_rng(C + H + half)
            x = (rng.standard_normal((B, H, W, C)) + 0.25).astype(dt)
            w1, w2 = SE._weights(rng, C, Hd)
            return dict(x=x, w1=w1, w2=w2, xd=dev(x), w1d=dev(w1), w2d=dev(w2))

        X, Y = problem(*shape), problem(*other)

        def run(p):
            out = torch.empty_like(p["xd"])
            assert out.dtype == tdt
            return {"out": ops.squeeze_excite_multi([dict(x=p["xd"], w1=p["w1d"], w2=p["w2d"], out=out)])[0]}

        def check(got):
            ref = SE._oracle(X["x"].astype(np.float32), X["w1"], X["w2"])
            if half:
                SE._half_bar(got["out"], ref)
            else:
                np.testing.assert_allclose(got["out"], ref, rtol=1e-5, atol=1e-5)

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case(f"se[{'x'.join(map(str, shape))}-{'f16' if half else 'f32'}]", ["se"], build, never_poison=["out"])


def _se_multi(half):
    """A fixed-capacity RoI level (3 images x 7 slots, 4 live) and two plain problems in one call: per-problem workspace
    offsets; the dead slots of the level's output keep what they held."""
    def build():
        from masklab_hip import ops
        import test_gpu_squeeze_excite as SE
        rng = np.random.default_rng(35)
        dt = np.float16 if half else np.float32
        cap, imgs, C, Hd, live = 7, 3, 128, 8, 4
        alive = np.array([n % cap < live for n in range(imgs * cap)])
        data = []
        for shape in ((imgs * cap, 14, 14, C), (2, 40, 24, C), (2, 5, 3, C)):
            x = (rng.standard_normal(shape) + 0.25).astype(dt)
            w1, w2 = SE._weights(rng, C, Hd)
            data.append(dict(x=x, w1=w1, w2=w2, xd=dev(x), w1d=dev(w1), w2d=dev(w2)))
        lv = torch.tensor([live], dtype=torch.int32, device="cuda")
        yx = (rng.standard_normal((2, 32, 48, C)) + 0.25).astype(dt)
        yw = SE._weights(rng, C, Hd)
        yd = dict(x=dev(yx), w1=dev(yw[0]), w2=dev(yw[1]))

        def run_x():
            probs = [dict(x=d["xd"], w1=d["w1d"], w2=d["w2d"], out=torch.empty_like(d["xd"])) for d in data]
            probs[0]["live"] = (lv, cap)
            outs = [host(o) for o in ops.squeeze_excite_multi(probs)]
            return {"level": outs[0][alive], "untouched:level": outs[0][~alive], "plain": outs[1:]}

        def check(got):
            for g, d, rows in zip([got["level"]] + got["plain"], data, (alive, slice(None), slice(None))):
                ref = SE._oracle(d["x"].astype(np.float32), d["w1"], d["w2"])[rows]
                if half:
                    SE._half_bar(g, ref)
                else:
                    np.testing.assert_allclose(g, ref, rtol=1e-5, atol=1e-5)

        return dict(run_x=run_x, run_y=lambda: {"out": ops.squeeze_excite_multi([dict(yd, out=torch.empty_like(yd["x"]))])[0]},
                    check=check)
    return Case(f"se_multi[{'f16' if half else 'f32'}]", ["se"], build, never_poison=["level", "plain"])


def _se_residual():
    def build():
        from masklab_hip import ops
        import test_gpu_seresnet34 as S34
        X, Y = S34._tail_problem(3, 1, 1, 128, seed=1128), S34._tail_problem(3, 17, 30, 512, seed=17512)
        names = ("x", "sc", "w1", "b1", "w2", "b2", "scale", "shift")
        Xd, Yd = [dev(X[n]) for n in names], [dev(Y[n]) for n in names]

        def run(args):
            act, y = ops.se_residual(*args, want_y=True)
            return {"act": act, "y": y}

        def check(got):
            want_act, want_y = S34._tail_ref(X)
            np.testing.assert_allclose(got["act"], want_act, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(got["y"], want_y, rtol=1e-5, atol=1e-6)

        return dict(run_x=lambda: run(Xd), run_y=lambda: run(Yd), check=check)
    return Case("se_residual", ["se_residual"], build, never_poison=["act", "y"])


def _se_bottleneck(half):
    def build():
        from masklab_hip import ops
        import test_gpu_senet as SN
        dt = np.float16 if half else np.float32
        X, Y = SN._tail_problem(3, 1, 1, 1024, 11024, dt), SN._tail_problem(3, 17, 30, 2048, 172048, dt)
        names = ("c3", "res", "w1", "b1", "w2", "b2")
        Xd, Yd = [dev(X[n]) for n in names], [dev(Y[n]) for n in names]

        def check(got):
            assert got["out"].dtype == dt
            if half:
                SN._check_half(got["out"], SN._tail_ref(X))
            else:
                np.testing.assert_allclose(got["out"], SN._tail_ref(X), rtol=1e-5, atol=1e-6)

        return dict(run_x=lambda: {"out": ops.se_bottleneck(*Xd)}, run_y=lambda: {"out": ops.se_bottleneck(*Yd)}, check=check)
    return Case(f"se_bottleneck[{'f16' if half else 'f32'}]", ["se_bottleneck"], build, never_poison=["out"])


# ------------------------------------------------------------------ detection
def _det(name, max_out, equal_scores=False):
    def build():
        from masklab_hip import ops
        from oracle import masklab as O
        import test_gpu_detect as TD
        if equal_scores:            # test_detection_proposal_many_equal_scores_falls_back_exactly: one bin overflows the LDS band
            pri = TD._anchors(256, 256)
            A = pri.shape[0]
            rng = np.random.default_rng(3)
            cls = np.zeros((1, A, 5), np.float32)
            cls[0, rng.choice(A, 6000, replace=False), 2] = 0.625
            cls[0, rng.choice(A, 50, replace=False), 2] = (0.7 + 0.25 * (rng.permutation(50) + 0.5) / 50).astype(np.float32)
            loc = (rng.normal(size=(1, A, 4)) * 0.2).astype(np.float32)
        else:
            pri, cls, loc = TD._synthetic_head(2, 128, 128, frac=0.01, seed=2)
        boxes = O.restore_boxes(loc, pri[None])
        ypri, ycls, yloc = TD._synthetic_head(3, 128, 256, frac=0.02, seed=3)
        yboxes = O.restore_boxes(yloc, ypri[None])
        Xd, Yd = (dev(cls), dev(boxes)), (dev(ycls), dev(yboxes))

        def run(args):
            prop, counts, kept, payload = ops.detection_proposal(*args, 0.5, 0.4, 0.6, max_out, want_kept=True, want_payload=True)
            return {"proposed": prop, "counts": counts, "kept": kept, "payload": payload}

        def check(got):
            ref, kept_ref = O.detection_proposal(cls, boxes, 0.5, 0.4, 0.6, max_out)
            prop, counts, kept = got["proposed"], got["counts"], got["kept"]
            n = max(1, int(counts.max()))
            assert ref.shape == (cls.shape[0], n, 6) and int(counts.max()) > 0
            np.testing.assert_array_equal(prop[:, :n], ref)                # rows incl. -1 padding, bit exact
            assert np.all(prop[:, n:] == -1)
            for b in range(cls.shape[0]):
                np.testing.assert_array_equal(kept[b, :counts[b]], kept_ref[kept_ref[:, 0] == b][:, 1:])
                assert np.all(kept[b, counts[b]:] == -1)
            np.testing.assert_array_equal(got["payload"][:, :-1], prop.reshape(prop.shape[0], -1))
            np.testing.assert_array_equal(got["payload"][:, -1].view(np.int32), counts)

        return dict(run_x=lambda: run(Xd), run_y=lambda: run(Yd), check=check)
    return Case(name, ["det"], build, never_poison=["counts"])


# ------------------------------------------------------------------ RoI distribution, crops, molding, trimming, mask tail
def _roi_levels():
    """test_mask_distribute_and_roi_crop: level slots with -1 tails, crops with -1 padded slots; and the same crops at
    capacity, where the slots past a level's maximum are not written."""
    def build():
        from masklab_hip import ops
        from masklab_hip.layers import PyramidRoiAlign
        from oracle import masklab as O

        def problem(B, H, W, n_real, cap, seed):
            rng = np.random.default_rng(seed)
            prop = np.full((B, cap, 6), -1.0, np.float32)
            for b, n in enumerate(n_real):
                cx, cy = rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)
                w, h = rng.uniform(10, 300, n), rng.uniform(10, 300, n)
                prop[b, :n] = np.stack([cx, cy, w, h, rng.integers(0, 5, n), rng.uniform(0.5, 1, n)], 1)
            fmaps = [rng.normal(size=(B, H // s, W // s, 128)).astype(np.float32) for s in (8, 16, 32)]
            return dict(prop=prop, fmaps=fmaps, hw=(H, W), cap=cap, pd=dev(prop), fd=[dev(f) for f in fmaps])

        X, Y = problem(3, 256, 256, [7, 0, 12], 12, 5), problem(2, 128, 128, [5, 2], 5, 6)
        pra = PyramidRoiAlign((14, 14))

        def run(p):
            slots, lcounts, lmax, kvals = ops.mask_distribute(p["pd"], 2, 36.0, want_k=True)
            rf, rb = pra.crop_levels(p["fd"], p["pd"], p["hw"], has_k=False, base_size=36)
            out = {"slots": slots, "lcounts": lcounts, "lmax": lmax, "kvals": kvals, "roi_fmaps": list(rf), "roi_boxes": rb}
            cf, cb, _ = pra.crop_capacity(p["fd"], p["pd"], p["hw"], slots, lcounts, lmax)
            cap, n_l = p["cap"], [max(1, int(v)) for v in host(lmax)]
            cb = host(cb)
            for l, (f, n) in enumerate(zip(cf, n_l)):
                f = host(f)
                out[f"capacity_fmaps{l}"], out[f"untouched:capacity_fmaps{l}"] = f[:, :n], f[:, n:]
                out[f"capacity_boxes{l}"] = cb[:, l * cap:l * cap + n]
                out[f"untouched:capacity_boxes{l}"] = cb[:, l * cap + n:(l + 1) * cap]
            return out

        def check(got):
            dist_ref = O.mask_distribute(X["prop"], 2, 36)
            rf_ref, rb_ref = O.pyramid_roi_align(X["fmaps"], dist_ref, X["hw"], (14, 14))
            np.testing.assert_array_equal(got["kvals"], dist_ref[..., 0])
            np.testing.assert_array_equal(got["lmax"], got["lcounts"].max(axis=0))
            np.testing.assert_array_equal(got["lcounts"].sum(axis=1), [7, 0, 12])
            for b in range(3):
                for l in range(3):
                    n = got["lcounts"][b, l]
                    np.testing.assert_array_equal(got["slots"][b, l, :n], np.flatnonzero(dist_ref[b, :, 0] == l))
                    assert np.all(got["slots"][b, l, n:] == -1)
            np.testing.assert_array_equal(got["roi_boxes"], rb_ref)
            off = 0
            for l, (g, r) in enumerate(zip(got["roi_fmaps"], rf_ref)):
                assert g.shape == r.shape
                np.testing.assert_array_equal(g == -1.0, r == -1.0)        # MoldBatch padding pattern
                np.testing.assert_allclose(g, r, atol=2e-5)
                np.testing.assert_array_equal(g == 0.0, r == 0.0)          # extrapolation cells
                DM.assert_same_bits(got[f"capacity_fmaps{l}"], g, f"level {l} at capacity")
                DM.assert_same_bits(got[f"capacity_boxes{l}"], got["roi_boxes"][:, off:off + g.shape[1]], f"level {l} boxes")
                off += g.shape[1]

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("mask_distribute_roi_crop", [], build, never_poison=["lcounts", "lmax"])


def _mold_levels_dev():
    """test_mold_levels_on_the_device...[2-3-10]: the molded tensor is the FRONT of a capacity buffer; the rest is not written."""
    def build():
        from masklab_hip import ops
        rng = np.random.default_rng(3)

        def problem(B, L, cap, tail, lmax):
            src = rng.normal(size=(B, L * cap) + tail).astype(np.float32)
            return dict(src=src, cap=cap, lmax=lmax, n_l=[min(max(1, v), cap) for v in lmax], sd=dev(src),
                        ld=dev(np.asarray(lmax, np.int32)))

        X, Y = problem(2, 3, 10, (6,), [10, 1, 3]), problem(1, 3, 100, (28, 28, 5), [37, 0, 12])

        def run(p):
            buf = ops.mold_levels_dev(p["sd"], p["ld"], p["cap"])
            front = ops.molded_front(buf, p["n_l"])
            assert front.is_contiguous() and front.data_ptr() == buf.data_ptr()
            return {"front": front, "untouched:rest": buf.view(-1)[front.numel():]}

        def check(got):
            want = np.concatenate([X["src"][:, l * X["cap"]:l * X["cap"] + n] for l, n in enumerate(X["n_l"])], axis=1)
            np.testing.assert_array_equal(got["front"], want)
            assert got["untouched:rest"].size == X["src"].size - want.size > 0

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("mold_levels_dev", [], build, never_poison=["front"])


def _trim_instances():
    def build():
        from masklab_hip import ops
        from oracle import masklab as O
        import test_gpu_deploy as TDP
        X, Y = TDP._molded_rois(2, 8, 5, 28, seed=8, holes=False), TDP._molded_rois(2, 37, 5, 28, seed=37, holes=True)
        Xd, Yd = [dev(a) for a in X], [dev(a) for a in Y]

        def run(args):
            boxes, masks, counts = ops.trim_instances(*args)
            return {"boxes": boxes, "masks": masks, "counts": counts}

        def check(got):
            wb, wm = O.trim_instances(X[0], X[1], mold=True)
            n = wb.shape[1]
            assert n == max(1, int(got["counts"].max()))
            np.testing.assert_array_equal(got["counts"], (X[0][..., 4] != -1).sum(axis=1))
            np.testing.assert_array_equal(got["boxes"][:, :n], wb)
            np.testing.assert_array_equal(got["masks"][:, :n], wm)
            assert np.all(got["boxes"][:, n:] == -1) and np.all(got["masks"][:, n:] == -1)      # MoldBatch padding

        return dict(run_x=lambda: run(Xd), run_y=lambda: run(Yd), check=check)
    return Case("trim_instances", [], build, never_poison=["counts"])


def _deconv_tail():
    """The 7 x 7 row of test_deconv2x2_out1x1_fused_tail into a tensor with two more RoI slots per image than the levels fill:
    every level lands at its `out_base`, the spare slots are not written."""
    def build():
        from masklab_hip import _lib, ops, packing
        from oracle import tfops as T
        rng = np.random.default_rng(36)
        cmid, K, ncls, h, w_, spare = 128, 64, 5, 7, 7, 2

        def problem(levels):
            B, total, items, off = levels[0][0], sum(n for _, n in levels), [], 0
            per_roi = 4 * h * w_ * ncls
            want = np.zeros((B, total, 2 * h, 2 * w_, ncls))
            for _, n in levels:
                x = _normal(rng, B * n, h, w_, K)
                wd, bd = _normal(rng, 2, 2, cmid, K, scale=0.05), _normal(rng, cmid)
                wo, bo = _normal(rng, 1, 1, cmid, ncls, scale=0.1), _normal(rng, ncls)
                y = T.sigmoid(T.conv2d(T.relu(T.conv2d_transpose_2x2_s2(x.astype(np.float64), wd, bd)), wo, bo))
                want[:, off:off + n] = y.reshape(B, n, 2 * h, 2 * w_, ncls)
                table, bo_p, _ = packing.pack_out1x1_table(wo, bo)
                items.append(dict(x=dev(x), dc=ops.DeviceConv(packing.pack_transpose2x2(wd, bd), "cuda"), wo_table=dev(table),
                                  bo=dev(bo_p), out_base=off * per_roi, rois_per_image=n))
                off += n
            return dict(B=B, total=total, items=items, want=want)

        X, Y = problem([(2, 9), (2, 30)]), problem([(3, 4)])

        def run(p):
            out = torch.empty((p["B"], p["total"] + spare, 2 * h, 2 * w_, ncls), dtype=torch.float32, device="cuda")
            ops.deconv2x2_out1x1_multi([dict(it, out=out) for it in p["items"]], ncls, _lib.ACT_RELU, _lib.ACT_SIGMOID)
            o = host(out)
            return {"masks": o[:, :p["total"]], "untouched:spare": o[:, p["total"]:]}

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y),
                    check=lambda got: np.testing.assert_allclose(got["masks"], X["want"], atol=2e-5))
    return Case("deconv2x2_out1x1_multi", [], build, never_poison=["masks"])


# ------------------------------------------------------------------ serving summary
def _summary():
    def build():
        from masklab_hip.layers import CropAndPadMask, SummaryOutput
        from oracle import masklab as O
        import test_gpu_serving as TS

        def problem(B, n, H, W, seed):
            det, ins, seg = TS._scene(B=B, n=n, H=H, W=W, seed=seed, crack=True)
            return dict(det=det, ins=ins, seg=seg, d=dev(det), i=dev(ins), s=dev(seg), im=dev(np.zeros((B, H, W, 3), np.uint8)))

        X, Y = problem(2, 7, 90, 160, 3), problem(3, 9, 130, 200, 11)
        layer = SummaryOutput(3.25)

        def run(p):
            masks = CropAndPadMask()([p["im"], p["d"], p["i"], p["s"]])              # ops.crop_pad_mask: the threshold word
            return {"masks": masks, "summary": layer([p["d"], p["s"], masks]),      # ops.instance_summary
                    "summary_rois": layer([p["d"], p["s"], p["i"]], from_rois=True)}  # ops.instance_summary_rois

        def check(got):
            H, W = X["seg"].shape[1:3]
            masks = O.crop_and_pad_mask((H, W), X["det"], X["ins"])
            np.testing.assert_array_equal(got["masks"], masks)                       # test_crop_and_pad_mask
            want, g = O.summary_output(X["det"], X["seg"], masks, 3.25), got["summary"]
            assert g.shape == want.shape == (2, X["det"].shape[1] + 1, 11)           # test_summary_output
            np.testing.assert_array_equal(g[..., :6], want[..., :6])
            np.testing.assert_allclose(g[..., 6], want[..., 6], rtol=1e-6)
            np.testing.assert_allclose(g[..., 7:10], want[..., 7:10], rtol=2e-3)
            np.testing.assert_array_equal(g[..., 10], want[..., 10])
            DM.assert_same_bits(got["summary_rois"], g, "from_rois against the materialised path")

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("summary", ["summary"], build, never_poison=["masks", "summary", "summary_rois"])


# ------------------------------------------------------------------ JPEG
def _jpeg_encode():
    def build():
        from masklab_hip import ops
        import test_gpu_jpeg as TJ
        with np.load(os.path.join(GOLDEN, "jpeg", "frames.npz")) as z:
            small, other = z["noise_37x53"], z["smooth_48x70"]
        with open(os.path.join(GOLDEN, "jpeg", "manifest.json")) as fh:
            manifest = json.load(fh)
        Xd, Yd = dev(small[None]), dev(other[None])

        def run(frames):
            buffer, lengths = ops.encode_jpeg(frames, 95)
            return {"lengths": lengths, "streams": ops.jpeg_contents(buffer, lengths)}      # (bytes past a length: unspecified)

        def check(got):
            assert got["streams"][0][:len(TJ.J.header(37, 53, 95))] == TJ.J.header(37, 53, 95)
            TJ.check_coefficients(got["streams"][0], small, 95, TJ.allowed(manifest, "noise_37x53", 95), "noise_37x53")

        return dict(run_x=lambda: run(Xd), run_y=lambda: run(Yd), check=check)
    return Case("jpeg_encode", ["jpeg"], build, never_poison=["lengths"])


def _jpeg_decode(name, other, entropy):
    def build():
        from masklab_hip import ops
        import jpeg_decode_ref as D
        cases = D.load_cases(GOLDEN)
        X, Y = cases[name], cases[other]
        assert X["supported"] and Y["supported"] and X["pixels"].shape != Y["pixels"].shape

        def run(c):
            return {"pixels": ops.decode_jpeg(c["stream"], "cuda:0", entropy=entropy)}

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y),
                    check=lambda got: np.testing.assert_array_equal(got["pixels"][0], X["pixels"], err_msg=name))
    tags = ["jpeg_decode"] + (["jpeg_entropy"] if entropy == "device" else [])
    return Case(f"jpeg_decode[{name}-{entropy}]", tags, build)


def _jpeg_entropy():
    """The smallest fixture and a scan across several workgroups in one call: packed bytes and all four status words."""
    def build():
        from masklab_hip import _lib, ops
        import jpeg_decode_ref as D
        import jpeg_entropy_streams as S
        cases = D.load_cases(GOLDEN)
        bits, per_wg = ops.jpeg_entropy_geometry()
        plain, _, subsequences = S.noise_across_workgroups(bits, per_wg)
        assert subsequences > 3 * per_wg
        X, Y = [cases["crop_1x1_q95"]["stream"], plain], [cases["photo_150x203_q95"]["stream"]]

        def run(streams):
            packed, offsets, status = ops.jpeg_entropy_device(streams, "cuda:0")
            data, out = host(packed), []
            for b in range(len(streams)):
                assert status[b, 0] == 0, status[b].tolist()
                n = int(data[offsets[b] + 24:offsets[b] + 28].view(np.uint32)[0])
                assert 224 < n <= offsets[b + 1] - offsets[b]
                out.append(data[offsets[b]:offsets[b] + n].tobytes())               # (past the header's length: unspecified)
            return {"packed": out, "status": status}

        def check(got):
            lib = _lib.load()
            for b, s in enumerate(X):
                assert got["packed"][b] == S.host_packed(lib, s)[0], f"stream {b}: packed bytes differ from the host decoder's"
            assert got["status"][1, 3] >= 1, "no state crossed a workgroup boundary"

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("jpeg_entropy", ["jpeg_entropy"], build)


# ------------------------------------------------------------------ evaluation kernels (counters added to by atomics)
def _evaluation():
    def build():
        from masklab_hip import ops
        import evaluate_cases as EC
        import evaluate_ref as REF
        _, gt_ins, _ = EC.ground_truth()

        def problem(size, shape):
            det, ins = EC.predictions(size)
            pairs = EC.all_pairs(2, det.shape[1], gt_ins.shape[1])
            pr = EC.semantic_prediction(shape)
            rng = np.random.default_rng(shape[1])
            gt = (rng.random(shape) < 0.4).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
            return dict(det=det, ins=ins, pairs=pairs, pr=pr, gt=gt, d=[dev(a) for a in (det, ins, gt_ins, pairs, pr, gt)])

        X, Y = problem(14, (2, 37, 53, 3)), problem(28, (2, EC.H, EC.W, 3))

        def run(p):
            det, ins, gti, pairs, pr, gt = p["d"]
            area = ops.eval_mask_area(gti)
            return {"area": area, "pairs": ops.eval_mask_pairs(det, ins, gti, area, pairs), "semantic": ops.eval_semantic_counts(pr, gt)}

        def check(got):
            np.testing.assert_array_equal(got["area"], REF.mask_areas(gt_ins))
            np.testing.assert_array_equal(got["pairs"], REF.pair_stats(X["det"], X["ins"], gt_ins, X["pairs"]))
            np.testing.assert_array_equal(got["pairs"][-5:], -1)                     # index out of range: (-1, -1) by contract
            np.testing.assert_array_equal(got["semantic"], REF.semantic_counts(X["pr"], X["gt"]))

        return dict(run_x=lambda: run(X), run_y=lambda: run(Y), check=check)
    return Case("evaluation_kernels", [], build, never_poison=["area", "semantic"])


CASES = [
    _conv_split_k("f32"), _conv_split_k("f32x3"), _conv_split_k("f16s"), _conv_multi(),
    _gn(), _gn_multi(),
    _se((2, 16, 16, 256, 16), (1, 160, 160, 128, 8), False), _se((2, 16, 16, 256, 16), (1, 160, 160, 128, 8), True),
    _se((1, 160, 160, 128, 8), (2, 16, 16, 256, 16), False), _se((1, 160, 160, 128, 8), (2, 16, 16, 256, 16), True),
    _se_multi(False), _se_multi(True),
    _se_residual(), _se_bottleneck(False), _se_bottleneck(True),
    _det("det[lds_stage2]", 100), _det("det[workspace_stage2]", 1000), _det("det[equal_scores_global_rounds]", 100, True),
    _roi_levels(), _mold_levels_dev(), _trim_instances(), _deconv_tail(),
    _summary(),
    _jpeg_encode(), _jpeg_decode("crop_1x1_q95", "noise_37x53_q95", "host"),
    _jpeg_decode("noise_37x53_q95", "photo_150x203_q95", "host"), _jpeg_decode("crop_1x1_q95", "noise_37x53_q95", "device"),
    _jpeg_entropy(),
    _evaluation(),
]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_launch_on_stale_memory(case):
    built = case.build()
    run_x, run_y, check = built["run_x"], built["run_y"], built["check"]
    with DM.zeroed():
        clean = DM.snapshot(run_x())
    with DM.poisoned():
        first, second = DM.interleaved(run_x, run_y)
    written = lambda r: {k: v for k, v in r.items() if not k.startswith("untouched:")}
    DM.assert_same_bits(written(first), written(clean), f"{case}: (a) poisoned against zeroed memory")
    for key in case.never_poison:                                               # (b)
        for a in (first[key] if isinstance(first[key], list) else [first[key]]):
            assert not DM.poison_elements(a).any(), f"{case}: (b) `{key}` still holds 0xFF elements"
    for key in first:                                                           # (c)
        if key.startswith("untouched:"):
            assert DM.holds(clean[key], 0x00) and DM.holds(first[key], DM.POISON) and DM.holds(second[key], DM.POISON), \
                f"{case}: (c) `{key[10:]}` was written where the op promises not to"
    DM.assert_same_bits(written(second), written(first), f"{case}: (d) X again after Y")
    check(first)                                                                # (e)


# ------------------------------------------------------------------ whole paths, eager, against their clean runs
def _hot(w):
    for k in w:             # scores near 0.5 for a fraction of the anchors (tests/test_gpu_model.py: hot_cls)
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)
    return w


def _model(cfg, seed=5):
    from masklab_hip import retinamasklab as R
    _, model = R.construct_masklab_networks(cfg)
    model.load_weights(_hot(model.init_weights(seed)), "cuda:0")
    return model


def _clean_then_poisoned(run, what):
    """run() on ordinary memory, then on poisoned memory: the same bits, and no NaN in a float output."""
    clean = DM.snapshot(run())
    with DM.poisoned():
        dirty = DM.snapshot(run())
    DM.assert_same_bits(dirty, clean, what)
    return dirty


def _forward_case(model, images, what):
    outs = _clean_then_poisoned(lambda: model.predict(images), what)
    for name, o in zip(model.output_names, outs):
        assert not np.isnan(o).any(), (what, name)
    boxes = outs[model.output_names.index("roi_boxes")]
    assert int((boxes[..., 4] >= 0).sum()) > 0, f"{what}: the fixture needs detections"


IMAGES = np.random.default_rng(256).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def resnext50():
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "resnext50"
    return _model(cfg)


@pytest.mark.parametrize("math", ["f32", "f32x3", "f16s"])
@pytest.mark.parametrize("device_counts", [False, True], ids=["host_counts", "device_counts"])
def test_resnext50_forward_on_stale_memory(resnext50, math, device_counts):
    from masklab_hip import ops
    resnext50.device_counts = device_counts
    ops.set_conv_math(math)
    try:
        _forward_case(resnext50, IMAGES, f"resnext50 {math}")
    finally:
        ops.set_conv_math("f32")
        resnext50.device_counts = "auto"


def test_shipped_se_heads_on_seresnet34_on_stale_memory():
    import backbone_cases as BC
    model = _model(BC.shipped_se_config("seresnet34", ('C3', 'C4', 'C5', 'P6')))
    for device_counts in (False, True):
        model.device_counts = device_counts
        _forward_case(model, IMAGES, f"seresnet34 shipped heads, device_counts={device_counts}")


def test_default_resnet50_with_the_projection_fusion_on_stale_memory():
    from masklab_hip import ModelConfiguration, ops
    cfg = ModelConfiguration()
    assert cfg.backbone.backbone_type == "resnet50"
    before = ops.PROJECTION_FUSION
    ops.set_projection_fusion("on")
    try:
        assert ops.projection_fused()
        _forward_case(_model(cfg), IMAGES, "resnet50, projection fusion on")
    finally:
        ops.set_projection_fusion(before)


def test_serving_chain_on_stale_memory():
    """Deploy -> summary -> visualize -> JPEG encode at the 128 x 256 working size of test_serving_model_end_to_end."""
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "mobilenet"
    cfg.postprocess.resolution = (128, 256)
    model = _model(cfg, seed=3)
    serving = R.construct_serving_network(cfg, R.construct_deploy_network(cfg, model), visualize=True, encode=True)
    images = np.random.default_rng(1234).integers(0, 256, (2, 320, 640, 3), dtype=np.uint8)
    contents, summary = _clean_then_poisoned(lambda: serving.predict(images), "serving chain")
    assert len(contents) == 2 and all(c[:2] == b"\xff\xd8" and c[-2:] == b"\xff\xd9" for c in contents)
    assert not np.isnan(summary).any() and (summary[..., 0] >= 0).any(), "the fixture needs detections"


from test_gpu_evaluate import shipped    # noqa: E402,F401  (the module-scoped fixture of the evaluation tests)


def test_evaluate_on_stale_memory(shipped):
    from masklab_hip.evaluate import evaluate
    deploy, dataset, _ = shipped
    got = _clean_then_poisoned(lambda: evaluate(deploy, dataset), "evaluate()")
    assert any(v["counts"] > 0 and 0 < v["miou"] < 1 for v in got.values())


# ------------------------------------------------------------------ captured graphs: the interleave only
@pytest.mark.parametrize("bt", ["mobilenet", "resnext50"])
def test_graph_replay_after_an_eager_forward_of_another_shape(bt):
    """predict (captured, then replayed), one eager predict of another batch and image size on the same workspaces and
    allocator, the first input again: the two graph results are the same bits.  torch.empty is not patched under capture."""
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
    model = _model(cfg)
    other = np.random.default_rng(7).integers(0, 256, (3, 128, 256, 3), dtype=np.uint8)
    model.enable_graphs(True)
    try:
        first, second = DM.interleaved(lambda: model.predict(IMAGES),
                                       lambda: model.predict(other, want_kept=True))     # (want_kept: launched eagerly)
        assert len(model._graphs) == 1, "the forward between the replays was captured too"
    finally:
        model.enable_graphs(False)
    DM.assert_same_bits(second, first, f"{bt}: replay after an eager forward of another shape")
    assert int((first[model.output_names.index("roi_boxes")][..., 4] >= 0).sum()) > 0
