"""GPU tests of the mask head's tail backward at the op level: ops.deconv2x2_out1x1_grad / _grad_multi
(csrc/deconv_out_grad.hip), the transposed conv's own gradients through its 1x1 view (ops.conv2d_wgrad_multi /
conv2d_dgrad_multi on the [1,1,cin,4 C_mid] packing, ops.deconv2x2_grad_relayout) and the forward's tape launch
(ops.deconv2x2_out1x1_multi(tape=)), against the float64 references of tests/mask_tail_grad_ref.py.

The bar is the project's gradient bar, |got - want| <= 1e-5 * S with S the uncancelled magnitude of the element, exact zeros
where S == 0 (tests/test_gpu_conv_grad.py's bar and definition; mask_tail_grad_ref.py states every S).  T is an INPUT here
and every element of it is exactly 0 or at least 0.05 from it, so no case depends on which side of the ReLU's kink a
rounding falls.  A slice's fp32 sum of L terms is off by at most L * 2^-24 * S (L = 4 rows x at most 128 pixels here), the
slices add in fp64.  Every op also holds: two launches give the same bits; the bits do not depend on what outputs, partials
and workspace held; the inputs are left unchanged; nothing outside the outputs is written (sentinel guards); a multi launch
gives the bits of its single launches; out=T (in place) gives the out-of-place bits.  -m gpu.

Largest |got - want| / S measured on the MI355X, per case (the bar is 1e-5):
    dT / dWo / dbo    m36_c128_n1 5.8e-08 / 3.1e-08 / 8.1e-10     m128_c256_n3 5.9e-08 / 4.7e-08 / 1.0e-09
                      m150_c128_n5 1.6e-07 / 2.9e-08 / 2.8e-09    slices_c256_n3 1.3e-07 / 2.5e-08 / 1.6e-09
                      slices_c128_sparse 5.9e-08 / 3.7e-08 / 1.4e-09   n32_c128 2.4e-07 / 4.0e-08 / 3.2e-09
                      n32_c256 5.9e-08 / 6.0e-08 / 2.8e-09        two_levels 5.9e-08 / 4.6e-08 / 2.6e-09
                      four_levels 1.7e-07 / 4.7e-08 / 3.9e-09
    dWd / dbd / dx    m36_c128_n1 1.8e-07 / 3.6e-08 / 1.6e-07     m128_c256_n3 2.4e-07 / 1.9e-08 / 1.3e-07
                      slices_c256_n3 1.6e-07 / 8.6e-09 / 6.0e-08  four_levels 1.4e-07 / 1.5e-08 / 9.3e-08
    the tape's T      m36_c128_n1 1.8e-07   m128_c256_n3 2.5e-07   m150_c128_n5 2.2e-07   slices_c256_n3 2.9e-07   n32_c128 2.4e-07
                      two_levels 2.6e-07   four_levels 2.5e-07"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import dirty_memory as DM
import mask_tail_grad_ref as R
from sentinel_dest import SENT
from test_gpu_resample_grad import _bits, _everything


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (inputs, per level the dict of (want, S)): computed once per case, shared and left unchanged"""
    inp = R.inputs(name)
    refs, off = [], 0
    for (n_l, h, w), lv in zip(R.CASES[name]["levels"], inp["levels"]):
        refs.append(R.op_reference(lv["T"], R.level_dy(inp["dy"], off, n_l), lv["wo"], lv["x"], lv["wd"]))
        off += n_l
    return inp, refs


def _problems(name, dyd=None):
    """-> (the problems of ops.deconv2x2_out1x1_grad_multi for the case, its (device tensor, host array) inputs)"""
    inp, _ = reference(name)
    c = R.CASES[name]
    dyd = dev(inp["dy"]) if dyd is None else dyd
    _, h, w = c["levels"][0]
    problems, pairs, off = [], [(dyd, inp["dy"])], 0
    for (n_l, _, _), lv in zip(c["levels"], inp["levels"]):
        Td, wod = dev(lv["T"]), dev(lv["wo"])
        problems.append(dict(dy=dyd, T=Td, wo=wod, hw=(h, w), rois_per_image=n_l, dy_base=off * 4 * h * w * c["ncls"]))
        pairs += [(Td, lv["T"]), (wod, lv["wo"])]
        off += n_l
    return problems, pairs


def _guarded(shape, head=8, tail=8):
    n = int(np.prod(shape))
    buf = torch.full((head + n + tail,), SENT, device="cuda", dtype=torch.float32)
    return buf, buf[head:head + n].view(*shape)


def _guards_hold(buf, n, head=8, what=""):
    flat = host(buf)
    assert (flat[:head] == SENT).all() and (flat[head + n:] == SENT).all(), f"{what}: written outside the output"


@pytest.mark.parametrize("name", list(R.CASES))
def test_tail_grad(name):
    """dT, dWo, dbo of every level in one launch against float64; the battery; multi against singles; in place; guards"""
    from masklab_hip import ops
    inp, refs = reference(name)
    c = R.CASES[name]
    problems, pairs = _problems(name)
    got = _everything(lambda: ops.deconv2x2_out1x1_grad_multi(problems), pairs, name)
    assert len(got) == len(refs)
    for i, (one, ref) in enumerate(zip(got, refs)):
        assert one[0].dtype == np.float32 and one[0].shape == inp["levels"][i]["T"].shape
        assert one[1].shape == (1, 1, c["C"], c["ncls"]) and one[2].shape == (c["ncls"],)
        R.check(one[0], *ref["dT"], f"{name} level {i} dT")
        R.check(one[1], *ref["dWo"], f"{name} level {i} dWo")
        R.check(one[2], *ref["dbo"], f"{name} level {i} dbo")
        assert not one[0][inp["levels"][i]["T"] <= 0].any()                # behind the ReLU's flat side: exact zeros, written
    # a multi launch gives the bits of its single launches (each level alone, with its own dy_base)
    singles = [DM.snapshot(ops.deconv2x2_out1x1_grad(**pr)) for pr in problems]
    DM.assert_same_bits(list(got), singles, f"{name}: one multi launch against single launches")
    # sentinel guards around dT, dkernel and dbias: the same bits, nothing written beside them
    bufs, guarded = [], []
    for pr, lv in zip(problems, inp["levels"]):
        tb, kb, bb = _guarded(lv["T"].shape), _guarded((1, 1, c["C"], c["ncls"])), _guarded((c["ncls"],))
        bufs.append((tb[0], kb[0], bb[0]))
        guarded.append(dict(pr, out=tb[1], out_kernel=kb[1], out_bias=bb[1]))
    ret = ops.deconv2x2_out1x1_grad_multi(guarded)
    _bits(ret, list(got), f"{name}: guarded outputs")
    for (tb, kb, bb), lv in zip(bufs, inp["levels"]):
        _guards_hold(tb, lv["T"].size, what=f"{name} dT")
        _guards_hold(kb, c["C"] * c["ncls"], what=f"{name} dkernel")
        _guards_hold(bb, c["ncls"], what=f"{name} dbias")
    # in place: dT over T, inside guards
    inplace, tbufs = [], []
    for pr, lv in zip(problems, inp["levels"]):
        tb, tv = _guarded(lv["T"].shape)
        tv.copy_(pr["T"])
        tbufs.append(tb)
        inplace.append(dict(pr, T=tv, out=tv))
    ret = ops.deconv2x2_out1x1_grad_multi(inplace)
    assert all(r[0].data_ptr() == pr["T"].data_ptr() for r, pr in zip(ret, inplace))
    _bits(ret, list(got), f"{name}: out=T against out of place")
    for tb, lv in zip(tbufs, inp["levels"]):
        _guards_hold(tb, lv["T"].size, what=f"{name} dT in place")


@pytest.mark.parametrize("name", ["m36_c128_n1", "m128_c256_n3", "slices_c256_n3", "four_levels"])
def test_transposed_conv_gradients_through_the_1x1_view(name):
    """dWd, dbd, dx: the existing weight- and data-gradient kernels on dT viewed [R,h,w,4 C_mid], fed the DEVICE's dT"""
    from masklab_hip import ops, packing
    inp, refs = reference(name)
    c = R.CASES[name]
    problems, _ = _problems(name)
    tails = ops.deconv2x2_out1x1_grad_multi(problems)
    _, h, w = c["levels"][0]
    dcs = [ops.DeviceConv(packing.pack_dense(packing.transpose2x2_as_1x1(lv["wd"]), np.tile(lv["bd"], 4)), torch.device("cuda:0"))
           for lv in inp["levels"]]
    xs = [dev(lv["x"]) for lv in inp["levels"]]
    dys = [t[0].view(x.shape[0], h, w, 4 * c["C"]) for t, x in zip(tails, xs)]
    args = dict(stride=1, padding="same", dilation=1)

    def run():
        pairs = ops.conv2d_wgrad_multi([dict(x=x, dy=dy, dc=dc, want_bias=True, **args) for x, dy, dc in zip(xs, dys, dcs)])
        own = [ops.deconv2x2_grad_relayout(dk1, db4) for dk1, db4 in pairs]
        dxs = ops.conv2d_dgrad_multi([dict(dy=dy, dc=dc, in_hw=(h, w), **args) for dy, dc in zip(dys, dcs)])
        return own, dxs, pairs

    own, dxs, pairs = _everything(run, [(x, lv["x"]) for x, lv in zip(xs, inp["levels"])], f"{name} 1x1 view")
    for i, ((dk, db), dx, (dk1, db4), ref) in enumerate(zip(own, dxs, pairs, refs)):
        np.testing.assert_array_equal(dk, packing.transpose2x2_from_1x1(dk1), err_msg="the kernel's re-layout is a transposition")
        b4 = db4.reshape(4, -1)
        np.testing.assert_array_equal(db, ((b4[0] + b4[1]) + b4[2]) + b4[3], err_msg="the bias: positions added in the order 0..3")
        R.check(dk, *ref["dWd"], f"{name} level {i} dWd")
        R.check(db, *ref["dbd"], f"{name} level {i} dbd")
        R.check(dx, *ref["dx"], f"{name} level {i} dx")


def test_a_workspace_that_is_too_small_is_refused():
    from masklab_hip import ops
    problems, _ = _problems("slices_c256_n3")
    need = ops.deconv2x2_out1x1_grad_plan(294, 49, 7, 3, 256, 3)[2]
    with pytest.raises(RuntimeError, match="workspace is too small"):
        ops.deconv2x2_out1x1_grad(**problems[0], workspace_bytes=need - 256)
    with pytest.raises(RuntimeError, match="write the same tensor"):
        shared = torch.empty((294, 4, 256), dtype=torch.float32, device="cuda")
        ops.deconv2x2_out1x1_grad_multi([dict(problems[0], out=shared), dict(problems[0], out=shared)])


# ------------------------------------------------------------------ the forward's tape launch
def _forward_problems(name, tape_out=None):
    from masklab_hip import ops, packing
    inp, _ = reference(name)
    c = R.CASES[name]
    total = sum(n for n, _, _ in c["levels"])
    _, h, w = c["levels"][0]
    out = torch.full((R.B, total, 2 * h, 2 * w, c["ncls"]), SENT, device="cuda", dtype=torch.float32)
    problems, off = [], 0
    for i, ((n_l, _, _), lv) in enumerate(zip(c["levels"], inp["levels"])):
        table, bo, _ = packing.pack_out1x1_table(lv["wo"], lv["bo"])
        pr = dict(x=dev(lv["x"]), dc=ops.DeviceConv(packing.pack_transpose2x2(lv["wd"], lv["bd"]), torch.device("cuda:0")),
                  wo_table=dev(table), bo=dev(bo), out=out, out_base=off * 4 * h * w * c["ncls"], rois_per_image=n_l)
        if tape_out is not None:
            pr["tape_out"] = tape_out[i]
        problems.append(pr)
        off += n_l
    return problems, out


@pytest.mark.parametrize("name", ["m36_c128_n1", "m128_c256_n3", "m150_c128_n5", "slices_c256_n3", "n32_c128", "two_levels",
                                  "four_levels"])
def test_the_tape_launch(name):
    """roi_masks bit-equal to the plain launch's; T within 1e-5 S of float64 relu(deconv); guards around the tapes"""
    from masklab_hip import _lib, ops
    inp, _ = reference(name)
    c = R.CASES[name]
    relu, sig = _lib.ACT_BY_NAME["relu"], _lib.ACT_BY_NAME["sigmoid"]
    plain_problems, plain_out = _forward_problems(name)
    ops.deconv2x2_out1x1_multi(plain_problems, c["ncls"], relu, sig)
    plain = DM.snapshot(plain_out)
    assert not (plain == SENT).any()

    def run(tape_out=None):
        problems, out = _forward_problems(name, tape_out)
        tape = []
        assert ops.deconv2x2_out1x1_multi(problems, c["ncls"], relu, sig, tape=tape) is None
        return out, tape

    out, tape = _everything(run, [], f"{name} tape launch")
    DM.assert_same_bits(out, plain, f"{name}: roi_masks of the tape launch against the plain launch")
    assert len(tape) == len(c["levels"])
    for i, (T, lv) in enumerate(zip(tape, inp["levels"])):
        x64, k = lv["x"].astype(np.float64).reshape(T.shape[0], -1), R.kernel_as_1x1(lv["wd"].astype(np.float64))
        want = np.maximum(x64 @ k + np.tile(lv["bd"].astype(np.float64), 4), 0.0).reshape(T.shape)
        S = (np.abs(x64) @ np.abs(k) + np.tile(np.abs(lv["bd"]).astype(np.float64), 4)).reshape(T.shape)
        assert T.dtype == np.float32 and (T >= 0).all()
        R.check(T, want, S, f"{name} level {i} T")
    # the tapes inside sentinel guards: the same bits, nothing written beside them (rows past a problem's end are not stored)
    bufs = [_guarded(lv["T"].shape, head=2048, tail=2048) for lv in inp["levels"]]
    out_g, tape_g = run([b[1] for b in bufs])
    _bits([out_g, tape_g], [out, list(tape)], f"{name}: guarded tapes")
    for (buf, _), lv in zip(bufs, inp["levels"]):
        _guards_hold(buf, lv["T"].size, head=2048, what=f"{name} tape")


def test_the_tape_feeds_the_backward():
    """Forward with tape, then the tail backward on that tape: against the op-level reference on the tape the device wrote
    (the standard bar), and dT against float64 autograd of the whole tail where the float64 pre-ReLU value lies at least
    1e-4 from 0 (elsewhere float32 may fall on the other side of the kink)"""
    from masklab_hip import _lib, ops
    name = "two_levels"
    inp, _ = reference(name)
    c = R.CASES[name]
    problems, out = _forward_problems(name)
    tape = []
    ops.deconv2x2_out1x1_multi(problems, c["ncls"], _lib.ACT_BY_NAME["relu"], _lib.ACT_BY_NAME["sigmoid"], tape=tape)
    back, _ = _problems(name)
    for pr, T in zip(back, tape):
        pr["T"] = T
    kept = DM.snapshot(tape)
    got = DM.snapshot(ops.deconv2x2_out1x1_grad_multi(back))
    DM.assert_same_bits(DM.snapshot(tape), kept, "the tape is left unchanged by an out-of-place backward")
    off = 0
    for (n_l, h, w), lv, one, T in zip(c["levels"], inp["levels"], got, kept):
        dyg = R.level_dy(inp["dy"], off, n_l)
        ref = R.op_reference(T, dyg, lv["wo"])
        for k, key in enumerate(("dT", "dWo", "dbo")):
            R.check(one[k], *ref[key], f"level of {n_l} RoIs: {key} on the device's tape")
        dz = inp["dy"][:, off:off + n_l].reshape(R.B * n_l, 2 * h, 2 * w, c["ncls"])
        _, _, pre = R.tail_autograd(lv["x"], lv["wd"], lv["bd"], lv["wo"], lv["bo"], dz, forward=R.tail_forward_gemm)
        far = np.abs(pre) >= 1e-4
        assert far.mean() > 0.99
        ref64 = R.op_reference(np.maximum(pre, 0.0), dyg, lv["wo"])
        R.check(np.where(far, one[0], 0.0), np.where(far, ref64["dT"][0], 0.0), ref64["dT"][1], f"level of {n_l} RoIs: dT, float64 tail")
        off += n_l
