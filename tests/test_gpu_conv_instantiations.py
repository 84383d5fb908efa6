"""GPU tests of every instantiation of the generic implicit-GEMM conv kernel (csrc/conv_mfma.hip, `kGenericKernels`), each
checked BY NAME: a case of tests/conv_cases.py is one launch -- small problems under test plus a filler -- that the library
plans onto exactly one instantiation, and the test asserts the profile name, the tile entries and the K slices of the launch
it made before it looks at a value.

Per case: values against fp64 oracle.tfops (operands rounded to half first where the math rounds them: "f16" on the way into
LDS, "f16s" in memory), the filler's own first and last 256 rows, and every destination a sentinel-filled flat buffer with
spare elements before, after and between pixels (tests/sentinel_dest.py); gn_partials and the split-K workspace start as NaN.
Tolerances are the suite's: 2e-5 abs for fp32 outputs on O(1) data with weights scaled 1 / sqrt(K) (tests/test_gpu_ops.py,
tests/test_gpu_f16.py on rounded operands), rtol 2^-10 / atol 1e-4 for half outputs (tests/test_gpu_f16_storage.py).  The
GroupNorm partial sums are compared with the kernel's own stored output, folded as the epilogue folds it (a float4 in fp32,
then fp64).

Bit identity ("the same k-ordered chain whatever the tile shape"): every problem whose K sum is one slice in both launches
is launched once alone -- 128 x 32 tiles -- and once under its filler, and "f32x3" also under the 256-row filler; all give
the same bits, and so does the gn_partials form of a kernel.  `k5` (3 slices alone) and `long_k` (9 slices alone, 4 under "f16s") are cut differently when alone: both
launches are compared with fp64 only.  The widest case of each math is launched three times: the same bits.

Instantiations covered and the worst error against fp64 as measured on the MI355X (fp32 outputs: max abs, bar 2e-5; half
outputs: max abs from the reference rounded to half -- 3.9e-3 is one half step at the top of ReLU6's range):
  f32    128x128, 128x64, 128x32, 128x128 gns, 128x128 split-K                         fp32 9.3e-6
  f32x3  128x128, 128x64, 128x32, 128x128 gns, 256x128, 256x128 gns, 128x128 split-K   fp32 4.2e-6
  f16    128x128, 128x64, 128x32                                                       fp32 3.9e-6, half 3.9e-3
  f16s   128x128, 128x64, 128x32, 128x128 gns                                          fp32 1.5e-6, half 3.9e-3
(The fp32 worst cases: the ReLU6 problems, whose sums run at magnitudes up to 8, and `long_k` under its filler -- ONE chain
of 2 304 terms, 8.6e-6.)"""
import collections
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import conv_cases as CC
from oracle import tfops as T
from sentinel_dest import Dest

F32_ATOL = 2e-5                              # tests/test_gpu_ops.py::test_conv2d_dense, tests/test_gpu_f16.py
HALF_RTOL, HALF_ATOL = 2.0 ** -10, 1e-4      # tests/test_gpu_f16_storage.py
SET_CASES = [c.name for c in CC.CASES if c.filler and not c.gns]
Run = collections.namedtuple("Run", "kernels tiles splits outs partials filler")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from masklab_hip import _lib, ops
    _lib.check(_lib.load().ml_device_check(), "ml_device_check")
    yield
    ops.set_conv_math("f32")


@functools.lru_cache(maxsize=None)
def _dc(prob, tile):
    from masklab_hip import ops
    return ops.DeviceConv(CC.packed(prob, tile), "cuda")


@functools.lru_cache(maxsize=None)
def _filler(spec, tile, half):
    from masklab_hip import ops, packing
    d = CC.filler_data(spec)
    x = d["x"].astype(np.float16) if half else d["x"]
    return dev(x), ops.DeviceConv(packing.pack_dense(d["w"], d["b"], tile=tile), "cuda")


class _Entry:
    """One problem of a launch: its device tensors, its sentinel destination and the keyword arguments of ops._conv_desc."""

    def __init__(self, prob, math, tile):
        from masklab_hip import _lib
        self.prob, self.math = prob, math
        d = CC.data(prob)
        x = d["x"]
        if prob.kind == "stem":
            x = np.concatenate([x, np.zeros_like(x[..., :1])], -1)             # the NHWC4 image
        self.x = dev(x.astype(np.float16) if CC.half_in(math) else x)
        self.dc = _dc(prob, tile)
        B, Ho, Wo, co = CC.out_shape(prob)
        hout = CC.half_out(prob, math)
        cstride, coff, head, bgap = CC.dest_layout(prob)
        self.dest = Dest((B, Ho, Wo), co, cstride, coff=coff, head=head, bgap=bgap,
                         dtype=torch.float16 if hout else torch.float32)
        self.kw = dict(stride=prob.stride, padding="valid" if prob.kind == "shuffle" else prob.padding, dilation=prob.dil,
                       act=_lib.ACT_BY_NAME[prob.act])
        if bgap or head % (8 if hout else 4):
            self.kw["out_view"] = self.dest.view
        else:
            self.kw.update(out=self.dest.out, out_coff=coff)
        self.res_coff = 0
        if CC.has_res(prob, math):
            r = d["res"]
            if prob.res == "slice":                  # the residual at channels [4, 4 + cout) of a wider buffer of large values
                wide = np.full(r.shape[:3] + (co + 8,), 1000.0, np.float32)
                wide[..., 4:4 + co] = r
                r, self.res_coff = wide, 4
            self.kw["residual"] = dev(r)
        self.partials = None
        if prob.gn:
            self.partials = torch.full(((B * Ho * Wo) // 128, 4, 2), float("nan"), dtype=torch.float64, device="cuda")
            self.kw["gn_partials"] = self.partials


class _FillerEntry:
    def __init__(self, spec, math, tile):
        from masklab_hip import _lib
        self.x, self.dc = _filler(spec, tile, CC.half_in(math))
        self.kw, self.res_coff = dict(padding="valid", act=_lib.ACT_RELU), 0


def _launch(entries):
    """One launch of `entries` through the package's own descriptor builder and launcher; the split-K workspace starts as
    NaN.  -> (profile names, (tile rows, tile columns) the library reports for these descriptors, K slices, results)."""
    from masklab_hip import _lib, ops
    lib = _lib.load()
    n = len(entries)
    arr = (_lib.ConvDesc * n)()
    rets, flops, nbytes, shapes = [], 0.0, 0.0, []
    for i, e in enumerate(entries):
        d, ret, (f, nb, shape) = ops._conv_desc(e.x, e.dc, **e.kw)
        d.res_coff = e.res_coff
        arr[i] = d
        rets.append(ret)
        flops, nbytes = flops + f, nbytes + nb
        shapes.append(shape)
    ops.workspace(int(lib.ml_conv2d_workspace_bytes()), "cuda:0", "conv").fill_(0xFF)       # fp32 NaN in every word
    tiles = (lib.ml_conv2d_launch_mtile(arr, n, 1), lib.ml_conv2d_launch_ntile(arr, n, 1))
    ops.PROFILE, ops.LAUNCH_LOG = [], []
    try:
        ops._launch_conv(arr, [(e.x, e.dc) for e in entries], flops, nbytes, shapes, multi=True)
        torch.cuda.synchronize()
        kernels, splits = [r["kernel"] for r in ops.PROFILE], [s for _, s in ops.LAUNCH_LOG]
    finally:
        ops.PROFILE = ops.LAUNCH_LOG = None
    assert len(splits) == 1
    return kernels, tiles, splits[0], rets


def _launch_case(case):
    from masklab_hip import ops
    ops.set_conv_math(case.math)
    try:
        entries = [_Entry(p, case.math, case.tile) for p in CC.case_probs(case)]
        fill = [_FillerEntry(case.filler, case.math, case.tile)] if case.filler else []
        kernels, tiles, splits, rets = _launch(entries + fill)
        outs = {e.prob.name: e.dest.read() for e in entries}
        partials = {e.prob.name: e.partials.cpu().numpy() for e in entries if e.partials is not None}
        return Run(kernels, tiles, splits, outs, partials, rets[-1].cpu().numpy() if fill else None)
    finally:
        ops.set_conv_math("f32")


@functools.lru_cache(maxsize=None)
def _run(case_name):
    return _launch_case(CC.BY_NAME[case_name])


@functools.lru_cache(maxsize=None)
def _alone(prob, math, tile):
    from masklab_hip import ops
    ops.set_conv_math(math)
    try:
        e = _Entry(prob, math, tile)
        kernels, tiles, splits, _ = _launch([e])
        return kernels, tiles, splits, e.dest.read()
    finally:
        ops.set_conv_math("f32")


def _compare(got, want, half, what):
    """-> the largest abs error; asserts the suite's tolerance for this output type."""
    got = got.astype(np.float64)
    assert got.shape == want.shape, what
    err = float(np.abs(got - want).max())
    print(f"  {what}: max abs vs fp64 {err:.3e}" + (" (half)" if half else ""))
    if half:
        np.testing.assert_allclose(got, want, rtol=HALF_RTOL, atol=HALF_ATOL, err_msg=what)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=F32_ATOL, err_msg=what)
    return err


def _check_filler(case, out):
    """The filler runs on the same kernel: its first and last 256 rows against fp64."""
    d = CC.filler_data(case.filler)
    rounded = case.math in ("f16", "f16s")
    cast = CC.h64 if rounded else (lambda a: a.astype(np.float64))
    for rows in (slice(0, 256), slice(case.filler[0] - 256, case.filler[0])):
        want = T.relu(T.conv2d(cast(d["x"][:, rows]), cast(d["w"]), d["b"].astype(np.float64), 1, "valid"))
        if CC.half_in(case.math):
            want = want.astype(np.float16).astype(np.float64)
        _compare(out[:, rows], want, CC.half_in(case.math), f"{case.name}/filler rows {rows.start}..")


def _check_partials(y, pt, what):
    """gn_partials [128-row tile][wave][sum, sum of squares] against the stored output `y`: wave w of a tile owns its rows
    2w, 2w + 1 mod 8 (on the 256-row tile: waves w and w + 4 together), a float4 is folded in fp32 -- (v0 + v1) + (v2 + v3) and
    fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 v0))) -- and the folds are added in fp64."""
    assert np.isfinite(pt).all(), what                               # every slot written
    v = y.astype(np.float32).reshape(-1, 128, 32, 4)                 # [tile][row][quad][4]
    s4 = ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])).astype(np.float64)
    q = v[..., 0] * v[..., 0]
    for e in (1, 2, 3):                                              # fma: the square is exact in fp64, one rounding to fp32
        q = (v[..., e].astype(np.float64) ** 2 + q.astype(np.float64)).astype(np.float32)
    q4 = q.astype(np.float64)
    for w in range(4):
        rows = [r for r in range(128) if (r % 8) // 2 == w]
        np.testing.assert_allclose(pt[:, w, 0], s4[:, rows].sum(axis=(1, 2)), rtol=1e-9, err_msg=what)
        np.testing.assert_allclose(pt[:, w, 1], q4[:, rows].sum(axis=(1, 2)), rtol=1e-9, err_msg=what)


@pytest.mark.parametrize("name", [c.name for c in CC.CASES])
def test_case_runs_on_its_instantiation_and_equals_fp64(name):
    case = CC.BY_NAME[name]
    run = _run(name)
    probs = CC.case_probs(case)
    # the kernel, by name
    assert run.kernels == [case.kernel], run.kernels
    assert run.tiles == (case.bm, case.bn)
    assert list(run.splits) == [case.splits] * len(probs) + [1] * bool(case.filler), run.splits
    # values (reading a destination has already asserted that nothing outside it was written)
    print(f"\n{name} on {case.kernel}:")
    worst = collections.defaultdict(float)
    for p in probs:
        half = CC.half_out(p, case.math)
        worst[half] = max(worst[half], _compare(run.outs[p.name], CC.expected(p, case.math), half, f"{name}/{p.name}"))
    if case.filler:
        _check_filler(case, run.filler)
    assert set(run.partials) == {p.name for p in probs if p.gn} and bool(run.partials) == case.gns
    for pname, pt in run.partials.items():
        _check_partials(run.outs[pname], pt, f"{name}/{pname}")
    print(f"{name}: worst fp32 {worst[False]:.3e}, worst half {worst[True]:.3e}")


@pytest.mark.parametrize("name", SET_CASES)
def test_alone_on_narrow_tiles_gives_the_bits_of_the_wide_launch(name):
    case = CC.BY_NAME[name]
    run = _run(name)
    for p in CC.case_probs(case):
        kernels, tiles, splits, got = _alone(p, case.math, case.tile)
        assert kernels == ["conv_mfma_128x32" + CC.SUFFIX[case.math]] and tiles == (128, 32), (p.name, kernels)
        assert list(splits) == [p.alone_splits(case.math)], (p.name, splits)
        if splits[0] == 1:
            assert np.array_equal(got, run.outs[p.name]), f"{name}/{p.name}: {int((got != run.outs[p.name]).sum())} elements differ"
        else:                                        # cut along K when alone: other chains, so fp64 only
            half = CC.half_out(p, case.math)
            _compare(got, CC.expected(p, case.math), half, f"{name}/{p.name} alone, {splits[0]} K slices")


@pytest.mark.parametrize("a,b", [("f32x3_128x128", "f32x3_256x128"), ("f32x3_128x128_gns", "f32x3_256x128_gns"),
                                 ("f32_128x128", "f32_128x128_gns"), ("f16s_128x128", "f16s_128x128_gns"),
                                 ("f32x3_128x128", "f32x3_128x128_gns")])
def test_a_problem_gives_the_same_bits_on_another_wide_instantiation(a, b):
    """f32x3: 256-row tiles against 128-row tiles; every math: the gn_partials form against the plain one (the problems the
    two cases share)."""
    ra, rb = _run(a), _run(b)
    shared = set(ra.outs) & set(rb.outs)
    assert shared
    for pname in shared:
        assert np.array_equal(ra.outs[pname], rb.outs[pname]), (a, b, pname)
    for pname in set(ra.partials) & set(rb.partials):    # (the 256-row form adds two waves' fp64 sums: last-bit differences)
        np.testing.assert_allclose(ra.partials[pname], rb.partials[pname], rtol=1e-12)


@pytest.mark.parametrize("math", list(CC.WIDEST))
def test_widest_case_three_launches_give_the_same_bits(math):
    case = CC.BY_NAME[CC.WIDEST[math]]
    runs = [_launch_case(case) for _ in range(3)]
    for r in runs:
        assert r.kernels == [case.kernel]
    for r in runs[1:]:
        for pname, out in runs[0].outs.items():
            assert np.array_equal(out, r.outs[pname]), (math, pname)
        assert np.array_equal(runs[0].filler, r.filler), math
