"""GPU tests of every instantiation of the ResNeXt grouped 3x3 (csrc/gconv_mfma4.hip): the rows of tests/gconv_cases.py, each
launched through the C entry itself (ml_gconv3x3_f32 / _f16, the arguments ops.gconv3x3 would pass) into a sentinel-filled
buffer (tests/sentinel_dest.py) with one image row of guard before and behind the output.

Per row: the library plans the launch the table names (tile shape, run, blocks; the table is written for the 256 compute units
of the MI355X -- on another count the row is skipped, never adapted); images 0 and B - 1 against the float64 reference of
gconv_cases.reference at the suite's bars -- fp32 2e-5 abs (tests/test_gpu_ops.py::test_gconv3x3_mfma4), half rtol 2^-10 /
atol 1e-4 against the reference rounded to half (tests/test_gpu_f16_storage.py); both guards intact and no output element
left holding the sentinel (with the values of image B - 1: no partial tile stores past row Ho or column Wo, none stops short);
a second launch gives the same bits.  Run rows: images 0 and B - 1 of the batch launch (runs of 3 + 2 tiles, the prefetch) are
bit-identical to the same image launched alone (one tile per block).  Rows without bias: the bits of the same row given an
all-zero bias.  Padding rows: ops.gconv3x3 with the row's `padding` gives the bits of the direct call.

Largest error against float64 measured on the MI355X, per kernel body over all its rows (fp32: max abs, bar 2e-5; half: max
abs from the reference rounded to half and the largest share of the bar rtol 2^-10 |want| + 1e-4 that any element uses):
    mfma4     fp32 c = 4, 8     2.0e-6   (run_f32_c8_s2)
    gconv16   fp32 c = 16       2.4e-6   (run_f32_c16_s1)
    mfma4h    half c = 4, 8     3.9e-3, 0.96 of the bar   (run_f16_c8_s1)
    gconv16h  half c = 16       2.0e-3, 0.92 of the bar   (run_f16_c16_s1)
    gconv32h  half c = 32       3.9e-3, 0.94 of the bar   (relu6_f16_c32_s1, same_f16_c32_s2)
The half figures are ONE half step -- 2^-8 = 3.9e-3 for a value in [4, 8), 2^-9 in [2, 4) -- where the fp32 sum lies within its
own rounding error of a rounding boundary and lands on the neighbouring half; just above 4 and 2 that step is 0.96 of the
bar, which the bar was set to admit.  No element is two steps off."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gconv_cases as GC
from sentinel_dest import SENT, Dest

F32_ATOL = 2e-5                              # tests/test_gpu_ops.py::test_gconv3x3_mfma4
HALF_RTOL, HALF_ATOL = 2.0 ** -10, 1e-4      # tests/test_gpu_f16_storage.py
ALL = [r.name for r in GC.ROWS]
RUN = [r.name for r in GC.ROWS if r.kind == "run" and r.c != 32]
NOBIAS = [r.name for r in GC.ROWS if not r.bias]
PADDING = [r.name for r in GC.ROWS if r.kind == "padding"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from masklab_hip import _lib
    _lib.check(_lib.load().ml_device_check(), "ml_device_check")


@functools.lru_cache(maxsize=None)
def _weights(row):
    from masklab_hip import packing
    k, b = GC.params(row)
    return dev(packing.pack_grouped_mfma4(k, row.C // row.c)), dev(b), torch.zeros(row.C, device="cuda")


def _launch(row, x, bias="row"):
    """One launch of the C entry on the images `x` [B, H, W, C] into a fresh sentinel destination -> Dest.
    bias: "row" = the row's own (none where it has none), "zero" = an all-zero tensor."""
    from masklab_hip import _lib, ops
    lib = _lib.load()
    wgt, b, zero = _weights(row)
    bt = zero if bias == "zero" else (b if row.bias else None)
    B, H, W, C = x.shape
    Ho, Wo, pt, pl = GC.out_hw(row)
    guard = Wo * C                                   # one image row (a multiple of 64 elements: the output stays 16-byte aligned)
    dest = Dest((B, Ho, Wo), C, C, head=guard, tail=guard, dtype=x.dtype)
    fn = lib.ml_gconv3x3_f16 if row.half else lib.ml_gconv3x3_f32
    _lib.check(fn(ops._ptr(x), ops._ptr(wgt), ops._ptr(bt), ops._ptr(dest.out), B, H, W, C, row.c, Ho, Wo, row.stride, pt, pl,
                  GC.ACT_CODE[row.act], ops._stream()), "ml_gconv3x3")
    return dest


def _guards_intact_and_output_written(dest, what):
    torch.cuda.synchronize()
    end = dest.head + dest.npix * dest.cstride
    assert bool((dest.buf[:dest.head] == SENT).all()), f"{what}: wrote before the output"
    assert bool((dest.buf[end:] == SENT).all()), f"{what}: wrote behind the output"
    left = int((dest.buf[dest.head:end] == SENT).sum())
    assert left == 0, f"{what}: {left} output elements not written"


@functools.lru_cache(maxsize=None)
def _run(name):
    """The row's launches, once: -> dict(first / last: images 0 and B - 1 of the batch launch (host arrays), repeat: a second
    launch gave the same bits, alone: the two images launched alone, zero_bias: the two images under an all-zero bias)."""
    row = GC.BY_NAME[name]
    B = row.shape[0]
    x = dev(GC.batch(row))
    dest = _launch(row, x)
    _guards_intact_and_output_written(dest, name)
    out = dest.out
    res = dict(first=out[0].cpu().numpy(), last=out[B - 1].cpu().numpy())
    again = _launch(row, x)
    _guards_intact_and_output_written(again, name + " (second launch)")
    res["repeat"] = torch.equal(out, again.out)
    del again
    if name in RUN:
        res["alone"] = []
        for i in (0, B - 1):
            d1 = _launch(row, x[i:i + 1].contiguous())
            _guards_intact_and_output_written(d1, f"{name} (image {i} alone)")
            res["alone"].append(d1.out[0].cpu().numpy())
    if not row.bias:
        dz = _launch(row, x, bias="zero")
        res["zero_bias"] = [dz.out[0].cpu().numpy(), dz.out[B - 1].cpu().numpy()]
    return res


def _compare(got, want, half, what):
    got = got.astype(np.float64)
    assert got.shape == want.shape, what
    diff = np.abs(got - want)
    bar = HALF_ATOL + HALF_RTOL * np.abs(want) if half else F32_ATOL
    print(f"GCONV_ERR {what} max_abs {diff.max():.3e} share_of_bar {float((diff / bar).max()):.3f}")
    if half:
        np.testing.assert_allclose(got, want, rtol=HALF_RTOL, atol=HALF_ATOL, err_msg=what)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=F32_ATOL, err_msg=what)


@pytest.mark.parametrize("name", ALL)
def test_row_is_planned_as_named_and_equals_fp64(name):
    row = GC.BY_NAME[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the table of tests/gconv_cases.py is written for 256 compute units, this device reports {cus}")
    rc, (th, tw, _, _, run, blocks) = GC.plan(row)
    assert rc == 0 and (th, tw, run, blocks) == row.plan
    res = _run(name)
    _, want = GC.reference(row)
    if row.act is not None:                           # the data reaches the clamps (also asserted without a GPU)
        pre, _ = GC.reference(row)
        assert (pre < 0).mean() >= 0.05 and (row.act != "relu6" or (pre > 6).mean() >= 0.05)
    print()
    _compare(res["first"], want[0], row.half, f"{row.body} {name} image 0")
    _compare(res["last"], want[1], row.half, f"{row.body} {name} image {row.shape[0] - 1}")
    assert res["repeat"], f"{name}: two launches differ"


@pytest.mark.parametrize("name", RUN)
def test_run_row_gives_the_bits_of_one_tile_per_block(name):
    row = GC.BY_NAME[name]
    rc, alone = GC.plan(row, B=1)
    assert rc == 0 and alone[4] == 1                 # (whatever the device: an image alone is far below 6 blocks per unit)
    rc, full = GC.plan(row)
    assert rc == 0 and full[4] > 1
    res = _run(name)
    for got, one, i in zip((res["first"], res["last"]), res["alone"], (0, row.shape[0] - 1)):
        assert np.array_equal(got, one), f"{name} image {i}: {int((got != one).sum())} elements differ from the launch alone"


@pytest.mark.parametrize("name", NOBIAS)
def test_no_bias_gives_the_bits_of_a_zero_bias(name):
    res = _run(name)
    for got, zero in zip((res["first"], res["last"]), res["zero_bias"]):
        assert np.array_equal(got, zero), name


@pytest.mark.parametrize("name", PADDING)
def test_ops_gconv3x3_passes_the_layers_padding(name):
    from masklab_hip import ops
    row = GC.BY_NAME[name]
    wgt, b, _ = _weights(row)
    got = ops.gconv3x3(dev(GC.batch(row)), wgt, b if row.bias else None, row.c, stride=row.stride, padding=row.padding,
                       act=GC.ACT_CODE[row.act])
    Ho, Wo, _, _ = GC.out_hw(row)
    assert tuple(got.shape) == (row.shape[0], Ho, Wo, row.C)
    torch.cuda.synchronize()
    res = _run(name)
    assert np.array_equal(got[0].cpu().numpy(), res["first"]) and np.array_equal(got[-1].cpu().numpy(), res["last"]), name
