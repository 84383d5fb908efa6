"""Fixed-capacity (`live`) launches, kernel by kernel against fp64.

Stage 2 without a host read launches the mask head for every RoI slot of every level; a device int tells each kernel which
slots exist (slot s of an image iff s < max(1, *live)).  The end-to-end tests mold the dead slots away, so they cannot see a
kernel that reads a dead slot's stale input into a live result, one that writes where it promised not to, or a `live` path
the shipped configurations do not reach.  Here every kernel that takes `live` is run on its own:

  * dead slots of every input hold NaN (in service: whatever the caching allocator left in torch.empty memory), live slots
    seeded normal data; the output is pre-filled with a finite canary;
  * live slots are compared with the fp64 oracle of the live slots only, and bit for bit with the same launch without
    `live` on clean data (convs: where the library reports the same K slices for both launches);
  * every element the documented contract says is not written still holds the canary: for the conv and the tail kernel the
    rows of tiles all of whose slots are dead (tests/live_cases.py, brute force over rows), for GroupNorm and the RoI crop
    every dead sample / slot.  Dead rows inside a tile that runs are unconstrained (they may be NaN);
  * *live is swept over 0, 1, 2, period - 1, period, period + 3: 0 behaves as 1, the last two equal the launch without
    `live` everywhere.

No tolerance is new: each is the one the `live`-less test of the same kernel and math uses (tests/test_gpu_ops.py:
2e-5 abs for dense convs, 3e-5 where K is cut, 2e-5 for GroupNorm, the RoI crop and the tail; tests/test_gpu_f16_heads.py:
close_half with HALF_RTOL / HALF_ATOL, rtol 1e-5 / atol 2e-5 for an fp32 destination).  Every conv case prints the kernel,
tiles and K slices the library reports for it.  -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import live_cases as LC
from oracle import masklab as O
from oracle import tfops as T

CANARY = -9.5                                   # exact in half and float
HALF_RTOL, HALF_ATOL = 2.0 ** -10, 1e-4         # tests/test_gpu_f16_heads.py
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from masklab_hip import _lib, ops
    _lib.check(_lib.load().ml_device_check(), "ml_device_check")
    ops.set_conv_math("f32")
    yield
    ops.set_conv_math("f32")


@pytest.fixture
def conv_math():
    from masklab_hip import ops

    def use(mode):
        ops.set_conv_math(mode)
    yield use
    ops.set_conv_math("f32")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def h64(a):
    return a.astype(np.float16).astype(np.float64)


def randn(seed, *shape, half=False):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
    return x.half() if half else x


def np_randn(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).normal(size=shape) * scale).astype(np.float32)


def live_int(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def slots_t(period, live, periods):
    return torch.from_numpy(LC.live_slots(period, live, periods)).cuda()


def poisoned(x, alive, fill=NAN):
    """A copy of x [slots, ...] whose dead slots hold `fill`."""
    xp = x.clone()
    xp[~alive] = fill
    return xp


def close_half(got, ref64, atol=HALF_ATOL):
    np.testing.assert_allclose(got.astype(np.float32), ref64.astype(np.float16).astype(np.float32), rtol=HALF_RTOL, atol=atol)


def close(got, ref64, atol, rtol=0):
    """The tolerance of the `live`-less test of the kernel: half results against the oracle rounded once to half."""
    if got.dtype == np.float16:
        close_half(got, ref64, atol=atol)
    else:
        np.testing.assert_allclose(got, ref64, rtol=rtol, atol=atol)


def holds_canary(t):
    return bool((t == CANARY).all())


# ------------------------------------------------------------------ the generic implicit-GEMM conv (csrc/conv_mfma.hip)
def _launch_convs(problems):
    """ops.conv2d_multi(problems) -> what the library reports for this launch: kernel name, N tile, M tile, K slices."""
    from masklab_hip import _lib, ops
    lib = _lib.load()
    ops.PROFILE, ops.LAUNCH_LOG = [], []
    try:
        ops.conv2d_multi(problems)
        torch.cuda.synchronize()
        names, log = [r["kernel"] for r in ops.PROFILE], ops.LAUNCH_LOG
    finally:
        ops.PROFILE = ops.LAUNCH_LOG = None
    assert len(names) == 1 and len(log) == 1 and names[0].startswith("conv_mfma_"), names
    n = len(problems)
    arr = (_lib.ConvDesc * n)()
    for i, pr in enumerate(problems):
        pr = dict(pr)
        arr[i] = ops._conv_desc(pr.pop("x"), pr.pop("dc"), **pr)[0]
    plan = dict(kernel=names[0], ntile=lib.ml_conv2d_launch_ntile(arr, n, 1), mtile=lib.ml_conv2d_launch_mtile(arr, n, 1),
                splits=tuple(log[0][1]))
    assert names[0].startswith("conv_mfma_%dx%d" % (plan["mtile"], plan["ntile"])), plan
    return plan


class ConvCase:
    """A 3x3 (or 1x1) conv of `periods` images x `period` slots of one crop size, its clean launch and its oracle."""

    def __init__(self, crop, period, periods, k=3, cout=128, tile=1, half=False, out_dtype=None, seed=7):
        from masklab_hip import ops, packing
        self.crop, self.period, self.periods, self.B, self.cout, self.half = crop, period, periods, period * periods, cout, half
        self.hw = crop[0] * crop[1]
        self.x = randn(seed, self.B, crop[0], crop[1], 128, half=half)
        self.w = np_randn(seed + 1, k, k, 128, cout, scale=1.0 / np.sqrt(k * k * 128))
        self.b = np_randn(seed + 2, cout)
        self.dc = ops.DeviceConv(packing.pack_dense(self.w, self.b, tile=tile), "cuda")
        self.odt = out_dtype or (torch.float16 if half else torch.float32)
        self._ref = {}

    def new_out(self):
        return torch.full((self.B, self.crop[0], self.crop[1], self.cout), CANARY, dtype=self.odt, device="cuda")

    def ref(self, i):
        """fp64 oracle of image i (on the half-rounded operands for half tensors, as tests/test_gpu_f16_heads.py)."""
        if i not in self._ref:
            xi = host(self.x[i:i + 1]).astype(np.float64)
            w = h64(self.w) if self.half else self.w
            self._ref[i] = T.relu(T.conv2d(xi, w, self.b.astype(np.float64)))[0]
        return self._ref[i]

    def launch(self, live=None, x=None):
        from masklab_hip import _lib
        out = self.new_out()
        pr = dict(x=self.x if x is None else x, dc=self.dc, act=_lib.ACT_RELU, out=out)
        if live is not None:
            pr["live"] = (live_int(live), self.period)
        return out, _launch_convs([pr])

    @functools.cached_property
    def plain(self):
        return self.launch()


def check_conv(case, live, atol, BM=LC.BM, sample=None, label="", rtol=0):
    """One `live` launch of `case` on poisoned input -> its plan.  sample: the live images held to fp64 (None: all)."""
    plain, plain_plan = case.plain
    alive = slots_t(case.period, live, case.periods)
    out, plan = case.launch(live, poisoned(case.x, alive))
    same_k = plan["splits"] == plain_plan["splits"]
    print(f"[live] {label} {case.crop} x{case.period} B={case.B} live={live}: {plan['kernel']} N tile {plan['ntile']} "
          f"M tile {plan['mtile']} K slices {plan['splits']} (without live: {plain_plan['kernel']} {plain_plan['splits']})"
          f"{' bit-exact branch' if same_k else ''}")
    assert plan["mtile"] == BM, plan
    live_idx = [i for i in range(case.B) if bool(alive[i])]
    got = host(out)
    for i in (live_idx if sample is None else sample):
        assert bool(alive[i])
        close(got[i], case.ref(i), atol, rtol)
    if same_k:                                  # the same k-ordered chains whatever the tile shape: the same bits
        assert torch.equal(out[alive], plain[alive])
    keep = torch.from_numpy(LC.keep_rows(case.hw, case.period, live, case.periods, BM)).cuda()
    assert holds_canary(out.view(case.B * case.hw, case.cout)[keep])
    if plan["splits"][0] > 1:                   # cut along K: splitk_reduce_kernel stores no row of a dead image at all
        assert holds_canary(out[~alive])
    if live >= case.period:                     # every slot live: the launch without `live`, everywhere
        assert bool(alive.all())
        if same_k:
            assert torch.equal(out, plain)
        else:                                   # K cut differently: both are held to the oracle, image by image
            for i in range(case.B):
                close(got[i], case.ref(i), atol, rtol)
    return plan, same_k


@functools.lru_cache(maxsize=None)
def _small_case(math, crop, period, half=False, out32=False, k=3):
    """(one per conv math: a case keeps the launch without `live` it was first asked for)"""
    return ConvCase(crop, period, LC.PERIODS, k=k, half=half, out_dtype=torch.float32 if out32 else None)


@pytest.mark.parametrize("crop,period", LC.SHAPES)
@pytest.mark.parametrize("math", ["f32", "f32x3"])
def test_conv3x3_narrowed_small_launch(math, crop, period, conv_math):
    """3x3 128 -> 128 packed for the direct kernel, three images: a `live` launch this small runs on 128 x 32 (or 128 x 64)
    tiles with the whole K sum per tile, while the launch without `live` is cut along K -- so the oracle is the bar here,
    and where both report the same slices the bits are."""
    conv_math(math)
    case = _small_case(math, crop, period)
    for live in LC.live_sweep(period):
        plan, _ = check_conv(case, live, atol=2e-5, label=math)
        assert plan["ntile"] in (32, 64), plan
        assert plan["kernel"].endswith("_x3") == (math == "f32x3")
    out0, _ = case.launch(0, poisoned(case.x, slots_t(period, 0, LC.PERIODS)))
    out1, _ = case.launch(1, poisoned(case.x, slots_t(period, 1, LC.PERIODS)))
    a1 = slots_t(period, 1, LC.PERIODS)
    assert torch.equal(out0[a1], out1[a1])      # *live = 0 is *live = 1


@pytest.mark.parametrize("crop,period", LC.SHAPES)
def test_conv1x1_pointwise(crop, period, conv_math):
    """The pointwise conv of MobileSeparableConv2D, 1x1 128 -> 128: four K chunks, never cut, so `live` changes no bit."""
    conv_math("f32")
    case = _small_case("f32", crop, period, k=1)
    for live in LC.live_sweep(period):
        plan, same_k = check_conv(case, live, atol=2e-5, label="f32 1x1")
        assert same_k and plan["ntile"] in (32, 64), plan


@pytest.mark.parametrize("math", ["f32", "f32x3", "f16s"])
def test_conv3x3_on_128x64_tiles_equals_the_launch_without_live(math, conv_math):
    """128 images of 14 x 14 = 196 tiles: neither launch is cut along K and both run on 128 x 64 tiles, so every live image
    has the bits of the launch without `live` -- the bit-exact branch of each math."""
    conv_math(math)
    half = math == "f16s"
    case = ConvCase((14, 14), 4, 32, half=half)
    sample = {1: [0, 4, 60, 124], 2: [0, 1, 65, 125], 4: [3, 127]}
    for live in (1, 2, 4):
        plan, same_k = check_conv(case, live, atol=HALF_ATOL if half else 2e-5, sample=sample[live], label=math)
        assert same_k and plan["ntile"] == 64, plan


def test_conv3x3_large_enough_for_128x128_tiles(conv_math):
    """A `live` launch of more than 1.5 tiles per compute unit keeps the 128 x 128 tile (narrow_tile_for_small_launch)."""
    conv_math("f32")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 3 * cus // 2 + 1
    periods = -(-tiles * 128 // (4 * 196))
    case = ConvCase((14, 14), 4, periods)
    B = case.B
    for live, sample in ((1, [0, 4, B - 4]), (2, [1, B // 2 // 4 * 4, B - 3]), (3, [2, B - 2])):
        plan, same_k = check_conv(case, live, atol=2e-5, sample=sample, label="f32 large")
        assert same_k and plan["ntile"] == 128 and plan["kernel"] == "conv_mfma_128x128", plan


@pytest.mark.parametrize("live", [1, 2])
def test_conv3x3_split_operand_256_row_tile(live, conv_math):
    """ML_MATH_F32X3 at capacity: x3_uses_256_row_tiles does not look at `live`, and the smallest batch of 14 x 14 crops that
    gives one 256-row tile per compute unit reaches that tile.  The skip predicate then works on 256-row tiles: every live
    image bit for bit the launch without `live`, six sampled ones against fp64, wholly dead 256-row tiles untouched."""
    conv_math("f32x3")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    periods = -(-((cus - 1) * 256 + 1) // (4 * 196))
    case = ConvCase((14, 14), 4, periods)
    B = case.B
    assert -(-B * 196 // 256) >= cus and B * 196 * 128 * 4 < 40 << 20
    for cls in ({1: (LC.DEAD, LC.DEAD_LIVE_DEAD, LC.LIVE_TO_DEAD), 2: (LC.DEAD_TO_LIVE, LC.LIVE)}[live]):
        assert cls in LC.tile_classes(196, 4, live, periods, 256)
    first = [i for i in range(B) if i % 4 < live]
    sample = [first[j] for j in (0, 1, len(first) // 3, len(first) // 2, len(first) - 2, len(first) - 1)]
    plan, same_k = check_conv(case, live, atol=2e-5, BM=256, sample=sample, label="f32x3 256-row")
    assert same_k and plan["mtile"] == 256 and plan["kernel"] == "conv_mfma_256x128_x3", plan


@pytest.mark.parametrize("crop,period,out32", [((14, 14), 4, False), ((7, 7), 4, True), ((7, 7), 3, False)])
def test_conv3x3_half_tensors(crop, period, out32, conv_math):
    """ML_MATH_F16S: half input with NaN in the dead slots, half or fp32 destination."""
    conv_math("f16s")
    case = _small_case("f16s", crop, period, half=True, out32=out32)
    for live in LC.live_sweep(period):
        plan, _ = check_conv(case, live, atol=2e-5 if out32 else HALF_ATOL, rtol=1e-5 if out32 else 0,
                             label="f16s fp32 out" if out32 else "f16s")
        assert plan["kernel"].endswith("_h") and plan["ntile"] in (32, 64), plan


@pytest.mark.parametrize("cout", [64, 32])
@pytest.mark.parametrize("math", ["f32", "f32x3", "f16s"])
def test_conv3x3_split_k_with_live(math, cout, conv_math):
    """Weights packed for a 64- / 32-wide N tile keep their K slices under `live`: seven tiles of 7 x 7 crops (four images
    of four slots) are cut along K, the slabs of skipped tiles hold stale workspace bytes, and splitk_reduce_kernel decides
    row by row what exists.  The same slices with and without `live`: the same bits."""
    conv_math(math)
    half = math == "f16s"
    case = ConvCase((7, 7), 4, 4, cout=cout, tile=0, half=half)
    for live in LC.live_sweep(4):
        plan, same_k = check_conv(case, live, atol=HALF_ATOL if half else 3e-5, label=f"{math} cout {cout} split-K")
        assert same_k and plan["splits"][0] > 1 and plan["ntile"] == 32, plan


def test_conv3x3_levels_in_one_launch(conv_math):
    """RoI levels in one launch: one problem per shape, their own `live` ints and periods, one of them without `live`."""
    from masklab_hip import _lib
    conv_math("f32")
    cases = [_small_case("f32", crop, period) for crop, period in LC.SHAPES]
    for lives in ((1, 2, None, 1), (None, 0, 3, 2), (2, None, 1, 0), (3, 5, 7, None)):
        outs = [c.new_out() for c in cases]
        problems = []
        for c, lv, out in zip(cases, lives, outs):
            alive = slots_t(c.period, c.period if lv is None else lv, c.periods)
            pr = dict(x=poisoned(c.x, alive), dc=c.dc, act=_lib.ACT_RELU, out=out)
            if lv is not None:
                pr["live"] = (live_int(lv), c.period)
            problems.append(pr)
        plan = _launch_convs(problems)
        print(f"[live] f32 {len(cases)} levels live={lives}: {plan}")
        for c, lv, out in zip(cases, lives, outs):
            eff = c.period if lv is None else lv
            alive = LC.live_slots(c.period, eff, c.periods)
            got = host(out)
            for i in np.flatnonzero(alive):
                close(got[i], c.ref(int(i)), 2e-5)
            keep = torch.from_numpy(LC.keep_rows(c.hw, c.period, eff, c.periods, plan["mtile"])).cuda()
            assert holds_canary(out.view(c.B * c.hw, c.cout)[keep])


# ------------------------------------------------------------------ GroupNormalization (csrc/groupnorm.hip, gn_dead)
GN_C, GN_G, GN_PERIOD = 128, 16, 4
GN_N = LC.PERIODS * GN_PERIOD
GN_SIZES = (7, 14, 20, 28)           # floats per chunk 392 / 1568 / 3200 / 6272: one-pass at 1, 2, 4 vectors per thread, two-pass
# (h, w, C, G), chunks of 120 / 60, one slice.  C = 12: scalar accesses as halves (C % 8 != 0), a one-pass vector problem as
# floats; C = 6: scalar accesses either way
GN_SCALAR, GN_SCALAR_F32 = (6, 5, 12, 3), (6, 5, 6, 3)


def _gn_dims(size):
    """a case of the sweep -> (h, w, C, G)"""
    return (size, size, GN_C, GN_G) if isinstance(size, int) else size


@functools.lru_cache(maxsize=None)
def _gn_case(size, half):
    h, w, C, G = _gn_dims(size)
    x = randn(100 + h + C % 8, GN_N, h, w, C) * 3 + 1.5
    if half:
        x = x.half()
    r = np.random.default_rng(200 + h)
    gamma, beta = r.uniform(0.5, 1.5, C).astype(np.float32), r.normal(size=C).astype(np.float32)
    ref = T.group_norm(host(x).astype(np.float64), gamma, beta, G)
    return x, dev(gamma), dev(beta), ref


def _gn_problem(size, half, relu, inplace, live):
    """-> (problem dict, alive slots, the tensor the result lands in).  Out of place: NaN in the dead samples of x, the
    canary in `out`; in place the dead samples of x hold the canary -- normalising one would change it."""
    x, gamma, beta, _ = _gn_case(size, half)
    alive = slots_t(GN_PERIOD, GN_PERIOD if live is None else live, LC.PERIODS)
    if inplace:
        xin = poisoned(x, alive, CANARY)
        out = xin
    else:
        xin = poisoned(x, alive)
        out = torch.full_like(x, CANARY)
    pr = dict(x=xin, gamma=gamma, beta=beta, groups=_gn_dims(size)[3], relu=relu, out=out)
    if live is not None:
        pr["live"] = (live_int(live), GN_PERIOD)
    return pr, alive, out


def _gn_check(size, half, relu, out, alive, plain):
    ref = _gn_case(size, half)[3]
    got = host(out)
    a = host(alive)
    close(got[a], (T.relu(ref) if relu else ref)[a], 2e-4 if half else 2e-5)
    assert torch.equal(out[alive], plain[alive])          # the launch without `live`, bit for bit
    assert holds_canary(out[~alive])                      # dead samples: nothing written, whole samples


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("size", GN_SIZES + (GN_SCALAR, GN_SCALAR_F32), ids=[str(s) for s in GN_SIZES] + ["scalar", "scalar_f32"])
def test_groupnorm_live(size, half):
    from masklab_hip import ops
    x, gamma, beta, _ = _gn_case(size, half)
    for relu in (False, True):
        (plain,) = ops.groupnorm_chunk_multi([dict(x=x, gamma=gamma, beta=beta, groups=_gn_dims(size)[3], relu=relu)])
        for inplace in (False, True):
            for live in LC.live_sweep(GN_PERIOD):
                pr, alive, out = _gn_problem(size, half, relu, inplace, live)
                ops.groupnorm_chunk_multi([pr])
                _gn_check(size, half, relu, out, alive, plain)
                if live >= GN_PERIOD:
                    assert torch.equal(out, plain)


@pytest.mark.parametrize("half", [False, True])
def test_groupnorm_four_sizes_in_one_launch(half):
    """One launch pair (statistics of the two-pass problems, then every apply) of the four vector forms and a scalar problem,
    each with its own `live` int, one or two without."""
    from masklab_hip import ops
    sizes = GN_SIZES + (GN_SCALAR_F32,)
    for lives in ((1, 2, 3, None, 2), (None, 0, 1, 2, None), (3, None, 6, 1, 0)):
        for inplace in (False, True):
            prs = [_gn_problem(s, half, True, inplace, lv) for s, lv in zip(sizes, lives)]
            ops.groupnorm_chunk_multi([p[0] for p in prs])
            for s, (pr, alive, out) in zip(sizes, prs):
                x, gamma, beta, _ = _gn_case(s, half)
                (plain,) = ops.groupnorm_chunk_multi([dict(x=x, gamma=gamma, beta=beta, groups=_gn_dims(s)[3], relu=True)])
                _gn_check(s, half, True, out, alive, plain)


# ------------------------------------------------------------------ RoI crop (csrc/detect.hip)
@functools.lru_cache(maxsize=None)
def _roi_fixture():
    """The geometry of tests/test_gpu_detect.py::test_mask_distribute_and_roi_crop: 3 images of 7 / 0 / 12 RoIs."""
    B, H, W, cap = 3, 256, 256, 12
    rng = np.random.default_rng(5)
    prop = np.full((B, cap, 6), -1.0, np.float32)
    for b, n in enumerate([7, 0, 12]):
        cx, cy = rng.uniform(20, 236, n), rng.uniform(20, 236, n)
        w, h = rng.uniform(10, 300, n), rng.uniform(10, 300, n)
        prop[b, :n] = np.stack([cx, cy, w, h, rng.integers(0, 5, n), rng.uniform(0.5, 1, n)], 1)
    fmaps = [rng.normal(size=(B, H // s, W // s, 128)).astype(np.float32) for s in (8, 16, 32)]
    return B, H, W, cap, prop, fmaps


@pytest.mark.parametrize("half", [False, True])
def test_roi_crop_at_capacity(half):
    """ml_roi_crop_resize launched at capacity (n_l = cap): slots below max(1, live) are the oracle's crops, -1 from the
    image's own count on (slot 0 of the image without a RoI included); the slots from there on keep the canary in
    roi_fmaps AND roi_boxes.  `live` = the level maximum ops.mask_distribute wrote on the device, then the sweep."""
    from masklab_hip import ops
    B, H, W, cap, prop, fmaps = _roi_fixture()
    if half:
        fmaps = [f.astype(np.float16) for f in fmaps]
    L = len(fmaps)
    rf_ref, rb_ref = O.pyramid_roi_align([f.astype(np.float64) for f in fmaps], O.mask_distribute(prop, L - 1, 36), (H, W), (14, 14))
    rows = dev(prop)
    slots, lcounts, lmax, _ = ops.mask_distribute(rows, L - 1, 36.0)
    n_ref = [r.shape[1] for r in rf_ref]
    assert [max(1, int(v)) for v in host(lmax)] == n_ref and max(n_ref) < cap
    off = 0
    for level in range(L):
        n = n_ref[level]
        want = np.full((B, cap) + rf_ref[level].shape[2:], -1.0)          # the oracle's level, padded to capacity
        want[:, :n] = rf_ref[level]
        want_b = np.full((B, cap, 6), -1.0, np.float32)
        want_b[:, :n] = rb_ref[:, off:off + n]
        off += n
        fm = dev(fmaps[level])
        for live in [lmax[level:level + 1]] + [live_int(v) for v in LC.live_sweep(cap)]:
            lim = min(cap, max(1, int(host(live)[0])))
            out = torch.full((B, cap, 14, 14, 128), CANARY, dtype=fm.dtype, device="cuda")
            boxes = torch.full((B, L * cap, 6), CANARY, dtype=torch.float32, device="cuda")
            ret = ops.roi_crop_resize(fm, rows, slots, lcounts, level, cap, (14, 14), (H, W), boxes, level * cap, live=live, out=out)
            assert ret is out
            got, got_b = host(out), host(boxes)
            # MoldBatch padding pattern, slot by slot (a half crop value may round to -1 by itself)
            np.testing.assert_array_equal((got[:, :lim] == -1.0).all(axis=(2, 3, 4)), (want[:, :lim] == -1.0).all(axis=(2, 3, 4)))
            close(got[:, :lim], want[:, :lim], HALF_ATOL if half else 2e-5)
            if not half:
                np.testing.assert_array_equal(got[:, :lim] == -1.0, want[:, :lim] == -1.0)
                np.testing.assert_array_equal(got[:, :lim] == 0.0, want[:, :lim] == 0.0)       # extrapolation cells
            np.testing.assert_array_equal(got_b[:, level * cap:level * cap + lim], want_b[:, :lim])
            assert (got[:, lim:] == CANARY).all()
            got_b[:, level * cap:level * cap + lim] = CANARY
            assert (got_b == CANARY).all()                                                    # the other levels' rows too


def test_roi_crop_out_argument_is_checked():
    from masklab_hip import ops
    B, H, W, cap, prop, fmaps = _roi_fixture()
    rows = dev(prop)
    slots, lcounts, lmax, _ = ops.mask_distribute(rows, 2, 36.0)
    boxes = torch.zeros((B, 3 * cap, 6), device="cuda")
    for bad in (torch.zeros((B, cap, 14, 14, 64), device="cuda"), torch.zeros((B, cap, 14, 14, 128), dtype=torch.float16, device="cuda")):
        with pytest.raises(ValueError, match="out"):
            ops.roi_crop_resize(dev(fmaps[0]), rows, slots, lcounts, 0, cap, (14, 14), (H, W), boxes, 0, live=lmax[:1], out=bad)


# ------------------------------------------------------------------ the fused mask-head tail (csrc/deconv_out.hip, locate())
TAIL_K = TAIL_CMID = 128
TAIL_NCLS = 3


class TailLevel:
    def __init__(self, crop, cap, B, seed, half, x=None):
        from masklab_hip import ops, packing
        self.crop, self.cap, self.B, self.half = crop, cap, B, half
        self.hw = crop[0] * crop[1]
        self.x = randn(seed, B * cap, crop[0], crop[1], TAIL_K, half=half) if x is None else x
        self.wd, self.bd = np_randn(seed + 1, 2, 2, TAIL_CMID, TAIL_K, scale=0.05), np_randn(seed + 2, TAIL_CMID)
        self.wo, self.bo = np_randn(seed + 3, 1, 1, TAIL_CMID, TAIL_NCLS, scale=0.1), np_randn(seed + 4, TAIL_NCLS)
        table, bo_p, _ = packing.pack_out1x1_table(self.wo, self.bo)
        self.dc = ops.DeviceConv(packing.pack_transpose2x2(self.wd, self.bd), "cuda")
        self.table, self.bo_p = dev(table), dev(bo_p)
        self.per_roi = 4 * self.hw * TAIL_NCLS
        self._ref = {}

    def ref(self, r):
        """fp64 oracle of RoI r: [2h, 2w, ncls]."""
        if r not in self._ref:
            x = host(self.x[r:r + 1]).astype(np.float64)
            t = T.relu(T.conv2d_transpose_2x2_s2(x, h64(self.wd) if self.half else self.wd, self.bd))
            self._ref[r] = T.sigmoid(T.conv2d(t, self.wo, self.bo))[0]
        return self._ref[r]

    def view(self, out, base):
        """This level's RoIs inside the image-major output: [B, cap, 2h, 2w, ncls]."""
        return out[:, base:base + self.cap * self.per_roi].reshape(self.B, self.cap, 2 * self.crop[0], 2 * self.crop[1], TAIL_NCLS)

    def keep(self, live):
        """bool [B, cap, 2h, 2w]: output pixels of input rows in wholly dead 128-row tiles."""
        k = LC.keep_rows(self.hw, self.cap, live, self.B, LC.BM).reshape(self.B, self.cap, self.crop[0], self.crop[1])
        return torch.from_numpy(np.repeat(np.repeat(k, 2, axis=2), 2, axis=3)).cuda()


def _tail_launch(levels, lives, xs=None):
    from masklab_hip import _lib, ops
    B = levels[0].B
    total = sum(lv.cap * lv.per_roi for lv in levels)
    out = torch.full((B, total), CANARY, device="cuda")
    problems, base, bases = [], 0, []
    for i, (lv, live) in enumerate(zip(levels, lives)):
        problems.append(dict(x=lv.x if xs is None else xs[i], dc=lv.dc, wo_table=lv.table, bo=lv.bo_p, out=out, out_base=base,
                             rois_per_image=lv.cap, live=None if live is None else live_int(live)))
        bases.append(base)
        base += lv.cap * lv.per_roi
    ops.deconv2x2_out1x1_multi(problems, TAIL_NCLS, _lib.ACT_RELU, _lib.ACT_SIGMOID)
    torch.cuda.synchronize()
    return out, bases


def _tail_check(levels, lives, plain, sample=None):
    xs = [poisoned(lv.x, slots_t(lv.cap, lv.cap if live is None else live, lv.B)) for lv, live in zip(levels, lives)]
    out, bases = _tail_launch(levels, lives, xs)
    for lv, live, base in zip(levels, lives, bases):
        eff = lv.cap if live is None else live
        alive = slots_t(lv.cap, eff, lv.B).view(lv.B, lv.cap)
        v, pv = lv.view(out, base), lv.view(plain, base)
        assert torch.equal(v[alive], pv[alive])                   # live RoIs: the launch without `live`, bit for bit
        got = host(v).reshape((lv.B * lv.cap,) + tuple(v.shape[2:]))
        rois = np.flatnonzero(host(alive).reshape(-1)) if sample is None else sample
        for r in rois:
            assert bool(alive.view(-1)[int(r)])
            np.testing.assert_allclose(got[int(r)], lv.ref(int(r)), rtol=0, atol=2e-5)
        keep = lv.keep(eff)
        assert holds_canary(v[keep])
        if eff >= lv.cap:
            assert torch.equal(v, pv)


TAIL_SHAPES = LC.SHAPES                # (crop, capacity): 7 x 7 at 4, 6 x 10 at 5, 14 x 14 at 4, 7 x 7 at 3


@pytest.mark.parametrize("half", [False, True])
def test_tail_levels_in_one_launch(half):
    """K = C_mid = 128, 3 classes, 3 images; 7 x 7 at capacity 4, 6 x 10 at 5, 14 x 14 at 4 and 7 x 7 at 3 in one launch,
    each level with its own `live`, one of them without: every value of the sweep reaches every level."""
    n = len(TAIL_SHAPES)
    levels = [TailLevel(crop, cap, LC.PERIODS, 300 + 10 * i, half) for i, (crop, cap) in enumerate(TAIL_SHAPES)]
    plain, _ = _tail_launch(levels, (None,) * n)
    sweeps = [LC.live_sweep(cap) for _, cap in TAIL_SHAPES]
    seen = [set() for _ in range(n)]
    for i in range(6):
        for none_at in (i % n, (i + 1) % n):
            lives = [None if j == none_at else sweeps[j][i] for j in range(n)]
            for j, v in enumerate(lives):
                seen[j].add(v)
            _tail_check(levels, lives, plain)
    assert all(set(sweeps[j]) | {None} == seen[j] for j in range(n))


@pytest.mark.parametrize("half", [False, True])
def test_tail_several_units_per_persistent_block(half):
    """8 images x capacity 100 at 14 x 14, 37 live: 1 225 tiles x 4 positions on a grid of resident blocks, so locate()
    walks past skipped units inside a block's own sequence.  Every live RoI bit for bit, eight sampled ones against fp64."""
    lv = TailLevel((14, 14), 100, 8, 400, half)
    plain, _ = _tail_launch([lv], (None,))
    _tail_check([lv], (37,), plain, sample=[0, 36, 100, 136, 250 // 100 * 100 + 18, 436, 700, 736])


# ------------------------------------------------------------------ what the library refuses (nothing is launched)
def _refused(fn, word):
    with pytest.raises(RuntimeError, match=word):
        fn()


def test_refusals(conv_math):
    from masklab_hip import _lib, ops, packing
    conv_math("f32")
    lib = _lib.load()
    dc = ops.DeviceConv(packing.pack_dense(np_randn(1, 3, 3, 128, 128, scale=0.03), np_randn(2, 128), tile=1), "cuda")
    lv = live_int(2)

    def conv(B, hw, period, **kw):
        x = torch.zeros((B, hw, hw, 128), device="cuda")
        return lambda: ops.conv2d_multi([dict(x=x, dc=dc, act=_lib.ACT_RELU, live=(lv, period), **kw)])

    _refused(conv(10, 14, 4), "live_period")                      # the period does not divide B
    _refused(conv(12, 5, 4), "128-row tile")                      # 100 rows per period
    # gn_partials: a launch big enough to be taken without `live` (whole 128-row tiles, 128 x 128 kernel, K uncut) ...
    B = 4 * (-(-int(lib.ml_conv2d_gn_min_launch_tiles()) * 2 * 128 // (4 * 196)))
    while (B * 196) % 128:
        B += 4
    x = torch.zeros((B, 14, 14, 128), device="cuda")
    part = torch.zeros((B * 196 // 128, 4, 2), dtype=torch.float64, device="cuda")
    d = ops._conv_desc(x, dc, act=_lib.ACT_RELU, gn_partials=part)[0]
    sp = (C.c_int32 * 1)()
    assert lib.ml_conv2d_launch_splits(C.byref(d), 1, int(lib.ml_conv2d_workspace_bytes()), sp) == 0 and sp[0] == 1
    # ... and refused with it
    _refused(lambda: ops.conv2d_multi([dict(x=x, dc=dc, act=_lib.ACT_RELU, gn_partials=part, live=(lv, 4))]), "gn_partials")
    xg = torch.zeros((10, 7, 7, 128), device="cuda")
    g = torch.ones(128, device="cuda")
    _refused(lambda: ops.groupnorm_chunk_multi([dict(x=xg, gamma=g, beta=g, groups=16, live=(lv, 4))]), "live_period must divide N")
    t = TailLevel((7, 7), 2, 3, 500, False, x=torch.zeros((6, 7, 7, TAIL_K), device="cuda"))
    _refused(lambda: _tail_launch([t], (1,)), "at least one tile per image")


# ------------------------------------------------------------------ the whole forward on poisoned allocations
def test_forward_does_not_depend_on_what_empty_memory_holds():
    """Fixed-capacity stage 2, eager: the forward again on stale memory (tests/dirty_memory.py: every workspace and every
    torch.empty / empty_like result of any dtype filled with 0xFF bytes -- NaN as a float, -1 as an integer) returns the same
    bits -- no output depends on a slot nobody wrote, which is what the caching allocator hands out in service."""
    import dirty_memory as DM
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "mobilenet"
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(5)
    for k in w:             # scores near 0.5 for a fraction of the anchors (tests/test_gpu_model.py: hot_cls)
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)
    model.load_weights(w, "cuda:0")
    model.device_counts = True
    images = np.random.default_rng(256).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    first = model.predict(images)
    boxes = first[model.output_names.index("roi_boxes")]
    n_det = int((boxes[..., 4] >= 0).sum())
    assert model._capacity_wanted(torch.from_numpy(images))
    slots = (cfg.instance.max_k + 1) * cfg.detection.nms_max_output_size
    assert n_det > 0 and boxes.shape[1] < slots, "the fixture needs detections and dead slots"

    with DM.poisoned():
        second = model.predict(images)
    for name, a, b in zip(model.output_names, first, second):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert not np.isnan(b).any(), name
        np.testing.assert_array_equal(a, b, err_msg=name)
