"""The case table of the generic implicit-GEMM conv kernel (csrc/conv_mfma.hip): one case per instantiation of
`kGenericKernels`, each a single LAUNCH that the library plans onto exactly that instantiation.  Importable without a GPU:
tests/test_conv_cases_cpu.py asks the library's host-only planning entries that every case lands where it says, and that
the table names every instantiation; tests/test_gpu_conv_instantiations.py runs the launches.

Which instantiation runs is decided on the whole launch (plan_launch: tile class, narrowing of small launches, the 256-row
f32x3 tile, split-K).  A case therefore carries its small problems under test TOGETHER WITH A FILLER: one large, cheap 1x1
problem of the same math and tile class that makes the launch big enough for the wide kernel and keeps every K sum in one
slice.  Every problem is packed with an explicit tile (1, 2 or 3), never 0: the Winograd and persistent 1x1 kernels only
take tile 0 (and 4 / 5 / 6), so a case cannot drift onto another family when a dispatch rule moves.

A set of problems reaches these arms of the epilogue (the smallest shape with the property):
  ragged           2x13x11 = 286 rows: two full 128-row tiles (fast full-tile arm) and a 30-row tail (partial-tile arm), an
                   image boundary inside tile 1; ReLU6; a channel slice of a wider buffer; half output under "f16"
  two_n_kpad_res   cin 136 (span_pad 160: K padding), two N tiles, 1x1; ReLU + residual read at res_coff 4 of a wider
                   buffer: `pre_res` on the full tiles and the tail, `late_res` in f32x3
  stride2_view     3x3 stride 2, explicit one-sided padding, linear, `out_view` with a batch stride (out_bstride arm)
  dil3_res         dilation 3, ReLU6 + residual; 144 rows
  k1s2_unaligned   1x1 stride 2 into a dword-aligned, not 16-byte-aligned view: the scalar stores of the generic arm
  k5               5x5 'same'
  sigmoid          the generic (un-unrolled) arm, vector stores
  cout75, cout130  cout % 4 != 0: the generic arm, scalar stores, a dead quad / a second N tile with two live channels
  shuffle2x2       Conv2DTranspose(2, 2, stride 2) packed by pack_transpose2x2: the pixel-shuffle store
  long_k           2x6x6x256, 3x3: 72 chunks; the filler holds it to ONE K slice, launched alone it is cut in 9 (slab arm).
                   (Not longer: ONE fp32 chain of 18 432 terms -- 2x6x6x2048 under the filler -- measured 2.9e-5 from fp64, the
                   rounding of the format, sqrt(K) 2^-24 |sum|, past the 2e-5 bar that the suite sets for K of a few thousand.)
  stem             (64-wide tile class) the row-span 7x7 stride-2 stem on the NHWC4 image (cpp_shift 2), half output under "f16"
  gn               2x16x16x64 -> 128: whole 128- and 256-row tiles, `gn_partials`
  split_k_wide     4x64x64x128 -> 128, 3x3, launched ALONE: 128 tiles x 4 K slices = 512 blocks, stays 128 wide (slab arm)

Left out, because validate() / plan_launch refuse them (no skip, no xfail):
  * a residual under "f16s": "the fp16-storage form of the generic kernel takes no residual" -- those problems run without;
  * the row-span stem under "f16s": "fp16 storage takes no image (row-span) input";
  * a half output with a residual, shuffle, batch stride, sigmoid or cout % 4: "out_f16 needs ... the dense fast epilogue";
  * gn_partials off the 128-wide tile, under "f16", or on a launch below ml_conv2d_gn_min_launch_tiles().

Activation data: weights are scaled 1 / sqrt(K) and inputs are N(0, 1), so a pre-activation value is about N(0, 2) and would
reach ReLU6's upper clamp once in 1e5.  ReLU6 problems spread their bias evenly over [-1.5, 7.5] (a sixth of the channels
sits above 6, a sixth below 0, none beyond 8, so the sums stay in the binade the tolerance was set for): about a tenth of the
fp64 reference lies above 6 and a tenth below 0 (asserted: at least 5 % each, tests/test_conv_cases_cpu.py)."""
import functools
import zlib
from dataclasses import dataclass, replace

import numpy as np

from masklab_hip import _lib
from oracle import tfops as T

MATH_CODE = {"f32": _lib.MATH_F32, "f16": _lib.MATH_F16, "f16s": _lib.MATH_F16S, "f32x3": _lib.MATH_F32X3}
SUFFIX = {"f32": "", "f16": "_f16", "f16s": "_h", "f32x3": "_x3"}  # of the profile name conv_mfma_<BM>x<BN><suffix>
ACT = {None: lambda v: v, "relu": T.relu, "relu6": T.relu6, "sigmoid": T.sigmoid}
STEM_PAD = ((3, 3), (3, 3))


@dataclass(frozen=True)
class Prob:
    name: str
    shape: tuple                    # input [B, H, W, cin] (the stem: the 3-channel image; it is fed as NHWC4)
    cout: int
    k: int = 3
    stride: int = 1
    padding: object = "same"
    dil: int = 1
    act: object = "relu"
    res: object = None              # None | "dense" | "slice": read at res_coff 4 of a buffer 8 channels wider
    dest: str = "dense"             # "dense" | "slice" (channels [4, 4 + cout) of a wider buffer) | "packed" (cstride = cout)
    #                                 | "view" (out_view, batch stride with a gap) | "unaligned" (out_view 3 floats in)
    kind: str = "dense"             # "dense" | "shuffle" (Conv2DTranspose 2x2 stride 2) | "stem" (row-span 7x7 stride 2)
    gn: bool = False                # asks for gn_partials
    half_out: bool = False          # under "f16": fp32 in, half out
    alone: object = 1               # K slices when the problem is launched alone: an int, or ((math, int), ...); 0 = never alone

    def alone_splits(self, math):
        return dict(self.alone)[math] if isinstance(self.alone, tuple) else self.alone


@dataclass(frozen=True)
class Case:
    name: str
    math: str                       # "f32" | "f16" | "f16s" | "f32x3"
    bm: int                         # the instantiation it is for: tile rows, tile columns, the gn_partials form
    bn: int
    gns: bool
    tile: int                       # what every problem is packed for: 1 (128 wide), 2 (64), 3 (32)
    probs: tuple
    filler: object                  # (rows, cin, cout) of the 1 x rows x 1 filler problem (1x1, ReLU), or None
    splits: int = 1                 # K slices of every problem under test in this launch

    @property
    def kernel(self):
        return "conv_mfma_%dx%d%s" % (self.bm, self.bn, SUFFIX[self.math])


def _problem_set(c, tail):
    return (
        Prob("ragged", (2, 13, 11, 32), c, act="relu6", dest="slice", half_out=True),
        Prob("two_n_kpad_res", (2, 13, 11, 136), 2 * c, k=1, padding="valid", res="slice"),
        Prob("stride2_view", (2, 13, 11, 32), c, stride=2, padding=((0, 1), (0, 1)), act=None, dest="view"),
        Prob("dil3_res", (1, 12, 12, 32), c, dil=3, act="relu6", res="dense"),
        Prob("k1s2_unaligned", (2, 13, 11, 64), c, k=1, stride=2, padding="valid", dest="unaligned"),
        Prob("k5", (1, 9, 10, 32), c, k=5, dest="slice", alone=3),
        Prob("sigmoid", (2, 6, 6, 32), c, act="sigmoid", dest="slice"),
        Prob("cout75", (2, 13, 11, 32), 75, act="relu6", dest="packed"),
        Prob("cout130", (1, 9, 10, 32), 130, k=1, padding="valid", dest="packed"),
        Prob("shuffle2x2", (2, 7, 9, 64), c // 4, kind="shuffle", dest="slice"),
        tail,
    )


def _long_k(c):
    return Prob("long_k", (2, 6, 6, 256), c, alone=(("f32", 9), ("f16", 9), ("f32x3", 9), ("f16s", 4)))


STEM = Prob("stem", (2, 29, 27, 3), 64, k=7, stride=2, padding=STEM_PAD, kind="stem", half_out=True)
GN = Prob("gn", (2, 16, 16, 64), 128, gn=True, alone=0)
SET_128 = _problem_set(128, _long_k(128))
SET_64 = _problem_set(64, STEM)
SET_32 = _problem_set(64, _long_k(64))
GN_SET = (GN, replace(SET_128[0], half_out=False))
SPLIT_K_WIDE = Prob("split_k_wide", (4, 64, 64, 128), 128, alone=0)

FILL_128, FILL_256ROWS, FILL_64, FILL_32 = (38400, 64, 128), (66560, 64, 128), (38400, 64, 64), (25600, 64, 32)

CASES = []
for _m in ("f32", "f16", "f16s", "f32x3"):
    CASES += [Case(f"{_m}_128x128", _m, 128, 128, False, 1, SET_128, FILL_128),
              Case(f"{_m}_128x64", _m, 128, 64, False, 2, SET_64, FILL_64),
              Case(f"{_m}_128x32", _m, 128, 32, False, 3, SET_32, FILL_32)]
    if _m != "f16":                                      # ("f16" has no gn_partials form)
        CASES.append(Case(f"{_m}_128x128_gns", _m, 128, 128, True, 1, GN_SET, FILL_128))
CASES += [Case("f32x3_256x128", "f32x3", 256, 128, False, 1, SET_128, FILL_256ROWS),
          Case("f32x3_256x128_gns", "f32x3", 256, 128, True, 1, GN_SET, FILL_256ROWS),
          # split-K on the wide tile (the 64-deep chunks of "f16s" leave this problem 2 slices and 128 x 64 tiles: not a case)
          Case("f32_128x128_split_k", "f32", 128, 128, False, 1, (SPLIT_K_WIDE,), None, splits=4),
          Case("f32x3_128x128_split_k", "f32x3", 128, 128, False, 1, (SPLIT_K_WIDE,), None, splits=4)]
CASES = tuple(CASES)
BY_NAME = {c.name: c for c in CASES}
WIDEST = {"f32": "f32_128x128", "f16": "f16_128x128", "f16s": "f16s_128x128", "f32x3": "f32x3_256x128"}


def case_probs(case):
    """The problems of `case` that its math runs (see the refusals in the module docstring)."""
    return tuple(p for p in case.probs if not (case.math == "f16s" and p.kind == "stem"))


def has_res(prob, math):
    return prob.res is not None and math != "f16s"


def half_in(math):
    return math == "f16s"


def half_out(prob, math):
    """Is the output stored as half?  "f16s": wherever the half epilogue may be used; "f16": where the problem asks."""
    plain = (prob.dest in ("dense", "slice", "packed") and prob.act != "sigmoid" and prob.kind != "shuffle" and
             prob.cout % 4 == 0 and not has_res(prob, math))
    return plain and (math == "f16s" or (math == "f16" and prob.half_out))


# ------------------------------------------------------------------ data and the fp64 reference
@functools.lru_cache(maxsize=None)
def data(prob):
    """-> dict of fp32 arrays x, w, b (+ res): N(0, 1) inputs, weights scaled 1 / sqrt(K), bias N(0, 1) -- spread over [-1.5, 7.5]
    for ReLU6 (module docstring).  Seeded by the problem's name and width."""
    rng = np.random.default_rng(zlib.crc32(f"{prob.name}/{prob.cout}".encode()))
    B, H, W, cin = prob.shape
    x = rng.normal(size=prob.shape).astype(np.float32)
    if prob.kind == "shuffle":
        w = (rng.normal(size=(2, 2, prob.cout, cin)) / np.sqrt(cin)).astype(np.float32)
    else:
        w = (rng.normal(size=(prob.k, prob.k, cin, prob.cout)) / np.sqrt(prob.k * prob.k * cin)).astype(np.float32)
    b = rng.normal(size=(prob.cout,))
    if prob.act == "relu6":
        b = rng.permutation(np.linspace(-1.5, 7.5, prob.cout))
    d = dict(x=x, w=w, b=b.astype(np.float32))
    if prob.res is not None:
        d["res"] = rng.normal(size=out_shape(prob)).astype(np.float32)
    return d


def out_shape(prob):
    from masklab_hip.packing import resolve_padding
    B, H, W, _ = prob.shape
    if prob.kind == "shuffle":
        return (B, 2 * H, 2 * W, prob.cout)
    Ho, Wo, _, _ = resolve_padding(H, W, prob.k, prob.k, prob.stride, prob.dil, prob.padding)
    return (B, Ho, Wo, prob.cout)


def h64(a):
    return a.astype(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(prob, rounded, with_res):
    """-> (pre-activation, activated) fp64 oracle output; rounded: the operands x and w are rounded to half
    first, as "f16" does on the way into LDS and "f16s" holds them in memory.  The bias stays fp32."""
    d = data(prob)
    cast = h64 if rounded else (lambda a: a.astype(np.float64))
    x, w, b = cast(d["x"]), cast(d["w"]), d["b"].astype(np.float64)
    if prob.kind == "shuffle":
        pre = T.conv2d_transpose_2x2_s2(x, w, b)
    else:
        pre = T.conv2d(x, w, b, prob.stride, prob.padding, prob.dil)
    if with_res:                                     # (fp32 as it is: only "f16s" would hold it in half, and takes none)
        pre = pre + d["res"].astype(np.float64)
    return pre, ACT[prob.act](pre)


def expected(prob, math):
    """The fp64 reference of `prob` under `math`, rounded to half where the kernel stores half."""
    _, want = reference(prob, math in ("f16", "f16s"), has_res(prob, math))
    return want.astype(np.float16).astype(np.float64) if half_out(prob, math) else want


@functools.lru_cache(maxsize=None)
def filler_data(spec):
    rows, cin, cout = spec
    rng = np.random.default_rng(rows + cout)
    return dict(x=rng.normal(size=(1, rows, 1, cin)).astype(np.float32),
                w=(rng.normal(size=(1, 1, cin, cout)) / np.sqrt(cin)).astype(np.float32),
                b=rng.normal(size=(cout,)).astype(np.float32))


# ------------------------------------------------------------------ packing and host-only descriptors
@functools.lru_cache(maxsize=None)
def packed(prob, tile):
    from masklab_hip import packing
    d = data(prob)
    if prob.kind == "shuffle":
        return packing.pack_transpose2x2(d["w"], d["b"], tile=tile)
    if prob.kind == "stem":
        return packing.pack_rowspan(d["w"], d["b"], tile=tile)
    return packing.pack_dense(d["w"], d["b"], tile=tile)


def dest_layout(prob):
    """-> (cstride, coff, head, bgap) of the sentinel destination (tests/sentinel_dest.py), in elements."""
    co = prob.cout
    return {"dense": (co, 0, 8, 0), "slice": (co + 8, 4, 8, 0), "packed": (co, 0, 3 * co, 0),
            "view": (co + 4, 0, 8, 12), "unaligned": (co + 4, 0, 3, 4)}[prob.dest]


def _host_desc(p, in_shape, math, stride, padding, dil, act, hout, res, dest, gn):
    """The ml_conv2d_desc ops._conv_desc builds for this problem, with aligned fake addresses: the planning entries
    dereference nothing on the host."""
    from masklab_hip.packing import resolve_padding
    B, H, W, cbuf = in_shape
    hs = math == "f16s"
    Ho, Wo, pt, pl = resolve_padding(H, W, p.kh_real, p.kw_real, stride, dil, padding)
    cstride, coff, head, bgap = dest
    d = _lib.ConvDesc()
    d.in_, d.wgt, d.bias = 0x100000, 0x200000, 0x300000
    d.B, d.H, d.W, d.in_cstride, d.in_coff = B, H, W, cbuf, 0
    d.span, d.span_pad, d.cpp_shift = p.span, (-(-p.span // 64) * 64 if hs else p.span_pad), p.cpp_shift
    d.Ho, d.Wo, d.KH, d.KW, d.stride, d.dil, d.pad_t, d.pad_l = Ho, Wo, p.KH, p.KW, stride, dil, pt, pl
    d.cout, d.n_pad = p.cout, p.n_pad
    d.act, d.group_cin_step, d.shuffle2x2, d.tile = _lib.ACT_BY_NAME[act], p.group_cin_step, p.shuffle2x2, p.tile
    d.math, d.out_f16 = MATH_CODE[math], int(hout)
    es = 2 if hout else 4
    if bgap or head % (16 // es):                                  # out_view: the offset is folded into the pointer
        d.out, d.out_cstride, d.out_coff, d.out_bstride = 0x400000 + es * (head + coff), cstride, 0, Ho * Wo * cstride + bgap
    else:
        d.out, d.out_cstride, d.out_coff, d.out_bstride = 0x400000 + es * head, cstride, coff, 0
    if res:
        d.residual, d.res_cstride, d.res_coff = 0x500000, (p.cout + 8 if res == "slice" else p.cout), (4 if res == "slice" else 0)
    if gn:
        d.gn_partials = 0x600000
    return d


def host_desc(prob, math, tile):
    p = packed(prob, tile)
    shape = prob.shape[:3] + (4,) if prob.kind == "stem" else prob.shape
    return _host_desc(p, shape, math, prob.stride, "valid" if prob.kind == "shuffle" else prob.padding, prob.dil, prob.act,
                      half_out(prob, math), prob.res if has_res(prob, math) else None, dest_layout(prob), prob.gn)


def filler_desc(spec, math, tile):
    from masklab_hip import packing
    rows, cin, cout = spec
    p = packing.pack_dense(np.zeros((1, 1, cin, cout), np.float32), np.zeros(cout, np.float32), tile=tile)
    return _host_desc(p, (1, rows, 1, cin), math, 1, "valid", 1, "relu", math == "f16s", None, (cout, 0, 0, 0), False)


def launch_descs(case):
    """The descriptors of the case's launch, problems under test first, the filler last."""
    ds = [host_desc(p, case.math, case.tile) for p in case_probs(case)]
    if case.filler:
        ds.append(filler_desc(case.filler, case.math, case.tile))
    return ds
