"""The case table of the ResNeXt grouped 3x3 (csrc/gconv_mfma4.hip): five kernel bodies, 14 instantiations

              c = 4         c = 8         c = 16        c = 32
  fp32        mfma4         mfma4         gconv16       (refused)         x stride 1, 2
  half        mfma4h        mfma4h        gconv16h      gconv32h          x stride 1, 2

Importable without a GPU: tests/test_gconv_cases_cpu.py asks the library's host-only ml_gconv3x3_launch_plan that every row
is launched with the tile shape, run and block count it names and that the table names every instantiation;
tests/test_gpu_gconv_instantiations.py runs the rows.

Tile shapes (rows x columns of output pixels): fp32 8 x 8 at stride 1 and 4 x 8 at stride 2; half 16 x 8 and 8 x 8; c = 32
8 x 8.  A block of the twelve WALKING instantiations (c = 4, 8, 16) covers a run of tiles down one tile column of an image and
64-channel slab, the next tile's halo prefetched under the current tile's MFMAs; `column_run` halves the run until the launch
has 6 blocks per compute unit, 1536 on the 256 units of the MI355X (the count the table is written for; without a device the
library assumes it too).  A c = 32 block always walks its whole column, without the prefetch.

Rows (B = 2 unless noted; bias + ReLU unless noted; padding ((1, 1), (1, 1)) unless noted):
  edge_*   one per instantiation, the smallest map with a full tile, a partial tile at the right and one at the bottom edge,
           odd H and W, and at stride 2 (H, W odd, pad 1) the last window row and column on the zero padding: 2 x 2 tiles,
           one tile per block.  C = 64 (c = 32: its two groups); C = 192 once per dtype, so that slabs 1 and 2 (cs0 > 0, the
           slab-relative group base) run.
  run_*    one per walking instantiation: B = 32, C = 512 (8 slabs), 3 tile columns and 5 tile rows, the last tile row one
           pixel high.  3 x 8 x 32 = 768 blocks of 5 tiles are too few, so the run is halved to 3: 1536 blocks, runs of 3 + 2.
           The same image alone (B = 1) plans one tile per block.  The two c = 32 rows: 3 tiles per column, the last partial.
  none_* / relu6_* / nobias_*   per body and stride, on the edge shape: linear + bias, ReLU6 + bias, ReLU without bias.
  pad01_* ((0, 1), (0, 1)) -- TF 'same' at stride 2 on an even map -- per body; pad11even_* ((1, 1), (1, 1)) at stride 2 on
           an even map per body (the odd maps are the edge rows); same_* "same" through resolve_padding; valid_* no padding.
  tiny_*   per dtype and c: a 1 x 1 map, a 1 x 9 map, and a map lower than a tile and wider than one (stride 2).

Data: per row a seeded generator; inputs N(0, 1) (image i has its own stream, so one image can be made without the batch),
weights N(0, 1) / sqrt(9 c), bias N(0, 1) -- for ReLU6 rows spread evenly over [-1.5, 7.5], as tests/conv_cases.py does, so
that about a sixth of the pre-activation lies above 6 and a sixth below 0 (asserted on the fp64 reference: at least 5 % each).

Reference: torch.nn.functional.conv2d on the CPU in float64 with groups = C / c on explicitly zero-padded input (independent
of oracle.grouped_conv_fast, and compared with it once).  Half rows: both operands rounded to half first, the activated
result rounded to half (as tests/test_gpu_f16_storage.py::test_grouped3x3_half_storage)."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

from masklab_hip import _lib

ACT_CODE = {None: _lib.ACT_NONE, "relu": _lib.ACT_RELU, "relu6": _lib.ACT_RELU6}
P11 = ((1, 1), (1, 1))
P01 = ((0, 1), (0, 1))
BODY = {("f32", 4): "mfma4", ("f32", 8): "mfma4", ("f32", 16): "gconv16",
        ("f16", 4): "mfma4h", ("f16", 8): "mfma4h", ("f16", 16): "gconv16h", ("f16", 32): "gconv32h"}
INSTANTIATIONS = tuple((d, c, s) for (d, c) in BODY for s in (1, 2))          # 14
WALKING = tuple(i for i in INSTANTIATIONS if i[1] != 32)                      # 12
WANT_BLOCKS = 6 * 256                                 # GCONV_BLOCKS_PER_CU x the compute units of the MI355X


@dataclass(frozen=True)
class Row:
    name: str
    kind: str                       # "edge" | "run" | "epilogue" | "padding" | "tiny"
    dtype: str                      # "f32" | "f16"
    c: int
    stride: int
    C: int
    shape: tuple                    # (B, H, W)
    plan: tuple                     # expected (tile_h, tile_w, run, blocks)
    padding: object = P11
    act: object = "relu"
    bias: bool = True

    @property
    def half(self):
        return self.dtype == "f16"

    @property
    def inst(self):
        return (self.dtype, self.c, self.stride)

    @property
    def body(self):
        return BODY[(self.dtype, self.c)]


def tile_of(dtype, c, stride):
    """(tile_h, tile_w) as the kernels are instantiated (gconv_tile_h); the CPU test holds the library to it row by row."""
    if c == 32:
        return 8, 8
    if dtype == "f32":
        return (8, 8) if stride == 1 else (4, 8)
    return (16, 8) if stride == 1 else (8, 8)


def out_hw(row):
    """-> (Ho, Wo, pad_t, pad_l), as ops.gconv3x3 resolves the layer's padding."""
    from masklab_hip.packing import resolve_padding
    _, H, W = row.shape
    return resolve_padding(H, W, 3, 3, row.stride, 1, row.padding)


def _one_tile_plan(dtype, c, stride, C, B, tiles):
    """Expected plan of a launch far below 1536 blocks: one tile per block (c = 32: one block per tile column)."""
    th, tw = tile_of(dtype, c, stride)
    ty, tx = tiles
    return (th, tw, ty, tx * (C // 64) * B) if c == 32 else (th, tw, 1, tx * ty * (C // 64) * B)


def _edge_shape(dtype, c, stride):
    """A 2 x 2-tile output, one pixel beyond the full tile each way; odd H and W."""
    th, tw = tile_of(dtype, c, stride)
    Ho, Wo = th + 1, tw + 1
    return (2, Ho, Wo) if stride == 1 else (2, 2 * Ho - 1, 2 * Wo - 1)        # pad 1: Ho = (H + 1) / 2 for odd H


def _name(dtype, c, stride):
    return f"{dtype}_c{c}_s{stride}"


ROWS = []
# ---- a. edge rows
WIDE = {("f32", 8, 1), ("f16", 16, 2)}                 # C = 192: three slabs
for _i in INSTANTIATIONS:
    _C = 192 if _i in WIDE else 64
    ROWS.append(Row("edge_" + _name(*_i), "edge", *_i, _C, _edge_shape(*_i), _one_tile_plan(*_i, _C, 2, (2, 2))))
# ---- b. run rows
for _d, _c, _s in WALKING:
    _th, _tw = tile_of(_d, _c, _s)
    _Ho, _Wo = 4 * _th + 1, 2 * _tw + 1
    _hw = (_Ho, _Wo) if _s == 1 else (2 * _Ho - 1, 2 * _Wo - 1)
    ROWS.append(Row("run_" + _name(_d, _c, _s), "run", _d, _c, _s, 512, (32,) + _hw, (_th, _tw, 3, WANT_BLOCKS)))
ROWS += [Row("run_f16_c32_s1", "run", "f16", 32, 1, 128, (2, 19, 11), (8, 8, 3, 8)),
         Row("run_f16_c32_s2", "run", "f16", 32, 2, 128, (2, 37, 21), (8, 8, 3, 8))]
# ---- c. epilogue rows, d. padding rows: per body and stride
BODY_INST = [("f32", 4, 1), ("f32", 8, 2), ("f32", 16, 1), ("f32", 16, 2), ("f16", 4, 1), ("f16", 8, 2),
             ("f16", 16, 1), ("f16", 16, 2), ("f16", 32, 1), ("f16", 32, 2)]
for _i in BODY_INST:
    _p = _one_tile_plan(*_i, 64, 2, (2, 2))
    for _tag, _act, _bias in (("none", None, True), ("relu6", "relu6", True), ("nobias", "relu", False)):
        ROWS.append(Row(f"{_tag}_" + _name(*_i), "epilogue", *_i, 64, _edge_shape(*_i), _p, act=_act, bias=_bias))
for _i in [i for i in BODY_INST if i[2] == 2]:
    _th, _tw = tile_of(*_i)
    _even = (2, 2 * _th + 2, 2 * _tw + 2)              # both paddings: Ho = H / 2 = tile_h + 1
    _p = _one_tile_plan(*_i, 64, 2, (2, 2))
    ROWS.append(Row("pad01_" + _name(*_i), "padding", *_i, 64, _even, _p, padding=P01, act=None))
    ROWS.append(Row("pad11even_" + _name(*_i), "padding", *_i, 64, _even, _p))
ROWS += [Row("same_f32_c16_s2", "padding", "f32", 16, 2, 64, (2, 10, 18), (4, 8, 1, 8), padding="same", act=None),
         Row("same_f16_c32_s2", "padding", "f16", 32, 2, 64, (2, 18, 18), (8, 8, 2, 4), padding="same", act=None),
         Row("same_f16_c4_s1", "padding", "f16", 4, 1, 64, (2, 17, 9), (16, 8, 1, 8), padding="same"),
         Row("valid_f32_c4_s1", "padding", "f32", 4, 1, 64, (2, 11, 11), (8, 8, 1, 8), padding="valid", act=None),
         Row("valid_f16_c16_s1", "padding", "f16", 16, 1, 64, (2, 19, 11), (16, 8, 1, 8), padding="valid", act=None)]
# ---- e. tiny maps
for (_d, _c) in BODY:
    ROWS.append(Row(f"tiny_1x1_{_d}_c{_c}", "tiny", _d, _c, 1, 64, (2, 1, 1), _one_tile_plan(_d, _c, 1, 64, 2, (1, 1))))
    ROWS.append(Row(f"tiny_1x9_{_d}_c{_c}", "tiny", _d, _c, 1, 64, (2, 1, 9), _one_tile_plan(_d, _c, 1, 64, 2, (1, 2))))
    ROWS.append(Row(f"tiny_low_wide_{_d}_c{_c}", "tiny", _d, _c, 2, 64, (2, 5, 21), _one_tile_plan(_d, _c, 2, 64, 2, (1, 2))))
ROWS = tuple(ROWS)
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


# ------------------------------------------------------------------ the plan entry
def plan(row, B=None):
    """-> (rc, [tile_h, tile_w, tiles_x, tiles_y, run, blocks]) of ml_gconv3x3_launch_plan for `row` (or its images alone)."""
    import ctypes as C
    Bn, H, W = row.shape
    Ho, Wo, _, _ = out_hw(row)
    out = (C.c_int32 * 6)()
    rc = _lib.load().ml_gconv3x3_launch_plan(Bn if B is None else B, H, W, row.C, row.c, row.stride, Ho, Wo, int(row.half), out)
    return rc, list(out)


# ------------------------------------------------------------------ data and the fp64 reference
def _seed(row):
    return zlib.crc32(row.name.encode())


@functools.lru_cache(maxsize=None)
def params(row):
    """-> (k [3, 3, C, c] fp32 in the reference's DepthwiseConv2D(depth_multiplier = c) layout, bias [C] fp32)."""
    rng = np.random.default_rng(_seed(row))
    k = (rng.standard_normal((3, 3, row.C, row.c)) / np.sqrt(9 * row.c)).astype(np.float32)
    b = rng.standard_normal(row.C)
    if row.act == "relu6":
        b = rng.permutation(np.linspace(-1.5, 7.5, row.C))
    return k, b.astype(np.float32)


def image(row, i):
    """Image i of the row's batch [H, W, C], fp32 or half: its own stream, whatever the batch."""
    _, H, W = row.shape
    x = np.random.default_rng([_seed(row), i]).standard_normal((H, W, row.C), dtype=np.float32)
    return x.astype(np.float16) if row.half else x


def batch(row):
    return np.stack([image(row, i) for i in range(row.shape[0])])


def h64(a):
    return a.astype(np.float16).astype(np.float64)


def conv_fp64(x, k, c, stride, Ho, Wo, pad_t, pad_l):
    """Grouped 3x3 in float64: x [B, H, W, C], k [3, 3, C, c] with out[g c + m] = sum_i x[g c + i] * k[.., g c + i, m]."""
    import torch
    B, H, W, C = x.shape
    Hp, Wp = (Ho - 1) * stride + 3, (Wo - 1) * stride + 3              # exactly the rows and columns the windows touch
    xp = np.zeros((B, C, Hp, Wp), np.float64)
    h, w = min(H, Hp - pad_t), min(W, Wp - pad_l)
    xp[:, :, pad_t:pad_t + h, pad_l:pad_l + w] = np.transpose(x[:, :h, :w].astype(np.float64), (0, 3, 1, 2))
    wt = k.astype(np.float64).reshape(3, 3, C // c, c, c).transpose(2, 4, 3, 0, 1).reshape(C, c, 3, 3)     # [g c + m][i][kh][kw]
    y = torch.nn.functional.conv2d(torch.from_numpy(xp), torch.from_numpy(np.ascontiguousarray(wt)), stride=stride, groups=C // c)
    return np.transpose(y.numpy(), (0, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def reference(row):
    """-> (pre-activation, expected output) of images 0 and B - 1, [2, Ho, Wo, C] float64; half rows: operands rounded to half
    (the images are halves already), the activated result rounded to half.  The bias stays fp32."""
    k, b = params(row)
    Ho, Wo, pt, pl = out_hw(row)
    x = np.stack([image(row, 0), image(row, row.shape[0] - 1)])
    pre = conv_fp64(x, h64(k) if row.half else k, row.c, row.stride, Ho, Wo, pt, pl)
    if row.bias:
        pre = pre + b.astype(np.float64)
    want = {None: pre, "relu": np.maximum(pre, 0.0), "relu6": np.clip(pre, 0.0, 6.0)}[row.act]
    if row.half:
        want = want.astype(np.float16).astype(np.float64)
    pre.setflags(write=False)
    want.setflags(write=False)
    return pre, want
