"""References for the backward of the resampling layers (test infrastructure, not collected: no `test_` prefix).

A float64 restatement of the three forwards in torch, differentiated by autograd:

1.  `resize`: resize_bilinear(align_corners=True) as bilinear_ac_kernel computes it (csrc/pointwise.hip);
2.  `roi_align`: crop_and_resize + MoldBatch(-1) as roi_crop_resize_kernel computes it (csrc/detect.hip);
3.  `global_mean`.

Every sample is a row of a per-axis weight matrix [samples, pixels], so a forward is one einsum and `scale` -- the uncancelled
magnitude S = sum |weight * dy| of every gradient element, which the bar is relative to -- is the transposed einsum over
absolute values.  With coords=F32 the sample COORDINATES are evaluated in float32 NumPy in the forward kernels' operation order
(one rounding per operation; the resize's fraction is the kernel's fma: the exact product, rounded once), which makes
crop_and_resize's in-range decision the device's decision; weights and sums are float64.  With coords=F64 everything is
float64: what the restatement is compared against torch's own resampling with.

`margin`: how far the RoI samples of a case keep from crop_and_resize's in-range test, the one point where the gradient is not
continuous in the coordinate.  Then the named cases of the GPU test."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
BAR = 1e-5          # the project's gradient bar: |got - want| <= BAR * S


# ------------------------------------------------------------------ resize_bilinear(align_corners=True)
def resize_axis_matrix(n_in, n_out, coords=F32):
    """[n_out, n_in] float64: f = o*s, i0 = max(floor f, 0), i1 = min(ceil f, n_in - 1), t = f - floor f, weights (1 - t)
    and t; where i0 == i1 the kernel's top + (bot - top)*t is the pixel itself."""
    o = np.arange(n_out, dtype=coords)
    s = coords(n_in - 1) / coords(n_out - 1) if n_out > 1 else coords(0)
    f = o * s
    fl = np.floor(f)
    t = (o.astype(F64) * F64(s) - fl.astype(F64)).astype(coords).astype(F64)        # fmaf(o, s, -floor f)
    i0 = np.maximum(fl, 0).astype(np.int64)
    i1 = np.minimum(np.ceil(f), n_in - 1).astype(np.int64)
    t = np.where(i0 == i1, 0.0, t)
    M = np.zeros((n_out, n_in), F64)
    np.add.at(M, (np.arange(n_out), i0), 1.0 - t)
    np.add.at(M, (np.arange(n_out), i1), t)
    return M


def _apply(My, Mx, x):
    return torch.einsum("ph,qw,...hwc->...pqc", torch.from_numpy(My), torch.from_numpy(Mx), x)


def _apply_t(My, Mx, dy):
    return torch.einsum("ph,qw,...pqc->...hwc", torch.from_numpy(My), torch.from_numpy(Mx), dy)


def resize(x, oh, ow, coords=F32):
    """x: float64 torch [B,H,W,C] -> [B,oh,ow,C]"""
    return _apply(resize_axis_matrix(x.shape[1], oh, coords), resize_axis_matrix(x.shape[2], ow, coords), x)


def resize_grad(dy, H, W, coords=F32):
    """-> (dx, S), float64 NumPy [B,H,W,C]: autograd of sum(resize(x) * dy) and its uncancelled magnitude"""
    dy = torch.from_numpy(np.asarray(dy, F64))
    x = torch.zeros((dy.shape[0], H, W, dy.shape[3]), dtype=torch.float64, requires_grad=True)
    (resize(x, dy.shape[1], dy.shape[2], coords) * dy).sum().backward()
    My, Mx = resize_axis_matrix(H, dy.shape[1], coords), resize_axis_matrix(W, dy.shape[2], coords)
    return x.grad.numpy(), _apply_t(np.abs(My), np.abs(Mx), dy.abs()).numpy()


def global_mean_grad(dpool, H, W):
    """-> (dx, S): autograd of sum(mean(x, (1, 2)) * dpool)"""
    dpool = torch.from_numpy(np.asarray(dpool, F64))
    x = torch.zeros((dpool.shape[0], H, W, dpool.shape[3]), dtype=torch.float64, requires_grad=True)
    (x.mean(dim=(1, 2), keepdim=True) * dpool).sum().backward()
    return x.grad.numpy(), np.broadcast_to(np.abs(dpool.numpy()) / (H * W), x.shape).copy()


# ------------------------------------------------------------------ crop_and_resize + MoldBatch
def roi_axis_coords(lo_px, hi_px, img, n_in, n_out, coords=F32):
    """The n_out sample coordinates of one axis of one box: lo_px / hi_px = centre -+ size/2 as the kernel forms them, then
    NormalizeBoxes by the image size, then tf.image.crop_and_resize's in = y1*(n_in-1) + o*hs (n_out > 1) or the centre."""
    y1, y2 = coords(lo_px) / coords(img), coords(hi_px) / coords(img)
    last = coords(n_in - 1)
    if n_out > 1:
        hs = (y2 - y1) * last / coords(n_out - 1)
        return y1 * last + np.arange(n_out, dtype=coords) * hs
    return np.full((1,), coords(0.5) * (y1 + y2) * last, coords)


def roi_axis_matrix(centre, size, img, n_in, n_out, coords=F32):
    """[n_out, n_in] float64; a sample outside [0, n_in - 1] is the extrapolation value: a zero row"""
    centre, size = coords(centre), coords(size)
    half = size / coords(2)
    c = roi_axis_coords(centre - half, centre + half, img, n_in, n_out, coords)
    ok = ~((c < 0) | (c > n_in - 1))
    cc = np.where(ok, c, 0)
    top, bot = np.floor(cc).astype(np.int64), np.ceil(cc).astype(np.int64)
    f = (cc - np.floor(cc)).astype(F64)
    M = np.zeros((n_out, n_in), F64)
    rows = np.arange(n_out)
    np.add.at(M, (rows[ok], top[ok]), (1.0 - f)[ok])
    np.add.at(M, (rows[ok], bot[ok]), f[ok])
    return M, c


def level_slots(rows, n_levels):
    """rows [B,cap,7] dist_boxes (k first) -> (slots [B,L,cap] int32 with -1 tails, counts [B,L] int32): MaskDistribute's
    assignment, tf.where order"""
    B, cap = rows.shape[:2]
    slots = np.full((B, n_levels, cap), -1, np.int32)
    counts = np.zeros((B, n_levels), np.int32)
    for b in range(B):
        for level in range(n_levels):
            idx = np.flatnonzero(rows[b, :, 0] == level)
            slots[b, level, :len(idx)] = idx
            counts[b, level] = len(idx)
    return slots, counts


def _roi_matrices(rows, shapes, crop, img_hw, coords):
    """-> {(level, b, j): (My, Mx, cy, cx)} for the live slots"""
    slots, counts = level_slots(rows, len(shapes))
    out = {}
    for level, (B, Hf, Wf, _) in enumerate(shapes):
        for b in range(B):
            for j in range(counts[b, level]):
                _, cx, cy, bw, bh = rows[b, slots[b, level, j], :5]
                My, yc = roi_axis_matrix(cy, bh, img_hw[0], Hf, crop[0], coords)
                Mx, xc = roi_axis_matrix(cx, bw, img_hw[1], Wf, crop[1], coords)
                out[level, b, j] = (My, Mx, yc, xc)
    return out


def roi_align(fmaps, rows, crop, img_hw, n_l, coords=F32):
    """fmaps: float64 torch [B,Hf,Wf,C] per level; rows [B,cap,7] float32 -> the molded crops [B,n_l[level],ch,cw,C] per
    level, -1 in the slots past an image's count"""
    shapes = [tuple(f.shape) for f in fmaps]
    mats = _roi_matrices(rows, shapes, crop, img_hw, coords)
    outs = []
    for level, f in enumerate(fmaps):
        parts = []
        for b in range(f.shape[0]):
            for j in range(n_l[level]):
                if (level, b, j) in mats:
                    parts.append(_apply(*mats[level, b, j][:2], f[b]))
                else:
                    parts.append(torch.full((crop[0], crop[1], f.shape[3]), -1.0, dtype=torch.float64))
        outs.append(torch.stack(parts).reshape(f.shape[0], n_l[level], crop[0], crop[1], f.shape[3]))
    return outs


def roi_align_grad(dys, rows, shapes, crop, img_hw, coords=F32):
    """-> ([dx per level], [S per level]) float64 NumPy: autograd of sum(roi_align * dy); dy of the padded slots takes no part"""
    n_l = [d.shape[1] for d in dys]
    fmaps = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in shapes]
    crops = roi_align(fmaps, rows, crop, img_hw, n_l, coords)
    _, counts = level_slots(rows, len(shapes))
    total = 0
    for level, (c, d) in enumerate(zip(crops, dys)):
        d = np.asarray(d, F64).copy()
        for b in range(d.shape[0]):
            d[b, counts[b, level]:] = 0            # the forward wrote the constant -1 there
        total = total + (c * torch.from_numpy(d)).sum()
    total.backward()
    mats = _roi_matrices(rows, shapes, crop, img_hw, coords)
    S = [np.zeros(s, F64) for s in shapes]
    for (level, b, j), (My, Mx, _, _) in mats.items():
        S[level][b] += _apply_t(np.abs(My), np.abs(Mx), torch.from_numpy(np.abs(np.asarray(dys[level][b, j], F64)))).numpy()
    return [f.grad.numpy() for f in fmaps], S


def margin(rows, shapes, crop, img_hw):
    """The smallest distance of any RoI sample coordinate (float32) from 0 and from Hf-1 / Wf-1, not counting coordinates that
    equal a bound exactly (y1 = 0 by construction, for example: those are in range on the device as they are here)."""
    worst = np.inf
    for (level, _, _), (_, _, yc, xc) in _roi_matrices(rows, shapes, crop, img_hw, F32).items():
        for c, n in ((yc, shapes[level][1]), (xc, shapes[level][2])):
            for bound in (0.0, float(n - 1)):
                d = np.abs(c.astype(F64) - bound)
                d = d[c != F32(bound)]
                if d.size:
                    worst = min(worst, float(d.min()))
    return worst


def interior_integer_samples(rows, shapes, crop, img_hw):
    """How many sample coordinates (float32) are whole numbers strictly inside the map: top == bottom"""
    n = 0
    for (level, _, _), (_, _, yc, xc) in _roi_matrices(rows, shapes, crop, img_hw, F32).items():
        for c, m in ((yc, shapes[level][1]), (xc, shapes[level][2])):
            n += int(((c == np.floor(c)) & (c > 0) & (c < m - 1)).sum())
    return n


def check(got, want, S, what, bar=BAR):
    """|got - want| <= bar * S elementwise, exact zeros where S == 0; prints the largest ratio.  -> that ratio"""
    g, w = np.asarray(got, F64), np.asarray(want, F64)
    assert g.shape == w.shape == S.shape and np.isfinite(g).all(), (what, g.shape, w.shape, S.shape)
    ratio = np.abs(g - w) / np.maximum(S, np.finfo(F64).tiny)
    ratio = np.where((S == 0) & (g == w), 0.0, ratio)
    worst = float(ratio.max())
    print(f"{what}: max |got - want| / S = {worst:.3g} (bar {bar:g})")
    assert worst <= bar, f"{what}: off by {worst:.3g} * S at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


# ------------------------------------------------------------------ the cases
IMG_HW = (64, 64)
CAP = 8
PAD = (-1, -1, -1, -1, -1, -1, -1)


def _level_shapes(C):
    return [(2, 16, 16, C), (2, 8, 8, C), (2, 4, 4, C)]


# Image 0, (k, cx, cy, w, h) in image pixels; a feature cell of level 0 / 1 / 2 is 64/15, 64/7, 64/3 pixels wide.
_IMAGE0 = [
    (0, 20.3, 18.7, 17.9, 13.3),        # A and B overlap on level 0: the summation order over slots
    (0, 24.1, 21.9, 15.2, 18.6),        # B
    (0, 41.3, 37.7, 1.1, 0.9),          # smaller than one cell: every sample between the same four pixels
    (2, 10.0, 12.0, 20.0, 24.0),        # top-left exactly (0, 0): the first sample of each axis sits on the bound
    (0, 32.0, 32.0, 63.0, 63.0),        # the whole image on the 16 x 16 level: sample spacing > 1, pixels no sample touches
    (1, 58.0, 5.0, 24.0, 22.0),         # hangs 6 pixels off the top and the right: those samples contribute nothing
]
# one more box per crop size whose coordinates hit whole numbers inside the map (float32 arithmetic, see
# interior_integer_samples); found by search, asserted in test_resample_grad_cpu.py
_INTEGER_BOX = {
    (14, 14): (1, 20.71428680419922, 20.71428680419922, 33.42857360839844, 33.42857360839844),   # sample 2 of each axis = 1.0
    (3, 5): (1, 14.285714149475098, 9.14285659790039, 20.571428298950195, 10.285712242126465),   # sample 1 of each axis = 1.0
    (1, 1): (2, 128.0 / 3, 64.0 / 3, 9.0, 7.0),                                                  # the centre = (1.0, 2.0)
}
# Image 1: level 1 filled to cap, no RoI on levels 0 and 2
_IMAGE1 = [(1, 9.0 + 6.1 * i, 50.0 - 5.3 * i, 11.0 + 2.7 * i, 30.5 - 3.1 * i) for i in range(CAP)]

ROI_CASES = {"crop14": ((14, 14), 8), "crop3x5": ((3, 5), 8), "crop1": ((1, 1), 8), "crop14_c4": ((14, 14), 4)}


def roi_case(name):
    """-> dict(rows [2,CAP,7] float32 dist_boxes (k, cx, cy, w, h, class, confidence; image 0 ends in a -1 padding row),
    shapes, crop, img_hw, and the gradients at the crops in the capacity form [2,CAP,ch,cw,C] with 1e30 in every slot
    past an image's count)"""
    crop, C = ROI_CASES[name]
    rows = np.empty((2, CAP, 7), F32)
    boxes0 = _IMAGE0 + [_INTEGER_BOX[crop]]
    if crop == (1, 1):                                  # the one sample is the box's centre: move that off the image
        boxes0[5] = (1, 67.0, 5.0, 24.0, 22.0)
    for b, boxes in enumerate((boxes0, _IMAGE1)):
        for i in range(CAP):
            rows[b, i] = boxes[i] + (float(i % 3), 0.5) if i < len(boxes) else PAD
    shapes = _level_shapes(C)
    r = np.random.default_rng(7 + list(ROI_CASES).index(name))
    _, counts = level_slots(rows, len(shapes))
    dys = []
    for level in range(len(shapes)):
        dy = r.normal(0, 1, (2, CAP, crop[0], crop[1], C)).astype(F32)
        for b in range(2):
            dy[b, counts[b, level]:] = F32(1e30)
        dys.append(dy)
    return dict(rows=rows, shapes=shapes, crop=crop, img_hw=IMG_HW, dys=dys, counts=counts)


def many_rois_case(n=70):
    """One 6 x 5 level, n RoIs of one image on it, all samples well inside the map: more RoIs than the kernel stages in LDS
    at a time (64), so the walk crosses a chunk boundary.  The same dict as roi_case."""
    r = np.random.default_rng(23)
    rows = np.empty((1, n, 7), F32)
    w, h = r.uniform(2, 30, n), r.uniform(2, 30, n)
    cx, cy = 2 + w / 2 + r.uniform(0, 1, n) * (60 - w), 2 + h / 2 + r.uniform(0, 1, n) * (60 - h)
    rows[0] = np.stack([np.zeros(n), cx, cy, w, h, np.ones(n), np.full(n, 0.5)], axis=1)
    crop, shapes = (3, 5), [(1, 6, 5, 4)]
    return dict(rows=rows, shapes=shapes, crop=crop, img_hw=IMG_HW, dys=[r.normal(0, 1, (1, n, 3, 5, 4)).astype(F32)],
                counts=level_slots(rows, 1)[1])


def sized(case):
    """The gradients as the sized forward shapes them: n_l = max(1, the level's largest count)"""
    n_l = [max(1, int(case["counts"][:, level].max())) for level in range(len(case["shapes"]))]
    return [np.ascontiguousarray(d[:, :n]) for d, n in zip(case["dys"], n_l)]


# (B, H, W, C) of the source, (Ho, Wo) of the resize's output
RESIZE_CASES = {
    "up2": ((2, 4, 4, 8), (8, 8)),
    "odd": ((2, 3, 5, 8), (7, 9)),
    "same": ((1, 8, 8, 8), (8, 8)),           # every coordinate a whole number
    "down": ((2, 8, 8, 8), (4, 4)),           # sources no sample touches: exact zeros
    "column": ((2, 5, 1, 8), (9, 1)),
    "pooled": ((2, 1, 1, 8), (6, 6)),         # the reduction path
    "tail": ((1, 33, 17, 12), (65, 33)),      # the grid's last block is partly empty
    "pooled_big": ((2, 1, 1, 72), (37, 29)),  # the reduction path with several slices and channel blocks, ragged
}


def resize_case(name, cs=None, coff=0):
    """-> (dy float32 [B,Ho,Wo,cs or C], source shape); with cs the gradient is channels coff : coff + C of a wider tensor"""
    (B, H, W, C), (Ho, Wo) = RESIZE_CASES[name]
    r = np.random.default_rng(50 + list(RESIZE_CASES).index(name))
    return r.normal(0, 1, (B, Ho, Wo, cs or C)).astype(F32), (B, H, W, C)
