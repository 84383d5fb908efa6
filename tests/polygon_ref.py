"""NumPy restatement of the "Dataset polygons" contract of include/masklab_hip.h (test infrastructure, not collected).
This text is the contract the library is held to, by exact equality; skimage parity is unpinned (the rule was written down
from memory of skimage.draw.polygon's 2019 releases and never run against skimage).

A vertex is clipped to the image first.  Pixel (x, y) is inside iff an odd number of edges (j -> i), j = i - 1 cyclically,
cross its row half-openly, (yp[i] <= y < yp[j]) or (yp[j] <= y < yp[i]), with
x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i] in float64: a multiply, a divide, an add, each rounded on its
own (NumPy never fuses them)."""
import numpy as np


def polygon_mask(verts, H, W):
    """float64 [V,2] (x, y) -> bool [H,W].  Every edge is tested against every pixel."""
    v = np.asarray(verts, np.float64).reshape(-1, 2)
    xp = np.minimum(np.maximum(v[:, 0], 0.0), float(W - 1))
    yp = np.minimum(np.maximum(v[:, 1], 0.0), float(H - 1))
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(W, dtype=np.float64)[None, :]
    inside = np.zeros((H, W), bool)
    for i in range(len(xp)):
        j = i - 1 if i else len(xp) - 1
        rows = ((yp[i] <= y) & (y < yp[j])) | ((yp[j] <= y) & (y < yp[i]))
        with np.errstate(divide="ignore", invalid="ignore"):                       # horizontal edges: no row crosses them
            e = (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]
        inside ^= rows & (x < e)
    return inside


def instance_planes(verts, plane_offsets, windows, B, n, H, W):
    """-> int8 [B,n,H,W]: -1 planes for empty vertex ranges, else the polygon inside its inclusive window."""
    verts = np.asarray(verts, np.float64).reshape(-1, 2)
    out = np.zeros((B * n, H, W), np.int8)
    for p in range(B * n):
        b, e = int(plane_offsets[p]), int(plane_offsets[p + 1])
        if b == e:
            out[p] = -1
            continue
        x1, y1, x2, y2 = (int(v) for v in windows[p])
        window = np.zeros((H, W), bool)
        window[max(y1, 0):min(y2, H - 1) + 1, max(x1, 0):min(x2, W - 1) + 1] = True
        out[p] = polygon_mask(verts[b:e], H, W) & window
    return out.reshape(B, n, H, W)


def semantic_maps(verts, poly_offsets, group_offsets, B, S, H, W):
    """-> uint8 [B,H,W,S]: per channel the union of its group's polygons minus the union of the except group's."""
    verts = np.asarray(verts, np.float64).reshape(-1, 2)
    out = np.zeros((B, H, W, S), np.uint8)

    def union(g):
        m = np.zeros((H, W), bool)
        for p in range(int(group_offsets[g]), int(group_offsets[g + 1])):
            m |= polygon_mask(verts[int(poly_offsets[p]):int(poly_offsets[p + 1])], H, W)
        return m
    for b in range(B):
        excepted = union(b * (S + 1) + S)
        for s in range(S):
            out[b, :, :, s] = union(b * (S + 1) + s) & ~excepted
    return out
