"""Case builders of the polygon tests (test infrastructure, not collected), shared by the CPU and the GPU tests.  Every case
is a few polygons as float64 [V,2] (x, y) arrays, scaled to the image so the same cases run at both sizes."""
import numpy as np

SIZES = [(45, 80), (37, 53)]                     # neither width is a multiple of 16


def circle(cx, cy, r, V=300):
    t = np.arange(V) * (2 * np.pi / V)
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1)


def polygons(H, W):
    """name -> float64 [V,2]: the single-polygon cases."""
    h, w = float(H), float(W)
    tri = np.array([[3.3, 2.2], [w - 7.6, h * 0.4], [w * 0.3, h - 3.7]])
    cases = {
        "triangle": tri,
        "concave": np.array([[2.5, 2.5], [w - 3.5, 3.1], [w - 4.2, h - 2.9], [w * 0.5, h * 0.35], [4.4, h - 4.6]]),
        "bow_tie": np.array([[4.2, 3.1], [w - 5.3, h - 4.2], [w - 5.8, 3.7], [4.9, h - 3.3]]),
        "horizontal_edges": np.array([[5.5, 4.0], [w - 6.5, 4.0], [w - 6.5, h * 0.5], [w * 0.5, h * 0.5], [w * 0.5, h - 5.0],
                                      [5.5, h - 5.0]]),
        # every vertex and two whole edges on integer coordinates: the half-open rows and the strict < on columns
        "on_integers": np.array([[4.0, 3.0], [20.0, 3.0], [28.0, 11.0], [20.0, 19.0], [4.0, 19.0], [12.0, 11.0]]),
        "duplicated_vertices": np.repeat(tri, [2, 3, 1], axis=0),
        "one_vertex": np.array([[10.0, 10.0]]),
        "two_vertices": np.array([[3.0, 4.0], [w - 5.0, h - 6.0]]),
        "collinear": np.array([[2.0, 2.0], [10.0, 6.0], [18.0, 10.0], [26.0, 14.0]]),
        "circle_300": circle(w * 0.45, h * 0.5, min(h, w) * 0.4),
        "clipped_on_four_sides": np.array([[-9.5, h * 0.3], [w * 0.3, -7.25], [w * 0.8, -5.0], [w + 12.5, h * 0.4], [w + 3.0, h * 0.8],
                                           [w * 0.55, h + 8.75], [w * 0.2, h + 4.0], [-6.0, h * 0.7]]),
        "touches_last_row_and_column": np.array([[w * 0.4, h * 0.3], [w - 1.0, h * 0.6], [w - 1.0, h - 1.0], [w * 0.5, h - 1.0]]),
    }
    return {k: np.ascontiguousarray(v, np.float64) for k, v in cases.items()}


DEGENERATE = ("one_vertex", "two_vertices", "collinear")


def pack(polys):
    """A list of [V,2] arrays -> (verts float64 [total,2], offsets int32 [len+1])."""
    offsets = np.zeros(len(polys) + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in polys])
    verts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in polys] + [np.zeros((0, 2))]).astype(np.float64)
    return np.ascontiguousarray(verts), offsets


def full_window(H, W):
    return [0, 0, W - 1, H - 1]


def instance_batch(H, W):
    """B = 2 images with 3 and 1 instances, n = 3: every single-polygon case would be too many planes, so the batch takes
    a cut window, a window with x2 >= W, a plain one; the second image has two padding planes.
    -> (verts, plane_offsets, windows, B, n)."""
    P = polygons(H, W)
    planes = [P["circle_300"], P["touches_last_row_and_column"], P["bow_tie"], P["triangle"], np.zeros((0, 2)), np.zeros((0, 2))]
    windows = np.array([[W // 3, H // 4, W // 3 + 21, H // 4 + 17], [5, 2, W + 30, H + 4], full_window(H, W), [0, 0, W - 1, H - 1],
                        [0, 0, 5, 5], [-1, -1, -1, -1]], np.int32)
    verts, offsets = pack(planes)
    return verts, offsets, windows, 2, 3


def semantic_batch(H, W):
    """B = 2, S = 3.  Image 0: label 0 = two overlapping polygons (a union, not an xor), label 1 = one polygon the except
    polygon cuts into, label 2 = nothing (zeros); the except group = one circle.  Image 1: label 2 only, no except polygon.
    -> (verts, poly_offsets, group_offsets, B, S)."""
    h, w = float(H), float(W)
    a = np.array([[3.5, 3.5], [w * 0.6, 4.5], [w * 0.55, h * 0.7], [4.5, h * 0.65]])
    b = a + np.array([w * 0.2, h * 0.15])
    c = polygons(H, W)["concave"]
    exc = circle(w * 0.5, h * 0.5, min(h, w) * 0.22, V=40)
    bow = polygons(H, W)["bow_tie"]
    polys = [a, b, c, exc, bow]
    verts, poly_offsets = pack(polys)
    #               image 0: s0   s1  s2  except | image 1: s0 s1 s2 except
    group_offsets = np.array([0, 2, 3, 3, 4, 4, 4, 5, 5], np.int32)
    return verts, poly_offsets, group_offsets, 2, 3


def random_batch(B, n, H, W, seed):
    """Random polygons of 3..40 vertices (some outside the image), random windows, some padding planes."""
    rng = np.random.default_rng(seed)
    planes, windows = [], []
    for p in range(B * n):
        if p % 4 == 3:
            planes.append(np.zeros((0, 2)))
            windows.append([0, 0, 0, 0])
            continue
        V = int(rng.integers(3, 41))
        planes.append(np.stack([rng.uniform(-8, W + 8, V), rng.uniform(-8, H + 8, V)], axis=1))
        x1, y1 = int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2))
        windows.append([x1, y1, x1 + int(rng.integers(1, W)), y1 + int(rng.integers(1, H))])
    verts, offsets = pack(planes)
    return verts, offsets, np.array(windows, np.int32)
