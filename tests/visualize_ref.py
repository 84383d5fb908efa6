"""NumPy restatement of the serving model's 'visualize' output (road_project/setup/serving.py:30-40; engine/layers/misc.py
DrawSegmentation :404-431, DrawInstance :434-475, DrawBoxes :478-503), written from the arithmetic contract: fp32, no
fused multiply-add, sums in the stated order.  CropAndPadMask is oracle.masklab.crop_and_pad_mask."""
import numpy as np

from oracle import masklab as O

F32 = np.float32


def draw_segmentation(images, maps, colors, alpha):
    """uint8(trunc(clip(img + S * alpha, 0, 255))), S = sum over k in order of colors[k] * float(maps[..., k])."""
    img = images.astype(F32)
    m = maps.astype(F32)
    col = np.asarray(colors, F32)
    S = np.zeros(img.shape, F32)
    for k in range(col.shape[0]):
        S = S + col[k] * m[..., k:k + 1]
    v = img + S * F32(alpha)
    return np.clip(v, F32(0), F32(255)).astype(np.uint8)


def draw_instance(images, det, cpm, colors, alpha):
    """Per class k: the canvases of the rows with class k summed in row order from 0.0f, > 0.5; then DrawSegmentation."""
    B, n = det.shape[:2]
    K = len(colors)
    H, W = images.shape[1:3]
    masks = np.zeros((B, H, W, K), F32)
    for b in range(B):
        for k in range(K):
            s = np.zeros((H, W), F32)
            for i in range(n):
                if det[b, i, 4] == k:
                    s = s + cpm[b, i]
            masks[b, ..., k] = (s > F32(0.5)).astype(F32)
    return draw_segmentation(images, masks, colors, alpha)


def box_lines(row, H, W):
    """tf.image.draw_bounding_boxes' rule for one (cx, cy, w, h) row: None when the box is skipped, else
    (r0, r1, c0, c1) -- unclamped line rows / columns as Python ints."""
    cx, cy, w, h = (F32(max(int(v), 0)) for v in row[:4])
    ymin, xmin = (cy - h / F32(2)) / F32(H), (cx - w / F32(2)) / F32(W)
    ymax, xmax = (cy + h / F32(2)) / F32(H), (cx + w / F32(2)) / F32(W)
    r0, r1 = int(ymin * F32(H - 1)), int(ymax * F32(H - 1))           # int() truncates toward zero
    c0, c1 = int(xmin * F32(W - 1)), int(xmax * F32(W - 1))
    if r0 > r1 or c0 > c1 or r0 >= H or r1 < 0 or c0 >= W or c1 < 0:
        return None
    return r0, r1, c0, c1


def draw_boxes(images, det):
    """White 1-pixel outlines of every row, whatever its class or confidence."""
    out = images.copy()
    B, H, W = images.shape[:3]
    for b in range(B):
        for i in range(det.shape[1]):
            lines = box_lines(det[b, i], H, W)
            if lines is None:
                continue
            r0, r1, c0, c1 = lines
            cl, ch = max(c0, 0), min(c1, W - 1)
            rl, rh = max(r0, 0), min(r1, H - 1)
            if r0 >= 0:
                out[b, r0, cl:ch + 1] = 255
            if r1 < H:
                out[b, r1, cl:ch + 1] = 255
            if c0 >= 0:
                out[b, rl:rh + 1, c0] = 255
            if c1 < W:
                out[b, rl:rh + 1, c1] = 255
    return out


def visualize(images, det, ins, seg, instance_colors, instance_alpha, semantic_colors, semantic_alpha):
    """serving.py:30-40: CropAndPadMask, DrawBoxes, DrawInstance, DrawSegmentation."""
    cpm = O.crop_and_pad_mask(images.shape[1:3], det, ins)
    v1 = draw_boxes(images, det)
    v2 = draw_instance(v1, det, cpm, instance_colors, instance_alpha)
    return draw_segmentation(v2, seg, semantic_colors, semantic_alpha)
