"""The serving 'visualize' output without a device: the NumPy restatement (tests/visualize_ref.py) against independent
rules, the C entry points' argument checks, the layer registry and the serving model's outputs."""
import ctypes

import numpy as np
import pytest

import visualize_ref as V


def _on_outline(r0, r1, c0, c1, y, x):
    """Pixel membership by the line definitions: a horizontal line covers the columns of the box inside the frame, a
    vertical one its rows; a line outside the frame is absent."""
    return ((y == r0 or y == r1) and c0 <= x <= c1) or ((x == c0 or x == c1) and r0 <= y <= r1)


def test_draw_boxes_restatement_matches_a_per_pixel_membership_rule():
    rng = np.random.default_rng(7)
    for H, W in ((1, 1), (1, 9), (7, 1), (12, 17), (31, 40)):
        n = 24
        det = np.zeros((1, n, 6), np.int32)
        det[0, :, 0] = rng.integers(-3 * W, 3 * W, n)
        det[0, :, 1] = rng.integers(-3 * H, 3 * H, n)
        det[0, :, 2] = rng.integers(0, 3 * W, n)
        det[0, :, 3] = rng.integers(0, 3 * H, n)
        det[0, 0] = (-2, -2, -2, -2, -1, -100)                       # a padded row: box (0, 0, 0, 0)
        det[0, 1, 2:4] = 0                                           # zero size
        det[0, 2, :4] = (10 ** 9, 10 ** 9, 10, 10)                   # far outside
        det[0, 3, :4] = (W // 2, H // 2, 40 * W, 40 * H)             # overhangs every side
        images = rng.integers(0, 255, (1, H, W, 3), dtype=np.uint8)
        got = V.draw_boxes(images, det)
        want = images.copy()
        for i in range(n):
            cx, cy, w, h = (np.float32(max(int(v), 0)) for v in det[0, i, :4])
            f = np.float32
            r0 = int(np.trunc(np.float32((cy - h / f(2)) / f(H)) * f(H - 1)))
            r1 = int(np.trunc(np.float32((cy + h / f(2)) / f(H)) * f(H - 1)))
            c0 = int(np.trunc(np.float32((cx - w / f(2)) / f(W)) * f(W - 1)))
            c1 = int(np.trunc(np.float32((cx + w / f(2)) / f(W)) * f(W - 1)))
            if r0 > r1 or c0 > c1:
                continue
            for y in range(H):
                for x in range(W):
                    if _on_outline(r0, r1, c0, c1, y, x):
                        want[0, y, x] = 255
        np.testing.assert_array_equal(got, want, err_msg=f"{H}x{W}")
        if H > 1 and W > 1:
            assert (got[0, 0, 0] == 255).all()                      # the padded row paints pixel (0, 0), as the reference does


def test_draw_segmentation_saturates_truncates_and_uses_alpha():
    images = np.array([[[[250, 10, 0], [0, 0, 0], [100, 101, 102]]]], np.uint8)
    maps = np.array([[[[1, 1], [0, 1], [0, 0]]]], np.int32)
    colors = [[20, 7, 3], [13, 0, 255]]
    got = V.draw_segmentation(images, maps, colors, 0.45)
    f = np.float32
    S = np.array([[33, 7, 258], [13, 0, 255], [0, 0, 0]], f)
    want = np.clip(images[0, 0].astype(f) + S * f(0.45), 0, 255)
    np.testing.assert_array_equal(got[0, 0], np.trunc(want).astype(np.uint8))
    assert got[0, 0, 0, 0] == 255 and got[0, 0, 0, 2] == 116        # 250 + 14.85 saturates; 0 + 116.1 truncates
    assert got[0, 0, 1, 0] == 5                                      # 13 * 0.45 = 5.85 -> 5


def test_draw_instance_sums_a_class_before_the_threshold():
    det = np.array([[[0, 0, 0, 0, 1, 90], [0, 0, 0, 0, 1, 90], [0, 0, 0, 0, 7, 90], [0, 0, 0, 0, -1, -100]]], np.int32)
    cpm = np.zeros((1, 4, 1, 2), np.float32)
    cpm[0, 0, 0] = (0.3, 0.3)
    cpm[0, 1, 0] = (0.3, 0.0)                                        # 0.6 together at x = 0, 0.3 alone at x = 1
    cpm[0, 2, 0] = (1.0, 1.0)                                        # class 7 has no colour: never drawn
    cpm[0, 3, 0] = (1.0, 1.0)                                        # padding
    images = np.zeros((1, 1, 2, 3), np.uint8)
    got = V.draw_instance(images, det, cpm, [[10, 10, 10], [100, 50, 0]], 0.5)
    np.testing.assert_array_equal(got[0, 0], [[50, 25, 0], [0, 0, 0]])


def test_sixteen_colours_at_most_in_abi_7():
    from masklab_hip import _lib
    assert _lib.DRAW_MAX_CLASSES == 16 and _lib.load().ml_version() == _lib.ABI_VERSION == 7


def test_entry_points_validate_their_arguments():
    """Pointers, colour counts and sizes are checked before anything reaches a device: ML_E_BADARG (-1) and the reason."""
    from masklab_hip import _lib
    lib = _lib.load()
    cols = (ctypes.c_float * 48)()
    a, d, m, s, o, t = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000

    def err():
        return lib.ml_last_error()

    assert lib.ml_serving_visualize_u8(None, d, m, s, o, t, cols, 5, 0.3, cols, 3, 0.3, 1, 1, 14, 14, 8, 8, None) == -1
    assert b"null pointer" in err()
    assert lib.ml_serving_visualize_u8(a, d, m, s, o, None, cols, 5, 0.3, cols, 3, 0.3, 1, 1, 14, 14, 8, 8, None) == -1
    assert b"null pointer" in err()
    for ki, ks in ((0, 3), (17, 3), (5, 0), (5, 17)):
        assert lib.ml_serving_visualize_u8(a, d, m, s, o, t, cols, ki, 0.3, cols, ks, 0.3, 1, 1, 14, 14, 8, 8, None) == -1
        assert b"1 <= K <= 16" in err()
    assert lib.ml_serving_visualize_u8(a, d, m, s, o, t, None, 5, 0.3, cols, 3, 0.3, 1, 1, 14, 14, 8, 8, None) == -1
    assert b"null colour table" in err()
    for dims in ((0, 1, 14, 14, 8, 8), (1, -1, 14, 14, 8, 8), (1, 1, 0, 14, 8, 8), (1, 1, 14, 14, -8, 8), (1, 1, 14, 14, 8, 0)):
        assert lib.ml_serving_visualize_u8(a, d, m, s, o, t, cols, 5, 0.3, cols, 3, 0.3, *dims, None) == -1
        assert b"bad dims" in err()
    assert lib.ml_serving_visualize_u8(a, d, m, s, s + 64, t, cols, 5, 0.3, cols, 3, 0.3, 1, 1, 14, 14, 8, 8, None) == -1
    assert b"overlaps" in err()                                      # the output inside the semantic map
    assert lib.ml_serving_visualize_u8(a, d, m, s, a + 3, t, cols, 5, 0.3, cols, 3, 0.3, 1, 1, 14, 14, 8, 8, None) == -1
    assert b"only out == images" in err()
    assert lib.ml_draw_boxes_u8(None, d, o, 1, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ml_draw_boxes_u8(a, d, o, 1, -1, 8, 8, None) == -1 and b"bad dims" in err()
    assert lib.ml_draw_boxes_u8(a, d, a + 1, 1, 1, 8, 8, None) == -1 and b"only out == images" in err()
    assert lib.ml_draw_instance_u8(a, d, None, o, cols, 5, 0.3, 1, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ml_draw_instance_u8(a, d, m, o, cols, 17, 0.3, 1, 1, 8, 8, None) == -1 and b"1 <= K <= 16" in err()
    assert lib.ml_draw_instance_u8(a, d, m, o, cols, 5, 0.3, 1, 1, -8, 8, None) == -1 and b"bad dims" in err()
    assert lib.ml_draw_segmentation_u8(a, None, 0, o, cols, 3, 0.3, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ml_draw_segmentation_u8(a, s, 0, o, cols, 0, 0.3, 1, 8, 8, None) == -1 and b"1 <= K <= 16" in err()
    assert lib.ml_draw_segmentation_u8(a, s, 0, o, cols, 3, 0.3, 1, 8, -8, None) == -1 and b"bad dims" in err()


def test_registry_and_configs():
    from masklab_hip import get_custom_objects
    from masklab_hip.layers import DrawBoxes, DrawInstance, DrawSegmentation
    reg = get_custom_objects()
    assert reg["DrawBoxes"] is DrawBoxes and reg["DrawInstance"] is DrawInstance and reg["DrawSegmentation"] is DrawSegmentation
    for cls in (DrawInstance, DrawSegmentation):
        cfg = cls([[1, 2, 3]], 0.25).get_config()
        assert cfg["colors"] == [[1, 2, 3]] and cfg["alpha"] == 0.25
        assert cls([[1, 2, 3]]).alpha == .3
    assert "name" in DrawBoxes().get_config()


def test_serving_output_names():
    from masklab_hip import ModelConfiguration, retinamasklab as R

    class _Deploy:
        model = None

    cfg = ModelConfiguration()
    plain = R.construct_serving_network(cfg, _Deploy())
    assert plain.output_names == ['summarize'] and not plain.visualize
    vis = R.construct_serving_network(cfg, _Deploy(), visualize=True)
    assert vis.output_names == ['visualize', 'summarize']
    assert vis.draw_instance.colors == cfg.postprocess.instance_colors and vis.draw_instance.alpha == cfg.postprocess.instance_alpha
    assert vis.draw_segmentation.colors == cfg.postprocess.semantic_colors
    assert vis.draw_segmentation.alpha == cfg.postprocess.semantic_alpha
    assert R.ServingModel(cfg, _Deploy(), visualize=True).output_names == ['visualize', 'summarize']
