"""The geometry the fixed-capacity (`live`) GPU tests stand on (tests/live_cases.py), checked without a GPU: the crop
shapes, with three images and the sweep of *live, put every kind of 128-row tile in front of the kernels' skip predicates
-- in particular the tile that starts and ends in dead slots with the live slot 0 of the next image in between, which a
predicate on slot numbers alone skips.  A condition on the chosen shapes, not a measurement: change a shape and this
must still pass."""
import numpy as np

import live_cases as LC


def _classes(crop, period, live, BM=LC.BM):
    return LC.tile_classes(crop[0] * crop[1], period, live, LC.PERIODS, BM)


def test_the_shapes_contain_every_tile_class():
    seen = set()
    for crop, period in LC.SHAPES:
        for live in LC.live_sweep(period):
            seen |= _classes(crop, period, live)
    assert LC.REQUIRED_CLASSES <= seen, LC.REQUIRED_CLASSES - seen


def test_where_each_class_comes_from():
    c1, c2 = _classes((7, 7), 4, 1), _classes((7, 7), 4, 2)
    assert {LC.DEAD, LC.DEAD_LIVE_DEAD, LC.LIVE_TO_DEAD} <= c1        # 49-row crops: a tile spans three or four slots
    assert LC.DEAD_TO_LIVE in c2
    assert LC.DEAD_PARTIAL in c1 and LC.DEAD_PARTIAL in c2            # rows 512 .. 587: slots 10 and 11 of 12
    assert LC.LIVE in _classes((14, 14), 4, 2)                        # 392 live rows in a run: whole tiles inside
    for crop, period in LC.SHAPES:
        for live in (period, period + 3):                            # every slot live
            assert _classes(crop, period, live) <= {LC.LIVE, LC.LIVE_PARTIAL}
        assert LC.LIVE_PARTIAL in _classes(crop, period, period)
        assert _classes(crop, period, 0) == _classes(crop, period, 1)


def test_only_the_three_slot_shape_has_the_tile_a_slot_number_predicate_skips():
    """7 x 7 crops, 3 slots per image: rows 128 .. 255 hold slots 2 | 0 1 2 -- first and last slot dead and EQUAL, the live
    slot 0 of the next image in between.  At 4 or 5 slots per image no 128-row tile of these crops holds more slots than an
    image, so the first slot's number is always above the last one's there."""
    for crop, period in LC.SHAPES:
        found = any(LC.DEAD_LIVE_DEAD_WRAPPED in _classes(crop, period, live) for live in LC.live_sweep(period))
        assert found == ((crop, period) == ((7, 7), 3)), (crop, period)
    assert LC.DEAD_LIVE_DEAD_WRAPPED in _classes((7, 7), 3, 1) and LC.DEAD_LIVE_DEAD_WRAPPED in _classes((7, 7), 3, 2)
    rows = LC.live_rows(49, 3, 1, LC.PERIODS)[128:256]
    assert not rows[0] and not rows[-1] and rows[19:68].all() and rows.sum() == 49        # slot 3 = slot 0 of image 1
    assert 7 * 7 * 3 >= LC.BM                                       # (the library wants one tile of rows per image)


def test_the_256_row_case():
    """14 x 14 crops at 4 slots per image on 256-row tiles (the split-operand conv's large tile)."""
    c1 = LC.tile_classes(196, 4, 1, 84, 256)
    c2 = LC.tile_classes(196, 4, 2, 84, 256)
    assert {LC.DEAD, LC.DEAD_LIVE_DEAD, LC.LIVE_TO_DEAD} <= c1
    assert {LC.DEAD_TO_LIVE, LC.LIVE} <= c2


def test_keep_rows_are_the_rows_of_wholly_dead_tiles():
    for hw, crop, period, live, keep in LC.cases():
        rows = LC.live_rows(hw, period, live, LC.PERIODS)
        assert keep.shape == rows.shape == (LC.PERIODS * period * hw,)
        assert not (keep & rows).any()                                # no live row is ever asked to keep the canary
        for m0 in range(0, len(rows), LC.BM):
            t = slice(m0, m0 + LC.BM)
            assert keep[t].all() == (not rows[t].any()) and keep[t].any() == keep[t].all()
        if live >= period:
            assert not keep.any()


def test_slot_rule():
    np.testing.assert_array_equal(LC.live_slots(4, 0, 2), [1, 0, 0, 0, 1, 0, 0, 0])
    np.testing.assert_array_equal(LC.live_slots(4, 3, 2), [1, 1, 1, 0, 1, 1, 1, 0])
    np.testing.assert_array_equal(LC.live_slots(3, 9, 1), [1, 1, 1])
    np.testing.assert_array_equal(LC.live_rows(2, 2, 1, 1), [1, 1, 0, 0])
