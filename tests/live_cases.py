"""Geometry of the fixed-capacity (`live`) test cases, in plain numpy: which RoI slots exist, how the row tiles of a
`live` launch fall over them, and which output rows a kernel promised not to write.

A fixed-capacity batch is `periods` images of `period` RoI slots, each slot a map of `hw` pixel rows; slot s exists iff
s % period < max(1, live) (include/masklab_hip.h: ml_conv2d_desc.live, ml_gn_desc.live, ml_deconv_out_problem.live).  The
implicit-GEMM conv and the mask-head tail work on tiles of BM consecutive rows and skip a tile all of whose slots are dead;
everything here is found by walking the rows, so it shares nothing with the kernels' own predicates.
tests/test_live_cases_cpu.py checks that the shapes below contain every tile class; tests/test_gpu_live_slots.py uses them."""
import numpy as np

DEAD, DEAD_PARTIAL = "wholly dead", "wholly dead, partial"
DEAD_LIVE_DEAD = "dead | live | dead"          # starts and ends in dead slots, slot 0 of the next image in between
# ... and the first slot's number is not above the last one's: a tile of more slots than an image has.  A predicate that
# compares slot numbers only (first <= last, first dead) takes it for a run of dead slots of ONE image and skips it.
DEAD_LIVE_DEAD_WRAPPED = "dead | live | dead, first slot <= last slot"
DEAD_TO_LIVE, LIVE_TO_DEAD = "dead -> live", "live -> dead"
LIVE, LIVE_PARTIAL = "wholly live", "wholly live, partial"
LIVE_DEAD_LIVE = "live | dead | live"          # (never skipped, never wholly written: no test depends on it)
REQUIRED_CLASSES = frozenset({DEAD, DEAD_PARTIAL, DEAD_LIVE_DEAD, DEAD_LIVE_DEAD_WRAPPED, DEAD_TO_LIVE, LIVE_TO_DEAD, LIVE,
                              LIVE_PARTIAL})

BM = 128                                       # rows of a tile of the generic conv and of the tail kernel
PERIODS = 3                                    # images per case
# (crop size, RoI slots per image).  7 x 7 at 3 slots is the one shape here whose 128-row tiles hold more slots (up to 4) than
# an image: only there can a tile start in a dead slot and end in a dead slot of the same or a higher number of the next image.
SHAPES = (((7, 7), 4), ((6, 10), 5), ((14, 14), 4), ((7, 7), 3))


def live_sweep(period):
    """The values of *live every kernel is run with: 0 behaves as 1, the last two make every slot live."""
    return (0, 1, 2, period - 1, period, period + 3)


def live_slots(period, live, periods):
    """bool [periods * period]: slot s exists."""
    lim = max(1, live)
    return np.array([s % period < lim for s in range(periods * period)], dtype=bool)


def live_rows(hw, period, live, periods):
    """bool [periods * period * hw]: the row belongs to a slot that exists."""
    return np.repeat(live_slots(period, live, periods), hw)


def _tiles(hw, period, live, periods, bm):
    """(first row, rows that exist, slot number inside its image of every row) of each tile."""
    rows = live_rows(hw, period, live, periods)
    slot = np.repeat(np.tile(np.arange(period), periods), hw)
    for m0 in range(0, len(rows), bm):
        yield m0, rows[m0:m0 + bm], slot[m0:m0 + bm]


def _class_of(t, slot, bm):
    partial = len(t) < bm
    if not t.any():
        return DEAD_PARTIAL if partial else DEAD
    if t.all():
        return LIVE_PARTIAL if partial else LIVE
    if not t[0] and not t[-1]:
        return DEAD_LIVE_DEAD_WRAPPED if slot[0] <= slot[-1] else DEAD_LIVE_DEAD
    if t[0] and t[-1]:
        return LIVE_DEAD_LIVE
    return LIVE_TO_DEAD if t[0] else DEAD_TO_LIVE


def tile_classes(hw, period, live, periods=PERIODS, BM=BM):
    """The set of classes the BM-row tiles of periods * period * hw rows fall into."""
    return {_class_of(t, slot, BM) for _, t, slot in _tiles(hw, period, live, periods, BM)}


def keep_rows(hw, period, live, periods=PERIODS, BM=BM):
    """bool [rows]: the row lies in a tile all of whose slots are dead -- the kernel stores nothing there, so the row must
    still hold what the output held before the launch.  (Dead rows inside a tile that runs are unconstrained.)"""
    keep = np.zeros(periods * period * hw, dtype=bool)
    for m0, t, _ in _tiles(hw, period, live, periods, BM):
        if not t.any():
            keep[m0:m0 + len(t)] = True
    return keep


def cases(BM=BM):
    """(hw rows, crop size, period, live, keep_rows) of every shape and every value of the sweep."""
    for crop, period in SHAPES:
        hw = crop[0] * crop[1]
        for live in live_sweep(period):
            yield hw, crop, period, live, keep_rows(hw, period, live, PERIODS, BM)
