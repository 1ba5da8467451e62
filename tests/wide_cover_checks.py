"""The wide boxes and simple waves of a frame restated in numpy: csrc/coverage_rule.hpp (coverage_rect_waves, coverage_is_wide, kMaxWide) and what csrc/coverage.hip
makes of them -- the list, the mask `fine`, the simple waves.  On top of tests/coverage_checks.py, whose rectangles are the header's bit for bit;
tests/test_wide_cover_restatement.py holds these functions to the header compiled on the host (tests/wide_cover_model.cpp), and tests/test_gpu_wide_cover.py
compares the library's counts with them.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np

import coverage_checks as cc

MAX_WIDE, WIDE_MIN_WAVES, WIDE_FRAME_SHARE = 16, 16, 128                 # kMaxWide, kWideMinWaves, kWideFrameShare


def rect_waves(rects):
    """coverage_rect_waves: the waves of every rectangle, 0 for an empty one (int64)."""
    w = (rects.bx1.astype(np.int64) - rects.bx0 + 1) * (rects.by1.astype(np.int64) - rects.by0 + 1)
    return np.where(cc.some(rects), w, 0)


def wide_min_waves(frame):
    """The smallest number of waves a wide rectangle of this frame covers: the floor, or the frame's share rounded up."""
    frame_waves = 4 * frame.tiles_x * frame.tiles_y
    return max(WIDE_MIN_WAVES, -(-frame_waves // WIDE_FRAME_SHARE))


def is_wide(frame, rects, root_end, slots=None):
    """coverage_is_wide per box; slots: the list slot of every box (default: its index)."""
    slots = np.arange(len(rects.bx0)) if slots is None else np.asarray(slots)
    waves = rect_waves(rects)
    return (slots < root_end) & (waves >= WIDE_MIN_WAVES) & (waves * WIDE_FRAME_SHARE >= 4 * frame.tiles_x * frame.tiles_y) & ~rects.whole


def classify(frame, rects, root_end, slots=None, order=None):
    """What the pass makes of the boxes of a frame.  order: the sequence in which the boxes ask for a record (default: as given); the first MAX_WIDE wide ones are
    listed, every other box that holds a wave is ordinary and goes into `fine`.  A box that reaches the whole frame sets every bit of both masks.
    Returns a dict: wide, listed (bool per box), mask, fine, simple ([waves_y, waves_x] bool), n_wide (listed boxes), n_simple, per_simple (listed boxes that
    reach each simple wave)."""
    n = len(rects.bx0)
    wide = is_wide(frame, rects, root_end, slots)
    order = np.arange(n) if order is None else np.asarray(order)
    listed = np.zeros(n, bool)
    listed[order[wide[order]][:MAX_WIDE]] = True
    mask = cc.mask_of_many(frame, rects)
    sel = lambda keep: cc.Rects(*(np.where(keep, v, e) for v, e in zip(rects[:4], (0, -1, 0, -1))), rects.whole & keep)
    fine = cc.mask_of_many(frame, sel(~listed))
    simple = mask & ~fine
    count = np.zeros(mask.shape, np.int64)
    for i in np.flatnonzero(listed):
        count[rects.by0[i]:rects.by1[i] + 1, rects.bx0[i]:rects.bx1[i] + 1] += 1
    assert not (simple & (count == 0)).any(), "a simple wave that no listed box reaches"
    return dict(wide=wide, listed=listed, mask=mask, fine=fine, simple=simple, n_wide=int(listed.sum()), n_simple=int(simple.sum()), per_simple=count[simple])


def approx_boxes(pos, pad):
    """(c, h) in fp32 of the triangles' bounding boxes padded by `pad`: close to the device's records, enough to choose scenes and to count on the CPU."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    lo, hi = pos.min(1) - pad, pos.max(1) + pad
    return ((lo + hi) * 0.5).astype(np.float32), ((hi - lo) * 0.5 * (1.0 + 2.0 ** -20)).astype(np.float32)
