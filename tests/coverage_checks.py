"""The coverage rule restated for any frame, in numpy f64: csrc/coverage_rule.hpp (coverage_frame, coverage_rect), the marking of csrc/coverage.hip as a plain
fill of rectangles, and coverage_state of csrc/frames.cpp.  Every function follows its original operation for operation, in the original's order: the library
is built with -ffp-contract=off on host and device, so these give the header's BITS, and tests/test_coverage_restatement.py holds them to that against the header
compiled on the host (tests/coverage_rule_model.cpp).  The GPU tests then compare the kernel's mask with mask_of(frame_of(..), rects_of(..)) bit for bit.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import math
from collections import namedtuple

import numpy as np

COORD_REL, ABS_PIX, REL_PIX = 1e-12, 1e-6, 1e-9              # kCoverCoordRel, kCoverAbsPix, kCoverRelPix
MAX_RESIDUAL, MAX_COND = 2.0 ** -43, 256.0                   # kCoverMaxResidual, kCoverMaxCond
MIN_WAVES, MAX_SLOTS_PER_WAVE = 49152, 4                     # frames.cpp: kCoverMinWaves, kCoverMaxSlotsPerWave
K_BLOCK, K_OWN_ITEMS = 256, 64                               # coverage.hip: kBlock, kOwnItems

Frame = namedtuple("Frame", "inv eye kx ky half_w top tiles_x tiles_y")      # CoverageFrame; inv: 3 rows of 3 floats
Rects = namedtuple("Rects", "bx0 bx1 by0 by1 whole")                         # int32 arrays, one entry per box; whole: coverage_is_whole_frame


# ------------------------------------------------------------------ coverage_frame
def frame_from_scales(width, height, x_scale, y_scale, z_value, right, up, forward, eye):
    """coverage_frame: the Frame, or None where the header returns false.  Python floats are f64 and every operation below is rounded on its own."""
    width, height = int(width), int(height)
    x_scale, y_scale, z_value = float(x_scale), float(y_scale), float(z_value)
    r, u, f, eye = ([float(v) for v in a] for a in (right, up, forward, eye))
    M = [[r[0], u[0], f[0]], [r[1], u[1], f[1]], [r[2], u[2], f[2]]]
    det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])
    if not (abs(det) > 0.0) or not math.isfinite(det):
        return None
    adj = [[M[1][1] * M[2][2] - M[1][2] * M[2][1], M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][1] * M[1][2] - M[0][2] * M[1][1]],
           [M[1][2] * M[2][0] - M[1][0] * M[2][2], M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][2] * M[1][0] - M[0][0] * M[1][2]],
           [M[1][0] * M[2][1] - M[1][1] * M[2][0], M[0][1] * M[2][0] - M[0][0] * M[2][1], M[0][0] * M[1][1] - M[0][1] * M[1][0]]]
    with np.errstate(all="ignore"):
        inv = [[float(np.float64(adj[i][j]) / np.float64(det)) for j in range(3)] for i in range(3)]      # (numpy's division: inf and NaN instead of an exception)
    fmax = lambda a, b: b if a != a else a if b != b else max(a, b)                                     # C's fmax: a NaN operand is ignored
    norm_m = norm_i = residual = 0.0
    for i in range(3):
        norm_m = fmax(norm_m, abs(M[i][0]) + abs(M[i][1]) + abs(M[i][2]))
        norm_i = fmax(norm_i, abs(inv[i][0]) + abs(inv[i][1]) + abs(inv[i][2]))
        for j in range(3):
            p = (inv[i][0] * M[0][j] + inv[i][1] * M[1][j]) + inv[i][2] * M[2][j]
            residual = fmax(residual, abs(p - (1.0 if i == j else 0.0)))
    if not (residual <= MAX_RESIDUAL) or not (norm_m * norm_i <= MAX_COND):
        return None
    with np.errstate(all="ignore"):
        kx, ky = float(np.float64(z_value) / np.float64(x_scale)), float(np.float64(z_value) / np.float64(y_scale))
    if not (z_value > 0.0) or not math.isfinite(kx) or not math.isfinite(ky):
        return None
    if not all(math.isfinite(v) for v in eye):
        return None
    return Frame(tuple(tuple(row) for row in inv), tuple(eye), kx, ky, float(width // 2), float(height - height // 2), (width + 7) // 8, (height + 7) // 8)


def scales_of(width, height, viewport):
    """frames.cpp, frame_params: one division each."""
    vp_w, vp_h, vp_d = (float(v) for v in viewport)
    return vp_w / float(width), vp_h / float(height), vp_d


def frame_of(width, height, viewport, right, up, forward, eye):
    """The Frame of a width x height frame of a raytracer created with `viewport`, in the pose (right, up, forward, eye); None where the pass is off ("camera")."""
    return frame_from_scales(width, height, *scales_of(width, height, viewport), right, up, forward, eye)


# ------------------------------------------------------------------ coverage_rect
def box_records(tboxes):
    """(c, h) as float32 [n, 3] of the bytes of RRT_BUF_TBOXES: 32-byte records, centre then half-extent at floats 0..2 and 3..5; behind the slots lie eight
    spare records that are never read as boxes of triangles."""
    rec = np.frombuffer(np.ascontiguousarray(tboxes).tobytes(), np.float32).reshape(-1, 8)[:-8]
    return rec[:, 0:3], rec[:, 3:6]


def rects_of(frame, c, h=None):
    """coverage_rect for every box (c, h float32 [n, 3]; or rects_of(frame, tbox_records) with the bytes of RRT_BUF_TBOXES)."""
    if h is None:
        c, h = box_records(c)
    c32, h32 = np.asarray(c, np.float32).reshape(-1, 3), np.asarray(h, np.float32).reshape(-1, 3)
    n = len(c32)
    c64, h64 = c32.astype(np.float64), h32.astype(np.float64)
    inv, eye = np.asarray(frame.inv, np.float64), np.asarray(frame.eye, np.float64)
    ainv = np.abs(inv)
    wx, wy = 2.0 * float(frame.tiles_x), 2.0 * float(frame.tiles_y)
    empty = (h32 < 0).any(1)
    whole = (h32 >= np.finfo(np.float32).max).any(1)                             # unbounded along an axis: the index's mark, not a length
    xlo = np.full(n, np.inf); xhi = np.full(n, -np.inf); ylo = np.full(n, np.inf); yhi = np.full(n, -np.inf)
    with np.errstate(all="ignore"):
        for k in range(8):
            sign = np.array([1.0 if (k >> j) & 1 else -1.0 for j in range(3)])
            d = (c64 + sign * h64) - eye                                         # (c + (-h) is c - h in every bit)
            ad = np.abs(d)
            a = (inv[0, 0] * d[:, 0] + inv[0, 1] * d[:, 1]) + inv[0, 2] * d[:, 2]
            b = (inv[1, 0] * d[:, 0] + inv[1, 1] * d[:, 1]) + inv[1, 2] * d[:, 2]
            g = (inv[2, 0] * d[:, 0] + inv[2, 1] * d[:, 1]) + inv[2, 2] * d[:, 2]
            s = np.zeros(n)
            for i in range(3):
                s = s + ((ainv[i, 0] * ad[:, 0] + ainv[i, 1] * ad[:, 1]) + ainv[i, 2] * ad[:, 2])
            E = COORD_REL * s
            g_lo = g - E
            front = g_lo > 0.0
            whole |= ~front
            rg, rg_lo = 1.0 / g, 1.0 / g_lo
            qa, qb = a * rg, b * rg
            xd, yd = qa * frame.kx, qb * frame.ky
            mx = (ABS_PIX + REL_PIX * np.abs(xd)) + (2.0 * abs(frame.kx)) * ((np.abs(qa) * E + E) * rg_lo)
            my = (ABS_PIX + REL_PIX * np.abs(yd)) + (2.0 * abs(frame.ky)) * ((np.abs(qb) * E + E) * rg_lo)
            finite = (xd - mx > -np.inf) & (xd + mx < np.inf) & (yd - my > -np.inf) & (yd + my < np.inf)
            whole |= front & ~finite
            # fmin / fmax ignore a NaN; such a corner makes the box `whole` anyway, so its value only has to stay out of the way
            upd = front & finite
            xlo = np.where(upd, np.minimum(xlo, xd - mx), xlo); xhi = np.where(upd, np.maximum(xhi, xd + mx), xhi)
            ylo = np.where(upd, np.minimum(ylo, yd - my), ylo); yhi = np.where(upd, np.maximum(yhi, yd + my), yhi)
        clamp = lambda x, lo, hi: np.where(x < lo, lo, np.where(x > hi, hi, x))
        ok = ~(whole | empty)
        z = lambda v: np.where(ok, v, 0.0)                                       # (the others are overwritten below)
        bx0 = clamp(np.ceil((z(xlo) + frame.half_w - 3.5) * 0.25), 0.0, wx).astype(np.int32)
        bx1 = clamp(np.floor((z(xhi) + frame.half_w) * 0.25), -1.0, wx - 1.0).astype(np.int32)
        by0 = clamp(np.ceil((frame.top - 3.0 - z(yhi)) * 0.25), 0.0, wy).astype(np.int32)
        by1 = clamp(np.floor((frame.top + 0.5 - z(ylo)) * 0.25), -1.0, wy - 1.0).astype(np.int32)
    whole &= ~empty
    last_x, last_y = np.int32(2 * frame.tiles_x - 1), np.int32(2 * frame.tiles_y - 1)
    bx0 = np.where(empty | whole, 0, bx0).astype(np.int32); by0 = np.where(empty | whole, 0, by0).astype(np.int32)
    bx1 = np.where(empty, -1, np.where(whole, last_x, bx1)).astype(np.int32); by1 = np.where(empty, -1, np.where(whole, last_y, by1)).astype(np.int32)
    is_whole = (bx0 == 0) & (by0 == 0) & (bx1 == last_x) & (by1 == last_y)       # coverage_is_whole_frame: also a rectangle that merely covers everything
    return Rects(bx0, bx1, by0, by1, is_whole)


def some(rects):
    """The boxes whose rectangle holds a wave."""
    return (rects.bx0 <= rects.bx1) & (rects.by0 <= rects.by1)


def mask_of(frame, rects):
    """[2 tiles_y, 2 tiles_x] bool: a whole-frame rectangle sets everything, any other fills its inclusive range."""
    mask = np.zeros((2 * frame.tiles_y, 2 * frame.tiles_x), bool)
    if (rects.whole & some(rects)).any():
        mask[:] = True
        return mask
    for i in np.flatnonzero(some(rects)):
        mask[rects.by0[i]:rects.by1[i] + 1, rects.bx0[i]:rects.bx1[i] + 1] = True
    return mask


def mask_of_many(frame, rects):
    """mask_of for scenes of very many boxes: the same fill as a 2-D difference array, no loop over the boxes."""
    wy, wx = 2 * frame.tiles_y, 2 * frame.tiles_x
    if (rects.whole & some(rects)).any():
        return np.ones((wy, wx), bool)
    k = some(rects)
    x0, x1, y0, y1 = (np.asarray(v[k], np.int64) for v in (rects.bx0, rects.bx1, rects.by0, rects.by1))
    acc = np.zeros((wy + 1, wx + 1), np.int64)
    np.add.at(acc, (y0, x0), 1); np.add.at(acc, (y1 + 1, x1 + 1), 1); np.add.at(acc, (y0, x1 + 1), -1); np.add.at(acc, (y1 + 1, x0), -1)
    return acc.cumsum(0).cumsum(1)[:wy, :wx] > 0


def boxes_reaching(rects, bx, by):
    """The indices of the boxes whose rectangle contains wave (bx, by)."""
    return np.flatnonzero((rects.bx0 <= bx) & (bx <= rects.bx1) & (rects.by0 <= by) & (by <= rects.by1))


def describe_difference(got, want, rects, limit=5):
    """Names the first differing waves of two masks and the boxes whose rectangles contain them."""
    bad = np.argwhere(got != want)
    lines = [f"{len(bad)} of {want.size} waves differ"]
    for by, bx in bad[:limit]:
        boxes = boxes_reaching(rects, bx, by)
        lines.append(f"wave (bx {bx}, by {by}): the kernel {'set' if got[by, bx] else 'left clear'}, the rule {'sets' if want[by, bx] else 'leaves clear'}; boxes that reach it: "
                     + (", ".join(f"#{i} x[{rects.bx0[i]}, {rects.bx1[i]}] y[{rects.by0[i]}, {rects.by1[i]}]" for i in boxes[:4]) or "none"))
    return "; ".join(lines)


# ------------------------------------------------------------------ coverage_state
def state_of(width, height, viewport, right, up, forward, eye, *, coverage=True, n_slots=0, no_cull=False, pad=1.0, suspects=0, cull_limit=np.float32(80.0)):
    """coverage_state (frames.cpp) in its order, as a name of COVERAGE_STATES: flag, the size bounds, no_cull, suspects, eye range, camera.  coverage: what the
    raytracer was created with (True, False or "always"); n_slots: the triangle slots (box records); pad: rrt_stats.filter_pad; suspects:
    rrt_stats.origin_plane_triangles; cull_limit: DevScene::cull_limit, the fp32 value of four times the scene's magnitude."""
    if not coverage:
        return "flag"
    tiles_x, tiles_y = (int(width) + 7) // 8, (int(height) + 7) // 8
    waves = 4 * tiles_x * tiles_y
    if coverage != "always" and (waves < MIN_WAVES or n_slots > MAX_SLOTS_PER_WAVE * waves):
        return "small_frame"
    if no_cull or not (pad > 0):
        return "no_cull"
    if suspects != 0:
        return "suspects"
    x_scale, y_scale, z_value = scales_of(width, height, viewport)
    limit = float(np.float32(cull_limit))
    a = (float(int(width) // 2) + 1.0) * abs(x_scale); b = (float(int(height) - int(height) // 2) + 1.0) * abs(y_scale); c = abs(z_value)
    for k in range(3):
        if not (abs(float(eye[k])) < limit):
            return "eye_range"
        if not (abs(float(right[k])) * a + abs(float(up[k])) * b + abs(float(forward[k])) * c < limit):
            return "eye_range"
    return "on" if frame_from_scales(width, height, x_scale, y_scale, z_value, right, up, forward, eye) is not None else "camera"


# ------------------------------------------------------------------ what a scene reaches in coverage_kernel and mark_word
def path_counters(frame, rects):
    """From the rectangles, by the kernel's own formulas: which paths of coverage_kernel and mark_word the boxes of a frame take.
      queued            boxes with tile_rows * words_per_row > kOwnItems (dealt over the block), and queued_256 those of at least 256 items
      split_rects       rectangles whose first and last word differ in some tile row
      two_row_words     (tile row, word) items whose word also holds tiles of another tile row
      bx0_odd / bx0_even / bx1_odd / bx1_even    the parities of the rectangle's first and last wave column
      bx0_odd_at_word_start / bx0_even_at_word_start     those parities among the rectangles whose first tile is the first tile of a word in some tile row
      bx1_odd_at_word_end / bx1_even_at_word_end         ... and whose last tile is the last tile of a word
      last_partial_word rectangles that end in the frame's last word where that word is not full
      whole             whole-frame boxes; blocks: 256-box blocks."""
    tiles_x, n_tiles = frame.tiles_x, frame.tiles_x * frame.tiles_y
    k = some(rects) & ~rects.whole
    bx0, bx1, by0, by1 = (np.asarray(v[k], np.int64) for v in (rects.bx0, rects.bx1, rects.by0, rects.by1))
    tile_rows = (by1 >> 1) - (by0 >> 1) + 1
    words_per_row = (((bx1 >> 1) - (bx0 >> 1)) >> 3) + 2
    items = tile_rows * words_per_row
    split = two_row = last_partial = 0
    at_start, at_end = [0, 0], [0, 0]
    for i in range(len(bx0)):
        ty = np.arange(by0[i] >> 1, (by1[i] >> 1) + 1)
        t0, t1 = ty * tiles_x + (bx0[i] >> 1), ty * tiles_x + (bx1[i] >> 1)
        split += bool(((t0 >> 3) != (t1 >> 3)).any())
        at_start[bx0[i] & 1] += bool(((t0 & 7) == 0).any()); at_end[bx1[i] & 1] += bool(((t1 & 7) == 7).any())
        for y, a, b in zip(ty, t0 >> 3, t1 >> 3):
            w = np.arange(a, b + 1)
            two_row += int((((w * 8) // tiles_x != y) | ((np.minimum(w * 8 + 7, n_tiles - 1)) // tiles_x != y)).sum())
        last_partial += bool(n_tiles % 8 != 0 and (t1[-1] >> 3) == (n_tiles - 1) >> 3)
    n = len(rects.bx0)
    return dict(boxes=n, some=int(k.sum()), queued=int((items > K_OWN_ITEMS).sum()), queued_256=int((items >= 256).sum()), split_rects=split, two_row_words=two_row,
                bx0_odd=int((bx0 & 1).sum()), bx0_even=int(((bx0 & 1) == 0).sum()), bx1_odd=int((bx1 & 1).sum()), bx1_even=int(((bx1 & 1) == 0).sum()),
                bx0_even_at_word_start=at_start[0], bx0_odd_at_word_start=at_start[1], bx1_even_at_word_end=at_end[0], bx1_odd_at_word_end=at_end[1],
                last_partial_word=last_partial,
                whole=int((rects.whole & some(rects)).sum()), blocks=(n + K_BLOCK - 1) // K_BLOCK)


def add_counters(total, c):
    for k, v in c.items():
        total[k] = total.get(k, 0) + v
    return total
