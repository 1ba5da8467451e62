"""Tile selection restated in numpy (include/rrt.h: rrt_mark_tiles, rrt_select_tiles), and the seeded planes of its tests.

The restatement is the definition read literally: an element is an unsigned integer of its size; the four tests are comparisons of those integers; the verdicts
of a region are padded into the frame, the frame into whole tiles, and a tile is marked when any verdict of its [8][8][per_pixel] block is set
(`passes`, `marks_of`, `list_of`).  tests/test_tile_restatement.py checks it against answers written by hand.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np

from bitwise import bits

KINDS = ("nonzero", "range", "set", "differs")
PLANE_KINDS = ((1, 1), (1, 4), (4, 1), (4, 4), (8, 1), (8, 4))          # (elem_bytes, per_pixel): every combination the library takes
ACCEPTS = {"nonzero": PLANE_KINDS, "differs": PLANE_KINDS, "range": ((4, 1), (4, 4)), "set": ((4, 1), (4, 4))}
FRAMES = ((203, 117), (64, 48), (9, 9), (8, 8), (1, 1), (128, 128))
REGIONS = (None, (13, 50, 77, 31), (5, 3, 1, 1), (200, 0, 3, 2), (8, 8, 8, 8))
GUARD = 0xA5                                                            # what marks and lists hold before a call, and behind their end afterwards
DTYPES = {1: np.uint8, 4: np.uint32, 8: np.float64}
# doubles whose bits matter: -0.0, two NaNs that differ in their payload only, the smallest subnormal
SPECIAL_DOUBLES = np.array([0x8000000000000000, 0x7FF8000000000001, 0x7FF8000000000002, 0x0000000000000001], np.uint64).view(np.float64)


def tiles_of(width, height):
    return (width + 7) // 8, (height + 7) // 8


def region_of(width, height, region):
    return (0, 0, width, height) if region is None else tuple(region)


def regions_in(width, height):
    """The regions of REGIONS that lie inside a frame."""
    return tuple(r for r in REGIONS if r is None or (r[0] + r[2] <= width and r[1] + r[3] <= height))


def set_words(values):
    """The 256-bit set of rrt_tile_test as eight words."""
    words = np.zeros(8, np.uint32)
    for v in values:
        assert 0 <= v < 256, f"value {v} of a set"
        words[v >> 5] |= np.uint32(1 << (v & 31))
    return words


def passes(kind, a, b=None, lo=0, hi=0, values=()):
    """[...] bool: the verdict of every element of the plane a (and b), read as unsigned integers."""
    x = bits(a)
    if kind == "nonzero":
        return x != 0
    if kind == "differs":
        assert np.asarray(b).shape == np.asarray(a).shape and np.asarray(b).dtype.itemsize == np.asarray(a).dtype.itemsize, "a and b differ in layout"
        return x != bits(b)
    assert x.dtype == np.uint32, f"{kind} reads 4-byte elements, not {x.dtype}"
    if kind == "range":
        return (x >= np.uint32(lo)) & (x < np.uint32(hi))
    if kind == "set":
        words = set_words(values)
        small = x < 256
        idx = np.where(small, x, 0)
        return small & (((words[idx >> 5] >> (idx & 31)) & 1) != 0)
    raise AssertionError(f"unknown kind {kind!r}")


def marks_of(verdicts, width, height, region=None):
    """[tiles_y][tiles_x] uint8 from the verdicts [h][w] or [h][w][per_pixel] of a region: pad, then any over [ty][8][tx][8][per_pixel]."""
    x0, y0, w, h = region_of(width, height, region)
    v = np.asarray(verdicts, bool)
    v = v.reshape(v.shape[0], v.shape[1], -1)
    assert v.shape[:2] == (h, w), f"verdicts of {v.shape[:2]} for a region of {(h, w)}"
    tx, ty = tiles_of(width, height)
    frame = np.zeros((ty * 8, tx * 8, v.shape[2]), bool)
    frame[y0:y0 + h, x0:x0 + w] = v
    return frame.reshape(ty, 8, tx, 8, v.shape[2]).any(axis=(1, 3, 4)).astype(np.uint8)


def list_of(marks):
    """The ascending numbers ty * tiles_x + tx of the marked tiles."""
    return np.flatnonzero(np.asarray(marks).reshape(-1)).astype(np.uint32)


# ------------------------------------------------------------------ seeded planes
def plane_shape(h, w, per_pixel):
    return (h, w) if per_pixel == 1 else (h, w, 4)


def sparse_plane(seed, h, w, elem_bytes, per_pixel, density=0.01):
    """A plane of zeros in which about `density` of the elements hold something: small values, all-ones, and for doubles the SPECIAL_DOUBLES (-0.0 among them).
    With the default density about half of the 8x8 tiles of a framebuffer hold something."""
    rng = np.random.default_rng(seed)
    shape = plane_shape(h, w, per_pixel)
    on = rng.random(shape) < density
    if elem_bytes == 8:
        pool = np.concatenate([SPECIAL_DOUBLES, np.array([1.5, -2.0])])
        return np.where(on, pool[rng.integers(0, len(pool), shape)], 0.0).astype(np.float64)
    dtype = DTYPES[elem_bytes]
    pool = np.array([1, 2, 128, np.iinfo(dtype).max], dtype)
    return np.where(on, pool[rng.integers(0, len(pool), shape)], 0).astype(dtype)


def material_like_plane(seed, h, w, per_pixel, pool, background=0.0):
    """A uint32 plane of blobs: every 5x7-pixel cell holds one value of `pool` (as a material plane holds runs of one material); with `background`, that share
    of the cells holds pool[0]."""
    rng = np.random.default_rng(seed)
    cells_shape = ((h + 4) // 5, (w + 6) // 7)
    pick = np.where(rng.random(cells_shape) < background, 0, rng.integers(0, len(pool), cells_shape))
    cells = np.asarray(pool, np.uint32)[pick]
    px = np.repeat(np.repeat(cells, 5, 0), 7, 1)[:h, :w]
    return np.ascontiguousarray(px if per_pixel == 1 else np.repeat(px[:, :, None], 4, 2))


def changed_copy(seed, a, density=0.01):
    """(b, changed): a copy of plane a in which about `density` of the elements differ from a in their bits -- one bit flipped, which turns 0.0 into -0.0 or a
    NaN into the NaN of another payload where it hits those."""
    rng = np.random.default_rng(seed)
    x = bits(a).copy()
    changed = rng.random(x.shape) < density
    flip = x.dtype.type(1) << rng.integers(0, 8 * x.dtype.itemsize, x.shape).astype(x.dtype)
    x[changed] ^= flip[changed]
    return x.view(np.asarray(a).dtype), changed


def differing_doubles(seed, h, w, per_pixel):
    """(a, b): float64 planes that differ in about 1 % of their elements, each time in the bits alone where the values allow it: 0.0 against -0.0, a NaN against
    the NaN of another payload, any other value against its neighbour in the last bit.  The NaNs that stay are the same NaN on both sides."""
    a = sparse_plane(seed, h, w, 8, per_pixel, density=0.03)
    x = bits(a)
    rng = np.random.default_rng(seed + 1)
    change = rng.random(x.shape) < 0.01
    nan1, nan2 = bits(SPECIAL_DOUBLES[1:3])
    y = np.where(change, np.where(x == 0, np.uint64(1) << np.uint64(63), np.where(x == nan1, nan2, x ^ np.uint64(1))), x)
    return a, y.view(np.float64)


def one_element_per_tile(width, height, elem_bytes, per_pixel, step=37, skip_every=None):
    """A plane of a whole frame of whole tiles in which tile t's only non-zero element sits at in-tile position (step * t) mod positions, positions =
    64 * per_pixel in the order [row][column][sub-sample]; with skip_every, every skip_every-th tile (t % skip_every == 0) holds nothing.  (plane, marks)"""
    assert width % 8 == 0 and height % 8 == 0, "whole tiles only"
    tx, ty = tiles_of(width, height)
    positions = 64 * per_pixel
    a = np.zeros((height, width, per_pixel), DTYPES[elem_bytes])
    marks = np.ones((ty, tx), np.uint8)
    for t in range(tx * ty):
        if skip_every and t % skip_every == 0:
            marks[t // tx, t % tx] = 0
            continue
        p = (step * t) % positions
        pix, sub = divmod(p, per_pixel)
        a[(t // tx) * 8 + pix // 8, (t % tx) * 8 + pix % 8, sub] = 1
    return np.ascontiguousarray(a.reshape(plane_shape(height, width, per_pixel))), marks
