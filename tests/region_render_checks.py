"""Helpers of the tests of the fused frame of a region and of a device-resident tile list (include/rrt.h: rrt_render_region, rrt_render_tile_list_device): the
conditions under which a comparison of two frames shows anything, the comparison of a region with the crop of a frame, and the pixels a tile list names.

A comparison of white with white shows nothing, so every frame compared holds at least MIN_PIXELS pixels that are neither the background nor 0, and every
multi-pixel rectangle compared holds at least one, unless it is one of the two that test the frame's corners.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np

from bitwise import assert_same_bits
from gpu_checks import MIN_PIXELS, traced_rows
from surface_checks import traced_cols

MAX_TILE_LIST = 16777215                                  # RRT_MAX_TILE_LIST: (2^32 - 1) threads / 256 per entry
SENTINEL = 0xA5A5A5A5                                     # what a buffer holds before a call; no pixel has a top byte
WHITE = 0x00FFFFFF
CORNER_REGIONS = ((5, 3, 1, 1), (200, 0, 3, 2))           # one pixel; the top-right corner, untraced row and column included: exempt from the content rule


def content(frame):
    """The pixels that are neither the background nor 0: the ones that come out of a shaded hit."""
    frame = np.asarray(frame)
    return (frame != WHITE) & (frame != 0)


def assert_frame_has_content(frame, what, least=MIN_PIXELS):
    n = int(content(frame).sum())
    print(f"{what}: {n} of {frame.size} pixels are neither 0x00FFFFFF nor 0")
    assert n >= least, f"{what}: only {n} pixels are neither 0x00FFFFFF nor 0 (< {least})"
    return n


def crop(frame, region):
    x0, y0, w, h = region
    return frame[y0:y0 + h, x0:x0 + w]


def assert_region_has_content(frame, region, what, hit=None):
    """A rectangle of more than one pixel that is compared holds a pixel of content, unless it is a corner case -- or, with hit ([h][w] bool: a sub-sample of
    the pixel hits a triangle), unless the scene has no geometry there."""
    if tuple(region) in CORNER_REGIONS or region[2] * region[3] == 1:
        return
    if hit is not None and not crop(hit, region).any():
        print(f"{what}: region {tuple(region)} sees no geometry")
        return
    n = int(content(crop(frame, region)).sum())
    assert n >= 1, f"{what}: region {tuple(region)} holds {n} pixels that are neither 0x00FFFFFF nor 0"


def assert_region_is_crop(rt, frame, w, h, region, what, hit=None):
    """render_region of the region (None: the whole frame) is the crop of `frame`, rt's own render(w, h), bit for bit."""
    r = (0, 0, w, h) if region is None else tuple(region)
    assert_region_has_content(frame, r, what, hit)
    assert_same_bits(rt.render_region(w, h, region), crop(frame, r), f"{what}: render_region {r} vs the crop of render", np.uint32)


def traced_count(region, w, h):
    """The traced pixels inside a region, restated from the rows and columns the reference writes."""
    x0, y0, rw, rh = region
    mask = np.zeros((h, w), bool)
    mask[np.ix_(traced_rows(h), traced_cols(w))] = True
    return int(mask[y0:y0 + rh, x0:x0 + rw].sum())


def tiles_of(w, h):
    return (w + 7) // 8, (h + 7) // 8


def listed_pixels(w, h, tiles):
    """[h][w] bool: the pixels of the frame inside a tile the list names; ids that name no tile of the frame name nothing."""
    tx_n, ty_n = tiles_of(w, h)
    mask = np.zeros((h, w), bool)
    for t in np.asarray(tiles, np.uint64):
        t = int(t)
        if t < tx_n * ty_n:
            tx, ty = t % tx_n, t // tx_n
            mask[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    return mask


def assert_listed_tiles_only(got, frame, tiles, what):
    """got, a buffer that held SENTINEL everywhere, equals `frame` inside the listed tiles and still holds SENTINEL outside them.  Returns the listed pixels."""
    h, w = frame.shape
    mask = listed_pixels(w, h, tiles)
    assert_same_bits(np.asarray(got, np.uint32).reshape(h, w), np.where(mask, frame, np.uint32(SENTINEL)).astype(np.uint32), what, np.uint32)
    return int(mask.sum())
