"""The numpy restatement of tile selection (tests/tile_checks.py) against answers written by hand, on a 9 x 9 frame: 2 x 2 tiles, of which tile 0 is whole, tile 1
is one column wide, tile 2 one row high and tile 3 a single pixel.  No GPU and no library: this is the yardstick of tests/test_gpu_tile_select.py."""
import numpy as np
import pytest

from tile_checks import (SPECIAL_DOUBLES, list_of, marks_of, material_like_plane, one_element_per_tile, passes, regions_in, set_words, sparse_plane, tiles_of,
                         changed_copy)

W = H = 9


def marks(*rows):
    return np.array(rows, np.uint8)


def test_the_tiles_of_a_frame():
    assert tiles_of(9, 9) == (2, 2) and tiles_of(8, 8) == (1, 1) and tiles_of(1, 1) == (1, 1) and tiles_of(203, 117) == (26, 15) and tiles_of(128, 128) == (16, 16)
    assert regions_in(9, 9) == (None, (5, 3, 1, 1)) and len(regions_in(203, 117)) == 5 and regions_in(1, 1) == (None,)


def test_nonzero_by_hand():
    a = np.zeros((H, W), np.uint8)
    assert (marks_of(passes("nonzero", a), W, H) == marks([0, 0], [0, 0])).all()
    a[7, 7] = 1                                             # the last pixel of the whole tile
    assert (marks_of(passes("nonzero", a), W, H) == marks([1, 0], [0, 0])).all()
    a[0, 8] = 200                                           # the one column of tile 1
    assert (marks_of(passes("nonzero", a), W, H) == marks([1, 1], [0, 0])).all()
    a[8, 8] = 255                                           # the one pixel of tile 3
    assert (marks_of(passes("nonzero", a), W, H) == marks([1, 1], [0, 1])).all()
    a[7, 7] = 0; a[8, 0] = 3                                # tile 0 empties, the one row of tile 2 fills
    m = marks_of(passes("nonzero", a), W, H)
    assert (m == marks([0, 1], [1, 1])).all() and m.dtype == np.uint8
    assert list_of(m).tolist() == [1, 2, 3] and list_of(m).dtype == np.uint32


def test_sub_samples_and_doubles_by_hand():
    a = np.zeros((H, W, 4))
    a[3, 2, 3] = -0.0                                       # a bit pattern that is not zero
    a[8, 3, 0] = SPECIAL_DOUBLES[1]                         # a NaN
    assert (marks_of(passes("nonzero", a), W, H) == marks([1, 0], [1, 0])).all()
    b = a.copy()
    assert not passes("differs", a, b).any(), "a NaN differs from itself"
    b[8, 3, 0] = SPECIAL_DOUBLES[2]                         # the NaN of another payload
    b[0, 8, 1] = -0.0                                       # 0.0 against -0.0
    assert (marks_of(passes("differs", a, b), W, H) == marks([0, 1], [1, 0])).all()


def test_range_and_set_by_hand():
    a = np.zeros((H, W), np.uint32)
    a[:] = 7
    a[1, 1], a[2, 8], a[8, 4], a[8, 8] = 10, 11, 0xFFFFFFFF, 256 + 10
    assert (marks_of(passes("range", a, lo=10, hi=11), W, H) == marks([1, 0], [0, 0])).all(), "hi is exclusive"
    assert (marks_of(passes("range", a, lo=10, hi=12), W, H) == marks([1, 1], [0, 0])).all()
    assert not passes("range", a, lo=10, hi=10).any(), "lo == hi selects nothing"
    assert (marks_of(passes("range", a, lo=12, hi=0xFFFFFFFF), W, H) == marks([0, 0], [0, 1])).all(), "0xFFFFFFFF is not below hi = 2^32 - 1"
    assert (marks_of(passes("range", a, lo=0, hi=8), W, H) == marks([1, 1], [1, 0])).all()
    assert set_words((0, 31, 32, 255)).tolist() == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]
    assert (marks_of(passes("set", a, values=(10,)), W, H) == marks([1, 0], [0, 0])).all(), "266 is not 10: elements at or above 256 never pass"
    assert (marks_of(passes("set", a, values=(10, 11, 255)), W, H) == marks([1, 1], [0, 0])).all()
    assert (marks_of(passes("set", a, values=(7,)), W, H) == marks([1, 1], [1, 0])).all()
    with pytest.raises(AssertionError):
        passes("range", a.astype(np.uint8), lo=0, hi=1)


def test_a_region_by_hand():
    a = np.ones((1, 1), np.uint8)                           # region (5, 3, 1, 1): one pixel of tile 0
    assert (marks_of(passes("nonzero", a), W, H, (5, 3, 1, 1)) == marks([1, 0], [0, 0])).all()
    a = np.zeros((2, 3), np.uint32)                         # region (6, 7, 3, 2): columns 6-8, rows 7-8 -- a pixel of each tile's corner
    for (y, x), want in (((0, 0), [[1, 0], [0, 0]]), ((0, 2), [[0, 1], [0, 0]]), ((1, 1), [[0, 0], [1, 0]]), ((1, 2), [[0, 0], [0, 1]])):
        a[:] = 0; a[y, x] = 5
        assert (marks_of(passes("nonzero", a), W, H, (6, 7, 3, 2)) == np.array(want, np.uint8)).all(), (y, x)
    with pytest.raises(AssertionError):
        marks_of(np.zeros((2, 2), bool), W, H, (6, 7, 3, 2))


def test_the_plane_makers():
    for eb, pp in ((1, 1), (4, 4), (8, 4)):
        a = sparse_plane(3, 117, 203, eb, pp)
        assert a.shape == ((117, 203) if pp == 1 else (117, 203, 4)) and a.dtype.itemsize == eb
        m = marks_of(passes("nonzero", a), 203, 117)
        assert 0 < m.sum() < m.size, f"sparse_plane {eb} x {pp}: {m.sum()} of {m.size} tiles"
        b, changed = changed_copy(4, a)
        assert (passes("differs", a, b) == changed).all() and changed.any() and not changed.all()
    assert sparse_plane(3, 9, 9, 8, 1).tobytes() == sparse_plane(3, 9, 9, 8, 1).tobytes(), "the seed decides the plane"
    mat = material_like_plane(5, 117, 203, 4, (0, 2, 3, 0xFFFFFFFF))
    assert mat.shape == (117, 203, 4) and mat.dtype == np.uint32 and set(np.unique(mat)) == {0, 2, 3, 0xFFFFFFFF}
    for eb, pp in ((1, 1), (4, 4), (8, 1)):
        a, m = one_element_per_tile(128, 128, eb, pp)
        assert m.all() and m.shape == (16, 16) and int(passes("nonzero", a).sum()) == 256
        assert (marks_of(passes("nonzero", a), 128, 128) == m).all()
        # the positions are all different rows and columns of the lane mapping: 37 is coprime to 64 * per_pixel
        flat = np.flatnonzero(passes("nonzero", a).reshape(16, 8, 16, 8, pp).transpose(0, 2, 1, 3, 4).reshape(256, -1).any(0))
        assert len(flat) == min(256, 64 * pp), f"{eb} x {pp}: {len(flat)} in-tile positions used"
        a3, m3 = one_element_per_tile(128, 128, eb, pp, skip_every=3)
        assert m3.sum() == 256 - 86 and (marks_of(passes("nonzero", a3), 128, 128) == m3).all()
