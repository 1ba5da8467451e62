"""The restatement of the XCD-aware block order that the GPU tests rest on (tests/xcd_order_checks.py), without a GPU: relabel is a permutation that leaves
the tail alone, two cases worked by hand from the kernel text, the three regimes of `full` in every kind of launch of the case table, enough moved blocks for a
case to show something, and the name of the environment variable the GPU tests set.
"""
import os

import numpy as np
import pytest

import xcd_order_checks as X
from conftest import ROOT
from scenes import H3, W3


def every_case():
    """[(kind, what, grid, chunk)] of the forced small cases and of the large scene under the default chunk."""
    return [(k, w, g, c) for k, w, g in X.small_grids() for c in X.FORCED_CHUNKS] + [(k, w, g, X.DEFAULT_CHUNK) for k, w, g in X.large_grids()]


def test_relabel_is_a_permutation_and_the_identity_on_the_tail():
    for kind, what, grid, chunk in every_case():
        full = X.full_blocks(grid, chunk)
        got = X.relabel(np.arange(grid), grid, chunk)
        assert full % (8 * chunk) == 0 and full <= grid < full + 8 * chunk, f"{what}, chunk {chunk}: full = {full} of {grid}"
        assert sorted(got.tolist()) == list(range(grid)), f"{what}, chunk {chunk}: not a permutation of [0, {grid})"
        assert sorted(got[:full].tolist()) == list(range(full)), f"{what}, chunk {chunk}: the blocks below full = {full} leave [0, {full})"
        assert (got[full:] == np.arange(full, grid)).all(), f"{what}, chunk {chunk}: the tail [{full}, {grid}) does not keep its index"


def test_answers_worked_by_hand_from_the_kernel_text():
    """`full = (gridDim.x / (8u * C)) * (8u * C); if (blk < full) { xcd = blk & 7u, i = blk >> 3; blk = ((i / C) * 8u + xcd) * C + (i % C); }`"""
    # grid 24, C = 2: full = (24 / 16) * 16 = 16.  Below it i is 0 (blocks 0..7) or 1 (blocks 8..15) and i / C is 0: blk = xcd * 2 + i.
    want = [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15] + list(range(16, 24))
    assert X.full_blocks(24, 2) == 16
    assert X.relabel(np.arange(24), 24, 2).tolist() == want
    assert [b for b in range(24) if want[b] != b] == list(range(1, 15)), "blocks 0 and 15 keep their label, the fourteen between them move"
    # C = 1: i / 1 = i and i % 1 = 0, blk = i * 8 + xcd = blk: the identity, useless as a forced value
    for grid in (24, 220, 1560):
        assert (X.relabel(np.arange(grid), grid, 1) == np.arange(grid)).all(), f"chunk 1 moves a block of a grid of {grid}"
    assert 1 not in X.FORCED_CHUNKS and 0 not in X.FORCED_CHUNKS
    assert (X.relabel(np.arange(220), 220, 0) == np.arange(220)).all() and X.full_blocks(220, 0) == 0
    # grid 220, C = 7: 8 C = 56, full = 3 * 56 = 168.
    assert X.full_blocks(220, 7) == 168
    got = X.relabel(np.arange(220), 220, 7)
    assert int(got[1]) == 7          # xcd 1, i 0: (0 * 8 + 1) * 7 + 0
    assert int(got[8]) == 1          # xcd 0, i 1: (0 * 8 + 0) * 7 + 1
    assert int(got[57]) == 63        # xcd 1, i 7: (1 * 8 + 1) * 7 + 0
    assert int(got[167]) == 167      # xcd 7, i 20: (2 * 8 + 7) * 7 + 6
    assert int(got[168]) == 168 and int(got[219]) == 219
    # the scalar form
    assert int(X.relabel(57, 220, 7)) == 63


def test_the_grids_of_the_case_table():
    """(full, tail) per chunk (2, 5, 7), from the grids the launches have by the host code."""
    tails = lambda grid: tuple(grid - X.full_blocks(grid, c) for c in (2, 5, 7))
    assert X.FORCED_CHUNKS == (2, 5, 7)
    assert X.frame_grid(64, 48) == 192 and tails(192) == (0, 32, 24)
    assert (W3, H3) == (203, 117) and X.frame_grid(W3, H3) == 1560 and tails(1560) == (8, 0, 48)
    assert X.frame_grid(9, 9) == 16 and tails(16) == (0, 16, 16) and X.full_blocks(16, 5) == 0 == X.full_blocks(16, 7)
    assert X.region_grid(W3, H3, (13, 50, 77, 31)) == 220 and tails(220) == (12, 20, 52)
    assert X.region_grid(W3, H3, None) == 1560 and X.region_grid(64, 48, None) == 192 and X.region_grid(9, 9, None) == 16
    assert X.share_grid(W3, H3, 3) == 520 and tails(520) == (8, 0, 16)
    assert X.share_grid(64, 48, 3) == 64 and tails(64) == (0, 24, 8)
    assert X.share_grid(9, 9, 3) == 8 and all(X.full_blocks(8, c) == 0 for c in (2, 5, 7))
    for r in ((200, 0, 3, 2), (8, 8, 8, 8)):
        assert X.region_grid(W3, H3, r) == 4 and all(X.full_blocks(4, c) == 0 for c in (2, 5, 7))
    assert X.region_grid(64, 48, (8, 8, 40, 24)) == 60 and tails(60) == (12, 20, 4)
    # the bands: H = 117, half = 58.  Chunks of 16 rows: scene rows [-58, -42) are canvas rows 102 .. 116 (the row that lands on 117 is rejected), tile rows 12 .. 14,
    # 3 x 26 tiles; [-42, -26) are canvas rows 86 .. 101, tile rows 10 .. 12; every band begins at a row that is 6 mod 8 and so spans three tile rows; the last,
    # [54, 58), is canvas rows 2 .. 5, tile row 0.
    assert X.band_grids(W3, H3, 16) == [312] * 7 + [104]
    assert X.band_grids(W3, H3, 50) == [728, 728, 312]          # canvas rows 68 .. 116 (tile rows 8 .. 14), 18 .. 67 (2 .. 8), 2 .. 17 (0 .. 2)
    assert X.band_grids(9, 9, 16) == [16]                        # canvas rows 2 .. 8: both tile rows of two tiles
    assert tails(312) == (8, 32, 32) and tails(104) == (8, 24, 48) and tails(728) == (8, 8, 0)
    # the large scene, under the default chunk
    assert X.DEFAULT_CHUNK == 256 and X.LARGE_TRIS >= X.DEFAULT_FROM == 50000
    assert X.frame_grid(*X.LARGE_SIZE) == 2244 and X.full_blocks(2244, 256) == 2048
    partial = [r for r in X.LARGE_REGIONS if r is not None]
    assert partial == [(8, 0, 256, 136)] and X.region_grid(*X.LARGE_SIZE, partial[0]) == 2176 and X.full_blocks(2176, 256) == 2048


def test_all_three_regimes_occur_in_every_kind_of_launch():
    seen = {}
    for kind, what, grid, chunk in [c for c in every_case() if c[3] in X.FORCED_CHUNKS]:
        full = X.full_blocks(grid, chunk)
        seen.setdefault(kind, set()).add("full == grid" if full == grid else "full == 0" if full == 0 else "0 < full < grid")
    assert set(seen) == {"frame", "share", "band", "region"}
    for kind, regimes in seen.items():
        assert regimes == {"full == grid", "0 < full < grid", "full == 0"}, f"{kind}: only {sorted(regimes)}"


def test_more_than_half_of_the_blocks_move_wherever_some_do():
    for kind, what, grid, chunk in every_case():
        if X.full_blocks(grid, chunk) > 0:
            moved = int((X.relabel(np.arange(grid), grid, chunk) != np.arange(grid)).sum())
            assert 2 * moved > grid, f"{what}, chunk {chunk}: {moved} of {grid} blocks move"


def test_the_variable_the_gpu_tests_set_is_the_one_the_library_reads():
    """A renamed variable must not turn the GPU tests into comparisons of the plain order with itself."""
    assert X.ENV == "RRT_XCD_CHUNK"
    with open(os.path.join(ROOT, "rust-ray-tracer_amd", "csrc", "frames.cpp")) as f:
        text = f.read()
    assert f'std::getenv("{X.ENV}")' in text, f"csrc/frames.cpp does not read {X.ENV}"
    assert "50000u ? 256u : 0u" in text, "csrc/frames.cpp: the default rule is no longer chunk 256 from 50 000 triangles"


@pytest.mark.parametrize("grid, chunk", [(24, 2), (220, 7), (2244, 256)])
def test_relabel_sends_the_blocks_of_one_xcd_to_whole_chunks(grid, chunk):
    """What the order is for: the blocks with one value of blk & 7 below `full` take chunks of `chunk` consecutive labels, chunk j * 8 + xcd for the j-th."""
    full = X.full_blocks(grid, chunk)
    got = X.relabel(np.arange(full), grid, chunk)
    for xcd in range(8):
        labels = got[xcd::8]
        want = np.concatenate([np.arange(chunk) + (j * 8 + xcd) * chunk for j in range(full // (8 * chunk))])
        assert (labels == want).all(), f"grid {grid}, chunk {chunk}, xcd {xcd}"
