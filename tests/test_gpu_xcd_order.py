"""Every launch that takes the XCD-aware block order (csrc/render.hip: render_kernel, stage_lane(const Region&); csrc/frames.cpp: frame_params), under the order
and without it, bit for bit.

The order switches on by itself for scenes of 50 000 triangles and more, and then only re-labels launches of 2048 blocks and more; RRT_XCD_CHUNK forces a chunk
for any scene, and is read once per process.  So:

 * the pytest process runs every small case of tests/xcd_order_checks.py in the plain order (nothing forced, every scene small), which the rest of the suite
   checks against the oracle: the reference here;
 * test_forced_chunk[C], C = 2, 5, 7, runs the same cases in a fresh child (tests/xcd_order_child.py) with RRT_XCD_CHUNK=C: whole frames with and without the
   coverage pass (and the mask itself), the bands of render_progressive, the tiles of every rank of a world of three and their de-tiled frame, the five region
   calls and pick, on the teapot in two poses at 64 x 48, 203 x 117 and 9 x 9 and on the 4 000-triangle soup with group records, in every walk -- grids in which
   `full` is the whole grid, part of it and nothing (tests/test_xcd_order_restatement.py);
 * test_the_default_rule_on_a_scene_of_50_000_triangles goes the other way: a 60 000-triangle soup at 264 x 136 (2244 blocks; a region of 2176) runs under the
   default chunk of 256 in the pytest process, and in a child with RRT_XCD_CHUNK=0.

Every output lies in a buffer that held 0xA5 in every byte before its call, so a block that never ran shows; the sets of names must be equal.  One child at a
time; a child that is killed, aborts or runs out of time fails its test with the end of its stderr and keeps the later ones from starting another.
profiles/xcd_order_mutants.txt: what wrong re-labellings these tests catch.

Wall time of a child, measured once on an MI355X (import of torch and the library included): small 3.1 to 3.3 s (1438 arrays; the same cases take 1.0 s in the
pytest process, where torch is loaded already), large 2.7 to 3.0 s (133 arrays; 0.4 s in the pytest process); the module 16 to 17 s.  Ten times that is below 120 s, so
both limits are 120 s: a slow import must not read as a hang.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import xcd_order_checks as X
from bitwise import assert_same_bits
from region_render_checks import assert_frame_has_content

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xcd_order_child.py")
TIMEOUT = {"small": 120, "large": 120}                    # seconds: ten times the measured wall time, and not below 120
DIED = []                                                  # why no further child is started: set by the first one that was killed, aborted or timed out


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def in_this_process(rrt, torch, which):
    """The outputs of one collector under the order this process has by itself; nothing is forced here."""
    assert X.ENV not in os.environ, f"{X.ENV} is set in the pytest process: its order is not the one the library chooses by itself"
    t0 = time.monotonic()
    out = X.COLLECTORS[which](rrt, torch)
    print(f"collector `{which}` in the pytest process: {len(out)} arrays in {time.monotonic() - t0:.1f} s")
    n_masks = X.assert_outputs_have_content(out, rrt)
    for a in out.values():
        a.setflags(write=False)
    return out, n_masks


@pytest.fixture(scope="module")
def plain(rrt, torch):
    """Every small case in the plain order: all scenes are below the size at which the default rule switches the order on."""
    out, n_masks = in_this_process(rrt, torch, "small")
    counts = {n: int(a[0]) for n, a in out.items() if n.endswith("root triangle_count")}
    assert sorted(counts) == ["soup, root triangle_count", "teapot, root triangle_count"], sorted(counts)
    for n, c in counts.items():
        assert 0 < c < X.DEFAULT_FROM, f"{n}: {c}, not below {X.DEFAULT_FROM}: the default rule re-labels this scene's launches"
    assert n_masks == len(X.ALL_MODES) * len(X.POSES) * 2, f"{n_masks} coverage masks of the teapot at 64x48 and 203x117"
    return out


def tail_of(stream, n=3000):
    text = stream.decode(errors="replace") if isinstance(stream, bytes) else (stream or "")
    return text[-n:]


def run_child(which, chunk, tmp_path):
    """One fresh process with RRT_XCD_CHUNK=chunk: its outputs.  No retry."""
    if DIED:
        pytest.fail(f"no child started: {DIED[0]}")
    out = str(tmp_path / f"{which}_{chunk}.npz")
    what = f"child `{which}` with {X.ENV}={chunk}"
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, CHILD, which, out], env=dict(os.environ, **{X.ENV: str(chunk)}), timeout=TIMEOUT[which], capture_output=True)
    except subprocess.TimeoutExpired as e:
        DIED.append(f"{what} was still running after {TIMEOUT[which]} s")
        pytest.fail(f"{DIED[0]}; its stderr ends:\n{tail_of(e.stderr)}")
    print(f"{what}: {time.monotonic() - t0:.1f} s of wall time, status {p.returncode}")
    if p.returncode < 0 or p.returncode in (134, 139):
        DIED.append(f"{what} ended with status {p.returncode}")
        pytest.fail(f"{DIED[0]}; its stderr ends:\n{tail_of(p.stderr)}")
    assert p.returncode == 0, f"{what} ended with status {p.returncode}; its stderr ends:\n{tail_of(p.stderr)}"
    with np.load(out) as z:
        return {n: z[n] for n in z.files}


def assert_same_outputs(got, want, what):
    assert set(got) == set(want), f"{what}: names only in the child {sorted(set(got) - set(want))[:5]}, only in the parent {sorted(set(want) - set(got))[:5]}"
    bad = []
    for n in want:
        try:
            assert_same_bits(got[n], want[n], f"{what}: {n}")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, f"{len(bad)} of {len(want)} arrays differ; the first three:\n" + "\n".join(bad[:3])


@pytest.mark.parametrize("chunk", X.FORCED_CHUNKS)
def test_forced_chunk(plain, tmp_path, chunk):
    assert_same_outputs(run_child("small", chunk, tmp_path), plain, f"chunk {chunk} vs the plain order")


def test_the_default_rule_on_a_scene_of_50_000_triangles(rrt, torch, tmp_path):
    """The only case at a size beyond the smallest: chunk 256 re-labels nothing below 2048 blocks."""
    if DIED:
        pytest.fail(f"nothing run: {DIED[0]}")
    ordered, _ = in_this_process(rrt, torch, "large")
    count = int(ordered["large soup, root triangle_count"][0])
    assert count >= X.DEFAULT_FROM, f"the root's triangle_count is {count}, below {X.DEFAULT_FROM}: the default rule leaves this scene in the plain order"
    w, h = X.LARGE_SIZE
    for mode in X.LARGE_MODES:
        assert_frame_has_content(ordered[f"large soup, walk {mode}, {w}x{h}, render_into coverage=False"], f"large soup, walk {mode}")
    assert_same_outputs(run_child("large", 0, tmp_path), ordered, "chunk 0 vs the default rule's chunk 256")
