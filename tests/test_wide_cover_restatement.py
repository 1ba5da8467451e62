"""tests/wide_cover_checks.py (wide boxes and simple waves restated in numpy) against csrc/coverage_rule.hpp itself, on the CPU: tests/wide_cover_model.cpp, built
with the host compiler and -ffp-contract=off as the library is, reads (frame, box, slot, root's slot range) tuples, frame by frame, and writes the rectangle, its
waves, coverage_is_wide and whether one pass over the frame's boxes lists the box; every field must equal the restatement's.

The tuples (a few thousand):
  random     the frames and boxes of tests/test_coverage_restatement.py (rotations, sheared and mirrored bases, refused frames; boxes in front of the eye, behind it,
             around it, empty, unbounded), slots 0 .. n - 1 in a random order and a root range that is empty, half of them, all of them or more;
  boundary   identity basis, 128x64 (512 waves: the floor of 16 waves decides) and 256x192 (3072 waves: the share decides, 24 waves): flat boxes whose rectangles
             are k x 1 and a x b waves for every k up to 30 and a, b up to 8 -- one wave below the threshold, on it, above it -- inside and outside the root's range;
             more than sixteen of them are wide: the list overflows;
  whole      boxes with a corner behind the eye among wide ones: never wide themselves.
Then the counts of tools/coverage_count.py (an independent restatement in its own arithmetic, from the triangles' f64 bounds) for the teapot at 256x144 against
classify() on fp32 boxes of the same triangles.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np

import coverage_checks as cc
import test_coverage_restatement as base
import wide_cover_checks as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "wide_cover_model.cpp")
INC = os.path.join(ROOT, "rust-ray-tracer_amd", "csrc")

TUPLE_IN = np.dtype(base.PAIR_IN.descr + [("slot", "<u4"), ("root_end", "<u4"), ("first", "<u4"), ("pad", "<u4")])
TUPLE_OUT = np.dtype([("ok", "<i4"), ("bx0", "<i4"), ("bx1", "<i4"), ("by0", "<i4"), ("by1", "<i4"), ("whole", "<i4"), ("wide", "<i4"), ("listed", "<i4"), ("waves", "<u8")])
assert TUPLE_IN.itemsize == 168 and TUPLE_OUT.itemsize == 40

IDENTITY = ([1.0, 1.0, 1.0], np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), np.array([0.0, 2.0, -10.0]))


def boundary_group(w, h, rng):
    """Flat boxes at depth 8 in front of the creation pose whose rectangles are k x 1 and a x b waves, placed at a random wave of the frame: a corner lies one
    quarter of a pixel inside its outermost waves (dyadic values: the projection is exact), and two boxes with a corner behind the eye."""
    args = (w, h, *IDENTITY)
    wx, wy, g = w // 4, h // 4, 8.0
    dims = [(k, 1) for k in range(1, min(30, wx) + 1)] + [(a, b) for a in range(1, 9) for b in range(1, 9)]
    c, hh = [], []
    for a, b in dims:
        bx0, by0 = int(rng.integers(0, wx - a + 1)), int(rng.integers(0, wy - b + 1))
        xlo, xhi = 4 * bx0 - w / 2 + 0.25, 4 * (bx0 + a - 1) - w / 2 + 0.25            # sub-sample columns of the first and the last wave
        yhi, ylo = (h - h // 2) - 4 * by0 - 0.25, (h - h // 2) - 4 * (by0 + b - 1) - 0.25
        lo = np.array([xlo * g / w, 2.0 + ylo * g / h, -2.0]); hi = np.array([xhi * g / w, 2.0 + yhi * g / h, -2.0])
        c.append((lo + hi) / 2); hh.append((hi - lo) / 2)
    c += [(0.0, 2.0, -9.0), (1.0, 2.0, -10.0)]; hh += [(0.5, 0.5, 2.0), (0.25, 0.25, 0.25)]
    return args, np.asarray(c, np.float32), np.asarray(hh, np.float32), dims


def tuples_of(args, c, hh, slots, root_end):
    rec, scales = base.records(args, c, hh)
    out = np.zeros(len(rec), TUPLE_IN)
    for name in base.PAIR_IN.names:
        out[name] = rec[name]
    out["slot"], out["root_end"] = slots, root_end
    out["first"][0] = 1
    return out, scales


def test_wide_rule_equals_the_header_in_every_field(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "wide_cover_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    rng = np.random.default_rng(20261)
    groups = []                                                                       # (args, c, h, slots, root_end, dims or None)
    for k in range(44):
        args = base.random_frame(rng, k)
        c, hh = base.random_boxes(rng, args, 60)
        groups.append((args, c, hh, rng.permutation(60), (0, 30, 60, 1000)[k % 4], None))
    for w, h in ((128, 64), (256, 192)):
        for root_end in (10 ** 6, 60):
            args, c, hh, dims = boundary_group(w, h, rng)
            groups.append((args, c, hh, np.arange(len(c)), root_end, dims))
    recs = [tuples_of(*g[:5]) for g in groups]
    blob = np.concatenate([r for r, _ in recs])
    assert len(blob) >= 3000, len(blob)
    run = subprocess.run([exe, "-", "-"], input=blob.tobytes(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = np.frombuffer(run.stdout, TUPLE_OUT)
    assert len(out) == len(blob), (len(out), len(blob))

    seen = dict(frames=0, frames_off=0, wide=0, listed=0, overflow_frames=0, below=0, on=0, above=0, outside_root=0, whole=0, empty=0, whole_among_wide=0)
    at = 0
    for (args, c, hh, slots, root_end, dims), (_, scales) in zip(groups, recs):
        w, h, vp, right, up, forward, eye = args
        o = out[at:at + len(c)]; at += len(c)
        F = cc.frame_from_scales(w, h, *scales, right, up, forward, eye)
        what = f"frame {w}x{h}, viewport {vp}, eye {np.asarray(eye).tolist()}, root range [0, {root_end})"
        assert bool(o["ok"][0]) == (F is not None), f"{what}: coverage_frame says {o['ok'][0]}"
        if F is None:
            seen["frames_off"] += 1
            assert not o["wide"].any() and not o["listed"].any() and not o["waves"].any(), what
            continue
        seen["frames"] += 1
        R = cc.rects_of(F, c, hh)
        for name in ("bx0", "bx1", "by0", "by1"):
            assert np.array_equal(getattr(R, name), o[name]), f"{what}: {name} differs"
        got = wc.classify(F, R, root_end, slots=slots)                                 # (the model takes the boxes in the order given: the default)
        for name, mine in (("whole", R.whole), ("waves", wc.rect_waves(R)), ("wide", got["wide"]), ("listed", got["listed"])):
            bad = np.flatnonzero(np.asarray(mine).astype(np.int64) != o[name].astype(np.int64))
            assert len(bad) == 0, (f"{what}: {name} differs on {len(bad)} of {len(c)} boxes; first: box c {c[bad[0]].tolist()} h {hh[bad[0]].tolist()} slot {slots[bad[0]]}: "
                                   f"the header {o[name][bad[0]]}, restated {np.asarray(mine)[bad[0]]}")
        waves, T = wc.rect_waves(R), wc.wide_min_waves(F)
        inside = np.asarray(slots) < root_end
        seen["wide"] += int(got["wide"].sum()); seen["listed"] += got["n_wide"]; seen["overflow_frames"] += bool(got["wide"].sum() > wc.MAX_WIDE)
        seen["whole"] += int((R.whole & cc.some(R)).sum()); seen["empty"] += int((~cc.some(R)).sum())
        seen["whole_among_wide"] += bool((R.whole & cc.some(R)).any() and got["wide"].any())
        assert got["n_wide"] == min(int(got["wide"].sum()), wc.MAX_WIDE) and not (got["wide"] & R.whole).any(), what
        if (R.whole & cc.some(R)).any():
            assert got["n_simple"] == 0 and got["fine"].all(), f"{what}: a box reaches the whole frame, but {got['n_simple']} waves are simple"
        if dims is not None:
            k = len(dims)
            assert [int(v) for v in waves[:k]] == [a * b for a, b in dims], f"{what}: the boundary boxes do not cover the waves they were built for"
            assert T == (16 if (w, h) == (128, 64) else 24), (what, T)
            assert np.array_equal(got["wide"][:k], inside[:k] & (waves[:k] >= T)), what
            seen["below"] += int((inside[:k] & (waves[:k] == T - 1)).sum()); seen["on"] += int((inside[:k] & (waves[:k] == T)).sum())
            seen["above"] += int((inside[:k] & (waves[:k] == T + 1)).sum()); seen["outside_root"] += int((~inside[:k] & (waves[:k] >= T)).sum())
            # the masks: a listed box alone makes simple waves, an overflowed or ordinary one none
            assert got["n_simple"] == 0, what                                            # (the two boxes at the eye reach the whole frame)
            front = cc.Rects(*(v[:k] for v in R))
            part = wc.classify(F, front, root_end)
            assert part["n_wide"] == min(int(part["wide"].sum()), wc.MAX_WIDE), what
            assert part["n_simple"] == int((part["mask"] & ~part["fine"]).sum()) and (part["per_simple"] >= 1).all(), what
            if part["wide"].sum() > wc.MAX_WIDE:                                       # the surplus is in `fine`
                surplus = np.flatnonzero(part["wide"] & ~part["listed"])
                for i in surplus:
                    assert part["fine"][front.by0[i]:front.by1[i] + 1, front.bx0[i]:front.bx1[i] + 1].all(), f"{what}: wide box {i} found the list full but is not in `fine`"
    print(f"\n[wide cover restatement] {len(blob)} tuples: {seen}")
    assert seen["frames"] >= 20 and seen["frames_off"] >= 2 and seen["wide"] >= 200 and seen["overflow_frames"] >= 2 and seen["listed"] < seen["wide"], seen
    assert seen["below"] >= 2 and seen["on"] >= 2 and seen["above"] >= 2 and seen["outside_root"] >= 10, seen
    assert seen["whole"] >= 50 and seen["empty"] >= 50 and seen["whole_among_wide"] >= 4, seen


def test_count_tool_agrees_on_the_teapot_at_256x144(rrt, teapot):
    """tools/coverage_count.py against classify() on fp32 boxes of the same triangles: wide boxes, simple waves, covered waves, wide boxes per simple wave."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "coverage_count.py"), "256", "144"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    m_wide = re.search(r"wide boxes \(.*\): (\d+)", run.stdout)
    m_simple = re.search(r"simple waves: (\d+) of (\d+) covered .* mean ([0-9.]+), max (\d+)", run.stdout)
    assert m_wide and m_simple, run.stdout
    pos = np.asarray(teapot.triangles()[0], np.float64).reshape(-1, 3, 3)
    tree = teapot.octree()
    own = tree["own_idx"][tree["own_off"][0]:tree["own_off"][1]]                       # the root's own list; its triangles first, as the slots are
    order = np.concatenate([own, np.setdiff1d(np.arange(len(pos)), own)])
    F = cc.frame_of(256, 144, (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 2.0, -10.0))
    R = cc.rects_of(F, *wc.approx_boxes(pos[order], 20.0 / 32768.0))
    got = wc.classify(F, R, len(own))
    print(f"\n[wide cover restatement] teapot 256x144: the tool {m_wide.group(1)} wide, {m_simple.group(1)} simple of {m_simple.group(2)}; restated {got['n_wide']}, {got['n_simple']} of {int(got['mask'].sum())}")
    assert got["n_wide"] == int(m_wide.group(1)) > 0
    assert (got["n_simple"], int(got["mask"].sum())) == (int(m_simple.group(1)), int(m_simple.group(2))) and got["n_simple"] > 0
    assert int(got["per_simple"].max()) == int(m_simple.group(4)) and abs(float(got["per_simple"].mean()) - float(m_simple.group(3))) < 0.006
