"""Tile selection on the GPU (include/rrt.h: rrt_mark_tiles[_device], rrt_select_tiles[_device]): tests over planes that produce the list
rrt_render_tile_list_device reads.

The statement under test: the marks and the list ARE what the numpy restatement of tests/tile_checks.py gives for the same planes (checked by hand in
tests/test_tile_restatement.py), bit for bit, for every element width, plane kind, frame, region and alignment; nothing behind their end is written; and a frame
repaired through such a list IS the frame rendered anew.  Every comparison is bitwise.assert_same_bits.  Marks and lists live in buffers longer than needed,
prefilled with 0xA5.
"""
import numpy as np
import pytest

from bitwise import assert_same_bits
from gpu_checks import ALL_MODES, traced_rows
from region_render_checks import WHITE, assert_frame_has_content
from scenes import EYE3, H3, TARGET, W3
from surface_checks import traced_cols
from tile_checks import (ACCEPTS, FRAMES, GUARD, KINDS, PLANE_KINDS, differing_doubles, changed_copy, list_of, marks_of, material_like_plane, one_element_per_tile,
                         passes, region_of, regions_in, sparse_plane, tiles_of)

pytestmark = pytest.mark.gpu

TAIL = 64                                                  # guard elements behind every output
DEAD = 0xFFFFFFFF
SET_POOL = (7, 0, 31, 32, 255, 256, 287, 0xFFFFFFFF)       # 256 and 287 are 0 and 31 with bit 8 set: an element at or above 256 must not pass as its low byte
SET_VALUES = (0, 31, 32, 255)
RANGE_POOL = (7, 2, 3, 5, 300, 0xFFFFFFFF)
RANGES = ((2, 4), (3, 3), (5, 0xFFFFFFFF))                 # ordinary; lo == hi: nothing; hi = 2^32 - 1: everything from 5 but the 0xFFFFFFFF elements


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def rt(rrt, teapot):
    """A raytracer for the calls that trace nothing: which scene it holds does not matter."""
    return rrt.RayTracer(teapot, rrt.default_lights())


def on_device(torch, a, lead=0):
    """A host plane as a device tensor of its shape (unsigned types as the signed type of their width); with lead, the plane begins `lead` elements into a
    longer tensor: it is aligned to its elements and, for lead * itemsize % 16 != 0, to no more."""
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    flat = a.reshape(-1) if signed is None else a.reshape(-1).view(signed)
    t = torch.from_numpy(np.concatenate([np.zeros(lead, flat.dtype), flat])).cuda()
    return t[lead:].view(a.shape)


class Guarded:
    """n elements of `itemsize` bytes (1 or 4) in front of TAIL more, all bytes GUARD (or `prefill` in the first n)."""

    def __init__(self, torch, n, itemsize, prefill=None):
        self.n, self.dtype = n, {1: np.uint8, 4: np.uint32}[itemsize]
        host = np.full(n + TAIL, GUARD if itemsize == 1 else 0xA5A5A5A5, self.dtype)
        if prefill is not None:
            host[:n] = np.asarray(prefill, self.dtype).reshape(-1)
        self.all = torch.from_numpy(host if itemsize == 1 else host.view(np.int32)).cuda()
        self.t = self.all[:n]

    def host(self, what):
        """The first n elements, after the check that the tail still holds the guard."""
        got = self.all.cpu().numpy().view(self.dtype)
        assert (got[self.n:] == (GUARD if self.dtype == np.uint8 else 0xA5A5A5A5)).all(), f"{what}: written behind element {self.n}"
        return got[:self.n].copy()


def device_test(rrt, torch, kind, a, b=None, lead=0, **kw):
    return rrt.tile_test(kind, on_device(torch, a, lead), None if b is None else on_device(torch, b, lead), **kw)


def device_marks(rrt, torch, rt, width, height, region, kind, a, b=None, lead=0, prefill=None, what="", **kw):
    """[tiles_y][tiles_x] uint8 of rt.mark_tiles_into over the host planes a (and b), from guarded marks"""
    tx, ty = tiles_of(width, height)
    marks = Guarded(torch, tx * ty, 1, prefill)
    rt.mark_tiles_into(marks.t, device_test(rrt, torch, kind, a, b, lead, **kw), width, height, region=region)
    torch.cuda.synchronize()
    return marks.host(what).reshape(ty, tx)


def device_list(rrt, torch, rt, width, height, region, tests, prefill=None, what="", tiles=True, count=True, stream=None):
    """(marks [tiles_y][tiles_x], list of count entries, count) of rt.select_tiles_into over tile_test structs of device planes; the list's tail is checked."""
    tx, ty = tiles_of(width, height)
    n = tx * ty
    marks, lst, cnt = Guarded(torch, n, 1, prefill), Guarded(torch, n, 4), Guarded(torch, 1, 4)
    scratch = torch.empty(rrt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    rt.select_tiles_into(lst.t if tiles else None, cnt.t if count else None, marks.t, scratch, tests, width, height, region=region, stream=stream)
    torch.cuda.synchronize()
    m, l, c = marks.host(what).reshape(ty, tx), lst.host(what), cnt.host(what)
    k = int(c[0]) if count else int((l != DEAD).sum())
    if tiles:
        assert (l[k:] == DEAD).all(), f"{what}: the tail of the list behind its {k} entries is not 0xFFFFFFFF"
    else:
        assert (l == 0xA5A5A5A5).all(), f"{what}: a list that was not asked for was written"
    if not count:
        assert c[0] == 0xA5A5A5A5, f"{what}: a count that was not asked for was written"
    return m, l[:k], k


def seeded_cases(kind, seed, h, w, eb, pp):
    """[(what, a, b, the test's keywords)] of one test kind over one plane kind"""
    if kind == "nonzero":
        return [("", sparse_plane(seed, h, w, eb, pp), None, {})]
    if kind == "differs":
        if eb == 8:
            a, b = differing_doubles(seed, h, w, pp)
        else:
            a = sparse_plane(seed, h, w, eb, pp, density=0.2)
            b, _ = changed_copy(seed + 1, a)
        return [("", a, b, {})]
    if kind == "range":
        a = material_like_plane(seed, h, w, pp, RANGE_POOL, background=0.75)
        return [(f" [{lo}, {hi})", a, None, dict(lo=lo, hi=hi)) for lo, hi in RANGES]
    a = material_like_plane(seed, h, w, pp, SET_POOL, background=0.75)
    return [(f" {values}", a, None, dict(values=values)) for values in (SET_VALUES, (7,), (255,), ())]


# ------------------------------------------------------------------ 1: the closed loop of a material edit
@pytest.mark.parametrize("mode", ALL_MODES)
def test_a_material_edit_repaired_through_a_tile_list(rrt, torch, teapot, mode):
    """Frame and material plane kept on the device -> set_materials -> SET {edited, the mirror} -> the list's tiles rendered into the old frame, on one stream
    with nothing in between: the new frame, bit for bit."""
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    rt.look_at(EYE3, TARGET)
    tx, ty = tiles_of(W3, H3)
    n = tx * ty
    assert n == 390
    fb = torch.zeros(W3 * H3, dtype=torch.int32, device="cuda")
    material = torch.zeros((H3, W3, 4), dtype=torch.int32, device="cuda")
    rt.render_into(fb, W3, H3)
    rt.surface_into({"material": material}, W3, H3)
    torch.cuda.synchronize()
    old = fb.cpu().numpy().view(np.uint32).reshape(H3, W3).copy()
    assert_frame_has_content(old, f"walk {mode}: teapot {W3}x{H3} at {EYE3}")
    mats = rt.materials()
    assert [k for k, m in enumerate(mats) if m["kr"] > 0] == [3], "material 3 is the scene's only mirror"
    mats[0] = dict(mats[0], kd=(0.3, 0.9, 0.5))
    rt.set_materials(mats)
    marks, lst, cnt = Guarded(torch, n, 1), Guarded(torch, n, 4), Guarded(torch, 1, 4)
    scratch = torch.empty(rrt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    rt.select_tiles_into(lst.t, cnt.t, marks.t, scratch, [rrt.tile_test("set", material, values=(0, 3))], W3, H3)
    rt.render_tile_list_into(fb, lst.t, W3, H3, bound_t=cnt.t)
    torch.cuda.synchronize()
    want_marks = marks_of(passes("set", material.cpu().numpy().view(np.uint32), values=(0, 3)), W3, H3)
    count = int(cnt.host("count")[0])
    print(f"walk {mode}: {count} of {n} tiles hold material 0 or 3")
    assert_same_bits(marks.host("marks").reshape(ty, tx), want_marks, f"walk {mode}: marks vs the restatement over the material plane", np.uint8)
    got = lst.host("list")
    assert_same_bits(got[:count], list_of(want_marks), f"walk {mode}: the list vs the restatement", np.uint32)
    assert (got[count:] == DEAD).all(), "the tail of the list is not 0xFFFFFFFF"
    assert 0 < count < n, f"{count} of {n} tiles selected: the repair is the whole frame or nothing"
    fresh = rt.render(W3, H3)
    changed = int((fresh != old).sum())
    print(f"walk {mode}: the edit changes {changed} pixels")
    assert changed >= 64, f"the edit changes {changed} pixels"
    assert_same_bits(fb.cpu().numpy().view(np.uint32).reshape(H3, W3), fresh, f"walk {mode}: the repaired frame vs a fresh render", np.uint32)


# ------------------------------------------------------------------ 2: the tiles that are not empty
@pytest.mark.parametrize("size", ((W3, H3), (64, 48)))
def test_the_tiles_with_a_hit_make_the_frame(rrt, torch, teapot, size):
    """NONZERO over the uint8 hit plane; its tiles rendered into the frame of an empty scene -- the background at the traced pixels, 0 at the others -- give the frame."""
    w, h = size
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    if size == (W3, H3):
        rt.look_at(EYE3, TARGET)                           # (the larger frame in the pose of the closed loop, the smaller in the creation pose)
    tx, ty = tiles_of(w, h)
    n = tx * ty
    hit = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    rt.visibility_into({"hit": hit}, w, h)
    empty = np.zeros((h, w), np.uint32)
    empty[np.ix_(traced_rows(h), traced_cols(w))] = WHITE
    fb = torch.from_numpy(empty.view(np.int32).reshape(-1).copy()).cuda()
    lst, cnt, marks = Guarded(torch, n, 4), Guarded(torch, 1, 4), Guarded(torch, n, 1)
    scratch = torch.empty(rrt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    rt.select_tiles_into(lst.t, cnt.t, marks.t, scratch, rrt.tile_test("nonzero", hit), w, h)
    rt.render_tile_list_into(fb, lst.t, w, h, bound_t=cnt.t)
    torch.cuda.synchronize()
    count = int(cnt.host("count")[0])
    print(f"{w}x{h}: {count} of {n} tiles hold a hit")
    assert 0 < count < n, f"{count} of {n} tiles hold a hit"
    assert_same_bits(lst.host("list")[:count], list_of(marks_of(passes("nonzero", hit.cpu().numpy()), w, h)), f"{w}x{h}: the list vs the restatement over the hit plane", np.uint32)
    frame = rt.render(w, h)
    assert_frame_has_content(frame, f"teapot {w}x{h}")
    assert_same_bits(fb.cpu().numpy().view(np.uint32).reshape(h, w), frame, f"{w}x{h}: the hit tiles over the empty frame vs render", np.uint32)


# ------------------------------------------------------------------ 3: seeded planes against the restatement
@pytest.mark.parametrize("size", FRAMES)
def test_seeded_planes_against_the_restatement(rrt, torch, rt, size):
    """All four tests over every plane kind they accept, on every region of the frame.  (Of these the 203-wide planes of 1- and 4-byte pixels and of single doubles
    have a pitch that is no multiple of 16 and take the element path, as do the regions that begin off a 16-byte boundary; the others take the 16-byte path.)"""
    width, height = size
    mixed = 0
    for region in regions_in(width, height):
        x0, y0, w, h = region_of(width, height, region)
        for kind in KINDS:
            for eb, pp in ACCEPTS[kind]:
                for case, a, b, kw in seeded_cases(kind, 1000 * eb + 10 * pp + KINDS.index(kind), h, w, eb, pp):
                    what = f"{width}x{height} region {region}: {kind}{case} over {eb}-byte elements x {pp}"
                    want = marks_of(passes(kind, a, b, **kw), width, height, region)
                    assert_same_bits(device_marks(rrt, torch, rt, width, height, region, kind, a, b, what=what, **kw), want, what, np.uint8)
                    mixed += 0 < want.sum() < want.size
    assert mixed >= 10 or width * height < 64 * 48, f"{width}x{height}: only {mixed} cases have both marked and unmarked tiles"


def test_planes_that_are_aligned_to_their_elements_only(rrt, torch, rt):
    """A plane that begins one element into a tensor (4 bytes for 4-byte elements) takes the element path though its pitch is a multiple of 16: the marks are those
    of the aligned plane."""
    width, height = 64, 48
    for kind in KINDS:
        for eb, pp in ACCEPTS[kind]:
            for case, a, b, kw in seeded_cases(kind, 77 + eb + pp, height, width, eb, pp):
                what = f"{kind}{case} over {eb}-byte elements x {pp}, one element into a tensor"
                want = marks_of(passes(kind, a, b, **kw), width, height)
                assert on_device(torch, a, lead=1).data_ptr() % 16 == eb, "the plane is still aligned to 16 bytes"
                assert_same_bits(device_marks(rrt, torch, rt, width, height, None, kind, a, b, lead=1, what=what, **kw), want, what, np.uint8)
                assert_same_bits(device_marks(rrt, torch, rt, width, height, None, kind, a, b, what=what, **kw), want, what + " (aligned)", np.uint8)


# ------------------------------------------------------------------ 4: the lane mapping
@pytest.mark.parametrize("plane_kind", PLANE_KINDS)
def test_every_position_of_a_tile_reaches_its_own_tile(rrt, torch, rt, plane_kind):
    """128 x 128, 256 tiles: tile t's only element sits at in-tile position 37 t mod positions, so every lane, every pass and every half of a chunk decides some
    tile alone; with the element of every third tile cleared exactly those tiles are unmarked.  On both paths."""
    eb, pp = plane_kind
    for skip in (None, 3):
        a, want = one_element_per_tile(128, 128, eb, pp, skip_every=skip)
        assert want.sum() == (256 if skip is None else 170)
        for lead in (0, 1):
            what = f"{eb}-byte elements x {pp}, every {skip} tile cleared, {'element' if lead else '16-byte'} path"
            assert_same_bits(device_marks(rrt, torch, rt, 128, 128, None, "nonzero", a, lead=lead, what=what), want, what, np.uint8)
            m, lst, count = device_list(rrt, torch, rt, 128, 128, None, device_test(rrt, torch, "nonzero", a, lead=lead), what=what)
            assert_same_bits(m, want, what + ": marks of select", np.uint8)
            assert_same_bits(lst, list_of(want), what + ": the list", np.uint32)
            assert count == want.sum()


# ------------------------------------------------------------------ 5: KEEP and the union
@pytest.mark.parametrize("size,region", (((W3, H3), None), ((W3, H3), (13, 50, 77, 31)), ((9, 9), None)))
def test_keep_joins_and_select_is_the_union(rrt, torch, rt, size, region):
    width, height = size
    x0, y0, w, h = region_of(width, height, region)
    tx, ty = tiles_of(width, height)
    a = sparse_plane(11, h, w, 1, 4, density=0.002)
    m = material_like_plane(12, h, w, 1, SET_POOL, background=0.9)
    want_a, want_m = marks_of(passes("nonzero", a), width, height, region), marks_of(passes("set", m, values=SET_VALUES), width, height, region)
    union = want_a | want_m
    what = f"{width}x{height} region {region}"
    if width > 9:
        assert want_a.any() and want_m.any() and (want_a != want_m).any() and not union.all(), f"{what}: the two tests do not tell a union from one of them"
    # two mark calls with KEEP over marks that hold 7: a selected byte becomes 1, every other byte keeps its 7
    sevens = np.full((ty, tx), 7, np.uint8)
    first = device_marks(rrt, torch, rt, width, height, region, "nonzero", a, prefill=sevens, keep=True, what=what)
    assert_same_bits(first, np.where(want_a != 0, 1, 7).astype(np.uint8), f"{what}: NONZERO | KEEP over sevens", np.uint8)
    both = device_marks(rrt, torch, rt, width, height, region, "set", m, prefill=first, keep=True, values=SET_VALUES, what=what)
    assert_same_bits(both, np.where(union != 0, 1, 7).astype(np.uint8), f"{what}: then SET | KEEP", np.uint8)
    # without KEEP every byte is written
    assert_same_bits(device_marks(rrt, torch, rt, width, height, region, "set", m, prefill=sevens, values=SET_VALUES, what=what), want_m, f"{what}: SET over sevens", np.uint8)
    # select with the two tests: the union, whatever the marks held
    tests = [device_test(rrt, torch, "nonzero", a), device_test(rrt, torch, "set", m, values=SET_VALUES)]
    marks, lst, count = device_list(rrt, torch, rt, width, height, region, tests, prefill=sevens, what=what)
    assert_same_bits(marks, union, f"{what}: the marks of select with two tests", np.uint8)
    assert_same_bits(lst, list_of(union), f"{what}: the list of select with two tests", np.uint32)
    assert count == union.sum()
    # ... in the other order, and with a KEEP on the second test, which changes nothing
    tests = [device_test(rrt, torch, "set", m, values=SET_VALUES), device_test(rrt, torch, "nonzero", a, keep=True)]
    assert_same_bits(device_list(rrt, torch, rt, width, height, region, tests, prefill=sevens, what=what)[1], list_of(union), f"{what}: the list, tests swapped", np.uint32)
    # tests[0] is applied as given: with KEEP it joins the marks that are there
    held = np.zeros((ty, tx), np.uint8)
    held[ty - 1, tx - 1] = 1
    tests = [device_test(rrt, torch, "nonzero", a, keep=True), device_test(rrt, torch, "set", m, values=SET_VALUES)]
    marks, lst, count = device_list(rrt, torch, rt, width, height, region, tests, prefill=held, what=what)
    assert_same_bits(marks, union | held, f"{what}: the marks of select whose first test keeps", np.uint8)
    assert_same_bits(lst, list_of(union | held), f"{what}: its list", np.uint32)
    # the list alone, and the count alone
    tests = [device_test(rrt, torch, "nonzero", a), device_test(rrt, torch, "set", m, values=SET_VALUES)]
    assert_same_bits(device_list(rrt, torch, rt, width, height, region, tests, what=what, count=False)[1], list_of(union), f"{what}: the list without a count", np.uint32)
    assert device_list(rrt, torch, rt, width, height, region, tests, what=what, tiles=False)[2] == union.sum()


# ------------------------------------------------------------------ 6: stream order
def test_the_planes_are_read_in_stream_order(rrt, torch, rt):
    """A torch op on the same stream writes the plane just before the call: the kernel reads what it wrote."""
    width, height = W3, H3
    a = sparse_plane(21, height, width, 4, 4, density=0.002)
    want = marks_of(passes("nonzero", a), width, height)
    assert 0 < want.sum() < want.size
    src = on_device(torch, a)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        plane = torch.zeros_like(src)
        for _ in range(8):                                 # (work in front of the write, so that a kernel that did not wait would run first)
            plane.add_(src).sub_(src)
        plane.add_(src)
        marks, lst, count = device_list(rrt, torch, rt, width, height, None, rrt.tile_test("nonzero", plane), what="stream order", stream=stream.cuda_stream)
    assert_same_bits(marks, want, "marks behind a torch op on the same stream", np.uint8)
    assert_same_bits(lst, list_of(want), "the list behind a torch op on the same stream", np.uint32)


# ------------------------------------------------------------------ 7: the host forms, and what no form touches
@pytest.mark.parametrize("size,region", (((W3, H3), None), ((W3, H3), (13, 50, 77, 31)), ((64, 48), (8, 8, 8, 8)), ((1, 1), None)))
def test_the_host_forms_are_the_device_forms(rrt, torch, teapot, size, region):
    width, height = size
    x0, y0, w, h = region_of(width, height, region)
    tx, ty = tiles_of(width, height)
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.render(64, 48)
    before = (rt.last_stats(), rt.coverage_info())
    what = f"{width}x{height} region {region}"
    dense = width == 1
    tests_of = {}
    for kind in KINDS:
        for eb, pp in ACCEPTS[kind]:
            for case, a, b, kw in seeded_cases(kind, 5 + eb + pp, h, w, eb, pp)[:2]:
                if dense:
                    a = np.ones_like(a) if kind != "differs" else a
                    b = None if b is None else np.ones_like(b)
                want = marks_of(passes(kind, a, b, **kw), width, height, region)
                host = rt.mark_tiles(rrt.tile_test(kind, a, b, **kw), width, height, region=region)
                assert_same_bits(host, want, f"{what}: host form, {kind}{case} over {eb} x {pp}", np.uint8)
                assert_same_bits(host, device_marks(rrt, torch, rt, width, height, region, kind, a, b, what=what, **kw), f"{what}: host vs device form, {kind}{case}", np.uint8)
                tests_of[(kind, eb, pp)] = (a, b, kw, want)
    # KEEP in the host form: the marks go up and come down
    a, b, kw, want = tests_of[("nonzero", 1, 4)]
    mine = np.full((ty, tx), 7, np.uint8)
    assert rt.mark_tiles(rrt.tile_test("nonzero", a, keep=True), width, height, region=region, marks=mine) is mine
    assert_same_bits(mine, np.where(want != 0, 1, 7).astype(np.uint8), f"{what}: host form with KEEP over sevens", np.uint8)
    # select: eight tests, one plane named twice
    picks = [("nonzero", 1, 4), ("differs", 8, 4), ("set", 4, 1), ("range", 4, 4), ("nonzero", 8, 1), ("differs", 1, 1), ("nonzero", 1, 4), ("differs", 4, 4)]
    union = np.zeros((ty, tx), np.uint8)
    host_tests, dev_tests = [], []
    for k, (kind, eb, pp) in enumerate(picks):
        a, b, kw, want = tests_of[(kind, eb, pp)]
        union |= want
        host_tests.append(rrt.tile_test(kind, a, b, keep=k == 0, **kw))        # (a KEEP on the first test of the host form has nothing to join)
        dev_tests.append(device_test(rrt, torch, kind, a, b, **kw))
    got = rt.select_tiles(host_tests, width, height, region=region)
    assert_same_bits(got, list_of(union), f"{what}: host select of eight tests vs the restatement", np.uint32)
    assert_same_bits(got, device_list(rrt, torch, rt, width, height, region, dev_tests, what=what)[1], f"{what}: host select vs device select", np.uint32)
    assert_same_bits(rt.select_tiles(host_tests[2], width, height, region=region), list_of(tests_of[picks[2]][3]), f"{what}: host select of one test", np.uint32)
    assert (rt.last_stats(), rt.coverage_info()) == before, f"{what}: the tile calls changed the stats or the coverage state"
    assert_same_bits(rt.render(64, 48), rrt.RayTracer(teapot, rrt.default_lights()).render(64, 48), f"{what}: a frame after the tile calls", np.uint32)
