"""Tile selection of the C ABI (include/rrt.h: rrt_tile_test, rrt_mark_tiles[_device], rrt_select_tiles[_device]) as far as no GPU is needed: the struct layout on
both sides, the exported symbols, every argument check the library makes before any HIP call and before it looks at the handle, the checks the Python mirror
makes before it calls the library, and what it hands over."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_layout, compiled_values, fake_device

FIELDS = ("test", "elem_bytes", "per_pixel", "lo", "hi", "set", "_pad", "a", "b")
OFFSETS = (0, 4, 8, 12, 16, 20, 52, 56, 64)


def test_the_struct_is_72_bytes_on_both_sides(rrt, tmp_path):
    assert C.sizeof(rrt.CTileTest) == 72 and rrt.STRUCTS["rrt_tile_test"] is rrt.CTileTest
    assert tuple(n for n, _ in rrt.CTileTest._fields_) == FIELDS
    assert tuple(getattr(rrt.CTileTest, n).offset for n in FIELDS) == OFFSETS and rrt.CTileTest.set.size == 32
    assert compiled_layout(tmp_path, "rrt_tile_test", FIELDS) == (72, list(OFFSETS))
    assert compiled_values(tmp_path, ("RRT_TILE_NONZERO", "RRT_TILE_RANGE", "RRT_TILE_SET", "RRT_TILE_DIFFERS", "RRT_TILE_KEEP", "RRT_MAX_TILE_TESTS", "RRT_MAX_TILE_LIST",
                                      "sizeof(((rrt_tile_test *)0)->set)", "sizeof(((rrt_tile_test *)0)->set[0])")) == [0, 1, 2, 3, 0x100, 8, rrt.MAX_TILE_LIST, 32, 4]
    assert rrt.TILE_TESTS == ("nonzero", "range", "set", "differs") and rrt.TILE_KEEP == 0x100 and rrt.MAX_TILE_TESTS == 8


def test_the_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    P, R, T, u32 = C.c_void_p, C.POINTER(rrt.CRegion), C.POINTER(rrt.CTileTest), C.c_uint32
    want = {"rrt_mark_tiles_device": (C.c_int, [P, u32, u32, R, T, P, P]),
            "rrt_mark_tiles": (C.c_int, [P, u32, u32, R, T, C.POINTER(C.c_uint8)]),
            "rrt_select_tiles_device": (C.c_int, [P, u32, u32, R, T, u32, P, P, P, P, C.c_size_t, P]),
            "rrt_select_tiles": (C.c_int, [P, u32, u32, R, T, u32, C.POINTER(u32), C.POINTER(u32)])}
    for name, sig in want.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == sig, name
        assert getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0]
    for method in ("mark_tiles", "mark_tiles_into", "select_tiles", "select_tiles_into"):
        assert callable(getattr(rrt.RayTracer, method)), method
    assert callable(rrt.tile_test) and rrt.tile_count(203, 117) == (26, 15)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """Every refusal of rrt.h in all four forms, through a handle that is the address of 4 KB of zeros: a check that came after the handle's first use would
    crash, not refuse.  (The device forms' pointers are host addresses here: a call that got as far as a launch would fail in another way.)  The error detail is
    set and the outputs keep their pattern."""
    L = rrt.lib()
    W, H = 16, 16                                                                  # 4 tiles
    plane = np.zeros((H, W, 4), np.uint64)                                         # (aligned to 8; its address + 4 is aligned to 4 only, + 1 to 1 only)
    outs = {name: np.full(64, PATTERN, np.uint32) for name in ("marks", "tiles", "count", "scratch")}
    at = lambda a: a.ctypes.data
    A = at(plane)
    scratch_bytes = rrt.compact_scratch_bytes(4)
    assert 0 < scratch_bytes <= outs["scratch"].nbytes
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)

    def T(test=0, elem_bytes=4, per_pixel=4, a=A, b=A, **kw):
        return rrt.CTileTest(test=test, elem_bytes=elem_bytes, per_pixel=per_pixel, a=a, b=b, **kw)
    good = T()
    ref = lambda s: None if s is None else C.byref(s)
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    M, TL, CN, S = outs["marks"], outs["tiles"], outs["count"], outs["scratch"]

    def pair(tests):                                                               # one test or a list of them -> (pointer, count)
        if tests is None or isinstance(tests, rrt.CTileTest):
            return ref(tests), 1
        arr = (rrt.CTileTest * max(1, len(tests)))(*tests)
        return arr, len(tests)

    def mark_dev(rt, t, w=W, h=H, region=None, marks=M, **kw):
        return L.rrt_mark_tiles_device(rt, w, h, ref(region), pair(t)[0], None if marks is None else at(marks), None)

    def mark_host(rt, t, w=W, h=H, region=None, marks=M, **kw):
        return L.rrt_mark_tiles(rt, w, h, ref(region), pair(t)[0], u8(marks))

    def select_dev(rt, t, w=W, h=H, region=None, marks=M, n=None, tiles=TL, count=CN, scratch=S, sb=scratch_bytes):
        p, k = pair(t)
        return L.rrt_select_tiles_device(rt, w, h, ref(region), p, k if n is None else n, None if marks is None else at(marks), None if tiles is None else at(tiles),
                                         None if count is None else at(count), None if scratch is None else at(scratch), sb, None)

    def select_host(rt, t, w=W, h=H, region=None, marks=M, n=None, tiles=TL, count=CN, **kw):
        p, k = pair(t)
        return L.rrt_select_tiles(rt, w, h, ref(region), p, k if n is None else n, u32(tiles), u32(count))
    forms = (("rrt_mark_tiles_device", mark_dev), ("rrt_mark_tiles", mark_host), ("rrt_select_tiles_device", select_dev), ("rrt_select_tiles", select_host))
    calls = []
    for form, call in forms:
        calls += [(f"{form}, a NULL raytracer", lambda call=call: call(None, good)),
                  (f"{form}, NULL test(s)", lambda call=call: call(fake, None)),
                  (f"{form}, width 0", lambda call=call: call(fake, good, w=0)),
                  (f"{form}, height 0", lambda call=call: call(fake, good, h=0)),
                  (f"{form}, 2^16 x 2^16 pixels", lambda call=call: call(fake, good, w=65536, h=65536)),
                  (f"{form}, a region without width", lambda call=call: call(fake, good, region=rrt.CRegion(0, 0, 0, 4))),
                  (f"{form}, a region without height", lambda call=call: call(fake, good, region=rrt.CRegion(0, 0, 4, 0))),
                  (f"{form}, a region beyond the right edge", lambda call=call: call(fake, good, region=rrt.CRegion(9, 0, 8, 4))),
                  (f"{form}, a region beyond the bottom edge", lambda call=call: call(fake, good, region=rrt.CRegion(0, 16, 1, 1))),
                  (f"{form}, a region whose end wraps", lambda call=call: call(fake, good, region=rrt.CRegion(0xFFFFFFFF, 0, 2, 1))),
                  (f"{form}, test 4", lambda call=call: call(fake, T(test=4))),
                  (f"{form}, test 4 | KEEP", lambda call=call: call(fake, T(test=4 | 0x100))),
                  (f"{form}, test 0x200", lambda call=call: call(fake, T(test=0x200))),
                  (f"{form}, test 0xFFFFFFFF", lambda call=call: call(fake, T(test=0xFFFFFFFF))),
                  (f"{form}, per_pixel 0", lambda call=call: call(fake, T(per_pixel=0))),
                  (f"{form}, per_pixel 2", lambda call=call: call(fake, T(per_pixel=2))),
                  (f"{form}, per_pixel 8", lambda call=call: call(fake, T(per_pixel=8))),
                  (f"{form}, RANGE over bytes", lambda call=call: call(fake, T(test=1, elem_bytes=1, hi=9))),
                  (f"{form}, RANGE over 8-byte elements", lambda call=call: call(fake, T(test=1, elem_bytes=8, hi=9))),
                  (f"{form}, SET over bytes", lambda call=call: call(fake, T(test=2, elem_bytes=1))),
                  (f"{form}, SET | KEEP over 8-byte elements", lambda call=call: call(fake, T(test=2 | 0x100, elem_bytes=8))),
                  (f"{form}, a NULL a", lambda call=call: call(fake, T(a=None))),
                  (f"{form}, DIFFERS with a NULL b", lambda call=call: call(fake, T(test=3, b=None))),
                  (f"{form}, a misaligned to 4", lambda call=call: call(fake, T(a=A + 2))),
                  (f"{form}, a misaligned to 8", lambda call=call: call(fake, T(elem_bytes=8, a=A + 4))),
                  (f"{form}, DIFFERS with b misaligned to 8", lambda call=call: call(fake, T(test=3, elem_bytes=8, b=A + 4))),
                  (f"{form}, more tiles than RRT_MAX_TILE_LIST", lambda call=call: call(fake, good, w=8 * 4097, h=8 * 4096))]
        calls += [(f"{form}, elem_bytes {e}", lambda call=call, e=e: call(fake, T(elem_bytes=e))) for e in (0, 2, 3, 16, 0xFFFFFFFF)]
    for form, call in forms[:3]:
        calls += [(f"{form}, NULL marks", lambda call=call: call(fake, good, marks=None))]
    for form, call in forms[2:]:
        calls += [(f"{form}, n_tests 0", lambda call=call: call(fake, [good], n=0)),
                  (f"{form}, n_tests 9", lambda call=call: call(fake, [good] * 9)),
                  (f"{form}, n_tests 0xFFFFFFFF", lambda call=call: call(fake, [good], n=0xFFFFFFFF)),
                  (f"{form}, a bad second test", lambda call=call: call(fake, [good, T(elem_bytes=2)])),
                  (f"{form}, a bad eighth test", lambda call=call: call(fake, [good] * 7 + [T(test=3, b=None)])),
                  (f"{form}, both list outputs NULL", lambda call=call: call(fake, good, tiles=None, count=None))]
    calls += [("rrt_select_tiles_device, a NULL scratch", lambda: select_dev(fake, good, scratch=None)),
              ("rrt_select_tiles_device, scratch one byte short", lambda: select_dev(fake, good, sb=scratch_bytes - 1)),
              ("rrt_select_tiles_device, scratch_bytes 0", lambda: select_dev(fake, good, sb=0))]
    assert len(calls) == 4 * (27 + 5) + 3 + 2 * 6 + 3
    assert_refused(rrt, L, calls, outs)
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"
    # what is NOT refused for its alignment: a plane aligned to its elements and no more gets past every check (and is stopped by the next one, the NULL marks)
    for eb, off in ((1, 1), (4, 4), (8, 8)):
        assert_refused(rrt, L, [(f"elem_bytes {eb} at +{off}", lambda: mark_dev(fake, T(test=3, elem_bytes=eb, a=A + off, b=A + off), marks=None))])
        assert b"marks" in L.rrt_last_error_detail(), L.rrt_last_error_detail()


def test_the_binding_builds_the_struct(rrt):
    a = np.zeros((6, 5, 4), np.uint32)
    t = rrt.tile_test("set", a, values=(0, 31, 32, 255))
    assert (t.test, t.elem_bytes, t.per_pixel, t.a, t.b) == (2, 4, 4, a.ctypes.data, None) and list(t.set) == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]
    t = rrt.tile_test("range", a, lo=3, hi=0xFFFFFFFF, keep=True)
    assert (t.test, t.lo, t.hi) == (1 | 0x100, 3, 0xFFFFFFFF) and list(t.set) == [0] * 8
    fb, fb2 = np.zeros((6, 5)), np.ones((6, 5))
    t = rrt.tile_test("differs", fb, fb2)
    assert (t.test, t.elem_bytes, t.per_pixel, t.a, t.b) == (3, 8, 1, fb.ctypes.data, fb2.ctypes.data)
    t = rrt.tile_test("nonzero", np.zeros((6, 5, 4), np.uint8), b=fb)             # (b is not read: not handed over)
    assert (t.test, t.elem_bytes, t.per_pixel, t.b) == (0, 1, 4, None)
    for kw, what in ((dict(kind="any", a=a), "unknown kind"), (dict(kind="nonzero", a=None), "needs plane a"), (dict(kind="differs", a=a), "needs plane b"),
                     (dict(kind="differs", a=a, b=np.zeros((6, 5, 4))), "differ in shape or element size"), (dict(kind="differs", a=a, b=a[:5]), "differ in shape"),
                     (dict(kind="nonzero", a=np.zeros(30, np.uint8)), "want \\[h\\]\\[w\\] or"), (dict(kind="nonzero", a=np.zeros((6, 5, 3))), "want \\[h\\]\\[w\\] or"),
                     (dict(kind="nonzero", a=np.zeros((6, 5), np.uint16)), "elements of 2 bytes"), (dict(kind="range", a=fb), "elements of 8 bytes, want 4"),
                     (dict(kind="set", a=np.zeros((6, 5), np.uint8)), "elements of 1 bytes, want 4"), (dict(kind="set", a=a, values=(256,)), "value 256 of a set"),
                     (dict(kind="set", a=a, values=(-1,)), "value -1 of a set")):
        with pytest.raises(ValueError, match=what):
            rrt.tile_test(**kw)


def test_the_binding_refuses_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    W, H = 20, 12                                                                  # 3 x 2 tiles
    dev = lambda shape, dtype=torch.int32: fake_device(torch.zeros(shape, dtype=dtype))
    u1, i4 = (lambda n: dev(n, torch.uint8)), (lambda n: dev(n))
    good = rrt.tile_test("nonzero", dev((H, W, 4)))
    host = rrt.tile_test("nonzero", np.zeros((H, W, 4), np.uint32))

    def into(tests=good, tiles_t=None, count_t=None, marks_t=None, scratch_t=None, region=None, none=()):
        given = dict(tiles_t=i4(6) if tiles_t is None else tiles_t, count_t=i4(1) if count_t is None else count_t)
        given.update({k: None for k in none})
        rt.select_tiles_into(given["tiles_t"], given["count_t"], u1(6) if marks_t is None else marks_t, u1(64) if scratch_t is None else scratch_t, tests, W, H,
                             region=region, stream=0)
    # host planes to a device form and device planes to a host form
    for call in (lambda: into(host), lambda: rt.mark_tiles_into(u1(6), host, W, H, stream=0)):
        with pytest.raises(AssertionError, match="a test's planes are host arrays"):
            call()
    for call in (lambda: rt.mark_tiles(good, W, H), lambda: rt.select_tiles([host, good], W, H)):
        with pytest.raises(AssertionError, match="a test's planes are device tensors"):
            call()
    with pytest.raises(AssertionError, match="not from tile_test"):
        into(rrt.CTileTest())
    # a plane that is not the region's
    with pytest.raises(ValueError, match="a plane of 12 x 20 pixels for a region of 4 x 7"):
        into(region=(1, 2, 7, 4))
    with pytest.raises(ValueError, match="a plane of 12 x 20 pixels for a region of 4 x 7"):
        rt.mark_tiles(host, W, H, region=(1, 2, 7, 4))
    # the number of tests
    for tests in ([], [good] * 9):
        with pytest.raises(ValueError, match="tests, want 1 to 8"):
            into(tests)
        with pytest.raises(ValueError, match="tests, want 1 to 8"):
            rt.select_tiles([host] * len(tests), W, H)
    # the outputs
    with pytest.raises(AssertionError, match="marks: not a device tensor"):
        into(marks_t=np.zeros(6, np.uint8))
    with pytest.raises(AssertionError, match="marks: want 6 contiguous elements of 1 bytes"):
        into(marks_t=u1(7))
    with pytest.raises(AssertionError, match="marks: want 6 contiguous elements of 1 bytes"):
        rt.mark_tiles_into(i4(6), good, W, H, stream=0)
    with pytest.raises(AssertionError, match="tiles: want 6 contiguous elements of 4 bytes"):
        into(tiles_t=i4(5))
    with pytest.raises(AssertionError, match="tiles: want 6 contiguous elements of 4 bytes"):
        into(tiles_t=u1(6))
    with pytest.raises(AssertionError, match="count: want 1 contiguous elements of 4 bytes"):
        into(count_t=i4(2))
    with pytest.raises(AssertionError, match="tiles and count are both None"):
        into(none=("tiles_t", "count_t"))
    with pytest.raises(AssertionError, match="scratch: not a contiguous device tensor"):
        into(scratch_t=np.zeros(64, np.uint8))
    with pytest.raises(AssertionError, match="marks is not a contiguous writable uint8 array of 6 elements"):
        rt.mark_tiles(host, W, H, marks=np.zeros((2, 4), np.uint8))
    with pytest.raises(AssertionError, match="marks is not a contiguous writable uint8 array of 6 elements"):
        rt.mark_tiles(host, W, H, marks=np.zeros((2, 3), np.uint32))


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    W, H = 20, 12                                                                  # 3 x 2 tiles
    dev = lambda shape, dtype=torch.int32: fake_device(torch.zeros(shape, dtype=dtype))
    mat, fb_a, fb_b = dev((4, 7, 4)), dev((4, 7)), dev((4, 7))
    tests = [rrt.tile_test("set", mat, values=(0, 3)), rrt.tile_test("differs", fb_a, fb_b, keep=True)]
    tiles, count, marks, scratch = dev(6), dev(1), dev(6, torch.uint8), dev(4, torch.int64)
    rt.select_tiles_into(tiles, count, marks, scratch, tests, W, H, region=(1, 2, 7, 4), stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_select_tiles_device" and len(args) == 12 and args[0] is None and args[1:3] == (W, H)
    r = args[3]._obj
    assert (r.x0, r.y0, r.w, r.h) == (1, 2, 7, 4)
    assert len(args[4]) == 2 and args[5] == 2
    assert (args[4][0].test, args[4][0].elem_bytes, args[4][0].per_pixel, args[4][0].a, args[4][0].b, args[4][0].set[0]) == (2, 4, 4, mat.data_ptr(), None, 0b1001)
    assert (args[4][1].test, args[4][1].elem_bytes, args[4][1].per_pixel, args[4][1].a, args[4][1].b) == (3 | 0x100, 4, 1, fb_a.data_ptr(), fb_b.data_ptr())
    assert (args[6].value, args[7].value, args[8].value, args[9].value, args[10], args[11].value) == (marks.data_ptr(), tiles.data_ptr(), count.data_ptr(),
                                                                                                      scratch.data_ptr(), 32, 0x51)
    # the count alone, the whole frame, one test that is not in a list
    rec.calls.clear()
    whole = rrt.tile_test("nonzero", dev((H, W), torch.uint8))
    rt.select_tiles_into(None, count, marks, scratch, whole, W, H, stream=7)
    (name, args), = rec.calls
    assert args[3] is None and len(args[4]) == 1 and args[5] == 1 and args[7] is None and args[8].value == count.data_ptr()
    # the mark call
    rec.calls.clear()
    rt.mark_tiles_into(marks, tests[1], W, H, region=(1, 2, 7, 4), stream=9)
    (name, args), = rec.calls
    assert name == "rrt_mark_tiles_device" and len(args) == 7 and args[1:3] == (W, H) and args[3]._obj.w == 7
    assert (args[4][0].test, args[4][0].b, args[5].value, args[6].value) == (3 | 0x100, fb_b.data_ptr(), marks.data_ptr(), 9)
    # the host forms
    rec.calls.clear()
    plane = np.zeros((H, W, 4))
    got = rt.mark_tiles(rrt.tile_test("nonzero", plane), W, H)
    mine = np.full((2, 3), 7, np.uint8)
    assert rt.mark_tiles(rrt.tile_test("nonzero", plane, keep=True), W, H, marks=mine) is mine
    lst = rt.select_tiles([rrt.tile_test("nonzero", plane), rrt.tile_test("differs", plane, plane)], W, H)
    (n1, a1), (n2, a2), (n3, a3) = rec.calls
    assert n1 == "rrt_mark_tiles" and len(a1) == 6 and a1[3] is None and (a1[4][0].elem_bytes, a1[4][0].per_pixel, a1[4][0].a) == (8, 4, plane.ctypes.data)
    assert got.shape == (2, 3) and got.dtype == np.uint8 and C.cast(a1[5], C.c_void_p).value == got.ctypes.data
    assert n2 == "rrt_mark_tiles" and a2[4][0].test == 0x100 and C.cast(a2[5], C.c_void_p).value == mine.ctypes.data and (mine == 7).all()
    assert n3 == "rrt_select_tiles" and len(a3) == 8 and a3[5] == 2 and a3[4][1].b == plane.ctypes.data
    assert lst.dtype == np.uint32 and lst.shape == (0,)
