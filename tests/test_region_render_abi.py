"""The part of the fused frame of a region and of a device-resident tile list that needs no GPU (include/rrt.h: rrt_render_region, rrt_render_region_device,
rrt_render_tile_list_device): the exports and the binding's methods, and the argument checks that are made before any HIP call -- through a handle of zeros
that is not a raytracer, so a call that got past its checks would show."""
import ctypes as C

import numpy as np

from abi_checks import PATTERN, assert_refused
from region_render_checks import MAX_TILE_LIST

EXPORTS = {"rrt_render_region_device": 7, "rrt_render_region": 6, "rrt_render_tile_list_device": 8}
W, H = 64, 48


def test_the_three_exports_exist_and_are_bound(rrt):
    L = rrt.lib()
    for name, arity in EXPORTS.items():
        assert name in rrt.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rrt.SYMBOLS[name][1], name
        assert len(rrt.SYMBOLS[name][1]) == arity, f"{name}: {len(rrt.SYMBOLS[name][1])} arguments, want {arity}"
    for method in ("render_region", "render_region_into", "render_tile_list_into"):
        assert callable(getattr(rrt.RayTracer, method)), method


def test_the_launch_bound_of_a_tile_list_is_the_headers(rrt, tmp_path):
    """RRT_MAX_TILE_LIST is what 2^32 - 1 threads hold at 256 per entry."""
    from abi_checks import compiled_values, host_compiler
    assert rrt.MAX_TILE_LIST == MAX_TILE_LIST == (2 ** 32 - 1) // 256
    if host_compiler() is not None:
        assert compiled_values(tmp_path, ["RRT_MAX_TILE_LIST"]) == [MAX_TILE_LIST]


def test_region_calls_are_refused_before_any_gpu_work(rrt):
    L = rrt.lib()
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    out = np.full(W * H, PATTERN, np.uint32)
    up, at = out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(out.ctypes.data)
    ref = lambda r: None if r is None else C.byref(rrt.CRegion(*r))
    forms = {"rrt_render_region": lambda rt, w, h, r, o, pitch: L.rrt_render_region(rt, w, h, ref(r), up if o else None, pitch),
             "rrt_render_region_device": lambda rt, w, h, r, o, pitch: L.rrt_render_region_device(rt, w, h, ref(r), at if o else None, pitch, None)}
    bad = [("a NULL raytracer", (None, W, H, None, True, 0)), ("a NULL raytracer and a region", (None, W, H, (1, 1, 2, 2), True, 2)),
           ("a NULL output", (fake, W, H, None, False, 0)), ("a NULL output and a region", (fake, W, H, (1, 1, 2, 2), False, 0)),
           ("width 0", (fake, 0, H, None, True, 0)), ("height 0", (fake, W, 0, None, True, 0)), ("a frame of 2^31 pixels", (fake, 65536, 32768, None, True, 0)),
           ("a pitch of w - 1", (fake, W, H, (5, 3, 50, 41), True, 49)), ("a pitch of w - 1, whole frame", (fake, W, H, None, True, W - 1)),
           ("a pitch of 1 for two columns", (fake, W, H, (0, 0, 2, 1), True, 1)),
           ("a region with w == 0", (fake, W, H, (1, 1, 0, 2), True, 0)), ("a region with h == 0", (fake, W, H, (1, 1, 2, 0), True, 0)),
           ("a region sticking out to the right", (fake, W, H, (60, 0, 5, 2), True, 0)), ("a region sticking out below", (fake, W, H, (0, 47, 2, 2), True, 0)),
           ("a region beyond 2^32", (fake, W, H, (0xFFFFFFFF, 0, 2, 2), True, 0))]
    calls = [(f"{form}, {what}", lambda call=call, args=args: call(*args)) for form, call in forms.items() for what, args in bad]
    assert len(calls) == 2 * 15
    assert_refused(rrt, L, calls, {"out": out})
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def test_tile_list_calls_are_refused_before_any_gpu_work(rrt):
    L = rrt.lib()
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    fb = np.full(W * H, PATTERN, np.uint32)
    tiles = np.full(8, PATTERN, np.uint32)
    count = np.full(1, PATTERN, np.uint32)
    at = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    call = lambda rt, w, h, n, c, t, f: L.rrt_render_tile_list_device(rt, w, h, n, at(c), at(t), at(f), None)
    bad = [("a NULL raytracer", (None, W, H, 8, count, tiles, fb)), ("a NULL raytracer, n = 0", (None, W, H, 0, None, None, fb)),
           ("width 0", (fake, 0, H, 8, None, tiles, fb)), ("height 0", (fake, W, 0, 8, None, tiles, fb)), ("a frame of 2^31 pixels", (fake, 65536, 32768, 8, None, tiles, fb)),
           ("a NULL list with n > 0", (fake, W, H, 8, None, None, fb)), ("a NULL list with n > 0 and a bound", (fake, W, H, 1, count, None, fb)),
           ("a NULL framebuffer", (fake, W, H, 8, None, tiles, None)), ("a NULL framebuffer, n = 0", (fake, W, H, 0, None, tiles, None)),
           ("n one beyond the launch bound", (fake, W, H, MAX_TILE_LIST + 1, None, tiles, fb)), ("n = 2^32 - 1", (fake, W, H, 0xFFFFFFFF, count, tiles, fb))]
    assert_refused(rrt, L, [(f"rrt_render_tile_list_device, {what}", lambda args=args: call(*args)) for what, args in bad], {"fb": fb, "tiles": tiles, "count": count})
    # n == 0 with a framebuffer: RRT_OK with nothing enqueued (the handle is not a raytracer), with or without a list and a bound
    assert call(fake, W, H, 0, None, None, fb) == rrt.OK and call(fake, W, H, 0, count, tiles, fb) == rrt.OK
    assert (fb == PATTERN).all() and (tiles == PATTERN).all() and count[0] == PATTERN, "an empty list wrote something"
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def test_the_binding_refuses_what_does_not_fit_the_buffer(rrt, monkeypatch):
    """render_region_into: the rows it names must lie inside the tensor; nothing reaches the library before that."""
    import pytest
    import torch

    from abi_checks import NoLibrary, bare_raytracer, fake_device
    rt = bare_raytracer(rrt)
    fb = fake_device(torch.zeros(31 * 96, dtype=torch.int32))
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    for what, kw in (("a pitch below the width", dict(pitch=76)), ("an offset that pushes the last row out", dict(pitch=96, offset=20)),
                     ("a negative offset", dict(pitch=96, offset=-1)), ("a tight region larger than the tensor", dict(region=(0, 0, 203, 117)))):
        with pytest.raises(AssertionError):
            rt.render_region_into(fb, 203, 117, **dict(dict(region=(13, 50, 77, 31), stream=0), **kw))
    with pytest.raises(AssertionError):
        rt.render_region_into(np.zeros(31 * 96, np.uint32), 203, 117, region=(13, 50, 77, 31), pitch=96, stream=0)
    with pytest.raises(AssertionError):
        rt.render_tile_list_into(fake_device(torch.zeros(64 * 47, dtype=torch.int32)), fake_device(torch.zeros(4, dtype=torch.int32)), 64, 48, stream=0)
    with pytest.raises(AssertionError):
        rt.render_tile_list_into(fake_device(torch.zeros(64 * 48, dtype=torch.int32)), fake_device(torch.zeros(4, dtype=torch.int64)), 64, 48, stream=0)


def test_what_the_binding_passes_on(rrt, monkeypatch):
    """The in-place form: the pointer is the tensor's plus 4 * offset, the pitch goes through; without a pitch the region's width; the list's length is n."""
    import torch

    from abi_checks import CallRecorder, bare_raytracer, fake_device
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    rt = bare_raytracer(rrt)
    fb = torch.zeros(117 * 203, dtype=torch.int32)
    rt.render_region_into(fake_device(fb), 203, 117, region=(13, 50, 77, 31), pitch=203, offset=50 * 203 + 13, stream=7)
    rt.render_region_into(fake_device(fb), 203, 117, stream=7)
    tiles, bound = torch.zeros(5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    rt.render_tile_list_into(fake_device(fb), fake_device(tiles), 203, 117, stream=7, bound_t=fake_device(bound))
    rt.render_tile_list_into(fake_device(fb), fake_device(tiles), 203, 117, stream=7)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = rec.calls
    assert (n0, n1, n2, n3) == ("rrt_render_region_device", "rrt_render_region_device", "rrt_render_tile_list_device", "rrt_render_tile_list_device")
    assert a0[1:3] == (203, 117) and a0[4].value == fb.data_ptr() + 4 * (50 * 203 + 13) and a0[5] == 203 and a0[6].value == 7, a0
    assert a1[3] is None and a1[4].value == fb.data_ptr() and a1[5] == 203, a1
    assert a2[1:4] == (203, 117, 5) and (a2[4].value, a2[5].value, a2[6].value) == (bound.data_ptr(), tiles.data_ptr(), fb.data_ptr()), a2
    assert a3[3] == 5 and a3[4] is None, a3
