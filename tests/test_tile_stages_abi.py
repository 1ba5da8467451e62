"""The part of the deferred stages over a device-resident tile list that needs no GPU (include/rrt.h: rrt_render_visibility_tile_list_device,
rrt_render_surface_tile_list_device, rrt_shade_surface_tile_list_device, rrt_ambient_surface_tile_list_device): the exports and the binding's methods, and the
argument checks that are made before any HIP call -- through a handle of zeros that is not a raytracer, so a call that got past its checks would show."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, assert_refused
from region_render_checks import MAX_TILE_LIST

EXPORTS = {"rrt_render_visibility_tile_list_device": 8, "rrt_render_surface_tile_list_device": 9, "rrt_shade_surface_tile_list_device": 10,
           "rrt_ambient_surface_tile_list_device": 10}
METHODS = ("visibility_tile_list_into", "surface_tile_list_into", "shade_tile_list_into", "ambient_tile_list_into")
W, H = 64, 48


def test_the_four_exports_exist_and_are_bound(rrt):
    L = rrt.lib()
    for name, arity in EXPORTS.items():
        assert name in rrt.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rrt.SYMBOLS[name][1], name
        assert len(rrt.SYMBOLS[name][1]) == arity, f"{name}: {len(rrt.SYMBOLS[name][1])} arguments, want {arity}"
    for method in METHODS:
        assert callable(getattr(rrt.RayTracer, method)), method


class Arrays:
    """Host arrays that stand for the planes of a W x H frame (a refused call never looks at what a pointer points to), a list and a bound, all filled with PATTERN."""

    def __init__(self):
        n = 4 * W * H
        self.a = {name: np.full(count, PATTERN, np.uint32) for name, count in
                  (("hit", n // 4), ("t", 2 * n), ("u", 2 * n), ("v", 2 * n), ("tri", n), ("albedo", n), ("point", 6 * n), ("normal", 6 * n), ("material", n),
                   ("lights", n), ("occluded", n), ("grey", W * H), ("fb", W * H), ("tiles", 8), ("count", 1))}
        self.dirs = np.tile(np.array([0.0, 0.0, 1.0]), (4, 1))

    def at(self, name):
        return self.a[name].ctypes.data

    def struct(self, rrt, cls, names):
        return C.byref(cls(**{n: self.at(n) for n in names}))

    def samples(self, rrt, n=4, max_t=1.0, dirs=True):
        d = self.dirs.ctypes.data_as(C.POINTER(C.c_double)) if dirs else None
        return C.byref(rrt.CAmbientSamples(dirs=d, n=n, max_t=max_t))


def stage_calls(rrt, L, A):
    """{symbol: (call(rt, w, h, n, count, tiles, **override), {override name: the refusals of the region call of the same name that it provokes})}.  An override
    replaces one of the call's struct or pointer arguments."""
    ptr = lambda name: None if name is None else C.c_void_p(A.at(name))
    vis_all, surf_all = ("hit", "t", "u", "v", "tri", "albedo"), ("point", "normal", "material", "lights")
    V, S = rrt.CVisibility, rrt.CSurface

    def visibility(rt, w, h, n, c, t, planes=A.struct(rrt, V, vis_all)):
        return L.rrt_render_visibility_tile_list_device(rt, w, h, n, ptr(c), ptr(t), planes, None)

    def surface(rt, w, h, n, c, t, vis=A.struct(rrt, V, vis_all), planes=A.struct(rrt, S, surf_all)):
        return L.rrt_render_surface_tile_list_device(rt, w, h, n, ptr(c), ptr(t), vis, planes, None)

    def shade(rt, w, h, n, c, t, vis=A.struct(rrt, V, ("albedo",)), planes=A.struct(rrt, S, surf_all), fb=ptr("fb")):
        return L.rrt_shade_surface_tile_list_device(rt, w, h, n, ptr(c), ptr(t), vis, planes, fb, None)

    def ambient(rt, w, h, n, c, t, planes=A.struct(rrt, S, surf_all[:3]), samples=A.samples(rrt), out=A.struct(rrt, rrt.CAmbient, ("occluded", "grey"))):
        return L.rrt_ambient_surface_tile_list_device(rt, w, h, n, ptr(c), ptr(t), planes, samples, out, None)

    nan_dirs = np.tile(np.array([0.0, np.nan, 1.0]), (4, 1))
    A.nan_dirs = nan_dirs                                                         # (kept alive)
    return {
        "rrt_render_visibility_tile_list_device": (visibility, {
            "a NULL planes struct": dict(planes=None), "no plane requested": dict(planes=A.struct(rrt, V, ()))}),
        "rrt_render_surface_tile_list_device": (surface, {
            "a NULL surface struct": dict(planes=None), "no surface plane requested": dict(planes=A.struct(rrt, S, ())),
            "no surface plane requested, no visibility struct": dict(vis=None, planes=A.struct(rrt, S, ()))}),
        "rrt_shade_surface_tile_list_device": (shade, {
            "a NULL visibility struct": dict(vis=None), "a NULL surface struct": dict(planes=None), "a NULL framebuffer": dict(fb=None),
            "no albedo": dict(vis=A.struct(rrt, V, ("hit", "t"))), "no point": dict(planes=A.struct(rrt, S, ("normal", "material", "lights"))),
            "no normal": dict(planes=A.struct(rrt, S, ("point", "material"))), "no material": dict(planes=A.struct(rrt, S, ("point", "normal", "lights")))}),
        "rrt_ambient_surface_tile_list_device": (ambient, {
            "a NULL surface struct": dict(planes=None), "a NULL sample table": dict(samples=None), "a NULL output struct": dict(out=None),
            "no point": dict(planes=A.struct(rrt, S, ("normal", "material"))), "no normal": dict(planes=A.struct(rrt, S, ("point", "material"))),
            "no material": dict(planes=A.struct(rrt, S, ("point", "normal"))), "no output requested": dict(out=A.struct(rrt, rrt.CAmbient, ())),
            "no sample": dict(samples=A.samples(rrt, n=0)), "a sample more than the table holds": dict(samples=A.samples(rrt, n=rrt.MAX_AMBIENT_SAMPLES + 1)),
            "NULL directions": dict(samples=A.samples(rrt, dirs=False)), "max_t = 0": dict(samples=A.samples(rrt, max_t=0.0)),
            "max_t = NaN": dict(samples=A.samples(rrt, max_t=float("nan"))),
            "a NaN direction": dict(samples=C.byref(rrt.CAmbientSamples(dirs=nan_dirs.ctypes.data_as(C.POINTER(C.c_double)), n=4, max_t=1.0)))}),
    }


def test_every_refusal_arrives_before_any_gpu_work(rrt):
    """What each of the four shares with the tile-list frame (rt, frame size, n, the list), and the refusals of the region call of the same name -- those also
    with n = 0, where a call that is not refused returns RRT_OK: the stage's checks come before the list's."""
    L = rrt.lib()
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    A = Arrays()
    calls = []
    for symbol, (call, own) in stage_calls(rrt, L, A).items():
        shared = [("a NULL raytracer", (None, W, H, 8, "count", "tiles")), ("a NULL raytracer, n = 0", (None, W, H, 0, None, None)),
                  ("width 0", (fake, 0, H, 8, None, "tiles")), ("height 0", (fake, W, 0, 8, None, "tiles")), ("a frame of 2^31 pixels", (fake, 65536, 32768, 8, None, "tiles")),
                  ("a NULL list with n > 0", (fake, W, H, 8, None, None)), ("a NULL list with n > 0 and a bound", (fake, W, H, 1, "count", None)),
                  ("n one beyond the launch bound", (fake, W, H, MAX_TILE_LIST + 1, None, "tiles")), ("n = 2^32 - 1", (fake, W, H, 0xFFFFFFFF, "count", "tiles"))]
        calls += [(f"{symbol}, {what}", lambda call=call, args=args: call(*args)) for what, args in shared]
        for what, kw in own.items():
            calls.append((f"{symbol}, {what}", lambda call=call, kw=kw: call(fake, W, H, 8, "count", "tiles", **kw)))
            calls.append((f"{symbol}, {what}, n = 0", lambda call=call, kw=kw: call(fake, W, H, 0, None, None, **kw)))
    assert len(calls) == 4 * 9 + 2 * (2 + 3 + 7 + 13)
    assert_refused(rrt, L, calls, A.a)
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def test_an_empty_list_is_ok_and_launches_nothing(rrt):
    """n == 0 with good arguments: RRT_OK with nothing enqueued (the handle is not a raytracer), with or without a list and a bound."""
    L = rrt.lib()
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    A = Arrays()
    for symbol, (call, _) in stage_calls(rrt, L, A).items():
        assert call(fake, W, H, 0, None, None) == rrt.OK and call(fake, W, H, 0, "count", "tiles") == rrt.OK, symbol
    assert all((a == PATTERN).all() for a in A.a.values()), "an empty list wrote something"
    assert bytes(blank) == bytes(4096), "a call with an empty list wrote through the handle"


def device_planes(torch, fake_device, w, h, names, short=None):
    """{plane: stand-in device tensor of a whole w x h frame}; `short` is one element short of it"""
    size = {"hit": (4, torch.uint8), "t": (4, torch.float64), "u": (4, torch.float64), "v": (4, torch.float64), "tri": (4, torch.int32), "albedo": (4, torch.int32),
            "point": (12, torch.float64), "normal": (12, torch.float64), "material": (4, torch.int32), "lights": (4, torch.int32), "occluded": (4, torch.int32),
            "grey": (1, torch.int32)}
    raw = {n: torch.zeros(size[n][0] * w * h - (1 if n == short else 0), dtype=size[n][1]) for n in names}
    return raw, {n: fake_device(t) for n, t in raw.items()}


VIS, SURF, SHADE_IN, AMB_IN, AMB_OUT = ("hit", "t", "u", "v", "tri", "albedo"), ("point", "normal", "material", "lights"), \
    ("point", "normal", "material", "albedo", "lights"), ("point", "normal", "material"), ("occluded", "grey")
DIRS = [[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]]


def test_the_binding_refuses_tensors_that_do_not_hold_a_whole_frame(rrt, monkeypatch):
    import torch

    from abi_checks import NoLibrary, bare_raytracer, fake_device
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    w, h = 203, 117
    tiles, bound = fake_device(torch.zeros(5, dtype=torch.int32)), fake_device(torch.zeros(1, dtype=torch.int32))
    fb = fake_device(torch.zeros(w * h, dtype=torch.int32))
    planes = lambda names, short=None: device_planes(torch, fake_device, w, h, names, short)[1]
    region = lambda names: device_planes(torch, fake_device, 77, 31, names)[1]           # what the twin takes for a region: not a whole frame
    refused = []
    for name in VIS:
        refused.append(lambda name=name: rt.visibility_tile_list_into(planes(VIS, name), tiles, w, h, stream=0))
    for name in VIS + SURF:
        refused.append(lambda name=name: rt.surface_tile_list_into(planes(VIS + SURF, name), tiles, w, h, stream=0))
    for name in SHADE_IN:
        refused.append(lambda name=name: rt.shade_tile_list_into(fb, planes(SHADE_IN, name), tiles, w, h, stream=0))
    for name in AMB_IN:
        refused.append(lambda name=name: rt.ambient_tile_list_into(planes(AMB_OUT), planes(AMB_IN, name), DIRS, 1.0, tiles, w, h, stream=0))
    for name in AMB_OUT:
        refused.append(lambda name=name: rt.ambient_tile_list_into(planes(AMB_OUT, name), planes(AMB_IN), DIRS, 1.0, tiles, w, h, stream=0))
    refused += [lambda: rt.visibility_tile_list_into(region(VIS), tiles, w, h, stream=0), lambda: rt.surface_tile_list_into(region(SURF), tiles, w, h, stream=0),
                lambda: rt.shade_tile_list_into(fb, region(SHADE_IN), tiles, w, h, stream=0),
                lambda: rt.shade_tile_list_into(fake_device(torch.zeros(77 * 31, dtype=torch.int32)), planes(SHADE_IN), tiles, w, h, stream=0),
                lambda: rt.shade_tile_list_into(fake_device(torch.zeros(w * h, dtype=torch.int64)), planes(SHADE_IN), tiles, w, h, stream=0),
                lambda: rt.ambient_tile_list_into(region(AMB_OUT), planes(AMB_IN), DIRS, 1.0, tiles, w, h, stream=0),
                lambda: rt.ambient_tile_list_into(planes(AMB_OUT), region(AMB_IN), DIRS, 1.0, tiles, w, h, stream=0),
                lambda: rt.ambient_tile_list_into(dict(planes(AMB_OUT), point=planes(("point",))["point"]), planes(AMB_IN), DIRS, 1.0, tiles, w, h, stream=0)]
    # the list and the bound, as render_tile_list_into checks them
    wide, two, host = fake_device(torch.zeros(5, dtype=torch.int64)), fake_device(torch.zeros(2, dtype=torch.int32)), torch.zeros(5, dtype=torch.int32)
    for bad in (dict(tiles_t=wide), dict(tiles_t=host), dict(bound_t=two), dict(bound_t=wide), dict(bound_t=host)):
        kw = dict(dict(tiles_t=tiles, bound_t=bound, stream=0), **bad)
        refused += [lambda kw=kw: rt.visibility_tile_list_into(planes(VIS), width=w, height=h, **kw),
                    lambda kw=kw: rt.surface_tile_list_into(planes(SURF), width=w, height=h, **kw),
                    lambda kw=kw: rt.shade_tile_list_into(fb, planes(SHADE_IN), width=w, height=h, **kw),
                    lambda kw=kw: rt.ambient_tile_list_into(planes(AMB_OUT), planes(AMB_IN), DIRS, 1.0, width=w, height=h, **kw)]
    assert len(refused) == 6 + 10 + 5 + 3 + 2 + 8 + 5 * 4
    for k, call in enumerate(refused):
        with pytest.raises(AssertionError):
            call()
            print(f"case {k} was not refused")
    # a host array where a device tensor belongs
    with pytest.raises(AssertionError):
        rt.shade_tile_list_into(np.zeros(w * h, np.uint32), planes(SHADE_IN), tiles, w, h, stream=0)


def test_what_the_binding_passes_on(rrt, monkeypatch):
    """The frame size, the list's length as n, the bound's and the list's pointers, the planes' pointers in their structs, the stream; without a bound NULL; an
    absent optional plane NULL."""
    import torch

    from abi_checks import CallRecorder, bare_raytracer, fake_device
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    rt = bare_raytracer(rrt)
    w, h = 203, 117
    tiles, bound, fb = torch.zeros(5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(w * h, dtype=torch.int32)
    ft, fbound, ffb = fake_device(tiles), fake_device(bound), fake_device(fb)
    raw, dev = device_planes(torch, fake_device, w, h, VIS + SURF + AMB_OUT)
    pick = lambda names: {n: dev[n] for n in names}
    rt.visibility_tile_list_into(pick(VIS), ft, w, h, stream=7, bound_t=fbound)
    rt.visibility_tile_list_into(pick(("t",)), ft, w, h, stream=7)
    rt.surface_tile_list_into(pick(VIS + SURF), ft, w, h, stream=7, bound_t=fbound)
    rt.surface_tile_list_into(pick(("lights",)), ft, w, h, stream=7)
    rt.shade_tile_list_into(ffb, pick(SHADE_IN), ft, w, h, stream=7, bound_t=fbound)
    rt.shade_tile_list_into(ffb, pick(SHADE_IN[:4]), ft, w, h, stream=7)
    rt.ambient_tile_list_into(pick(AMB_OUT), pick(AMB_IN), DIRS, 2.5, ft, w, h, stream=7, bound_t=fbound)
    rt.ambient_tile_list_into(pick(("grey",)), pick(AMB_IN), DIRS, 2.5, ft, w, h, stream=7)
    names = [n for n, _ in rec.calls]
    assert names == [s for s in EXPORTS for _ in (0, 1)], names
    fields = lambda ref, want: {n: getattr(ref._obj, n) for n in want}
    ptrs = lambda want, have: {n: (raw[n].data_ptr() if n in have else None) for n in want}
    for k, (_, a) in enumerate(rec.calls):
        assert a[1:4] == (w, h, 5) and a[5].value == tiles.data_ptr(), (k, a)
        assert (a[4].value == bound.data_ptr()) if k % 2 == 0 else (a[4] is None), (k, a)
        assert a[-1].value == 7, (k, a)
    a = [args for _, args in rec.calls]
    assert fields(a[0][6], VIS) == ptrs(VIS, VIS) and fields(a[1][6], VIS) == ptrs(VIS, ("t",))
    assert fields(a[2][6], VIS) == ptrs(VIS, VIS) and fields(a[2][7], SURF) == ptrs(SURF, SURF)
    assert fields(a[3][6], VIS) == ptrs(VIS, ()) and fields(a[3][7], SURF) == ptrs(SURF, ("lights",))
    assert fields(a[4][6], VIS) == ptrs(VIS, ("albedo",)) and fields(a[4][7], SURF) == ptrs(SURF, SURF) and a[4][8].value == fb.data_ptr()
    assert fields(a[5][7], SURF) == ptrs(SURF, SURF[:3]) and a[5][8].value == fb.data_ptr()
    assert fields(a[6][6], SURF) == ptrs(SURF, AMB_IN) and fields(a[6][8], AMB_OUT) == ptrs(AMB_OUT, AMB_OUT)
    assert fields(a[7][8], AMB_OUT) == ptrs(AMB_OUT, ("grey",))
    for args in a[6:]:
        s = args[7]._obj
        assert s.n == 2 and s.max_t == 2.5 and [s.dirs[j] for j in range(6)] == [0.0, 0.0, 1.0, 0.6, 0.0, 0.8]
