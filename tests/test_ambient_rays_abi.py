"""Ambient occlusion for ray records of the C ABI (include/rrt.h: rrt_ray_ambient, rrt_ambient_rays, rrt_ambient_rays_device) as far as no GPU is needed: the
struct layout on both sides, the exported symbols, the argument checks the library makes before any HIP call, the checks the Python mirror makes before it calls
the library, and what it hands to the library."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_layout, fake_device
from ambient_checks import T8, T8_MAX_T
from ambient_rays_checks import INPUTS, OUTPUTS
from ray_surface_checks import NAMES

SIGNATURES = {"rrt_ambient_rays": lambda rrt: [C.c_void_p, C.c_uint32, C.POINTER(rrt.CRaySurface), C.POINTER(C.c_double), C.POINTER(rrt.CAmbientSamples),
                                               C.POINTER(rrt.CRayAmbient)],
              "rrt_ambient_rays_device": lambda rrt: [C.c_void_p, C.c_uint32, C.POINTER(rrt.CRaySurface), C.c_void_p, C.POINTER(rrt.CAmbientSamples),
                                                      C.POINTER(rrt.CRayAmbient), C.c_void_p]}


def test_the_struct_is_16_bytes_on_both_sides(rrt, tmp_path):
    assert C.sizeof(rrt.CRayAmbient) == 16
    assert tuple(n for n, _ in rrt.CRayAmbient._fields_) == rrt.RAY_AMBIENT_OUTPUTS == OUTPUTS
    assert [getattr(rrt.CRayAmbient, n).offset for n in OUTPUTS] == [0, 8]
    assert rrt.STRUCTS["rrt_ray_ambient"] is rrt.CRayAmbient
    assert tuple(rrt.RAY_AMBIENT_INPUTS) == INPUTS and set(INPUTS) < set(NAMES)
    assert compiled_layout(tmp_path, "rrt_ray_ambient", ("occluded", "open")) == (16, [0, 8])


def test_both_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    for name, want in SIGNATURES.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == (C.c_int, want(rrt)), name
        assert getattr(L, name).argtypes == rrt.SYMBOLS[name][1] and getattr(L, name).restype is C.c_int
    assert callable(rrt.RayTracer.ambient_rays) and callable(rrt.RayTracer.ambient_rays_into)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """A NULL raytracer in both forms whatever else is passed, NULL structs and each bad sample table -- also with n == 0 -- through a handle that is not a
    raytracer: a check that came after the handle's first use would crash, not refuse.  The error detail is set and nothing is written."""
    L = rrt.lib()
    vec = (C.c_double * 6)(0, 0, 0, 0, 1, 0)
    word = (C.c_uint32 * 1)(0)
    rot = (C.c_double * 2)(1, 0)
    buf = np.full(2, PATTERN, np.uint32)
    p = C.addressof(vec)
    rec = rrt.CRaySurface(point=p, normal=p + 24, material=C.addressof(word))
    out = rrt.CRayAmbient(occluded=buf.ctypes.data, open=buf.ctypes.data + 4)
    dirs = np.ascontiguousarray(T8)

    def samples(d=dirs, n=8, max_t=T8_MAX_T):
        return rrt.CAmbientSamples(dirs=None if d is None else d.ctypes.data_as(C.POINTER(C.c_double)), n=n, max_t=max_t)

    def bad_dir(value):
        d = dirs.copy()
        d[5, 1] = value
        return d
    nan_dirs, inf_dirs, many = bad_dir(np.nan), bad_dir(-np.inf), np.ascontiguousarray(np.tile(dirs, (5, 1)))   # (kept alive here: the structs only point at them)
    good = samples()
    host = lambda rt, n, r, s, o: L.rrt_ambient_rays(rt, n, r, C.cast(rot, rrt._dp), s, o)
    dev = lambda rt, n, r, s, o: L.rrt_ambient_rays_device(rt, n, r, C.addressof(rot), s, o, None)
    calls = []
    for form, call in (("rrt_ambient_rays", host), ("rrt_ambient_rays_device", dev)):
        calls += [(f"{form}, a NULL raytracer", lambda call=call: call(None, 1, C.byref(rec), C.byref(good), C.byref(out))),
                  (f"{form}, a NULL raytracer, n = 0", lambda call=call: call(None, 0, C.byref(rec), C.byref(good), C.byref(out))),
                  (f"{form}, a NULL raytracer and NULL structs", lambda call=call: call(None, 1, None, None, None))]
    # From here on the handle is the address of 4 KB of zeros: no raytracer.  Every refusal below has to be made before the handle is looked at.
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    tables = [("n == 0", samples(n=0)), ("n == 33", samples(d=many, n=33)), ("NULL dirs", samples(d=None)), ("a NaN direction component", samples(d=nan_dirs)),
              ("an infinite direction component", samples(d=inf_dirs)), ("max_t NaN", samples(max_t=np.nan)), ("max_t 0", samples(max_t=0.0)),
              ("max_t -1", samples(max_t=-1.0)), ("max_t -inf", samples(max_t=-np.inf))]
    for form, call in (("rrt_ambient_rays", host), ("rrt_ambient_rays_device", dev)):
        for n in (1, 0):
            calls += [(f"{form}, n = {n}, a NULL record struct", lambda call=call, n=n: call(fake, n, None, C.byref(good), C.byref(out))),
                      (f"{form}, n = {n}, a NULL samples struct", lambda call=call, n=n: call(fake, n, C.byref(rec), None, C.byref(out))),
                      (f"{form}, n = {n}, a NULL output struct", lambda call=call, n=n: call(fake, n, C.byref(rec), C.byref(good), None))]
            calls += [(f"{form}, n = {n}, {what}", lambda call=call, n=n, s=s: call(fake, n, C.byref(rec), C.byref(s), C.byref(out))) for what, s in tables]
        for name in INPUTS:
            less = rrt.CRaySurface(**{k: getattr(rec, k) for k in INPUTS if k != name})
            calls.append((f"{form}, NULL {name}", lambda call=call, less=less: call(fake, 1, C.byref(less), C.byref(good), C.byref(out))))
        calls.append((f"{form}, both outputs NULL", lambda call=call: call(fake, 1, C.byref(rec), C.byref(good), C.byref(rrt.CRayAmbient()))))
    assert len(calls) == 2 * (3 + 2 * 12 + 3 + 1)
    assert_refused(rrt, L, calls, dict(buf=buf))
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def test_the_binding_refuses_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    f4 = lambda n: fake_device(torch.zeros(n, dtype=torch.float32))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    rec = dict(point=f8(12), normal=f8(12), material=i4(4))
    into = lambda out, planes=rec, rot_t=None: rt.ambient_rays_into(out, planes, T8, T8_MAX_T, rot_t=rot_t, stream=0)
    # not a device tensor
    with pytest.raises(AssertionError, match="not a device tensor"):
        into({"occluded": np.zeros(4, np.uint32)})
    with pytest.raises(AssertionError, match="not a device tensor"):
        into({"open": np.zeros(4, np.uint32)})
    for name in INPUTS:
        with pytest.raises(AssertionError, match="not a device tensor"):
            into({"occluded": i4(4)}, dict(rec, **{name: np.zeros((4, 3)) if name != "material" else np.zeros(4, np.uint32)}))
    with pytest.raises(AssertionError, match="not a device tensor"):
        into({"occluded": i4(4)}, rot_t=np.zeros((4, 2)))
    # a wrong dtype and a wrong length, for each of point / normal / material / rot / occluded / open
    with pytest.raises(AssertionError, match="point: want 12 contiguous elements of 8 bytes"):
        into({"open": i4(4)}, dict(rec, point=f4(12)))
    with pytest.raises(AssertionError, match="point: want 12 contiguous elements of 8 bytes"):
        into({"open": i4(4)}, dict(rec, point=f8(4)))
    with pytest.raises(AssertionError, match="normal: want 12 contiguous elements of 8 bytes"):
        into({"open": i4(4)}, dict(rec, normal=i4(12)))
    with pytest.raises(AssertionError, match="normal: want 12 contiguous elements of 8 bytes"):
        into({"open": i4(4)}, dict(rec, normal=f8(15)))
    with pytest.raises(AssertionError, match="material: want 4 contiguous elements of 4 bytes"):
        into({"open": i4(4)}, dict(rec, material=f8(4)))
    with pytest.raises(AssertionError, match="point: want 15 contiguous elements of 8 bytes"):             # (the batch is as long as its material array)
        into({"open": i4(5)}, dict(rec, material=i4(5)))
    with pytest.raises(AssertionError, match="rot: want 8 contiguous elements of 8 bytes"):
        into({"open": i4(4)}, rot_t=f4(8))
    with pytest.raises(AssertionError, match="rot: want 8 contiguous elements of 8 bytes"):
        into({"open": i4(4)}, rot_t=f8(4))
    with pytest.raises(AssertionError, match="occluded: want 4 contiguous elements of 4 bytes"):
        into({"occluded": f8(4)})
    with pytest.raises(AssertionError, match="occluded: want 4 contiguous elements of 4 bytes"):
        into({"occluded": i4(5)})
    with pytest.raises(AssertionError, match="open: want 4 contiguous elements of 4 bytes"):
        into({"open": f8(4)})
    with pytest.raises(AssertionError, match="open: want 4 contiguous elements of 4 bytes"):
        into({"open": i4(3)})
    with pytest.raises(AssertionError, match="no material array"):
        into({"open": i4(4)}, {n: rec[n] for n in ("point", "normal")})
    # unknown names
    with pytest.raises(ValueError, match="unknown output 'grey'"):
        into({"grey": i4(4)})
    with pytest.raises(ValueError, match="unknown plane 'occluded'"):                                     # an output is not a record
        into({"open": i4(4)}, dict(rec, occluded=i4(4)))
    host = dict(point=np.zeros((4, 3)), normal=np.ones((4, 3)), material=np.zeros(4, np.uint32))
    with pytest.raises(ValueError, match="unknown output 'grey'"):
        rt.ambient_rays(host, T8, T8_MAX_T, outputs=("occluded", "grey"))
    with pytest.raises(ValueError, match="unknown plane 'open'"):
        rt.ambient_rays(dict(host, open=np.zeros(4, np.uint32)), T8, T8_MAX_T)
    with pytest.raises(AssertionError, match="array normal has 15 elements for 4 rays"):
        rt.ambient_rays(dict(host, normal=np.zeros((5, 3))), T8, T8_MAX_T)
    with pytest.raises(AssertionError, match="array point has 9 elements for 4 rays"):
        rt.ambient_rays(dict(host, point=np.zeros((3, 3))), T8, T8_MAX_T)
    with pytest.raises(AssertionError, match="rot has 6 elements for 4 rays"):
        rt.ambient_rays(host, T8, T8_MAX_T, rot=np.zeros((3, 2)))
    with pytest.raises(AssertionError, match="no material array"):
        rt.ambient_rays({n: host[n] for n in ("point", "normal")}, T8, T8_MAX_T)


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))

    def table_of(s):
        return s.n, s.max_t, [s.dirs[i] for i in range(3 * s.n)]
    # the device form: all twelve arrays of a surface_rays_into call are passed, the three that are read arrive, the nine others are NULL
    twelve = {n: (f8(12) if n in ("point", "normal", "next_origin", "next_dir") else f8(4) if n in ("t", "u", "v") else
                  fake_device(torch.zeros(4, dtype=torch.uint8)) if n == "hit" else i4(4)) for n in NAMES}
    out = dict(occluded=i4(4), open=i4(4))
    rot = f8(8)
    rt.ambient_rays_into(out, twelve, T8, T8_MAX_T, rot_t=rot, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_ambient_rays_device" and len(args) == 7 and args[0] is None and args[1] == 4 and args[3].value == rot.data_ptr() and args[6].value == 0x51
    s, t, o = args[2]._obj, args[4]._obj, args[5]._obj
    assert isinstance(s, rrt.CRaySurface) and isinstance(t, rrt.CAmbientSamples) and isinstance(o, rrt.CRayAmbient)
    assert {n: getattr(s, n) for n in NAMES} == {n: (twelve[n].data_ptr() if n in INPUTS else None) for n in NAMES}
    assert {n: getattr(o, n) for n in OUTPUTS} == {n: out[n].data_ptr() for n in OUTPUTS}
    assert table_of(t) == (8, T8_MAX_T, T8.reshape(-1).tolist())
    # ... without a rotation (absent, or None): NULL; one output only: the other is NULL
    for kw in ({}, dict(rot_t=None)):
        rec.calls.clear()
        only = i4(4)
        rt.ambient_rays_into({"open": only}, {n: twelve[n] for n in INPUTS}, T8[:3], float("inf"), stream=7, **kw)
        (name, args), = rec.calls
        assert name == "rrt_ambient_rays_device" and args[3] is None and args[6].value == 7
        assert {n: getattr(args[5]._obj, n) for n in OUTPUTS} == dict(occluded=None, open=only.data_ptr())
        assert table_of(args[4]._obj) == (3, float("inf"), T8[:3].reshape(-1).tolist())
    # the host form
    rec.calls.clear()
    host = dict(point=np.zeros((4, 3)), normal=np.ones((4, 3)), material=np.zeros(4, np.uint32), albedo=np.zeros(4, np.uint32), lights=np.zeros(4, np.uint32),
                hit=np.zeros(4, np.uint8), next_dir=np.zeros((4, 3)))
    got = rt.ambient_rays(host, T8)
    (name, args), = rec.calls
    assert name == "rrt_ambient_rays" and len(args) == 6 and args[1] == 4 and not args[3], "rot absent: NULL"
    assert set(got) == set(OUTPUTS) and all(a.shape == (4,) and a.dtype == np.uint32 for a in got.values())
    s, t, o = args[2]._obj, args[4]._obj, args[5]._obj
    assert {n: getattr(s, n) for n in NAMES} == {n: (host[n].ctypes.data if n in INPUTS else None) for n in NAMES}
    assert {n: getattr(o, n) for n in OUTPUTS} == {n: got[n].ctypes.data for n in OUTPUTS}
    assert table_of(t) == (8, float("inf"), T8.reshape(-1).tolist()), "max_t is +inf by default"
    rec.calls.clear()
    r = np.arange(8, dtype=np.float64).reshape(4, 2)
    got = rt.ambient_rays({n: host[n] for n in INPUTS}, T8, T8_MAX_T, rot=r, outputs=("occluded",))
    (name, args), = rec.calls
    assert [args[3][i] for i in range(8)] == list(range(8)) and args[4]._obj.max_t == T8_MAX_T
    assert set(got) == {"occluded"} and {n: getattr(args[5]._obj, n) for n in OUTPUTS} == dict(occluded=got["occluded"].ctypes.data, open=None)
