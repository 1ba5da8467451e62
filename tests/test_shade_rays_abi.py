"""Shading of arbitrary rays from kept records of the C ABI (include/rrt.h: rrt_ray_shade, rrt_shade_rays, rrt_shade_rays_device) as far as no GPU is needed: the
struct layout on both sides, the exported symbols, the argument checks the library makes before any HIP call, the checks the Python mirror makes before it calls
the library, and what it hands to the library."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_layout, fake_device
from ray_surface_checks import NAMES
from shade_rays_checks import INPUTS, OUTPUTS, OUT_DTYPES

SIGNATURES = {"rrt_shade_rays": lambda rrt: [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(rrt.CRaySurface), C.c_uint32, C.POINTER(rrt.CRayShade)],
              "rrt_shade_rays_device": lambda rrt: [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(rrt.CRaySurface), C.c_uint32, C.POINTER(rrt.CRayShade), C.c_void_p]}


def test_the_struct_is_24_bytes_on_both_sides(rrt, tmp_path):
    assert C.sizeof(rrt.CRayShade) == 24
    assert tuple(n for n, _ in rrt.CRayShade._fields_) == rrt.RAY_SHADE_OUTPUTS == OUTPUTS
    assert [getattr(rrt.CRayShade, n).offset for n in OUTPUTS] == [0, 8, 16]
    assert rrt.STRUCTS["rrt_ray_shade"] is rrt.CRayShade
    assert set(rrt.RAY_SHADE_INPUTS) == set(INPUTS) and set(INPUTS) < set(NAMES)
    assert compiled_layout(tmp_path, "rrt_ray_shade", ("colour", "local", "kr")) == (24, [0, 8, 16])


def test_both_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    for name, want in SIGNATURES.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == (C.c_int, want(rrt)), name
        assert getattr(L, name).argtypes == rrt.SYMBOLS[name][1] and getattr(L, name).restype is C.c_int
    assert callable(rrt.RayTracer.shade_rays) and callable(rrt.RayTracer.shade_rays_into)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """A NULL raytracer in both forms, whatever else is passed; nothing is written."""
    L = rrt.lib()
    rays = (C.c_double * 6)(0, 0, 1, 0, 0, 0)
    words = (C.c_uint32 * 2)(0, 0x808080)
    buf = (C.c_double * 4)()
    p = C.addressof(rays)
    rec = rrt.CRaySurface(point=p + 24, normal=p, material=C.addressof(words), albedo=C.addressof(words) + 4)
    out = rrt.CRayShade(kr=C.addressof(buf), local=C.addressof(buf) + 8)
    host = lambda r, o: L.rrt_shade_rays(None, 1, C.cast(p, rrt._dp), r, 0, o)
    assert_refused(rrt, L, (("rrt_shade_rays", lambda: host(C.byref(rec), C.byref(out))),
                            ("rrt_shade_rays, NULL structs", lambda: host(None, None)),
                            ("rrt_shade_rays_device", lambda: L.rrt_shade_rays_device(None, 1, p, C.byref(rec), 0, C.byref(out), None)),
                            ("rrt_shade_rays_device, n = 0", lambda: L.rrt_shade_rays_device(None, 0, None, C.byref(rec), 7, C.byref(out), None))))
    assert list(buf) == [0.0] * 4


def _records(torch, n):
    f8 = lambda k: fake_device(torch.zeros(k, dtype=torch.float64))
    i4 = lambda k: fake_device(torch.zeros(k, dtype=torch.int32))
    return dict(point=f8(3 * n), normal=f8(3 * n), material=i4(n), albedo=i4(n), lights=i4(n))


def test_the_binding_refuses_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    d, rec = f8(12), _records(torch, 4)
    with pytest.raises(AssertionError, match="dirs: not a device tensor"):
        rt.shade_rays_into({"colour": i4(4)}, np.ones((4, 3)), rec, stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.shade_rays_into({"colour": np.zeros(4, np.uint32)}, d, rec, stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.shade_rays_into({"colour": i4(4)}, d, dict(rec, normal=np.zeros((4, 3))), stream=0)
    with pytest.raises(AssertionError, match="not a multiple of 3"):
        rt.shade_rays_into({"colour": i4(4)}, f8(11), rec, stream=0)
    with pytest.raises(AssertionError, match="dirs: want 12 contiguous elements of 8 bytes"):              # a wrong dtype
        rt.shade_rays_into({"colour": i4(4)}, fake_device(torch.zeros(12, dtype=torch.float32)), rec, stream=0)
    with pytest.raises(AssertionError, match="colour: want 4 contiguous elements of 4 bytes"):
        rt.shade_rays_into({"colour": f8(4)}, d, rec, stream=0)
    with pytest.raises(AssertionError, match="local: want 12 contiguous elements of 8 bytes"):             # a wrong length: n where 3 n are wanted
        rt.shade_rays_into({"local": f8(4)}, d, rec, stream=0)
    with pytest.raises(AssertionError, match="kr: want 4 contiguous elements of 8 bytes"):
        rt.shade_rays_into({"kr": f8(5)}, d, rec, stream=0)
    with pytest.raises(AssertionError, match="point: want 12 contiguous elements of 8 bytes"):
        rt.shade_rays_into({"kr": f8(4)}, d, dict(rec, point=f8(4)), stream=0)
    with pytest.raises(AssertionError, match="material: want 4 contiguous elements of 4 bytes"):
        rt.shade_rays_into({"kr": f8(4)}, d, dict(rec, material=f8(4)), stream=0)
    with pytest.raises(AssertionError, match="lights: want 4 contiguous elements of 4 bytes"):
        rt.shade_rays_into({"kr": f8(4)}, d, dict(rec, lights=i4(3)), stream=0)
    with pytest.raises(ValueError, match="unknown output 'grey'"):
        rt.shade_rays_into({"grey": i4(4)}, d, rec, stream=0)
    with pytest.raises(ValueError, match="unknown plane 'colour'"):                                       # an output is not a record
        rt.shade_rays_into({"kr": f8(4)}, d, dict(rec, colour=i4(4)), stream=0)
    host = {n: np.zeros((4, 3)) if n in ("point", "normal") else np.zeros(4, np.uint32) for n in INPUTS}
    with pytest.raises(ValueError, match="unknown output 'hit'"):
        rt.shade_rays(np.ones((4, 3)), host, outputs=("colour", "hit"))
    with pytest.raises(ValueError, match="unknown plane 'occluded'"):
        rt.shade_rays(np.ones((4, 3)), dict(host, occluded=np.zeros(4, np.uint32)))
    with pytest.raises(AssertionError, match="array normal has 15 elements for 4 rays"):
        rt.shade_rays(np.ones((4, 3)), dict(host, normal=np.zeros((5, 3))))
    with pytest.raises(AssertionError, match="array albedo has 3 elements for 4 rays"):
        rt.shade_rays(np.ones((4, 3)), dict(host, albedo=np.zeros(3, np.uint32)))


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    # the device form: all twelve arrays of a surface_rays_into call are passed, the five that are read arrive, the seven others are NULL
    d = f8(12)
    twelve = {n: (f8(12) if n in ("point", "normal", "next_origin", "next_dir") else f8(4) if n in ("t", "u", "v") else
                  fake_device(torch.zeros(4, dtype=torch.uint8)) if n == "hit" else i4(4)) for n in NAMES}
    out = dict(local=f8(12), kr=f8(4))
    rt.shade_rays_into(out, d, twelve, depth=3, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_shade_rays_device" and args[1] == 4 and args[2].value == d.data_ptr() and args[4] == 3 and args[6].value == 0x51
    s, o = args[3]._obj, args[5]._obj
    assert isinstance(s, rrt.CRaySurface) and isinstance(o, rrt.CRayShade)
    assert {n: getattr(s, n) for n in NAMES} == {n: (twelve[n].data_ptr() if n in INPUTS else None) for n in NAMES}
    assert {n: getattr(o, n) for n in OUTPUTS} == dict(colour=None, local=out["local"].data_ptr(), kr=out["kr"].data_ptr())
    # ... without a mask (absent, or None), depth 0 by default
    for planes in ({n: twelve[n] for n in INPUTS if n != "lights"}, dict(twelve, lights=None)):
        rec.calls.clear()
        colour = i4(4)
        rt.shade_rays_into({"colour": colour}, d, planes, stream=7)
        (name, args), = rec.calls
        assert args[3]._obj.lights is None and args[3]._obj.albedo == twelve["albedo"].data_ptr() and args[4] == 0
        assert {n: getattr(args[5]._obj, n) for n in OUTPUTS} == dict(colour=colour.data_ptr(), local=None, kr=None)
    # the host form
    rec.calls.clear()
    dirs = np.arange(12, dtype=np.float64).reshape(4, 3)
    host = dict(point=np.zeros((4, 3)), normal=np.ones((4, 3)), material=np.zeros(4, np.uint32), albedo=np.zeros(4, np.uint32), lights=np.zeros(4, np.uint32),
                hit=np.zeros(4, np.uint8), next_dir=np.zeros((4, 3)))
    got = rt.shade_rays(dirs, host)
    (name, args), = rec.calls
    assert name == "rrt_shade_rays" and args[1] == 4 and args[4] == 0 and [args[2][i] for i in range(12)] == list(range(12))
    assert set(got) == {"colour"} and got["colour"].shape == (4,) and got["colour"].dtype == np.uint32
    s, o = args[3]._obj, args[5]._obj
    assert {n: getattr(s, n) for n in NAMES} == {n: (host[n].ctypes.data if n in INPUTS else None) for n in NAMES}
    assert {n: getattr(o, n) for n in OUTPUTS} == dict(colour=got["colour"].ctypes.data, local=None, kr=None)
    rec.calls.clear()
    got = rt.shade_rays(dirs, {n: host[n] for n in INPUTS if n != "lights"}, depth=2, outputs=OUTPUTS)
    (name, args), = rec.calls
    assert args[4] == 2 and args[3]._obj.lights is None
    assert {n: (a.shape, a.dtype) for n, a in got.items()} == {n: ((4, 3) if n == "local" else (4,), np.dtype(OUT_DTYPES[n])) for n in OUTPUTS}
    assert {n: getattr(args[5]._obj, n) for n in OUTPUTS} == {n: got[n].ctypes.data for n in OUTPUTS}
