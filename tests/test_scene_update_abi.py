"""Scene updates (include/rrt.h: rrt_raytracer_set_lights / _get_lights / _set_triangles / _set_triangles_device / _release_update_memory) without a GPU:
the five exports reject a NULL handle with a status code before any device is touched, the Python mirror has the five methods, and set_triangles_from
refuses tensors the library must never see a pointer of."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import fake_device


def test_the_five_calls_reject_a_null_handle(rrt):
    L = rrt.lib()
    n = C.c_uint32(7)
    light = (rrt.CLight * 1)(rrt.CLight(0, 0, 0.5, rrt.Vec3(0, 0, 0)))
    tri = np.zeros(9); mat = np.zeros(1, np.uint32)
    d, u = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert L.rrt_raytracer_set_lights(None, light, 1) == rrt.ERR_INVALID_ARG
    assert L.rrt_raytracer_get_lights(None, light, 1, C.byref(n)) == rrt.ERR_INVALID_ARG and n.value == 7
    assert L.rrt_raytracer_set_triangles(None, 1, d(tri), d(tri), d(tri), u(mat), None) == rrt.ERR_INVALID_ARG
    assert L.rrt_raytracer_set_triangles(None, 0, None, None, None, None, None) == rrt.ERR_INVALID_ARG
    assert L.rrt_raytracer_set_triangles_device(None, 1, None, None, None, None, None, None) == rrt.ERR_INVALID_ARG
    assert L.rrt_raytracer_release_update_memory(None) == rrt.ERR_INVALID_ARG
    assert b"null raytracer" in L.rrt_last_error_detail()


def test_python_mirror_has_the_methods(rrt):
    for name in ("set_lights", "lights", "set_triangles", "set_triangles_from", "release_update_memory"):
        assert callable(getattr(rrt.RayTracer, name, None)), name
    for name in ("rrt_raytracer_set_lights", "rrt_raytracer_get_lights", "rrt_raytracer_set_triangles", "rrt_raytracer_set_triangles_device",
                 "rrt_raytracer_release_update_memory"):
        assert name in rrt.SYMBOLS, name


def test_set_triangles_from_rejects_tensors_before_any_call(rrt, monkeypatch):
    """A CPU tensor, a non-contiguous one and a wrong dtype are ValueErrors raised by the mirror: the library is never called (its entry point is replaced
    by one that fails the test)."""
    import torch

    def never(*a):
        raise AssertionError("rrt_raytracer_set_triangles_device was called")
    rt = rrt.RayTracer.__new__(rrt.RayTracer)                 # no handle: nothing below may reach the library
    rt._h, rt.device = None, 0
    monkeypatch.setattr(rrt.lib(), "rrt_raytracer_set_triangles_device", never, raising=False)
    pos = torch.zeros((4, 3, 3), dtype=torch.float64); mat = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="not a device tensor"):
        rt.set_triangles_from(pos, pos, pos, mat)
    with pytest.raises(ValueError):
        rt.set_triangles_from(np.zeros((4, 3, 3)), np.zeros((4, 3, 3)), np.zeros((4, 3, 3)), np.zeros(4, np.uint32))

    FakeDeviceTensor = lambda t: fake_device(t, torch.device("cuda", 0))
    ok = FakeDeviceTensor(pos)
    with pytest.raises(ValueError, match="contiguous"):
        rt.set_triangles_from(FakeDeviceTensor(torch.zeros((4, 3, 6), dtype=torch.float64)[:, :, ::2]), ok, ok, FakeDeviceTensor(mat))
    with pytest.raises(ValueError, match="uv"):
        rt.set_triangles_from(ok, FakeDeviceTensor(pos.float()), ok, FakeDeviceTensor(mat))                       # float32
    with pytest.raises(ValueError, match="float64"):
        rt.set_triangles_from(FakeDeviceTensor(pos.view(torch.int64)), ok, ok, FakeDeviceTensor(mat))             # 8 bytes, not float64
    with pytest.raises(ValueError, match="mat"):
        rt.set_triangles_from(ok, ok, ok, FakeDeviceTensor(mat.long()))                                           # 8-byte indices
    with pytest.raises(ValueError, match="mat"):
        rt.set_triangles_from(ok, ok, ok, FakeDeviceTensor(mat[:3]))                                              # one index short
