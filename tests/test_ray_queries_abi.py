"""The device-resident ray batches and the occlusion query of the C ABI (include/rrt.h: rrt_intersect_rays_device, rrt_get_ray_colours_device,
rrt_occluded_rays, rrt_occluded_rays_device, rrt_tune_rays_device) as far as no GPU is needed: the argument checks made before any HIP call, and
the checks the Python mirror makes before it calls the library."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import NoLibrary, assert_refused


def test_ray_query_calls_refuse_a_null_raytracer(rrt):
    L = rrt.lib()
    rays = (C.c_double * 6)(0, 0, 0, 0, 0, 1)
    out = (C.c_double * 4)()
    variant = C.c_uint32(7)
    p, o = C.addressof(rays), C.addressof(out)
    assert_refused(rrt, L, (("rrt_intersect_rays_device", lambda: L.rrt_intersect_rays_device(None, 1, p, p + 24, None, o, o, o, o, o, None)),
                            ("rrt_get_ray_colours_device", lambda: L.rrt_get_ray_colours_device(None, 1, p, p + 24, o, None)),
                            ("rrt_occluded_rays", lambda: L.rrt_occluded_rays(None, 1, C.cast(p, rrt._dp), C.cast(p + 24, rrt._dp), None, C.cast(o, rrt._u8p))),
                            ("rrt_occluded_rays_device", lambda: L.rrt_occluded_rays_device(None, 1, p, p + 24, None, o, None)),
                            ("rrt_tune_rays_device", lambda: L.rrt_tune_rays_device(None, 1, p, p + 24, None, C.byref(variant)))))
    assert list(out) == [0.0] * 4 and variant.value == 7


def test_the_mirror_has_the_device_forms(rrt):
    for name in ("occluded", "occluded_into", "intersect_rays_into", "get_ray_colours_into", "tune_rays"):
        assert callable(getattr(rrt.RayTracer, name)), name


def test_into_forms_refuse_numpy_arrays_before_any_library_call(rrt, monkeypatch):
    rt = rrt.RayTracer.__new__(rrt.RayTracer)                                # no handle: nothing below may get as far as needing one
    rt._h = None
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    o = np.zeros((4, 3)); d = np.ones((4, 3)); m = np.ones(4)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.occluded_into(o, d, np.zeros(4, np.uint8), m, stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.intersect_rays_into(o, d, {"hit": np.zeros(4, np.uint8)}, stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.get_ray_colours_into(o, d, np.zeros(4, np.uint32), stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.tune_rays(o, d)
