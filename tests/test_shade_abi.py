"""The part of shading from kept buffers and of the material update that needs no GPU (include/rrt.h: rrt_shade_surface, rrt_shade_surface_device,
rrt_raytracer_set_materials, rrt_raytracer_get_materials): the exports, and the argument checks that are made before any HIP call."""
import ctypes as C

from abi_checks import assert_refused

EXPORTS = ("rrt_shade_surface_device", "rrt_shade_surface", "rrt_raytracer_set_materials", "rrt_raytracer_get_materials")


def test_the_four_exports_exist_and_are_bound(rrt):
    L = rrt.lib()
    for name in EXPORTS:
        assert name in rrt.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rrt.SYMBOLS[name][1], name
    assert len(rrt.SYMBOLS["rrt_shade_surface_device"][1]) == 8 and len(rrt.SYMBOLS["rrt_shade_surface"][1]) == 7
    for method in ("shade", "shade_into", "set_materials", "materials"):
        assert callable(getattr(rrt.RayTracer, method)), method


def test_a_null_raytracer_is_refused(rrt):
    L = rrt.lib()
    point, normal = (C.c_double * 12)(), (C.c_double * 12)()
    material, albedo, lights = (C.c_uint32 * 4)(), (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    fb = (C.c_uint32 * 1)(0xA5A5A5A5)
    planes = rrt.CSurface(point=C.addressof(point), normal=C.addressof(normal), material=C.addressof(material), lights=C.addressof(lights))
    vis = rrt.CVisibility(albedo=C.addressof(albedo))
    region = rrt.CRegion(0, 0, 1, 1)
    mats = (rrt.CMaterial * 1)()
    mats[0].ns, mats[0].bump = 7.5, -1
    count = C.c_uint32(12345)
    assert_refused(rrt, L, (("rrt_shade_surface", lambda: L.rrt_shade_surface(None, 64, 48, C.byref(region), C.byref(vis), C.byref(planes), fb)),
                            ("rrt_shade_surface_device", lambda: L.rrt_shade_surface_device(None, 64, 48, C.byref(region), C.byref(vis), C.byref(planes), C.addressof(fb), None)),
                            ("rrt_raytracer_set_materials", lambda: L.rrt_raytracer_set_materials(None, mats, 1)),
                            ("rrt_raytracer_get_materials", lambda: L.rrt_raytracer_get_materials(None, mats, 1, C.byref(count)))))
    assert fb[0] == 0xA5A5A5A5, "the output of a refused shade call was written"
    assert (mats[0].ns, mats[0].bump, count.value) == (7.5, -1, 12345), "the outputs of a refused rrt_raytracer_get_materials were written"
