"""The part of ambient occlusion from kept buffers that needs no GPU (include/rrt.h: rrt_ambient_samples, rrt_ambient, rrt_ambient_surface,
rrt_ambient_surface_device): the struct layouts, the exports, and the argument checks that are made before any HIP call."""
import ctypes as C

from abi_checks import assert_refused

EXPORTS = ("rrt_ambient_surface_device", "rrt_ambient_surface")


def test_ambient_structs_have_the_header_layout(rrt):
    assert C.sizeof(rrt.CAmbientSamples) == 24 and C.sizeof(rrt.CAmbient) == 16
    assert [(n, getattr(rrt.CAmbientSamples, n).offset) for n, _ in rrt.CAmbientSamples._fields_] == [("dirs", 0), ("n", 8), ("_pad", 12), ("max_t", 16)]
    assert tuple(n for n, _ in rrt.CAmbient._fields_) == rrt.AMBIENT_OUTPUTS == ("occluded", "grey")
    assert [getattr(rrt.CAmbient, n).offset for n in rrt.AMBIENT_OUTPUTS] == [0, 8]
    assert rrt.MAX_AMBIENT_SAMPLES == 32


def test_the_two_exports_exist_and_are_bound(rrt):
    L = rrt.lib()
    for name in EXPORTS:
        assert name in rrt.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rrt.SYMBOLS[name][1], name
    assert len(rrt.SYMBOLS["rrt_ambient_surface_device"][1]) == 8 and len(rrt.SYMBOLS["rrt_ambient_surface"][1]) == 7
    for method in ("ambient", "ambient_into"):
        assert callable(getattr(rrt.RayTracer, method)), method


def test_ambient_calls_refuse_a_null_raytracer(rrt):
    L = rrt.lib()
    point, normal, material = (C.c_double * 12)(), (C.c_double * 12)(), (C.c_uint32 * 4)()
    occluded, grey = (C.c_uint32 * 4)(*([0xA5A5A5A5] * 4)), (C.c_uint32 * 1)(0xA5A5A5A5)
    dirs = (C.c_double * 3)(0.0, 0.0, 1.0)
    planes = rrt.CSurface(point=C.addressof(point), normal=C.addressof(normal), material=C.addressof(material))
    samples = rrt.CAmbientSamples(dirs=dirs, n=1, max_t=2.0)
    out = rrt.CAmbient(occluded=C.addressof(occluded), grey=C.addressof(grey))
    region = rrt.CRegion(0, 0, 1, 1)
    assert_refused(rrt, L, (("rrt_ambient_surface", lambda: L.rrt_ambient_surface(None, 64, 48, C.byref(region), C.byref(planes), C.byref(samples), C.byref(out))),
                            ("rrt_ambient_surface, whole frame", lambda: L.rrt_ambient_surface(None, 64, 48, None, C.byref(planes), C.byref(samples), C.byref(out))),
                            ("rrt_ambient_surface_device", lambda: L.rrt_ambient_surface_device(None, 64, 48, C.byref(region), C.byref(planes), C.byref(samples), C.byref(out), None))))
    assert list(occluded) == [0xA5A5A5A5] * 4 and grey[0] == 0xA5A5A5A5, "an output of a refused ambient call was written"
