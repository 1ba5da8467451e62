"""The surface part of the C ABI that needs no GPU (include/rrt.h: rrt_surface, rrt_render_surface, rrt_render_surface_device): the struct layout, and the
argument checks that are made before any HIP call."""
import ctypes as C

from abi_checks import assert_refused


def test_surface_struct_has_the_header_size(rrt):
    assert C.sizeof(rrt.CSurface) == 32
    assert tuple(n for n, _ in rrt.CSurface._fields_) == rrt.SURFACE_PLANES == ("point", "normal", "material", "lights")
    assert [getattr(rrt.CSurface, n).offset for n in rrt.SURFACE_PLANES] == [0, 8, 16, 24]


def test_surface_calls_refuse_a_null_raytracer(rrt):
    L = rrt.lib()
    buf = (C.c_double * 12)()
    tbuf = (C.c_double * 4)()
    planes = rrt.CSurface(point=C.addressof(buf))
    vis = rrt.CVisibility(t=C.addressof(tbuf))
    region = rrt.CRegion(0, 0, 1, 1)
    assert_refused(rrt, L, (("rrt_render_surface", lambda: L.rrt_render_surface(None, 64, 48, C.byref(region), None, C.byref(planes))),
                            ("rrt_render_surface, whole frame, with visibility planes", lambda: L.rrt_render_surface(None, 64, 48, None, C.byref(vis), C.byref(planes))),
                            ("rrt_render_surface_device", lambda: L.rrt_render_surface_device(None, 64, 48, C.byref(region), None, C.byref(planes), None)),
                            ("rrt_render_surface_device, with visibility planes", lambda: L.rrt_render_surface_device(None, 64, 48, C.byref(region), C.byref(vis), C.byref(planes), None))))
    assert list(buf) == [0.0] * 12 and list(tbuf) == [0.0] * 4
