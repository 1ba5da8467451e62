"""The visibility part of the C ABI that needs no GPU (include/rrt.h: rrt_region, rrt_visibility, rrt_pick_result): struct layouts, and the argument checks
that are made before any HIP call."""
import ctypes as C

from abi_checks import assert_refused


def test_visibility_structs_have_the_header_sizes(rrt):
    assert C.sizeof(rrt.CRegion) == 16 and C.sizeof(rrt.CVisibility) == 48 and C.sizeof(rrt.CPickResult) == 40
    assert [n for n, _ in rrt.CRegion._fields_] == ["x0", "y0", "w", "h"]
    assert tuple(n for n, _ in rrt.CVisibility._fields_) == rrt.PLANES == ("hit", "t", "u", "v", "tri", "albedo")
    assert [n for n, _ in rrt.CPickResult._fields_] == ["hit", "tri", "t", "u", "v", "albedo", "_pad"]
    assert (rrt.CPickResult.t.offset, rrt.CPickResult.albedo.offset) == (8, 32)


def test_visibility_calls_refuse_a_null_raytracer(rrt):
    L = rrt.lib()
    buf = (C.c_double * 4)()
    planes = rrt.CVisibility(t=C.addressof(buf))
    region = rrt.CRegion(0, 0, 1, 1)
    out = rrt.CPickResult()
    assert_refused(rrt, L, (("rrt_render_visibility", lambda: L.rrt_render_visibility(None, 64, 48, C.byref(region), C.byref(planes))),
                            ("rrt_render_visibility, whole frame", lambda: L.rrt_render_visibility(None, 64, 48, None, C.byref(planes))),
                            ("rrt_render_visibility_device", lambda: L.rrt_render_visibility_device(None, 64, 48, C.byref(region), C.byref(planes), None)),
                            ("rrt_pick", lambda: L.rrt_pick(None, 64, 48, 0, 0, C.byref(out)))))
    assert list(buf) == [0.0] * 4
