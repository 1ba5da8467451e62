"""Surface records from kept hits of the C ABI (include/rrt.h: rrt_resolve_hits, rrt_resolve_hits_device, rrt_resolve_hits_counted_device) as far as no GPU is
needed: the exported symbols, the buffer id of the triangle -> slot table, the argument checks the library makes before any HIP call and before it looks at the
handle, the checks the Python mirror makes before it calls the library, and what it hands to the library."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, fake_device

OUTPUTS = ("albedo", "point", "normal", "material", "lights", "next_origin", "next_dir")
READS_UV = ("albedo", "normal", "lights", "next_origin", "next_dir")


def test_the_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    P, S, D = C.c_void_p, C.POINTER(rrt.CRaySurface), C.POINTER(C.c_double)
    want = {"rrt_resolve_hits": (C.c_int, [P, C.c_uint32, D, D, S]),
            "rrt_resolve_hits_device": (C.c_int, [P, C.c_uint32, P, P, S, P]),
            "rrt_resolve_hits_counted_device": (C.c_int, [P, C.c_uint32, P, P, P, S, P])}
    for name, sig in want.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == sig, name
        assert getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0]
    for method in ("resolve_hits", "resolve_hits_into"):
        assert callable(getattr(rrt.RayTracer, method)), method
    assert rrt.RESOLVE_INPUTS == ("t", "u", "v", "tri") and rrt.RESOLVE_OUTPUTS == OUTPUTS
    assert rrt.BUFFERS[-1] == "tri_slot" and rrt.BUFFERS.index("tri_slot") == 16, "RRT_BUF_TRI_SLOT is appended at the end of the enum"


def test_the_library_refuses_before_any_gpu_work(rrt):
    """Every refusal of rrt.h in all three forms, through a handle that is the address of 4 KB of zeros: a check that came after the handle's first use would
    crash, not refuse.  (The device forms' pointers are host addresses here: a call that got as far as a launch would fail in another way.)  The error detail is
    set and the outputs keep their pattern."""
    L = rrt.lib()
    n = 4
    vec = np.zeros((n, 3))
    f8 = np.zeros(n)
    tri = np.zeros(n, np.uint32)
    outs = {name: np.full(8 * n, PATTERN, np.uint32) for name in OUTPUTS}
    at = lambda a: a.ctypes.data
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ptr = lambda a: None if a is None else at(a)
    ref = lambda s: None if s is None else C.byref(s)

    def rec(wanted=OUTPUTS, **reads):
        r = dict(t=at(f8), u=at(f8), v=at(f8), tri=at(tri))
        r.update(reads)
        return rrt.CRaySurface(**{k: p for k, p in r.items() if p is not None}, **{name: at(outs[name]) for name in wanted})

    def host(rt, n, o, d, s):
        return L.rrt_resolve_hits(rt, n, dp(o), dp(d), ref(s))

    def dev(rt, n, o, d, s):
        return L.rrt_resolve_hits_device(rt, n, ptr(o), ptr(d), ref(s), None)

    def counted(rt, n, o, d, s):
        return L.rrt_resolve_hits_counted_device(rt, n, at(tri), ptr(o), ptr(d), ref(s), None)
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    calls = []
    for form, call in (("rrt_resolve_hits", host), ("rrt_resolve_hits_device", dev), ("rrt_resolve_hits_counted_device", counted)):
        calls += [(f"{form}, a NULL raytracer", lambda call=call: call(None, n, vec, vec, rec())),
                  (f"{form}, a NULL raytracer, n = 0", lambda call=call: call(None, 0, vec, vec, rec())),
                  (f"{form}, a NULL struct", lambda call=call: call(fake, n, vec, vec, None)),
                  (f"{form}, a NULL struct, n = 0", lambda call=call: call(fake, 0, vec, vec, None)),
                  (f"{form}, NULL origins", lambda call=call: call(fake, n, None, vec, rec())),
                  (f"{form}, NULL dirs", lambda call=call: call(fake, n, vec, None, rec())),
                  (f"{form}, NULL t", lambda call=call: call(fake, n, vec, vec, rec(t=None))),
                  (f"{form}, NULL tri", lambda call=call: call(fake, n, vec, vec, rec(tri=None))),
                  (f"{form}, NULL t, point alone", lambda call=call: call(fake, n, vec, vec, rec(("point",), t=None))),
                  (f"{form}, all seven outputs NULL", lambda call=call: call(fake, n, vec, vec, rec(()))),
                  (f"{form}, only the five arrays that are read or ignored", lambda call=call: call(fake, n, vec, vec, rrt.CRaySurface(hit=at(tri), t=at(f8), u=at(f8), v=at(f8), tri=at(tri))))]
        for name in READS_UV:
            calls += [(f"{form}, {name} without u", lambda call=call, name=name: call(fake, n, vec, vec, rec((name,), u=None))),
                      (f"{form}, {name} and point without v", lambda call=call, name=name: call(fake, n, vec, vec, rec((name, "point"), v=None)))]
    assert len(calls) == 3 * (11 + 2 * 5)
    assert_refused(rrt, L, calls, outs)
    # n == 0 with a valid struct: RRT_OK, nothing enqueued (the handle is not a raytracer), also without rays and without the arrays a longer batch would need
    for call in (host, dev, counted):
        assert call(fake, 0, vec, vec, rec()) == rrt.OK
        assert call(fake, 0, None, None, rrt.CRaySurface()) == rrt.OK
    for name, a in outs.items():
        assert (a == PATTERN).all(), f"n == 0: {name} was written"
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def test_the_binding_refuses_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    f4 = lambda n: fake_device(torch.zeros(n, dtype=torch.float32))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    planes = dict(t=f8(4), u=f8(4), v=f8(4), tri=i4(4))

    def into(out, o=None, d=None, planes=planes, bound_t=None):
        rt.resolve_hits_into(out, f8(12) if o is None else o, f8(12) if d is None else d, planes, stream=0, bound_t=bound_t)
    with pytest.raises(ValueError, match="unknown output 'hit'"):
        into({"hit": i4(4)})
    with pytest.raises(ValueError, match="unknown output 'tri'"):
        rt.resolve_hits(np.zeros((4, 3)), np.zeros((4, 3)), dict(t=np.zeros(4), tri=np.zeros(4, np.uint32)), outputs=("tri",))
    with pytest.raises(ValueError, match="unknown plane 'colour'"):
        into({"point": f8(12)}, planes=dict(planes, colour=i4(4)))
    for kw in (dict(out={"point": np.zeros(12)}), dict(out={"point": f8(12)}, o=np.zeros(12)), dict(out={"point": f8(12)}, planes=dict(planes, tri=np.zeros(4, np.uint32))),
               dict(out={"point": f8(12)}, bound_t=np.zeros(1, np.uint32))):
        with pytest.raises(AssertionError, match="not a device tensor"):
            into(**kw)
    with pytest.raises(AssertionError, match="dirs: want 12 contiguous elements of 8 bytes"):
        into({"point": f8(12)}, d=f4(12))
    with pytest.raises(AssertionError, match="t: want 4 contiguous elements of 8 bytes"):
        into({"point": f8(12)}, planes=dict(planes, t=f8(5)))
    with pytest.raises(AssertionError, match="tri: want 4 contiguous elements of 4 bytes"):
        into({"point": f8(12)}, planes=dict(planes, tri=f8(4)))
    with pytest.raises(AssertionError, match="normal: want 12 contiguous elements of 8 bytes"):
        into({"normal": f8(4)})
    with pytest.raises(AssertionError, match="lights: want 4 contiguous elements of 4 bytes"):
        into({"lights": f8(4)})
    with pytest.raises(AssertionError, match="bound: want 1 contiguous elements of 4 bytes"):
        into({"point": f8(12)}, bound_t=i4(2))
    # the host form
    with pytest.raises(AssertionError, match="array u has 5 elements for 4 rays"):
        rt.resolve_hits(np.zeros((4, 3)), np.zeros((4, 3)), dict(t=np.zeros(4), u=np.zeros(5), v=np.zeros(4), tri=np.zeros(4, np.uint32)))


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))
    names = tuple(n for n, _ in rrt.CRaySurface._fields_)
    pointers = lambda s: {n: getattr(s, n) for n in names}
    o, d = f8(15), f8(15)
    # the device form: the arrays it reads and the outputs in ONE struct; hit, and an output among the planes, are not handed on
    planes = dict(hit=u1(5), t=f8(5), u=f8(5), v=f8(5), tri=i4(5), albedo=i4(5))
    out = dict(normal=f8(15), lights=i4(5))
    rt.resolve_hits_into(out, o, d, planes, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_resolve_hits_device" and len(args) == 6 and args[0] is None and args[1] == 5
    assert (args[2].value, args[3].value, args[5].value) == (o.data_ptr(), d.data_ptr(), 0x51)
    want = {n: None for n in names}
    want.update({n: planes[n].data_ptr() for n in ("t", "u", "v", "tri")}, **{n: t.data_ptr() for n, t in out.items()})
    assert pointers(args[4]._obj) == want
    # with a bound: the counted symbol, the bound directly after n; point alone from t and tri
    rec.calls.clear()
    bound = i4(1)
    rt.resolve_hits_into({"point": out["normal"]}, o, d, dict(t=planes["t"], tri=planes["tri"], u=None), stream=7, bound_t=bound)
    (name, args), = rec.calls
    assert name == "rrt_resolve_hits_counted_device" and len(args) == 7 and args[1] == 5 and args[2].value == bound.data_ptr() and args[6].value == 7
    assert (args[3].value, args[4].value) == (o.data_ptr(), d.data_ptr())
    assert pointers(args[5]._obj) == dict({n: None for n in names}, t=planes["t"].data_ptr(), tri=planes["tri"].data_ptr(), point=out["normal"].data_ptr())
    # the host form: every output by default, in the shapes surface_rays returns
    rec.calls.clear()
    host = dict(hit=np.ones(4, np.uint8), t=np.ones(4), u=np.ones(4), v=np.ones(4), tri=np.zeros(4, np.uint32))
    O, D = np.zeros((4, 3)), np.ones((4, 3))
    got = rt.resolve_hits(O, D, host)
    (name, args), = rec.calls
    assert name == "rrt_resolve_hits" and len(args) == 5 and args[0] is None and args[1] == 4
    assert C.cast(args[2], C.c_void_p).value == O.ctypes.data and C.cast(args[3], C.c_void_p).value == D.ctypes.data
    assert tuple(got) == OUTPUTS and got["point"].shape == (4, 3) and got["next_dir"].dtype == np.float64 and got["lights"].shape == (4,) and got["albedo"].dtype == np.uint32
    s = pointers(args[4]._obj)
    assert s["hit"] is None and all(s[n] == host[n].ctypes.data for n in ("t", "u", "v", "tri")) and all(s[n] == got[n].ctypes.data for n in OUTPUTS)
    # a frame's visibility planes are valid input as they are: [h][w][4]
    rec.calls.clear()
    vis = dict(t=np.ones((2, 3, 4)), u=np.ones((2, 3, 4)), v=np.ones((2, 3, 4)), tri=np.zeros((2, 3, 4), np.uint32), albedo=np.zeros((2, 3, 4), np.uint32))
    got = rt.resolve_hits(np.zeros((24, 3)), np.ones((24, 3)), vis, outputs=("material",))
    (name, args), = rec.calls
    assert args[1] == 24 and tuple(got) == ("material",) and got["material"].shape == (24,)
