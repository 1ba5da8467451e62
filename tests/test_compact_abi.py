"""Compaction of ray batches and records of the C ABI (include/rrt.h: rrt_ray_set, rrt_compact_scratch_bytes, rrt_compact_rays[_device], rrt_scatter_rays[_device])
as far as no GPU is needed: the struct layout on both sides, the exported symbols, the scratch size, the argument checks the library makes before any HIP call and
before it looks at the handle, and the checks the Python mirror makes before it calls the library."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_layout, compiled_values, fake_device
from compact_checks import ELEM_BYTES, NAMES, OFFSETS, RECORD_NAMES, SCRATCH_SIZES as SIZES, SELECTS


def test_the_struct_is_128_bytes_on_both_sides(rrt, tmp_path):
    assert C.sizeof(rrt.CRaySet) == 128 and rrt.STRUCTS["rrt_ray_set"] is rrt.CRaySet
    assert [n for n, _ in rrt.CRaySet._fields_] == list(NAMES[:4]) + ["rec"] and rrt.CRaySet.rec.offset == 32 and rrt.CRaySet.rec.size == 96
    assert tuple(rrt.RAY_SET_ARRAYS) == NAMES and tuple(rrt.RAY_SURFACE_PLANES) == RECORD_NAMES
    mirror = {n: getattr(rrt.CRaySet, n).offset for n in NAMES[:4]}
    mirror.update({n: rrt.CRaySet.rec.offset + getattr(rrt.CRaySurface, n).offset for n in RECORD_NAMES})
    assert mirror == OFFSETS
    assert {n: np.dtype(rrt._ray_plane(n, rrt.CRaySet)[0]).itemsize * rrt._ray_plane(n, rrt.CRaySet)[1] for n in NAMES} == ELEM_BYTES
    assert tuple(rrt.SELECT_MODES) == SELECTS
    fields = [n if n in NAMES[:4] else f"rec.{n}" for n in NAMES]
    assert compiled_layout(tmp_path, "rrt_ray_set", fields) == (128, [OFFSETS[n] for n in NAMES])
    assert compiled_values(tmp_path, ("RRT_SELECT_HIT", "RRT_SELECT_MIRROR", "RRT_SELECT_FLAG")) == [0, 1, 2]


def test_the_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    P, S = C.c_void_p, C.POINTER(rrt.CRaySet)
    want = {"rrt_compact_scratch_bytes": (C.c_size_t, [C.c_uint32]),
            "rrt_compact_rays_device": (C.c_int, [P, C.c_uint32, C.c_uint32, P, S, S, P, P, P, C.c_size_t, P]),
            "rrt_compact_rays": (C.c_int, [P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), S, S, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
            "rrt_scatter_rays_device": (C.c_int, [P, C.c_uint32, P, C.c_uint32, P, P, P]),
            "rrt_scatter_rays": (C.c_int, [P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, P, P])}
    for name, sig in want.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == sig, name
        assert getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0]
    for method in ("compact_rays", "compact_rays_into", "scatter_rays", "scatter_rays_into", "compact_scratch_bytes"):
        assert callable(getattr(rrt.RayTracer, method)), method
    assert callable(rrt.compact_scratch_bytes)


def test_the_scratch_size(rrt):
    assert rrt.compact_scratch_bytes(0) == 0
    sizes = [rrt.compact_scratch_bytes(n) for n in sorted(SIZES)]
    assert all(s > 0 and s % 4 == 0 for s in sizes), sizes
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), f"the scratch size decreases somewhere: {sizes}"
    every = [rrt.compact_scratch_bytes(n) for n in range(1, 5000)]
    assert all(a <= b for a, b in zip(every, every[1:]))
    for n in (2 ** 16, 70001, 2 ** 20, 2 ** 20 + 4097, 2 ** 32 - 1):
        assert rrt.compact_scratch_bytes(n) < n, f"n = {n}: {rrt.compact_scratch_bytes(n)} bytes"
    assert rrt.compact_scratch_bytes(2 ** 32 - 1) >= rrt.compact_scratch_bytes(2 ** 20 + 4097)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """Every refusal of rrt.h in both forms, through a handle that is the address of 4 KB of zeros: a check that came after the handle's first use would crash,
    not refuse.  (The device form's pointers are host addresses here: a call that got as far as a launch would fail in another way.)  The error detail is set
    and the outputs keep their pattern."""
    L = rrt.lib()
    n = 4
    vec = np.zeros((n, 3))
    mat = np.zeros(n, np.uint32)
    flag = np.ones(n, np.uint8)
    outs = {name: np.full(8 * n, PATTERN, np.uint32) for name in ("vec", "mat", "max_t", "index", "count", "scratch", "dst")}
    at = lambda a: a.ctypes.data
    scratch_bytes = rrt.compact_scratch_bytes(n)
    assert 0 < scratch_bytes <= outs["scratch"].nbytes

    src = rrt.CRaySet(origins=at(vec), rec=rrt.CRaySurface(material=at(mat), point=at(vec)))
    dst = rrt.CRaySet(origins=at(outs["vec"]), max_t=at(outs["max_t"]), rec=rrt.CRaySurface(material=at(outs["mat"])))
    no_material = rrt.CRaySet(origins=at(vec))
    orphan = rrt.CRaySet(dirs=at(outs["vec"]))                                   # dst.dirs without src.dirs
    orphan_rec = rrt.CRaySet(rec=rrt.CRaySurface(normal=at(outs["vec"])))        # dst.rec.normal without src.rec.normal
    empty = rrt.CRaySet()
    ref = lambda s: None if s is None else C.byref(s)
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))

    def host(rt, n, select, f, s, d, index, count, scratch=None, sb=None):
        return L.rrt_compact_rays(rt, n, select, u8(f), ref(s), ref(d), u32(index), u32(count))

    def dev(rt, n, select, f, s, d, index, count, scratch=outs["scratch"], sb=scratch_bytes):
        return L.rrt_compact_rays_device(rt, n, select, None if f is None else at(f), ref(s), ref(d), None if index is None else at(index),
                                         None if count is None else at(count), None if scratch is None else at(scratch), sb, None)
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    I, Cn = outs["index"], outs["count"]
    calls = []
    for form, call in (("rrt_compact_rays", host), ("rrt_compact_rays_device", dev)):
        calls += [(f"{form}, a NULL raytracer", lambda call=call: call(None, n, 0, flag, src, dst, I, Cn)),
                  (f"{form}, a NULL raytracer, n = 0", lambda call=call: call(None, 0, 0, flag, src, dst, I, Cn)),
                  (f"{form}, select 3", lambda call=call: call(fake, n, 3, flag, src, dst, I, Cn)),
                  (f"{form}, select 3, n = 0", lambda call=call: call(fake, 0, 3, flag, src, dst, I, Cn)),
                  (f"{form}, select 0xFFFFFFFF", lambda call=call: call(fake, n, 0xFFFFFFFF, flag, src, dst, I, Cn)),
                  (f"{form}, HIT without src", lambda call=call: call(fake, n, 0, flag, None, None, I, Cn)),
                  (f"{form}, HIT without src.rec.material", lambda call=call: call(fake, n, 0, flag, no_material, None, I, Cn)),
                  (f"{form}, MIRROR without src.rec.material", lambda call=call: call(fake, n, 1, flag, no_material, None, I, Cn)),
                  (f"{form}, FLAG without flag", lambda call=call: call(fake, n, 2, None, src, dst, I, Cn)),
                  (f"{form}, dst.dirs without src.dirs", lambda call=call: call(fake, n, 0, flag, src, orphan, I, Cn)),
                  (f"{form}, dst.rec.normal without src.rec.normal", lambda call=call: call(fake, n, 2, flag, src, orphan_rec, I, Cn)),
                  (f"{form}, dst.origins without src", lambda call=call: call(fake, n, 2, flag, None, dst, I, Cn)),
                  (f"{form}, every output NULL (no dst)", lambda call=call: call(fake, n, 0, flag, src, None, None, None)),
                  (f"{form}, every output NULL (an empty dst)", lambda call=call: call(fake, n, 2, flag, None, empty, None, None))]
    calls += [("rrt_compact_rays_device, scratch one byte short", lambda: dev(fake, n, 0, flag, src, dst, I, Cn, sb=scratch_bytes - 1)),
              ("rrt_compact_rays_device, scratch_bytes 0", lambda: dev(fake, n, 2, flag, None, None, I, Cn, sb=0)),
              ("rrt_compact_rays_device, a NULL scratch", lambda: dev(fake, n, 0, flag, src, dst, I, Cn, scratch=None))]
    D = outs["dst"]
    for form, call in (("rrt_scatter_rays", lambda rt, k, i, e, s, d: L.rrt_scatter_rays(rt, k, u32(i), e, None if s is None else at(s), None if d is None else at(d))),
                       ("rrt_scatter_rays_device", lambda rt, k, i, e, s, d: L.rrt_scatter_rays_device(rt, k, None if i is None else at(i), e, None if s is None else at(s),
                                                                                                       None if d is None else at(d), None))):
        calls += [(f"{form}, a NULL raytracer", lambda call=call: call(None, n, mat, 4, mat, D)),
                  (f"{form}, a NULL raytracer, n = 0", lambda call=call: call(None, 0, mat, 4, mat, D)),
                  (f"{form}, a NULL index", lambda call=call: call(fake, n, None, 4, mat, D)),
                  (f"{form}, a NULL src", lambda call=call: call(fake, n, mat, 4, None, D)),
                  (f"{form}, a NULL dst", lambda call=call: call(fake, n, mat, 4, mat, None))]
        calls += [(f"{form}, elem_bytes {e}", lambda call=call, e=e: call(fake, n, mat, e, mat, D)) for e in (0, 2, 3, 5, 12, 32, 0xFFFFFFFF)]
        calls += [(f"{form}, elem_bytes 2, n = 0", lambda call=call: call(fake, 0, mat, 2, mat, D))]
    assert len(calls) == 2 * 14 + 3 + 2 * (5 + 7 + 1)
    assert_refused(rrt, L, calls, outs)
    # n == 0 with valid arguments: RRT_OK, nothing enqueued (the handle is not a raytracer); the host form writes *count = 0 and nothing else
    assert dev(fake, 0, 0, flag, src, dst, I, Cn, scratch=None, sb=0) == rrt.OK and (Cn == PATTERN).all()
    assert host(fake, 0, 2, None, None, None, I, Cn) == rrt.OK
    assert Cn[0] == 0 and (Cn[1:] == PATTERN).all() and (I == PATTERN).all()
    Cn[0] = PATTERN
    assert L.rrt_scatter_rays(fake, 0, None, 8, None, None) == rrt.OK and L.rrt_scatter_rays_device(fake, 0, None, 24, None, None, None) == rrt.OK
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
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))
    src = dict(point=f8(12), material=i4(4), rot=f8(8))

    def into(out, src=src, select="hit", index_t=None, count_t=None, scratch_t=None, flag_t=None):
        rt.compact_rays_into(out, src, select, i4(4) if index_t is None else index_t, i4(1) if count_t is None else count_t,
                             u1(64) if scratch_t is None else scratch_t, flag_t=flag_t, stream=0)
    # an unknown select, in both forms
    for call in (lambda: into({}, select="miss"), lambda: rt.compact_rays(dict(material=np.zeros(4, np.uint32)), select="all")):
        with pytest.raises(ValueError, match="unknown select"):
            call()
    # a tensor on the host
    for kw in (dict(out={"point": np.zeros(12)}), dict(out={}, src=dict(src, point=np.zeros(12))), dict(out={}, index_t=np.zeros(4, np.uint32)),
               dict(out={}, count_t=np.zeros(1, np.uint32)), dict(out={}, src=dict(src, material=np.zeros(4, np.uint32))),
               dict(out={}, select="flag", flag_t=np.zeros(4, np.uint8))):
        with pytest.raises(AssertionError, match="not a device tensor"):
            into(**kw)
    with pytest.raises(AssertionError, match="scratch: not a contiguous device tensor"):
        into({}, scratch_t=np.zeros(64, np.uint8))
    # a wrong dtype and a wrong length
    with pytest.raises(AssertionError, match="src point: want 12 contiguous elements of 8 bytes"):
        into({}, dict(src, point=f4(12)))
    with pytest.raises(AssertionError, match="src point: want 12 contiguous elements of 8 bytes"):
        into({}, dict(src, point=f8(4)))
    with pytest.raises(AssertionError, match="out point: want 12 contiguous elements of 8 bytes"):
        into({"point": f8(15)})
    with pytest.raises(AssertionError, match="out rot: want 8 contiguous elements of 8 bytes"):
        into({"rot": f8(4)})
    with pytest.raises(AssertionError, match="out max_t: want 4 contiguous elements of 8 bytes"):
        into({"max_t": f4(4)})
    with pytest.raises(AssertionError, match="out material: want 4 contiguous elements of 4 bytes"):
        into({"material": u1(4)})
    with pytest.raises(AssertionError, match="index: want 4 contiguous elements of 4 bytes"):
        into({}, index_t=i4(5))
    with pytest.raises(AssertionError, match="index: want 4 contiguous elements of 4 bytes"):
        into({}, index_t=f8(4))
    with pytest.raises(AssertionError, match="count: want 1 contiguous elements of 4 bytes"):
        into({}, count_t=i4(2))
    with pytest.raises(AssertionError, match="flag: want 4 contiguous elements of 1 bytes"):
        into({}, select="flag", flag_t=i4(4))
    with pytest.raises(AssertionError, match="src point: want 15 contiguous elements of 8 bytes"):          # (the batch is as long as its flag array)
        into({}, select="flag", flag_t=u1(5))
    with pytest.raises(AssertionError, match="needs a material tensor"):
        into({}, dict(point=f8(12)))
    with pytest.raises(AssertionError, match="needs a flag tensor"):
        into({}, select="flag")
    with pytest.raises(ValueError, match="unknown output 'occluded'"):
        into({"occluded": i4(4)})
    # the scatter
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.scatter_rays_into(np.zeros(4, np.uint32), f8(4), f8(4), stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.scatter_rays_into(i4(4), np.zeros(4), f8(4), stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.scatter_rays_into(i4(4), f8(4), np.zeros(4), stream=0)
    with pytest.raises(AssertionError, match="index: want 4 contiguous elements of 4 bytes"):
        rt.scatter_rays_into(f8(4), f8(4), f8(4), stream=0)
    with pytest.raises(AssertionError, match="src: 6 elements for 4 entries"):
        rt.scatter_rays_into(i4(4), f8(6), f8(6), stream=0)
    with pytest.raises(AssertionError, match="dst: want 12 contiguous elements of 8 bytes"):
        rt.scatter_rays_into(i4(4), f8(12), f8(4), stream=0)
    with pytest.raises(AssertionError, match="dst: want 4 contiguous elements of 8 bytes"):
        rt.scatter_rays_into(i4(4), f8(4), f4(4), stream=0)
    # the host forms
    host = dict(point=np.zeros((4, 3)), material=np.zeros(4, np.uint32))
    with pytest.raises(AssertionError, match="array point has 9 elements for 4 entries"):
        rt.compact_rays(dict(host, point=np.zeros((3, 3))))
    with pytest.raises(AssertionError, match="array rot has 6 elements for 4 entries"):
        rt.compact_rays(host, rot=np.zeros((3, 2)))
    with pytest.raises(AssertionError, match="flag has 5 elements for 4 entries"):
        rt.compact_rays(host, flag=np.zeros(5, np.uint8))
    with pytest.raises(AssertionError, match="needs a material array"):
        rt.compact_rays(dict(point=np.zeros((4, 3))))
    with pytest.raises(AssertionError, match="needs a flag array"):
        rt.compact_rays(host, select="flag")
    with pytest.raises(ValueError, match="unknown plane 'open'"):
        rt.compact_rays(dict(host, open=np.zeros(4, np.uint32)))
    with pytest.raises(AssertionError, match="src has 3 elements and dst 4 for 4 entries"):
        rt.scatter_rays(np.zeros(4, np.uint32), np.zeros(3), np.zeros(4))
    with pytest.raises(AssertionError, match="not a contiguous writable array"):
        rt.scatter_rays(np.zeros(4, np.uint32), np.zeros(4), np.zeros((4, 2))[:, 0])


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))

    def pointers(s):
        return {n: (getattr(s, n) if n in NAMES[:4] else getattr(s.rec, n)) for n in NAMES}
    # the device form: next_origin / next_dir passed as origins / dirs, a synthesised max_t
    src = dict(material=i4(4), point=f8(12), next_origin=f8(12), next_dir=f8(12))
    src.update(origins=src["next_origin"], dirs=src["next_dir"])
    out = dict(origins=f8(12), dirs=f8(12), max_t=f8(4), point=f8(12), material=i4(4))
    index, count, scratch = i4(4), i4(1), u1(48)
    rt.compact_rays_into(out, src, "mirror", index, count, scratch, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_compact_rays_device" and len(args) == 11 and args[0] is None and args[1:3] == (4, 1) and args[3] is None
    assert pointers(args[4]._obj) == {n: (src[n].data_ptr() if n in src else None) for n in NAMES}
    assert pointers(args[5]._obj) == {n: (out[n].data_ptr() if n in out else None) for n in NAMES}
    assert args[4]._obj.origins == args[4]._obj.rec.next_origin
    assert (args[6].value, args[7].value, args[8].value, args[9], args[10].value) == (index.data_ptr(), count.data_ptr(), scratch.data_ptr(), 48, 0x51)
    # FLAG with index and count alone: both structs NULL
    rec.calls.clear()
    flag = u1(5)
    rt.compact_rays_into({}, {}, "flag", i4(5), None, fake_device(torch.zeros(4, dtype=torch.int64)), flag_t=flag, stream=7)
    (name, args), = rec.calls
    assert args[1:3] == (5, 2) and args[3].value == flag.data_ptr() and args[4] is None and args[5] is None and args[7] is None and args[9] == 32
    # the host form
    rec.calls.clear()
    host = dict(point=np.ones((4, 3)), material=np.zeros(4, np.uint32), hit=np.ones(4, np.uint8))
    got = rt.compact_rays(host, rot=np.zeros((4, 2)), max_t=True)
    (name, args), = rec.calls
    assert name == "rrt_compact_rays" and len(args) == 8 and args[1:3] == (4, 0) and not args[3]
    assert set(got) == {"point", "material", "hit", "rot", "max_t", "index", "count"} and got["count"] == 0
    s, d = pointers(args[4]._obj), pointers(args[5]._obj)
    assert {n for n, p in s.items() if p} == {"point", "material", "hit", "rot"} and {n for n, p in d.items() if p} == {"point", "material", "hit", "rot", "max_t"}
    assert all(d[n] == got[n].ctypes.data for n in d if d[n]) and got["max_t"].shape == (4,) and got["point"].shape == (4, 3)
    assert C.cast(args[6], C.c_void_p).value == got["index"].ctypes.data
    # the scatters
    rec.calls.clear()
    a, b = f8(12), f8(12)
    rt.scatter_rays_into(index, a, b, stream=9)
    dst = np.zeros((4, 2))
    assert rt.scatter_rays(np.arange(4), np.ones((4, 2)), dst) is dst
    (n1, a1), (n2, a2) = rec.calls
    assert n1 == "rrt_scatter_rays_device" and (a1[1], a1[2].value, a1[3], a1[4].value, a1[5].value, a1[6].value) == (4, index.data_ptr(), 24, a.data_ptr(), b.data_ptr(), 9)
    assert n2 == "rrt_scatter_rays" and (a2[1], a2[3], a2[5].value) == (4, 16, dst.ctypes.data)
