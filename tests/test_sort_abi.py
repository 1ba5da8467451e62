"""The sort of ray batches and records of the C ABI (include/rrt.h: rrt_sort_scratch_bytes, rrt_sort_rays[_device]) as far as no GPU is needed: the enum on both
sides, the exported symbols, the scratch size, the argument checks the library makes before any HIP call and before it looks at the handle, the checks the Python
mirror makes before it calls the library, and the numpy restatement of the key (tests/sort_checks.py) on values worked out by hand."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_values, fake_device
from compact_checks import SCRATCH_SIZES as SIZES
from sort_checks import DEAD_KEY, KEY_MODES, dead_rays, key_patterns, ray_key, sorted_batch

ROOT20 = (np.full(3, -20.0), np.full(3, 20.0))


def test_the_enum_on_both_sides(rrt, tmp_path):
    assert tuple(rrt.SORT_KEY_MODES) == KEY_MODES == ("given", "ray", "record") and rrt.DEAD_KEY == DEAD_KEY
    assert compiled_values(tmp_path, ("RRT_SORT_KEY_GIVEN", "RRT_SORT_KEY_RAY", "RRT_SORT_KEY_RECORD")) == [0, 1, 2]


def test_the_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    P, S, U = C.c_void_p, C.POINTER(rrt.CRaySet), C.POINTER(C.c_uint32)
    want = {"rrt_sort_scratch_bytes": (C.c_size_t, [C.c_uint32]),
            "rrt_sort_rays_device": (C.c_int, [P, C.c_uint32, C.c_uint32, P, S, S, P, P, P, P, C.c_size_t, P]),
            "rrt_sort_rays": (C.c_int, [P, C.c_uint32, C.c_uint32, U, S, S, U, U, U])}
    for name, sig in want.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == sig, name
        assert getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0]
    for method in ("sort_rays", "sort_rays_into", "sort_scratch_bytes"):
        assert callable(getattr(rrt.RayTracer, method)), method
    assert callable(rrt.sort_scratch_bytes)


def test_the_scratch_size(rrt):
    assert rrt.sort_scratch_bytes(0) == 0
    sizes = [rrt.sort_scratch_bytes(n) for n in sorted(SIZES)]
    assert all(s > 0 and s % 4 == 0 for s in sizes), sizes
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), f"the scratch size decreases somewhere: {sizes}"
    every = [rrt.sort_scratch_bytes(n) for n in range(1, 9000)]
    assert all(a <= b for a, b in zip(every, every[1:])) and all(s % 4 == 0 for s in every)
    for n in tuple(SIZES) + (8191, 8192, 8193, 2 ** 23, 2 ** 32 - 1):
        assert 16 * n <= rrt.sort_scratch_bytes(n) <= 20 * n + 65536, f"n = {n}: {rrt.sort_scratch_bytes(n)} bytes"
    assert rrt.sort_scratch_bytes(2 ** 32 - 1) >= rrt.sort_scratch_bytes(2 ** 20 + 4097)
    assert rrt.RayTracer.sort_scratch_bytes(70001) == rrt.sort_scratch_bytes(70001)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """Every refusal of rrt.h in both forms, through a handle that is the address of 4 KB of zeros: a check that came after the handle's first use would crash,
    not refuse.  (The device form's pointers are host addresses here: a call that got as far as a launch would fail in another way.)  The error detail is set
    and the outputs keep their pattern."""
    L = rrt.lib()
    n = 4
    vec = np.zeros((n, 3))
    mat = np.zeros(n, np.uint32)
    keys = np.arange(n, dtype=np.uint32)
    outs = {name: np.full(256 * n, PATTERN, np.uint32) for name in ("vec", "mat", "index", "keys_out", "count", "scratch")}
    at = lambda a: a.ctypes.data
    scratch_bytes = rrt.sort_scratch_bytes(n)
    assert 0 < scratch_bytes <= outs["scratch"].nbytes

    ray = rrt.CRaySet(origins=at(vec), dirs=at(vec), rec=rrt.CRaySurface(material=at(mat), point=at(vec), normal=at(vec)))
    dst = rrt.CRaySet(origins=at(outs["vec"]), rec=rrt.CRaySurface(material=at(outs["mat"])))
    rec = rrt.CRaySurface
    lacking = {"origins": rrt.CRaySet(dirs=at(vec)), "dirs": rrt.CRaySet(origins=at(vec)),
               "point": rrt.CRaySet(rec=rec(normal=at(vec), material=at(mat))), "normal": rrt.CRaySet(rec=rec(point=at(vec), material=at(mat))),
               "material": rrt.CRaySet(rec=rec(point=at(vec), normal=at(vec)))}
    orphan_max_t = rrt.CRaySet(max_t=at(outs["vec"]))                            # dst.max_t without src.max_t: no exception here
    orphan_rec = rrt.CRaySet(rec=rec(tri=at(outs["mat"])))                       # dst.rec.tri without src.rec.tri
    empty = rrt.CRaySet()
    ref = lambda s: None if s is None else C.byref(s)
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    ptr = lambda a: None if a is None else at(a)

    def host(rt, n, mode, k, s, d, index, keys_out, count, scratch=None, sb=None):
        return L.rrt_sort_rays(rt, n, mode, u32(k), ref(s), ref(d), u32(index), u32(keys_out), u32(count))

    def dev(rt, n, mode, k, s, d, index, keys_out, count, scratch=outs["scratch"], sb=scratch_bytes):
        return L.rrt_sort_rays_device(rt, n, mode, ptr(k), ref(s), ref(d), ptr(index), ptr(keys_out), ptr(count), ptr(scratch), sb, None)
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    I, K, Cn = outs["index"], outs["keys_out"], outs["count"]
    calls = []
    for form, call in (("rrt_sort_rays", host), ("rrt_sort_rays_device", dev)):
        calls += [(f"{form}, a NULL raytracer", lambda call=call: call(None, n, 0, keys, ray, dst, I, K, Cn)),
                  (f"{form}, a NULL raytracer, n = 0", lambda call=call: call(None, 0, 0, keys, ray, dst, I, K, Cn)),
                  (f"{form}, mode 3", lambda call=call: call(fake, n, 3, keys, ray, dst, I, K, Cn)),
                  (f"{form}, mode 3, n = 0", lambda call=call: call(fake, 0, 3, keys, ray, dst, I, K, Cn)),
                  (f"{form}, mode 0xFFFFFFFF", lambda call=call: call(fake, n, 0xFFFFFFFF, keys, ray, dst, I, K, Cn)),
                  (f"{form}, GIVEN without keys", lambda call=call: call(fake, n, 0, None, ray, dst, I, K, Cn)),
                  (f"{form}, RAY without src", lambda call=call: call(fake, n, 1, keys, None, None, I, K, Cn)),
                  (f"{form}, RAY without src.origins", lambda call=call: call(fake, n, 1, keys, lacking["origins"], None, I, K, Cn)),
                  (f"{form}, RAY without src.dirs", lambda call=call: call(fake, n, 1, keys, lacking["dirs"], None, I, K, Cn)),
                  (f"{form}, RECORD without src", lambda call=call: call(fake, n, 2, keys, None, None, I, K, Cn)),
                  (f"{form}, RECORD without src.rec.point", lambda call=call: call(fake, n, 2, keys, lacking["point"], None, I, K, Cn)),
                  (f"{form}, RECORD without src.rec.normal", lambda call=call: call(fake, n, 2, keys, lacking["normal"], None, I, K, Cn)),
                  (f"{form}, RECORD without src.rec.material", lambda call=call: call(fake, n, 2, keys, lacking["material"], None, I, K, Cn)),
                  (f"{form}, dst.max_t without src.max_t", lambda call=call: call(fake, n, 1, keys, ray, orphan_max_t, I, K, Cn)),
                  (f"{form}, dst.rec.tri without src.rec.tri", lambda call=call: call(fake, n, 0, keys, ray, orphan_rec, I, K, Cn)),
                  (f"{form}, dst.origins without src", lambda call=call: call(fake, n, 0, keys, None, dst, I, K, Cn)),
                  (f"{form}, every output NULL (no dst)", lambda call=call: call(fake, n, 1, keys, ray, None, None, None, None)),
                  (f"{form}, every output NULL (an empty dst)", lambda call=call: call(fake, n, 0, keys, None, empty, None, None, None))]
    calls += [("rrt_sort_rays_device, scratch one byte short", lambda: dev(fake, n, 0, keys, ray, dst, I, K, Cn, sb=scratch_bytes - 1)),
              ("rrt_sort_rays_device, scratch_bytes 0", lambda: dev(fake, n, 0, keys, None, None, I, K, Cn, sb=0)),
              ("rrt_sort_rays_device, a NULL scratch", lambda: dev(fake, n, 2, keys, ray, dst, I, K, Cn, scratch=None))]
    assert len(calls) == 2 * 18 + 3
    assert_refused(rrt, L, calls, outs)
    # n == 0 with valid arguments: RRT_OK, nothing enqueued (the handle is not a raytracer); the host form writes *count = 0 and nothing else
    assert dev(fake, 0, 1, None, ray, dst, I, K, Cn, scratch=None, sb=0) == rrt.OK and (Cn == PATTERN).all()
    assert host(fake, 0, 0, None, None, None, I, K, Cn) == rrt.OK
    assert Cn[0] == 0 and (Cn[1:] == PATTERN).all() and (I == PATTERN).all() and (K == PATTERN).all()
    Cn[0] = PATTERN
    assert host(fake, 0, 2, None, None, None, None, None, None) == rrt.OK
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
    src = dict(origins=f8(12), dirs=f8(12), point=f8(12), normal=f8(12), material=i4(4))

    def into(out, src=src, key="ray", index_t=None, keys_out_t=None, count_t=None, scratch_t=None, keys_t=None):
        rt.sort_rays_into(out, src, key, i4(4) if index_t is None else index_t, keys_out_t, i4(1) if count_t is None else count_t,
                          u1(4096) if scratch_t is None else scratch_t, keys_t=keys_t, stream=0)
    for call in (lambda: into({}, key="morton"), lambda: rt.sort_rays({}, key="hit", keys=np.zeros(4, np.uint32))):
        with pytest.raises(ValueError, match="unknown key"):
            call()
    for kw in (dict(out={"point": np.zeros(12)}), dict(out={}, src=dict(src, origins=np.zeros(12))), dict(out={}, index_t=np.zeros(4, np.uint32)),
               dict(out={}, keys_out_t=np.zeros(4, np.uint32)), dict(out={}, count_t=np.zeros(1, np.uint32)),
               dict(out={}, key="record", src=dict(src, material=np.zeros(4, np.uint32))), dict(out={}, key="given", keys_t=np.zeros(4, np.uint32))):
        with pytest.raises(AssertionError, match="not a device tensor"):
            into(**kw)
    with pytest.raises(AssertionError, match="scratch: not a contiguous device tensor"):
        into({}, scratch_t=np.zeros(4096, np.uint8))
    with pytest.raises(AssertionError, match="src dirs: want 12 contiguous elements of 8 bytes"):
        into({}, dict(src, dirs=f4(12)))
    with pytest.raises(AssertionError, match="src point: want 12 contiguous elements of 8 bytes"):
        into({}, dict(src, point=f8(9)))
    with pytest.raises(AssertionError, match="out rot: want 8 contiguous elements of 8 bytes"):
        into({"rot": f8(4)})
    with pytest.raises(AssertionError, match="out material: want 4 contiguous elements of 4 bytes"):
        into({"material": u1(4)})
    with pytest.raises(AssertionError, match="index: want 4 contiguous elements of 4 bytes"):
        into({}, index_t=i4(5))
    with pytest.raises(AssertionError, match="keys_out: want 4 contiguous elements of 4 bytes"):
        into({}, keys_out_t=f8(4))
    with pytest.raises(AssertionError, match="count: want 1 contiguous elements of 4 bytes"):
        into({}, count_t=i4(2))
    with pytest.raises(AssertionError, match="keys: want 5 contiguous elements of 4 bytes"):
        into({}, key="given", keys_t=f8(5))
    with pytest.raises(AssertionError, match="src origins: want 15 contiguous elements of 8 bytes"):        # (GIVEN: the batch is as long as its keys)
        into({}, key="given", keys_t=i4(5))
    with pytest.raises(AssertionError, match="key 'ray' needs the tensor dirs"):
        into({}, dict(origins=f8(12)))
    with pytest.raises(AssertionError, match="key 'record' needs the tensor normal"):
        into({}, dict(point=f8(12), material=i4(4)), key="record")
    with pytest.raises(AssertionError, match="key 'given' needs a keys tensor"):
        into({}, key="given")
    with pytest.raises(ValueError, match="unknown output 'occluded'"):
        into({"occluded": i4(4)})
    # the host form
    with pytest.raises(AssertionError, match="key 'ray' needs the array origins"):
        rt.sort_rays({}, dirs=np.zeros((4, 3)))
    with pytest.raises(AssertionError, match="key 'record' needs the array material"):
        rt.sort_rays(dict(point=np.zeros((4, 3)), normal=np.zeros((4, 3))), key="record")
    with pytest.raises(AssertionError, match="key 'given' needs a keys array"):
        rt.sort_rays({}, key="given")
    with pytest.raises(AssertionError, match="keys has 5 elements for 4 entries"):
        rt.sort_rays({}, origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), keys=np.zeros(5, np.uint32))
    with pytest.raises(AssertionError, match="array rot has 6 elements for 4 entries"):
        rt.sort_rays({}, key="given", keys=np.zeros(4, np.uint32), rot=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="unknown plane 'open'"):
        rt.sort_rays(dict(open=np.zeros(4, np.uint32)), key="given", keys=np.zeros(4, np.uint32))


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    from compact_checks import NAMES
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))

    def pointers(s):
        return {n: (getattr(s, n) if n in NAMES[:4] else getattr(s.rec, n)) for n in NAMES}
    src = dict(origins=f8(12), dirs=f8(12), max_t=f8(4), material=i4(4))
    out = dict(origins=f8(12), dirs=f8(12), max_t=f8(4))
    index, keys_out, count, scratch = i4(4), i4(4), i4(1), u1(4096)
    rt.sort_rays_into(out, src, "ray", index, keys_out, count, scratch, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_sort_rays_device" and len(args) == 12 and args[0] is None and args[1:3] == (4, 1) and args[3] is None
    assert pointers(args[4]._obj) == {n: (src[n].data_ptr() if n in src else None) for n in NAMES}
    assert pointers(args[5]._obj) == {n: (out[n].data_ptr() if n in out else None) for n in NAMES}
    assert (args[6].value, args[7].value, args[8].value, args[9].value, args[10], args[11].value) == (index.data_ptr(), keys_out.data_ptr(), count.data_ptr(),
                                                                                                      scratch.data_ptr(), 4096, 0x51)
    # GIVEN with index alone: both structs NULL
    rec.calls.clear()
    keys = i4(5)
    rt.sort_rays_into({}, {}, "given", i4(5), None, None, fake_device(torch.zeros(512, dtype=torch.int64)), keys_t=keys, stream=7)
    (name, args), = rec.calls
    assert args[1:3] == (5, 0) and args[3].value == keys.data_ptr() and args[4] is None and args[5] is None and args[7] is None and args[8] is None and args[10] == 4096
    # the host form
    rec.calls.clear()
    host = dict(point=np.ones((4, 3)), normal=np.ones((4, 3)), material=np.zeros(4, np.uint32), hit=np.ones(4, np.uint8))
    got = rt.sort_rays(host, key="record", rot=np.zeros((4, 2)))
    (name, args), = rec.calls
    assert name == "rrt_sort_rays" and len(args) == 9 and args[1:3] == (4, 2) and not args[3]
    assert set(got) == {"point", "normal", "material", "hit", "rot", "index", "keys", "count"} and got["count"] == 0
    s, d = pointers(args[4]._obj), pointers(args[5]._obj)
    assert {n for n, p in s.items() if p} == {"point", "normal", "material", "hit", "rot"} == {n for n, p in d.items() if p}
    assert all(d[n] == got[n].ctypes.data for n in d if d[n]) and got["rot"].shape == (4, 2) and got["point"].shape == (4, 3)
    assert C.cast(args[6], C.c_void_p).value == got["index"].ctypes.data and C.cast(args[7], C.c_void_p).value == got["keys"].ctypes.data


def test_the_model_of_the_key():
    """tests/sort_checks.py on values worked out by hand, root box +-20: 12.8 cells per unit."""
    p = np.array([[-20.0, -20.0, -20.0],          # cell (0, 0, 0)
                  [20.0, 20.0, 20.0],             # q = 512 on every axis: clamped to 511
                  [-19.99, 0.0, 19.99],           # cells 0, 256, 511
                  [np.nan, np.inf, -np.inf],      # 0, 511, 0
                  [-25.0, 25.0, 0.078125],        # clamped below and above; z: q = 257.0 exactly
                  [0.0, 0.0, 0.0]])
    d = np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [-0.0, 0.0, np.nan], [0.0, -1e-300, 0.0], [np.inf, -np.inf, -5.0], [1.0, 1.0, 1.0]])
    dead = np.array([0, 0, 0, 0, 0, 1], bool)
    key = ray_key(p, d, dead, ROOT20)
    morton = lambda x, y, z: sum((((x >> b) & 1) << (3 * b)) | (((y >> b) & 1) << (3 * b + 1)) | (((z >> b) & 1) << (3 * b + 2)) for b in range(9))
    want = [0, 0x07FFFFFF | (7 << 27), morton(0, 256, 511), morton(0, 511, 0) | (2 << 27), morton(0, 511, 257) | (6 << 27), DEAD_KEY]
    assert key.dtype == np.uint32 and key.tolist() == want, [hex(k) for k in key]
    assert morton(0, 511, 0) == 0x02492492 and morton(0, 511, 0) | (1 << 27) == 0x0a492492
    assert dead_rays(np.array([1.0, 0.0, -1.0, np.nan, np.inf, -0.0]), 6).tolist() == [False, True, True, True, False, True]
    assert not dead_rays(None, 3).any()
    # the sort of the model: ascending, ties in source order, the dead ones last
    keys = np.array([5, DEAD_KEY, 3, 5, 0, DEAD_KEY, 3], np.uint32)
    got = sorted_batch(keys, dict(tri=np.arange(7, dtype=np.uint32) * 10))
    assert got["index"].tolist() == [4, 2, 6, 0, 3, 1, 5] and got["count"] == 5 and got["tri"].tolist() == [40, 20, 60, 0, 30, 10, 50]
    for n in (1, 2, 64, 1025):
        pats = key_patterns(n)
        assert len(pats) == 8 and all(k.dtype == np.uint32 and k.shape == (n,) for k in pats.values())
        assert n == 1 or (np.diff(pats["strictly descending"].astype(np.int64)) < 0).all()
