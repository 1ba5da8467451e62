"""The counted device forms of the C ABI (include/rrt.h: COUNTED DEVICE FORMS -- the nine `_device` calls of the per-ray pipeline with a launch bound in device
memory directly after n) as far as no GPU is needed: the exported symbols and their signatures, every refusal of the uncounted forms made by the counted ones with a
bound given, before any HIP call and through a handle that is no raytracer, and what the Python mirror checks and hands over."""
import ctypes as C

import os

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, fake_device
from conftest import ROOT

COUNTED = ("intersect_rays", "get_ray_colours", "occluded_rays", "surface_rays", "shade_rays", "ambient_rays", "compact_rays", "scatter_rays", "mix_rays")


def test_the_nine_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    P, U, Z = C.c_void_p, C.c_uint32, C.c_size_t
    RS, SH, AM, SM, SET = (C.POINTER(t) for t in (rrt.CRaySurface, rrt.CRayShade, rrt.CRayAmbient, rrt.CAmbientSamples, rrt.CRaySet))
    want = {"rrt_intersect_rays_counted_device": [P, U, P, P, P, P, P, P, P, P, P, P],
            "rrt_get_ray_colours_counted_device": [P, U, P, P, P, P, P],
            "rrt_occluded_rays_counted_device": [P, U, P, P, P, P, P, P],
            "rrt_surface_rays_counted_device": [P, U, P, P, P, P, RS, P],
            "rrt_shade_rays_counted_device": [P, U, P, P, RS, U, SH, P],
            "rrt_ambient_rays_counted_device": [P, U, P, RS, P, SM, AM, P],
            "rrt_compact_rays_counted_device": [P, U, P, U, P, SET, SET, P, P, P, Z, P],
            "rrt_scatter_rays_counted_device": [P, U, P, P, U, P, P, P],
            "rrt_mix_rays_counted_device": [P, U, P, P, P, P, P, P, P]}
    assert sorted(want) == sorted(f"rrt_{c}_counted_device" for c in COUNTED)
    for name, args in want.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == (C.c_int, args), name
        assert getattr(L, name).argtypes == args and getattr(L, name).restype is C.c_int
        # the counted form is the uncounted one with ONE more argument, a pointer, directly after n
        plain = rrt.SYMBOLS[name.replace("_counted_device", "_device")]
        assert plain == (C.c_int, args[:2] + args[3:]) and args[2] is P, name
    header = open(os.path.join(ROOT, "include", "rrt.h")).read()
    for name in want:
        assert f"int {name}(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, " in header, name


def test_the_library_refuses_before_any_gpu_work(rrt):
    """Every refusal of the nine uncounted device forms, made by the counted ones with a bound that is not NULL, through a handle that is the address of 4 KB of
    zeros: a check that came after the handle's first use would crash, not refuse.  (Pointers are host addresses here: a call that got as far as a launch would
    fail in another way.)  The error detail is set, the outputs keep their pattern, the bound and the handle are unwritten."""
    L = rrt.lib()
    n = 4
    at = lambda a: None if a is None else a.ctypes.data
    vec, mat, flag = np.zeros((n, 3)), np.zeros(n, np.uint32), np.ones(n, np.uint8)
    bound = np.full(2, 3, np.uint32)
    B = at(bound)
    outs = {name: np.full(8 * n, PATTERN, np.uint32) for name in ("a", "b", "c", "d", "e", "index", "count", "scratch")}
    A, Bo, Co, D, E, I, Cn, S = (outs[k] for k in ("a", "b", "c", "d", "e", "index", "count", "scratch"))
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    ref = lambda s: None if s is None else C.byref(s)
    calls = []

    # ---- the ray calls that take rays: a NULL raytracer, NULL origins or directions, no output
    intersect = lambda rt, k, o, d, outp: L.rrt_intersect_rays_counted_device(rt, k, B, at(o), at(d), at(vec), *outp, None)
    five = (at(A), at(Bo), at(Co), at(D), at(E))
    colours = lambda rt, k, o, d, outp: L.rrt_get_ray_colours_counted_device(rt, k, B, at(o), at(d), outp, None)
    occluded = lambda rt, k, o, d, outp: L.rrt_occluded_rays_counted_device(rt, k, B, at(o), at(d), None, outp, None)
    surf_out = rrt.CRaySurface(hit=at(A), point=at(Bo), lights=at(Co))
    surface = lambda rt, k, o, d, outp: L.rrt_surface_rays_counted_device(rt, k, B, at(o), at(d), None, ref(outp), None)
    for form, call, good, none in (("intersect", intersect, five, (None,) * 5), ("get_ray_colours", colours, at(A), None), ("occluded", occluded, at(A), None),
                                   ("surface", surface, surf_out, rrt.CRaySurface())):
        calls += [(f"{form}, a NULL raytracer", lambda call=call, good=good: call(None, n, vec, vec, good)),
                  (f"{form}, a NULL raytracer, n = 0", lambda call=call, good=good: call(None, 0, vec, vec, good)),
                  (f"{form}, NULL origins", lambda call=call, good=good: call(fake, n, None, vec, good)),
                  (f"{form}, NULL directions", lambda call=call, good=good: call(fake, n, vec, None, good)),
                  (f"{form}, no output", lambda call=call, none=none: call(fake, n, vec, vec, none))]
    calls += [("surface, a NULL output struct", lambda: surface(fake, n, vec, vec, None)),
              ("surface, a NULL output struct, n = 0", lambda: surface(fake, 0, vec, vec, None))]

    # ---- shade
    rec = rrt.CRaySurface(albedo=at(mat), point=at(vec), normal=at(vec), material=at(mat))
    sh_out = rrt.CRayShade(colour=at(A), local=at(Bo), kr=at(Co))
    shade = lambda rt, k, d, r, o: L.rrt_shade_rays_counted_device(rt, k, B, at(d), ref(r), 0, ref(o), None)
    calls += [("shade, a NULL raytracer", lambda: shade(None, n, vec, rec, sh_out)),
              ("shade, a NULL raytracer, n = 0", lambda: shade(None, 0, vec, rec, sh_out)),
              ("shade, a NULL record struct", lambda: shade(fake, n, vec, None, sh_out)),
              ("shade, a NULL record struct, n = 0", lambda: shade(fake, 0, vec, None, sh_out)),
              ("shade, a NULL output struct", lambda: shade(fake, n, vec, rec, None)),
              ("shade, no output", lambda: shade(fake, n, vec, rec, rrt.CRayShade())),
              ("shade, NULL directions", lambda: shade(fake, n, None, rec, sh_out))]
    for name in ("albedo", "point", "normal", "material"):
        less = rrt.CRaySurface(**{k: getattr(rec, k) for k in ("albedo", "point", "normal", "material") if k != name})
        calls.append((f"shade, NULL {name}", lambda less=less: shade(fake, n, vec, less, sh_out)))

    # ---- ambient
    dirs = np.ascontiguousarray([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
    def samples(d=dirs, k=2, max_t=10.0):
        return rrt.CAmbientSamples(dirs=None if d is None else d.ctypes.data_as(C.POINTER(C.c_double)), n=k, max_t=max_t)
    nan_dirs = dirs.copy(); nan_dirs[1, 1] = np.nan
    many = np.ascontiguousarray(np.tile(dirs, (17, 1)))
    good = samples()
    arec = rrt.CRaySurface(point=at(vec), normal=at(vec), material=at(mat))
    am_out = rrt.CRayAmbient(occluded=at(A), open=at(Bo))
    ambient = lambda rt, k, r, s, o: L.rrt_ambient_rays_counted_device(rt, k, B, ref(r), None, ref(s), ref(o), None)
    calls += [("ambient, a NULL raytracer", lambda: ambient(None, n, arec, good, am_out)),
              ("ambient, a NULL raytracer, n = 0", lambda: ambient(None, 0, arec, good, am_out)),
              ("ambient, both outputs NULL", lambda: ambient(fake, n, arec, good, rrt.CRayAmbient()))]
    tables = [("n == 0", samples(k=0)), ("n == 33", samples(d=many, k=33)), ("NULL dirs", samples(d=None)), ("a NaN direction component", samples(d=nan_dirs)),
              ("max_t NaN", samples(max_t=np.nan)), ("max_t 0", samples(max_t=0.0)), ("max_t -1", samples(max_t=-1.0))]
    for k in (n, 0):
        calls += [(f"ambient, n = {k}, a NULL record struct", lambda k=k: ambient(fake, k, None, good, am_out)),
                  (f"ambient, n = {k}, a NULL samples struct", lambda k=k: ambient(fake, k, arec, None, am_out)),
                  (f"ambient, n = {k}, a NULL output struct", lambda k=k: ambient(fake, k, arec, good, None))]
        calls += [(f"ambient, n = {k}, {what}", lambda k=k, s=s: ambient(fake, k, arec, s, am_out)) for what, s in tables]
    for name in ("point", "normal", "material"):
        less = rrt.CRaySurface(**{k: getattr(arec, k) for k in ("point", "normal", "material") if k != name})
        calls.append((f"ambient, NULL {name}", lambda less=less: ambient(fake, n, less, good, am_out)))

    # ---- compaction (the cases of tests/test_compact_abi.py) and its own refusal
    scratch_bytes = rrt.compact_scratch_bytes(n)
    assert 0 < scratch_bytes <= S.nbytes
    src = rrt.CRaySet(origins=at(vec), rec=rrt.CRaySurface(material=at(mat), point=at(vec)))
    dst = rrt.CRaySet(origins=at(A), max_t=at(Bo), rec=rrt.CRaySurface(material=at(Co)))
    no_material = rrt.CRaySet(origins=at(vec))
    orphan = rrt.CRaySet(dirs=at(A))
    orphan_rec = rrt.CRaySet(rec=rrt.CRaySurface(normal=at(A)))
    empty = rrt.CRaySet()

    def compact(rt, k, select, f, s, d, index, count, scratch=S, sb=scratch_bytes, b=B):
        return L.rrt_compact_rays_counted_device(rt, k, b, select, at(f), ref(s), ref(d), at(index), at(count) if isinstance(count, np.ndarray) else count,
                                                 at(scratch), sb, None)
    calls += [("compact, a NULL raytracer", lambda: compact(None, n, 0, flag, src, dst, I, Cn)),
              ("compact, a NULL raytracer, n = 0", lambda: compact(None, 0, 0, flag, src, dst, I, Cn)),
              ("compact, select 3", lambda: compact(fake, n, 3, flag, src, dst, I, Cn)),
              ("compact, select 3, n = 0", lambda: compact(fake, 0, 3, flag, src, dst, I, Cn)),
              ("compact, select 0xFFFFFFFF", lambda: compact(fake, n, 0xFFFFFFFF, flag, src, dst, I, Cn)),
              ("compact, HIT without src", lambda: compact(fake, n, 0, flag, None, None, I, Cn)),
              ("compact, HIT without src.rec.material", lambda: compact(fake, n, 0, flag, no_material, None, I, Cn)),
              ("compact, MIRROR without src.rec.material", lambda: compact(fake, n, 1, flag, no_material, None, I, Cn)),
              ("compact, FLAG without flag", lambda: compact(fake, n, 2, None, src, dst, I, Cn)),
              ("compact, dst.dirs without src.dirs", lambda: compact(fake, n, 0, flag, src, orphan, I, Cn)),
              ("compact, dst.rec.normal without src.rec.normal", lambda: compact(fake, n, 2, flag, src, orphan_rec, I, Cn)),
              ("compact, dst.origins without src", lambda: compact(fake, n, 2, flag, None, dst, I, Cn)),
              ("compact, every output NULL (no dst)", lambda: compact(fake, n, 0, flag, src, None, None, None)),
              ("compact, every output NULL (an empty dst)", lambda: compact(fake, n, 2, flag, None, empty, None, None)),
              ("compact, scratch one byte short", lambda: compact(fake, n, 0, flag, src, dst, I, Cn, sb=scratch_bytes - 1)),
              ("compact, scratch_bytes 0", lambda: compact(fake, n, 2, flag, None, None, I, Cn, sb=0)),
              ("compact, a NULL scratch", lambda: compact(fake, n, 0, flag, src, dst, I, Cn, scratch=None)),
              ("compact, the bound and the output count are the same word", lambda: compact(fake, n, 0, flag, src, dst, I, B)),
              ("compact, the bound and the output count are the same word, count alone", lambda: compact(fake, n, 2, flag, None, None, None, at(Cn), b=at(Cn)))]

    # ---- scatter and mix
    scatter = lambda rt, k, i, e, s, d: L.rrt_scatter_rays_counted_device(rt, k, B, at(i), e, at(s), at(d), None)
    calls += [("scatter, a NULL raytracer", lambda: scatter(None, n, mat, 4, mat, D)),
              ("scatter, a NULL raytracer, n = 0", lambda: scatter(None, 0, mat, 4, mat, D)),
              ("scatter, a NULL index", lambda: scatter(fake, n, None, 4, mat, D)),
              ("scatter, a NULL src", lambda: scatter(fake, n, mat, 4, None, D)),
              ("scatter, a NULL dst", lambda: scatter(fake, n, mat, 4, mat, None)),
              ("scatter, elem_bytes 2, n = 0", lambda: scatter(fake, 0, mat, 2, mat, D))]
    calls += [(f"scatter, elem_bytes {e}", lambda e=e: scatter(fake, n, mat, e, mat, D)) for e in (0, 2, 3, 5, 12, 32, 0xFFFFFFFF)]
    mix = lambda rt, k, local, colour: L.rrt_mix_rays_counted_device(rt, k, B, at(mat), at(local), at(vec), at(mat), at(colour), None)
    calls += [("mix, a NULL raytracer", lambda: mix(None, n, vec, A)),
              ("mix, a NULL raytracer, n = 0", lambda: mix(None, 0, vec, A)),
              ("mix, a NULL local", lambda: mix(fake, n, None, A)),
              ("mix, a NULL colour", lambda: mix(fake, n, vec, None))]

    assert len(calls) == 4 * 5 + 2 + 11 + (3 + 2 * 10 + 3) + 19 + 13 + 4
    assert_refused(rrt, L, calls, dict(outs, bound=bound))

    # n == 0 with valid arguments and a bound: RRT_OK, nothing enqueued (the handle is not a raytracer), nothing written
    oks = [intersect(fake, 0, vec, vec, five), colours(fake, 0, vec, vec, at(A)), occluded(fake, 0, vec, vec, at(A)), surface(fake, 0, vec, vec, surf_out),
           shade(fake, 0, vec, rec, sh_out), ambient(fake, 0, arec, good, am_out), compact(fake, 0, 0, flag, src, dst, I, Cn, scratch=None, sb=0),
           scatter(fake, 0, None, 24, None, None), mix(fake, 0, None, None),
           # (and with NULL arrays, which n == 0 does not look at)
           intersect(fake, 0, None, None, (None,) * 5), L.rrt_mix_rays_counted_device(fake, 0, None, None, None, None, None, None, None)]
    assert oks == [rrt.OK] * len(oks), oks
    for name, a in outs.items():
        assert (a == PATTERN).all(), f"n == 0: {name} was written"
    assert (bound == 3).all()
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def _nine_calls(rrt, rt, torch):
    """{call: into(bound_t)} -- each of the nine _into methods with valid fake device tensors of a batch of 4 and the given bound."""
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))
    o, d, b1, w4, w1, d4, e4, scratch = f8(12), f8(12), u1(4), i4(4), i4(1), f8(4), f8(4), u1(64)      # (made once: both calls of a pair see the same tensors)
    rec = dict(albedo=i4(4), point=f8(12), normal=f8(12), material=i4(4))
    table = np.array([[0.0, 0.0, 1.0]])
    return {
        "intersect_rays": lambda b: rt.intersect_rays_into(o, d, {"hit": b1, "t": d4}, stream=5, bound_t=b),
        "get_ray_colours": lambda b: rt.get_ray_colours_into(o, d, w4, stream=5, bound_t=b),
        "occluded_rays": lambda b: rt.occluded_into(o, d, b1, stream=5, bound_t=b),
        "surface_rays": lambda b: rt.surface_rays_into(o, d, {"material": w4}, stream=5, bound_t=b),
        "shade_rays": lambda b: rt.shade_rays_into({"colour": w4}, d, rec, depth=2, stream=5, bound_t=b),
        "ambient_rays": lambda b: rt.ambient_rays_into({"open": w4}, rec, table, 3.0, stream=5, bound_t=b),
        "compact_rays": lambda b: rt.compact_rays_into({"point": o}, rec, "hit", w4, w1, scratch, stream=5, bound_t=b),
        "scatter_rays": lambda b: rt.scatter_rays_into(w4, d4, e4, stream=5, bound_t=b),
        "mix_rays": lambda b: rt.mix_rays_into(w4, o, stream=5, bound_t=b),
    }


def test_the_binding_refuses_a_bad_bound_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    calls = _nine_calls(rrt, rt, torch)
    assert tuple(calls) == COUNTED
    for name, into in calls.items():
        with pytest.raises(AssertionError, match="bound: not a device tensor"):                 # a tensor on the host
            into(np.zeros(1, np.uint32))
        with pytest.raises(AssertionError, match="bound: not a device tensor"):
            into(torch.zeros(1, dtype=torch.int32))
        for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.float64),   # a wrong dtype
                    torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)[::2]):   # a wrong length, not contiguous
            with pytest.raises(AssertionError, match="bound: want 1 contiguous elements of 4 bytes"):
                into(fake_device(bad))


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    """With a bound: the counted symbol, the bound's pointer in position 2, and around it the arguments of the uncounted call.  Without one: the old symbol with
    the old arguments."""
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)

    def plain(v):                                                            # an argument as something comparable: pointers by value, structs by their bytes
        if isinstance(v, C.c_void_p):
            return ("ptr", v.value)
        if hasattr(v, "_obj"):
            return ("struct", bytes(v._obj))
        return v
    for name, into in _nine_calls(rrt, rt, torch).items():
        bound = fake_device(torch.zeros(1, dtype=torch.int32))
        rec.calls.clear()
        into(None)
        into(bound)
        (n0, a0), (n1, a1) = rec.calls
        assert n0 == f"rrt_{name}_device" and n1 == f"rrt_{name}_counted_device", (n0, n1)
        assert len(a0) == len(rrt.SYMBOLS[n0][1]) and len(a1) == len(rrt.SYMBOLS[n1][1]) == len(a0) + 1
        assert isinstance(a1[2], C.c_void_p) and a1[2].value == bound.data_ptr(), name
        assert a1[0] is None and a1[1] == 4 and plain(a1[-1]) == ("ptr", 5)
        rest1, rest0 = list(a1[:2] + a1[3:]), list(a0)                       # around the bound: the arguments of the uncounted call
        if name == "ambient_rays":                                          # (the sample table is a host array made per call: compare what the struct holds)
            t1, t0 = rest1.pop(4)._obj, rest0.pop(4)._obj
            assert (t1.n, t1.max_t, t1.dirs[2]) == (t0.n, t0.max_t, t0.dirs[2]) == (1, 3.0, 1.0)
        assert [plain(v) for v in rest1] == [plain(v) for v in rest0], name
    # the compaction keeps its output count where it was, two places behind the bound's neighbours: n, BOUND, select, flag, src, dst, index, COUNT
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))
    rec.calls.clear()
    src, out, index, count, scratch, bound = dict(material=i4(4), point=f8(12)), dict(point=f8(12)), i4(4), i4(1), u1(48), i4(1)
    rt.compact_rays_into(out, src, "mirror", index, count, scratch, stream=0x51, bound_t=bound)
    rt.compact_rays_into(out, src, "mirror", index, count, scratch, stream=0x51)
    (n1, a1), (n0, a0) = rec.calls
    assert (n1, n0) == ("rrt_compact_rays_counted_device", "rrt_compact_rays_device") and len(a1) == 12 and len(a0) == 11
    assert a1[1] == 4 and a1[2].value == bound.data_ptr() and a1[3] == 1 and a1[4] is None
    assert a1[5]._obj.rec.point == src["point"].data_ptr() and a1[6]._obj.rec.point == out["point"].data_ptr()
    assert (a1[7].value, a1[8].value, a1[9].value, a1[10], a1[11].value) == (index.data_ptr(), count.data_ptr(), scratch.data_ptr(), 48, 0x51)
    assert [plain(v) for v in a1[:2] + a1[3:]] == [plain(v) for v in a0]
    # the scatter and the mix, argument by argument
    rec.calls.clear()
    a, b, colour, local = f8(12), f8(12), i4(4), f8(12)
    rt.scatter_rays_into(index, a, b, stream=9, bound_t=bound)
    rt.mix_rays_into(colour, local, stream=3, bound_t=bound)
    (n1, a1), (n2, a2) = rec.calls
    assert n1 == "rrt_scatter_rays_counted_device" and (a1[1], a1[2].value, a1[3].value, a1[4], a1[5].value, a1[6].value, a1[7].value) == \
        (4, bound.data_ptr(), index.data_ptr(), 24, a.data_ptr(), b.data_ptr(), 9)
    assert n2 == "rrt_mix_rays_counted_device" and (a2[1], a2[2].value, a2[3], a2[4].value, a2[5], a2[6], a2[7].value, a2[8].value) == \
        (4, bound.data_ptr(), None, local.data_ptr(), None, None, colour.data_ptr(), 3)
