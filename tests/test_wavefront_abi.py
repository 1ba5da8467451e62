"""The two ends of the per-ray pipeline and the frame by ray generations of the C ABI (include/rrt.h: rrt_frame_ray_count, rrt_frame_rays, rrt_mix_rays,
rrt_mix_pixels, rrt_wavefront_work_bytes, rrt_render_wavefront and their _device forms) as far as no GPU is needed: the enum on both sides, the exported symbols,
the entry count against the numpy restatement (tests/wavefront_checks.py), the argument checks the library makes before any HIP call and before it looks at the
handle, the work size for bad arguments, and what the Python mirror checks and hands to the library."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import PATTERN, CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_values, fake_device
from wavefront_checks import ORDERS, ROWS, TILES, alive_entries, entries, expected_pixels, mix_level, ray_count, tile_rectangle


def test_the_enum_on_both_sides(rrt, tmp_path):
    assert (rrt.ORDER_ROWS, rrt.ORDER_TILES) == (ROWS, TILES) == (0, 1) and rrt.FRAME_RAY_ARRAYS == ("origins", "dirs", "max_t")
    assert compiled_values(tmp_path, ("RRT_ORDER_ROWS", "RRT_ORDER_TILES", "sizeof(rrt_region)")) == [0, 1, 16]
    assert C.sizeof(rrt.CRegion) == 16


def test_the_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    P, R, U, D, u32 = C.c_void_p, C.POINTER(rrt.CRegion), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_uint32
    want = {"rrt_frame_ray_count": (u32, [u32, u32, R, u32]),
            "rrt_frame_rays_device": (C.c_int, [P, u32, u32, R, u32, P, P, P, P]),
            "rrt_frame_rays": (C.c_int, [P, u32, u32, R, u32, D, D, D]),
            "rrt_mix_rays_device": (C.c_int, [P, u32, P, P, P, P, P, P]),
            "rrt_mix_rays": (C.c_int, [P, u32, U, D, D, U, U]),
            "rrt_mix_pixels_device": (C.c_int, [P, u32, u32, R, u32, P, P, P]),
            "rrt_mix_pixels": (C.c_int, [P, u32, u32, R, u32, U, U]),
            "rrt_wavefront_work_bytes": (C.c_size_t, [P, u32, u32, R, u32]),
            "rrt_render_wavefront_device": (C.c_int, [P, u32, u32, R, u32, P, P, C.c_size_t, P]),
            "rrt_render_wavefront": (C.c_int, [P, u32, u32, R, u32, U])}
    for name, sig in want.items():
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert rrt.SYMBOLS[name] == sig, name
        assert getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0]
    for method in ("frame_ray_count", "frame_rays", "frame_rays_into", "mix_rays", "mix_rays_into", "mix_pixels", "mix_pixels_into", "wavefront_work_bytes",
                   "render_wavefront", "render_wavefront_into"):
        assert callable(getattr(rrt.RayTracer, method)), method
    assert callable(rrt.frame_ray_count)


def grid_regions(w, h):
    """The whole frame, single pixels in the corners, and regions that start and end on and off multiples of 4 (clipped to the frame, made non-empty)"""
    out = [None, (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, w, 1), (0, 0, 1, h)]
    for x0, y0, rw, rh in ((3, 5, 13, 7), (4, 4, 8, 8), (1, 2, 3, 2), (7, 3, 1, 9), (5, 0, 40, 11), (0, 6, 6, 40), (90, 1, 7, 58), (2, 1, 2, 2)):
        x0, y0 = min(x0, w - 1), min(y0, h - 1)
        out.append((x0, y0, max(1, min(rw, w - x0)), max(1, min(rh, h - y0))))
    return out


def test_the_entry_count_against_the_restatement(rrt):
    cases = 0
    for w, h in ((1, 1), (2, 2), (3, 1), (1, 5), (4, 4), (5, 3), (8, 8), (9, 7), (16, 12), (31, 33), (64, 48), (97, 61)):
        for region in grid_regions(w, h):
            for order in ORDERS:
                n = rrt.frame_ray_count(w, h, region, order)
                want = ray_count(w, h, region, order)
                assert n == want > 0 and n % 4 == 0, f"{w}x{h}, region {region}, order {order}: {n} entries, the restatement says {want}"
                x0, y0, rw, rh = (0, 0, w, h) if region is None else region
                tx0, ty0, tw, th = tile_rectangle((x0, y0, rw, rh))
                assert n == (4 * rw * rh if order == ROWS else 64 * tw * th)
                assert order == ROWS or (n >= 4 * rw * rh and tx0 * 4 <= x0 and (tx0 + tw) * 4 >= x0 + rw and ty0 * 4 <= y0 and (ty0 + th) * 4 >= y0 + rh)
                # the restated order is a bijection between the entries inside the region and its sub-samples
                px, py, sub, inside = entries(w, h, region, order)
                key = ((py[inside] - y0) * rw + (px[inside] - x0)) * 4 + sub[inside]
                assert len(key) == 4 * rw * rh and len(np.unique(key)) == len(key), f"{w}x{h}, region {region}, order {order}: the entries do not cover the region once"
                assert order == TILES or (key == np.arange(n)).all()
                cases += 1
    assert cases == 12 * 13 * 2
    assert rrt.RayTracer.frame_ray_count(97, 61, (3, 5, 13, 7), TILES) == 64 * 4 * 2
    # a run of 64 entries in tiles order is one 4x4 tile; the traced entries of a frame are four per traced pixel
    px, py, sub, inside = entries(97, 61, (3, 5, 13, 7), TILES)
    assert (np.ptp((px // 4).reshape(-1, 64), 1) == 0).all() and (np.ptp((py // 4).reshape(-1, 64), 1) == 0).all()
    assert int(alive_entries(97, 61, None, ROWS).sum()) == 4 * 96 * 59 == int(alive_entries(97, 61, None, TILES).sum())
    # counts beyond a ray batch, and the largest that fit
    assert rrt.frame_ray_count(32768, 32768, None, ROWS) == 0 == rrt.frame_ray_count(32768, 32768, None, TILES)
    assert rrt.frame_ray_count(32768, 32767, None, ROWS) == 4 * 32768 * 32767 and rrt.frame_ray_count(32768, 32767, None, TILES) == 0   # (64 * 8192 * 8192 = 2^32)
    assert ray_count(32768, 32767, None, ROWS) == 4 * 32768 * 32767 and ray_count(32768, 32767, None, TILES) == 0 == ray_count(32768, 32768, None, ROWS)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """Every refusal of rrt.h in both forms, through a handle that is the address of 4 KB of zeros: a check that came after the handle's first use in a HIP call
    would crash or fail in another way, not refuse.  (The device forms' pointers are host addresses here.)  The error detail is set, the outputs keep their
    pattern, the count and the work size are 0."""
    L = rrt.lib()
    w, h = 16, 12
    n = 4 * w * h
    outs = {name: np.full(3 * n, PATTERN, np.uint32) for name in ("a", "b", "c", "fb", "work")}
    local, kr, mat, refl = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    at = lambda a: None if a is None else a.ctypes.data
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    up = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    ref = lambda r: None if r is None else C.byref(rrt.CRegion(*r))
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    A, B, Cc, FB, WORK = (outs[k] for k in ("a", "b", "c", "fb", "work"))
    work_bytes = WORK.nbytes

    frame_forms = {
        "rrt_frame_rays": lambda rt, fw, fh, r, o, x=A, y=B, z=Cc: L.rrt_frame_rays(rt, fw, fh, ref(r), o, dp(x), dp(y), dp(z)),
        "rrt_frame_rays_device": lambda rt, fw, fh, r, o, x=A, y=B, z=Cc: L.rrt_frame_rays_device(rt, fw, fh, ref(r), o, at(x), at(y), at(z), None),
        "rrt_mix_pixels": lambda rt, fw, fh, r, o, x=A, y=FB, z=None: L.rrt_mix_pixels(rt, fw, fh, ref(r), o, up(x), up(y)),
        "rrt_mix_pixels_device": lambda rt, fw, fh, r, o, x=A, y=FB, z=None: L.rrt_mix_pixels_device(rt, fw, fh, ref(r), o, at(x), at(y), None),
        "rrt_render_wavefront": lambda rt, fw, fh, r, o, x=FB, y=None, z=None: L.rrt_render_wavefront(rt, fw, fh, ref(r), o, up(x)),
        "rrt_render_wavefront_device": lambda rt, fw, fh, r, o, x=FB, y=WORK, z=work_bytes: L.rrt_render_wavefront_device(rt, fw, fh, ref(r), o, at(x), at(y), z, None),
    }
    bad_frames = [("a NULL raytracer", (None, w, h, None, 0)), ("width 0", (fake, 0, h, None, 0)), ("height 0", (fake, w, 0, None, 1)),
                  ("a frame of 2^31 pixels", (fake, 65536, 32768, None, 0)), ("a region with w == 0", (fake, w, h, (1, 1, 0, 2), 0)),
                  ("a region with h == 0", (fake, w, h, (1, 1, 2, 0), 1)), ("a region sticking out to the right", (fake, w, h, (10, 0, 7, 2), 0)),
                  ("a region sticking out below", (fake, w, h, (0, 11, 2, 2), 1)), ("a region beyond 2^32", (fake, w, h, (0xFFFFFFFF, 0, 2, 2), 0)),
                  ("order 2", (fake, w, h, None, 2)), ("order 0xFFFFFFFF", (fake, w, h, (3, 5, 4, 4), 0xFFFFFFFF))]
    calls = [(f"{form}, {what}", lambda call=call, args=args: call(*args)) for form, call in frame_forms.items() for what, args in bad_frames]
    calls += [("rrt_frame_rays, all three arrays NULL", lambda: frame_forms["rrt_frame_rays"](fake, w, h, None, 0, None, None, None)),
              ("rrt_frame_rays_device, all three arrays NULL", lambda: frame_forms["rrt_frame_rays_device"](fake, w, h, (3, 5, 4, 4), 1, None, None, None)),
              ("rrt_mix_pixels, NULL colours", lambda: frame_forms["rrt_mix_pixels"](fake, w, h, None, 0, None, FB)),
              ("rrt_mix_pixels, a NULL framebuffer", lambda: frame_forms["rrt_mix_pixels"](fake, w, h, None, 1, A, None)),
              ("rrt_mix_pixels_device, NULL colours", lambda: frame_forms["rrt_mix_pixels_device"](fake, w, h, None, 0, None, FB)),
              ("rrt_mix_pixels_device, a NULL framebuffer", lambda: frame_forms["rrt_mix_pixels_device"](fake, w, h, None, 1, A, None)),
              ("rrt_render_wavefront, a NULL framebuffer", lambda: frame_forms["rrt_render_wavefront"](fake, w, h, None, 0, None)),
              ("rrt_render_wavefront_device, a NULL framebuffer", lambda: frame_forms["rrt_render_wavefront_device"](fake, w, h, None, 0, None)),
              ("rrt_render_wavefront_device, NULL work memory", lambda: frame_forms["rrt_render_wavefront_device"](fake, w, h, None, 0, FB, None)),
              ("rrt_render_wavefront_device, work memory of 0 bytes", lambda: frame_forms["rrt_render_wavefront_device"](fake, w, h, None, 0, FB, WORK, 0)),
              ("rrt_render_wavefront_device, work memory one byte short",
               lambda: frame_forms["rrt_render_wavefront_device"](fake, 2, 2, None, 0, FB, WORK, L.rrt_wavefront_work_bytes(fake, 2, 2, None, 0) - 1)),
              ("rrt_mix_rays, a NULL raytracer", lambda: L.rrt_mix_rays(None, n, up(mat), dp(local), dp(kr), up(refl), up(A))),
              ("rrt_mix_rays, a NULL raytracer, n = 0", lambda: L.rrt_mix_rays(None, 0, up(mat), dp(local), dp(kr), up(refl), up(A))),
              ("rrt_mix_rays, NULL local", lambda: L.rrt_mix_rays(fake, n, up(mat), None, dp(kr), up(refl), up(A))),
              ("rrt_mix_rays, NULL colour", lambda: L.rrt_mix_rays(fake, n, up(mat), dp(local), dp(kr), up(refl), None)),
              ("rrt_mix_rays_device, a NULL raytracer", lambda: L.rrt_mix_rays_device(None, n, at(mat), at(local), at(kr), at(refl), at(A), None)),
              ("rrt_mix_rays_device, NULL local", lambda: L.rrt_mix_rays_device(fake, n, at(mat), None, at(kr), at(refl), at(A), None)),
              ("rrt_mix_rays_device, NULL colour", lambda: L.rrt_mix_rays_device(fake, n, None, at(local), None, None, None, None))]
    assert len(calls) == 6 * 11 + 18
    assert 0 < L.rrt_wavefront_work_bytes(fake, 2, 2, None, 0) <= work_bytes and WORK.ctypes.data % 8 == 0
    assert_refused(rrt, L, calls, outs)
    # the count and the work size of the same arguments
    for what, (rt, fw, fh, r, o) in bad_frames:
        assert L.rrt_wavefront_work_bytes(rt, fw, fh, ref(r), o) == 0, f"rrt_wavefront_work_bytes, {what}"
        if rt is not None:
            assert L.rrt_frame_ray_count(fw, fh, ref(r), o) == 0, f"rrt_frame_ray_count, {what}"
    # n == 0: RRT_OK with nothing enqueued (the handle is not a raytracer), whatever the arrays are
    assert L.rrt_mix_rays(fake, 0, None, None, None, None, None) == rrt.OK and L.rrt_mix_rays_device(fake, 0, None, None, None, None, None, None) == rrt.OK
    assert bytes(blank) == bytes(4096), "a refused call wrote through the handle"


def test_the_work_size(rrt):
    """Through a handle of zeros (max_reflection_depth 0: one level) the size is a function of the entry count alone: monotone, and inside the header's bound."""
    L = rrt.lib()
    blank = (C.c_char * 4096)()
    fake = C.addressof(blank)
    sizes = []
    for w, h in ((1, 1), (2, 2), (5, 3), (16, 12), (64, 48), (97, 61), (1920, 1080)):
        for order in ORDERS:
            n = rrt.frame_ray_count(w, h, None, order)
            b = L.rrt_wavefront_work_bytes(fake, w, h, None, order)
            assert 0 < b <= n * (229 + 40 * 1) + 16384 and b % 256 == 0 and b >= n * (228 + 40), f"{w}x{h}, order {order}: {b} bytes for {n} entries"
            sizes.append((n, b))
    sizes.sort()
    assert all(a[1] <= b[1] for a, b in zip(sizes, sizes[1:])), f"the work size decreases somewhere: {sizes}"
    inner = L.rrt_wavefront_work_bytes(fake, 97, 61, C.byref(rrt.CRegion(3, 5, 13, 7)), ROWS)
    outer = L.rrt_wavefront_work_bytes(fake, 97, 61, C.byref(rrt.CRegion(2, 4, 15, 9)), ROWS)
    assert 0 < inner <= outer <= L.rrt_wavefront_work_bytes(fake, 97, 61, None, ROWS)
    for order in ORDERS:                               # a region that grows never needs less, in either order
        prev = 0
        for k in range(1, 30):
            b = L.rrt_wavefront_work_bytes(fake, 97, 61, C.byref(rrt.CRegion(3, 5, k, k)), order)
            assert b >= prev > -1
            prev = b


def test_the_restatements_on_values_worked_out_by_hand():
    # 5 x 3: the reference traces row 2, columns 0..3; the region (3, 1, 2, 2) holds one traced pixel, (3, 2)
    assert alive_entries(5, 3, (3, 1, 2, 2), ROWS).tolist() == [False] * 8 + [True] * 4 + [False] * 4
    px, py, sub, inside = entries(5, 3, (3, 1, 2, 2), TILES)
    assert len(px) == 128 and int(inside.sum()) == 16 and px[:8].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and py[16:20].tolist() == [1] * 4 and px[64] == 4
    e = (0 * 16 + 2 * 4 + 3) * 4                            # tile 0, pixel (3, 2)
    alive = alive_entries(5, 3, (3, 1, 2, 2), TILES)
    assert np.flatnonzero(alive).tolist() == [e, e + 1, e + 2, e + 3]
    local = np.array([[300.0, -1.0, 10.5], [np.nan, np.inf, -np.inf], [100.0, 100.0, 100.0], [8.0, 8.0, 8.0]])
    kr = np.array([0.0, 0.0, 0.5, 0.25])
    got = mix_level(local, kr, np.array([0, 0, 0xAB0A141E, 0x00FFFFFF], np.uint32), np.array([0, 1, 0, 7], np.uint32), 2)
    assert [hex(int(c)) for c in got] == ["0xff000a", "0xff00", hex((55 << 16) | (60 << 8) | 65), "0xffffff"]
    assert mix_level(local, None, None, None, 2).tolist() == [0xFF000A, 0x00FF00, 0x646464, 0x080808]
    cols = np.arange(64, dtype=np.uint32) * 0x010203 + 0xFF000000
    fb = expected_pixels(cols, 4, 4, None, ROWS)
    assert fb.shape == (4, 4) and (fb[0] == 0).all() and int(fb[1, 0]) == ((16 + 17 + 18 + 19) // 4) * 0x010000 + ((32 + 34 + 36 + 38) // 4) * 0x0100 + (48 + 51 + 54 + 57) // 4
    assert (expected_pixels(cols, 4, 4, None, TILES) == fb).all()      # (one tile: the two orders coincide)


def test_the_binding_refuses_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    u1 = lambda n: fake_device(torch.zeros(n, dtype=torch.uint8))
    n = rrt.frame_ray_count(8, 6, None, ROWS)                      # (the one library call the _into forms make first: no handle, no GPU)
    assert n == 192
    for call in (lambda: rt.frame_rays_into({}, 8, 6, order=2), lambda: rt.mix_pixels_into(i4(48), i4(n), 8, 6, order="tiles"), lambda: rt.render_wavefront(8, 6, order=-1),
                 lambda: rt.wavefront_work_bytes(8, 6, order=7), lambda: rrt.frame_ray_count(8, 6, None, 3), lambda: rt.frame_rays(8, 6, order=None)):
        with pytest.raises(ValueError, match="unknown order"):
            call()
    count = rrt.lib().rrt_frame_ray_count

    class _CountOnly(NoLibrary):
        rrt_frame_ray_count = staticmethod(count)
    monkeypatch.setattr(rrt, "lib", lambda: _CountOnly())
    with pytest.raises(ValueError, match="unknown array 'rot'"):
        rt.frame_rays_into({"rot": f8(2 * n)}, 8, 6, stream=0)
    with pytest.raises(ValueError, match="unknown array 'point'"):
        rt.frame_rays(8, 6, arrays=("point",))
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.frame_rays_into({"dirs": np.zeros(3 * n)}, 8, 6, stream=0)
    with pytest.raises(AssertionError, match=f"dirs: want {3 * n} contiguous elements of 8 bytes"):
        rt.frame_rays_into({"dirs": f8(n)}, 8, 6, stream=0)
    with pytest.raises(AssertionError, match="max_t: want 256 contiguous elements of 8 bytes"):
        rt.frame_rays_into({"max_t": f8(n)}, 8, 6, region=(3, 1, 2, 4), order=TILES, stream=0)
    with pytest.raises(AssertionError, match="origins: want 96 contiguous elements of 8 bytes"):
        rt.frame_rays_into({"origins": i4(96)}, 8, 6, region=(3, 1, 2, 4), stream=0)
    with pytest.raises(AssertionError, match="colour: want 4 contiguous elements of 4 bytes"):
        rt.mix_rays_into(f8(4), f8(12), stream=0)
    with pytest.raises(AssertionError, match="kr: want 4 contiguous elements of 8 bytes"):
        rt.mix_rays_into(i4(4), f8(12), kr_t=i4(4), stream=0)
    with pytest.raises(AssertionError, match="reflected: want 4 contiguous elements of 4 bytes"):
        rt.mix_rays_into(i4(4), f8(12), reflected_t=i4(5), stream=0)
    with pytest.raises(AssertionError, match="material: not a device tensor"):
        rt.mix_rays_into(i4(4), f8(12), material_t=np.zeros(4, np.uint32), stream=0)
    with pytest.raises(AssertionError, match="the element count is not a multiple of 3"):
        rt.mix_rays_into(i4(4), f8(13), stream=0)
    with pytest.raises(AssertionError, match="kr has 3 elements for 4 entries"):
        rt.mix_rays(np.zeros((4, 3)), kr=np.zeros(3))
    with pytest.raises(AssertionError, match=f"colours: want {n} contiguous elements of 4 bytes"):
        rt.mix_pixels_into(i4(48), i4(n - 4), 8, 6, stream=0)
    with pytest.raises(AssertionError, match="fb: want 8 contiguous elements of 4 bytes"):
        rt.mix_pixels_into(i4(48), i4(256), 8, 6, region=(3, 1, 2, 4), order=TILES, stream=0)
    with pytest.raises(AssertionError, match="colours has 100 elements for 192 entries"):
        rt.mix_pixels(np.zeros(100, np.uint32), 8, 6)
    with pytest.raises(AssertionError, match="fb: want 48 contiguous elements of 4 bytes"):
        rt.render_wavefront_into(f8(48), u1(4096), 8, 6, stream=0)
    with pytest.raises(AssertionError, match="work: not a contiguous device tensor"):
        rt.render_wavefront_into(i4(48), np.zeros(4096, np.uint8), 8, 6, stream=0)


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    count = rrt.lib().rrt_frame_ray_count

    class _Rec(CallRecorder):
        rrt_frame_ray_count = staticmethod(count)
    rec = _Rec()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    i4 = lambda n: fake_device(torch.zeros(n, dtype=torch.int32))
    region_of = lambda arg: None if arg is None else tuple(getattr(arg._obj, k) for k in ("x0", "y0", "w", "h"))
    val = lambda p: None if p is None else p.value
    # frame rays, device form: a region in tiles order, two of the three arrays
    dirs, max_t = f8(3 * 256), f8(256)
    rt.frame_rays_into(dict(max_t=max_t, dirs=dirs), 8, 6, region=(3, 1, 2, 4), order=TILES, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_frame_rays_device" and len(args) == 9 and args[0] is None and args[1:3] == (8, 6) and region_of(args[3]) == (3, 1, 2, 4) and args[4] == 1
    assert (val(args[5]), val(args[6]), val(args[7]), val(args[8])) == (None, dirs.data_ptr(), max_t.data_ptr(), 0x51)
    # ... host form: the whole frame, every array, in the shapes of the contract
    rec.calls.clear()
    got = rt.frame_rays(8, 6)
    (name, args), = rec.calls
    assert name == "rrt_frame_rays" and len(args) == 8 and args[1:3] == (8, 6) and args[3] is None and args[4] == 0
    assert {k: (a.shape, a.dtype) for k, a in got.items()} == dict(origins=((192, 3), np.float64), dirs=((192, 3), np.float64), max_t=((192,), np.float64))
    assert [C.cast(a, C.c_void_p).value for a in args[5:8]] == [got[k].ctypes.data for k in ("origins", "dirs", "max_t")]
    rec.calls.clear()
    got = rt.frame_rays(8, 6, region=(0, 0, 3, 2), order=TILES, arrays=("max_t",))
    (name, args), = rec.calls
    assert set(got) == {"max_t"} and got["max_t"].shape == (64,) and args[5] is None and args[6] is None and C.cast(args[7], C.c_void_p).value == got["max_t"].ctypes.data
    # mix rays
    rec.calls.clear()
    colour, local, kr, refl, mat = i4(4), f8(12), f8(4), i4(4), i4(4)
    rt.mix_rays_into(colour, local, kr_t=kr, reflected_t=refl, material_t=mat, stream=7)
    rt.mix_rays_into(colour, local, stream=7)
    (name, a), (_, b) = rec.calls
    assert name == "rrt_mix_rays_device" and len(a) == 8 and a[1] == 4
    assert [val(x) for x in a[2:]] == [mat.data_ptr(), local.data_ptr(), kr.data_ptr(), refl.data_ptr(), colour.data_ptr(), 7]
    assert [val(x) for x in b[2:]] == [None, local.data_ptr(), None, None, colour.data_ptr(), 7]
    rec.calls.clear()
    out = rt.mix_rays(np.ones((5, 3)), kr=np.zeros(5), reflected=np.zeros(5, np.uint32))
    (name, args), = rec.calls
    assert name == "rrt_mix_rays" and args[1] == 5 and args[2] is None and all(args[3:7]) and out.shape == (5,) and out.dtype == np.uint32
    assert C.cast(args[6], C.c_void_p).value == out.ctypes.data
    # pixels
    rec.calls.clear()
    fb, cols = i4(8), i4(256)
    rt.mix_pixels_into(fb, cols, 8, 6, region=(3, 1, 2, 4), order=TILES, stream=9)
    out = rt.mix_pixels(np.zeros(192, np.uint32), 8, 6)
    (name, a), (name_h, b) = rec.calls
    assert name == "rrt_mix_pixels_device" and a[1:3] == (8, 6) and region_of(a[3]) == (3, 1, 2, 4) and a[4] == 1 and [val(x) for x in a[5:]] == [cols.data_ptr(), fb.data_ptr(), 9]
    assert name_h == "rrt_mix_pixels" and b[3] is None and b[4] == 0 and out.shape == (6, 8) and C.cast(b[6], C.c_void_p).value == out.ctypes.data
    # the frame by generations
    rec.calls.clear()
    work = fake_device(torch.zeros(512, dtype=torch.int64))
    rt.render_wavefront_into(fb, work, 8, 6, region=(3, 1, 2, 4), order=TILES, stream=11)
    out = rt.render_wavefront(8, 6, region=(1, 1, 4, 3))
    rt.wavefront_work_bytes(8, 6, region=(1, 1, 4, 3), order=TILES)
    (name, a), (name_h, b), (name_w, c) = rec.calls
    assert name == "rrt_render_wavefront_device" and len(a) == 9 and region_of(a[3]) == (3, 1, 2, 4) and a[4] == 1
    assert (val(a[5]), val(a[6]), a[7], val(a[8])) == (fb.data_ptr(), work.data_ptr(), 4096, 11)
    assert name_h == "rrt_render_wavefront" and region_of(b[3]) == (1, 1, 4, 3) and b[4] == 0 and out.shape == (3, 4) and C.cast(b[5], C.c_void_p).value == out.ctypes.data
    assert name_w == "rrt_wavefront_work_bytes" and c[0] is None and c[1:3] == (8, 6) and region_of(c[3]) == (1, 1, 4, 3) and c[4] == 1
