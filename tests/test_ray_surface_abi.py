"""The per-ray surface query of the C ABI (include/rrt.h: rrt_ray_surface, rrt_surface_rays, rrt_surface_rays_device) as far as no GPU is needed: the struct
layout on both sides, the exported symbols, the argument checks the library makes before any HIP call, the checks the Python mirror makes before it calls the
library, and -- on the CPU, with the oracle -- that tests/ray_surface_checks.py restates tests/surface_checks.py."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import CallRecorder, NoLibrary, assert_refused, bare_raytracer, compiled_layout, fake_device
from bitwise import assert_same_arrays
from gpu_checks import ORIGIN, oracle_for
from ray_surface_checks import DTYPES, NAMES, VECTORS, assert_miss_values, expected_ray_planes, kr_of, rows
from scenes import CREATION
from surface_checks import expected_planes, frame_dirs


def test_the_struct_is_96_bytes_on_both_sides(rrt, tmp_path):
    assert C.sizeof(rrt.CRaySurface) == 96
    assert tuple(n for n, _ in rrt.CRaySurface._fields_) == rrt.RAY_SURFACE_PLANES == NAMES
    assert [getattr(rrt.CRaySurface, n).offset for n in NAMES] == list(range(0, 96, 8))
    assert rrt.STRUCTS["rrt_ray_surface"] is rrt.CRaySurface
    assert compiled_layout(tmp_path, "rrt_ray_surface", ("point", "next_dir")) == (96, [48, 88])


def test_both_symbols_are_exported_and_bound(rrt):
    L = rrt.lib()
    for name in ("rrt_surface_rays", "rrt_surface_rays_device"):
        assert name in rrt.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes == rrt.SYMBOLS[name][1]
    assert callable(rrt.RayTracer.surface_rays) and callable(rrt.RayTracer.surface_rays_into)


def test_the_library_refuses_before_any_gpu_work(rrt):
    """A NULL raytracer in both forms, whatever else is passed; nothing is written."""
    L = rrt.lib()
    rays = (C.c_double * 6)(0, 0, 0, 0, 0, 1)
    buf = (C.c_double * 4)()
    p = C.addressof(rays)
    out = rrt.CRaySurface(t=C.addressof(buf))
    host = lambda *a: L.rrt_surface_rays(None, 1, C.cast(p, rrt._dp), C.cast(p + 24, rrt._dp), None, *a)
    assert_refused(rrt, L, (("rrt_surface_rays", lambda: host(C.byref(out))),
                            ("rrt_surface_rays, NULL struct", lambda: host(None)),
                            ("rrt_surface_rays_device", lambda: L.rrt_surface_rays_device(None, 1, p, p + 24, None, C.byref(out), None)),
                            ("rrt_surface_rays_device, n = 0", lambda: L.rrt_surface_rays_device(None, 0, None, None, None, C.byref(out), None))))
    assert list(buf) == [0.0] * 4


def test_the_binding_refuses_before_it_calls_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    monkeypatch.setattr(rrt, "lib", lambda: NoLibrary())
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    o, d = f8(12), f8(12)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.surface_rays_into(np.zeros((4, 3)), np.ones((4, 3)), {"t": np.zeros(4)}, stream=0)
    with pytest.raises(AssertionError, match="not a device tensor"):
        rt.surface_rays_into(o, d, {"t": np.zeros(4)}, stream=0)
    with pytest.raises(AssertionError, match="t: want 4 contiguous elements of 8 bytes"):                  # a wrong dtype
        rt.surface_rays_into(o, d, {"t": fake_device(torch.zeros(4, dtype=torch.float32))}, stream=0)
    with pytest.raises(AssertionError, match="hit: want 4 contiguous elements of 1 bytes"):
        rt.surface_rays_into(o, d, {"hit": fake_device(torch.zeros(4, dtype=torch.int32))}, stream=0)
    with pytest.raises(AssertionError, match="normal: want 12 contiguous elements of 8 bytes"):           # a wrong length: n where 3 n are wanted
        rt.surface_rays_into(o, d, {"normal": f8(4)}, stream=0)
    with pytest.raises(AssertionError, match="lights: want 4 contiguous elements of 4 bytes"):
        rt.surface_rays_into(o, d, {"lights": fake_device(torch.zeros(5, dtype=torch.int32))}, stream=0)
    with pytest.raises(AssertionError, match="max_t: want 4 contiguous elements"):
        rt.surface_rays_into(o, d, {"t": f8(4)}, max_t_t=f8(3), stream=0)
    with pytest.raises(AssertionError, match="not a multiple of 3"):
        rt.surface_rays_into(f8(11), f8(11), {"t": f8(4)}, stream=0)
    with pytest.raises(ValueError, match="unknown plane 'colour'"):
        rt.surface_rays_into(o, d, {"colour": f8(4)}, stream=0)
    with pytest.raises(ValueError, match="unknown plane 'grey'"):                                          # a plane of another struct is not one of this one
        rt.surface_rays(np.zeros((4, 3)), np.ones((4, 3)), planes=("hit", "grey"))
    with pytest.raises(AssertionError):
        rt.surface_rays(np.zeros((4, 3)), np.ones((5, 3)))


def test_what_the_binding_hands_to_the_library(rrt, monkeypatch):
    torch = pytest.importorskip("torch")
    rt = bare_raytracer(rrt)
    rec = CallRecorder()
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    f8 = lambda n: fake_device(torch.zeros(n, dtype=torch.float64))
    o, d, m = f8(12), f8(12), f8(4)
    out = dict(normal=f8(12), lights=fake_device(torch.zeros(4, dtype=torch.int32)), next_dir=f8(12))
    rt.surface_rays_into(o, d, out, max_t_t=m, stream=0x51)
    (name, args), = rec.calls
    assert name == "rrt_surface_rays_device" and args[1] == 4
    assert [a.value for a in args[2:5]] == [o.data_ptr(), d.data_ptr(), m.data_ptr()] and args[6].value == 0x51
    s = args[5]._obj
    assert isinstance(s, rrt.CRaySurface)
    assert {n: getattr(s, n) for n in NAMES} == {n: (out[n].data_ptr() if n in out else None) for n in NAMES}
    rec.calls.clear()
    got = rt.surface_rays(np.zeros((4, 3)), np.ones((4, 3)), max_t=2.0, planes=("hit", "point", "tri"))
    (name, args), = rec.calls
    assert name == "rrt_surface_rays" and args[1] == 4 and [args[4][i] for i in range(4)] == [2.0] * 4
    assert set(got) == {"hit", "point", "tri"} and got["point"].shape == (4, 3) and got["hit"].dtype == np.uint8 and got["tri"].dtype == np.uint32
    s = args[5]._obj
    assert {n: getattr(s, n) for n in NAMES} == {n: (got[n].ctypes.data if n in got else None) for n in NAMES}
    for n in NAMES:
        a = rt.surface_rays(np.zeros((2, 3)), np.ones((2, 3)), planes=(n,))[n]
        assert a.shape == ((2, 3) if n in VECTORS else (2,)) and a.dtype == DTYPES[n]


# ------------------------------------------------------------------ the restatement, on the CPU
W, H = 64, 48


def test_for_one_eye_the_restatement_is_surface_checks(rrt, ob, teapot):
    """expected_ray_planes with every ray at the eye returns what surface_checks.expected_planes returns, bit for bit, on the teapot 64 x 48 frame; what it adds
    has the stated miss values and shapes; and the oracle's counts of the frame and of its level 1 are those the tests' thresholds were set below."""
    pos, uv, nrm, mat = teapot.triangles()
    A = dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=teapot.materials(), textures=teapot.textures())
    lights = rrt.default_lights()
    osc = oracle_for(ob, A, lights)
    d = frame_dirs(CREATION, W, H)
    old = expected_planes(osc, A, lights, ORIGIN, d)
    new = expected_ray_planes(osc, A, lights, ORIGIN, d)
    assert set(new) == set(NAMES) | {"bumped"} and set(old) == set(new) - {"albedo", "next_origin", "next_dir"}
    assert_same_arrays(new, old, sorted(old), "one eye")
    per_ray = expected_ray_planes(osc, A, lights, np.broadcast_to(np.asarray(ORIGIN), d.shape), d, np.full(d.shape[:-1], np.inf))
    assert_same_arrays(per_ray, new, sorted(new), "the eye and +inf repeated per ray")
    hit = new["hit"].astype(bool)
    mirror = hit & (kr_of(A, new["material"]) > 0.0)
    masks = set(np.unique(new["lights"][hit]).tolist())
    print(f"{hit.size} rays, {int(hit.sum())} hit, {int(mirror.sum())} on the mirror, masks {sorted(masks)}")
    assert (hit.size, int(hit.sum()), int(mirror.sum())) == (12032, 7142, 2272) and {9, 11, 13, 15} <= masks
    flat = {n: new[n].reshape((-1, 3) if n in VECTORS else (-1,)) for n in NAMES}
    assert_miss_values(rows(flat, ~hit.reshape(-1)), slice(None), "misses of the frame")
    assert all(new[n].shape == d.shape for n in VECTORS) and (new["albedo"][hit] <= 0xFFFFFF).all()
    # the reflection rays are unit vectors that leave the surface on the side they came from, from a point one offset off it
    r, n = new["next_dir"][hit], new["normal"][hit]
    assert np.abs(np.sqrt((r * r).sum(-1)) - 1.0).max() < 1e-15
    assert np.allclose((r * n).sum(-1), -(d[hit] * n).sum(-1) / np.sqrt((d[hit] * d[hit]).sum(-1)), rtol=0, atol=1e-12)
    assert np.abs(np.sqrt(((new["next_origin"][hit] - new["point"][hit]) ** 2).sum(-1)) - 1e-4).max() < 1e-12
    # level 1: the reflection rays of the mirror samples
    lvl1 = expected_ray_planes(osc, A, lights, new["next_origin"][mirror], new["next_dir"][mirror])
    assert int(lvl1["hit"].sum()) == 206, int(lvl1["hit"].sum())
    # a bound at or below zero, or NaN, is a miss whatever the ray
    some = np.flatnonzero(hit.reshape(-1))[:64]
    for bound in (0.0, -1.0, np.nan):
        dead = expected_ray_planes(osc, A, lights, ORIGIN, d.reshape(-1, 3)[some], np.full(len(some), bound))
        assert_miss_values({n: dead[n] for n in NAMES}, slice(None), f"max_t {bound}")
