"""The paths every entry point of frames.cpp, regions.cpp, ray_queries.cpp and ray_batches.cpp shares (launches.hpp) -- the timed launch and its record in rrt_stats, the device buffers a raytracer keeps between calls, the
way back into page-locked or pageable host memory, and the measurement of the variants on a rank's share -- on the GPU, where nothing else pins them.

Scene: assets/model.obj under the default lights.  The traced pixels of a W x H frame are the columns [0, 2*(W/2)) of the rows [H - 2*(H/2) + 1, H)
(engine.rs:146-158, 196-211): four primary rays each.  All comparisons of frames and planes are bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T
from bitwise import assert_same_arrays, bits
from conftest import ASSETS
from gpu_checks import traced_rows
from surface_checks import traced_pixels_in

pytestmark = pytest.mark.gpu

W, H = 24, 17            # the odd height: a partial row of tiles, and rows 0 and 1 are never traced
W2, H2 = 40, 33          # more than one row and column of tiles, and larger than W x H: a kept buffer has to grow
REGION = (3, 2, 9, 7)
N_RAYS = 100
GEOMETRY = ("hit", "t", "u", "v", "tri")


def random_rays(n, seed):
    """Rays in all directions from points around the model (as tools/random_rays_probe.py draws them)."""
    rng = np.random.default_rng(seed)
    return rng.uniform([-5, 0, -8], [5, 6, 5], (n, 3)), rng.normal(size=(n, 3))


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def model(rrt):
    return rrt.parse_obj_file(os.path.join(ASSETS, "model.obj"))


def device_planes(torch, rrt, w, h, names=None):
    kinds = dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, tri=torch.int32, albedo=torch.int32)
    return {n: torch.empty((h, w, 4), dtype=kinds[n], device="cuda") for n in (names or rrt.PLANES)}


def planes_to_host(torch, rrt, tensors):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(rrt.SURFACE_DTYPES.get(n) or rrt.PLANE_DTYPES[n]) for n, t in tensors.items()}


def device_surface_planes(torch, rrt, w, h, visibility=()):
    """The four surface planes, and the visibility planes named, as surface_into takes them."""
    out = {n: torch.empty((h, w, 4, 3) if rrt.SURFACE_WIDTHS[n] == 3 else (h, w, 4), dtype=torch.float64 if rrt.SURFACE_WIDTHS[n] == 3 else torch.int32, device="cuda")
           for n in rrt.SURFACE_PLANES}
    out.update(device_planes(torch, rrt, w, h, visibility))
    return out


def device_ambient_outputs(torch, w, h):
    return dict(occluded=torch.empty((h, w, 4), dtype=torch.int32, device="cuda"), grey=torch.empty((h, w), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------ 1
def test_every_entry_point_records_its_launch(rrt, torch, model):
    """last_stats() after each entry point: the size (or (n, 1) for n rays), four primary rays per traced pixel (0 for a rank's share, n for n rays), the
    forced variant, and a kernel time."""
    rt = rrt.RayTracer(model, rrt.default_lights(), box_filter="lane")
    frame_rays = 4 * traced_pixels_in((0, 0, W, H), W, H)
    assert frame_rays == 4 * 24 * 15
    fb = torch.empty((H, W), dtype=torch.int32, device="cuda")
    tiles = torch.empty((2, rrt.tiles_per_rank(W, H, 2) * 64), dtype=torch.int32, device="cuda")
    o, d = random_rays(N_RAYS, 11)
    to, td = torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda")
    five = {n: torch.empty(N_RAYS, dtype=dt, device="cuda") for n, dt in
            dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, tri=torch.int32).items()}
    occ = torch.empty(N_RAYS, dtype=torch.uint8, device="cuda")
    col = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
    px, py = 12, 9
    assert traced_pixels_in((px, py, 1, 1), W, H) == 1 and traced_pixels_in((0, 0, 1, 1), W, H) == 0
    region_rays = 4 * traced_pixels_in(REGION, W, H)
    rw, rh = REGION[2:]
    vis_t, vis_rt = device_planes(torch, rrt, W, H), device_planes(torch, rrt, rw, rh)
    surf_t, amb_t = device_surface_planes(torch, rrt, W, H, ("albedo",)), device_ambient_outputs(torch, W, H)
    kept = rt.surface(W, H, visibility=("albedo",))                  # the planes the host forms of shade and ambient read
    kept_r = rt.surface(W, H, region=REGION, visibility=("albedo",))
    table = [
        ("render", lambda: rt.render(W, H), (W, H), frame_rays),
        ("render_into", lambda: rt.render_into(fb, W, H), (W, H), frame_rays),
        ("render_progressive", lambda: rt.render_progressive(W, H, chunk_rows=5), (W, H), frame_rays),
        ("render_tiles_into, rank 0 of 2", lambda: rt.render_tiles_into(tiles[0], W, H, 0, 2), (W, H), 0),
        ("render_tiles_into, rank 1 of 2", lambda: rt.render_tiles_into(tiles[1], W, H, 1, 2), (W, H), 0),
        ("visibility", lambda: rt.visibility(W, H), (W, H), frame_rays),
        ("visibility of a region", lambda: rt.visibility(W, H, region=REGION), (W, H), 4 * traced_pixels_in(REGION, W, H)),
        ("pick of a traced pixel", lambda: rt.pick(W, H, px, py), (W, H), 4),
        ("pick of pixel (0, 0)", lambda: rt.pick(W, H, 0, 0), (W, H), 0),
        ("visibility_into", lambda: rt.visibility_into(vis_t, W, H), (W, H), frame_rays),
        ("visibility_into of a region", lambda: rt.visibility_into(vis_rt, W, H, region=REGION), (W, H), region_rays),
        ("surface", lambda: rt.surface(W, H), (W, H), frame_rays),
        ("surface of a region", lambda: rt.surface(W, H, region=REGION), (W, H), region_rays),
        ("surface_into", lambda: rt.surface_into(surf_t, W, H), (W, H), frame_rays),
        ("shade", lambda: rt.shade(W, H, kept), (W, H), frame_rays),
        ("shade of a region", lambda: rt.shade(W, H, kept_r, region=REGION), (W, H), region_rays),
        ("shade_into", lambda: rt.shade_into(fb, surf_t, W, H), (W, H), frame_rays),      # (surf_t: filled by the surface_into row)
        ("ambient", lambda: rt.ambient(W, H, kept, T8, T8_MAX_T), (W, H), frame_rays),
        ("ambient of a region", lambda: rt.ambient(W, H, kept_r, T8, T8_MAX_T, region=REGION), (W, H), region_rays),
        ("ambient_into", lambda: rt.ambient_into(amb_t, surf_t, T8, T8_MAX_T, W, H), (W, H), frame_rays),
        ("get_ray_colours", lambda: rt.get_ray_colours(o, d), (N_RAYS, 1), N_RAYS),
        ("intersect_rays", lambda: rt.intersect_rays(o, d), (N_RAYS, 1), N_RAYS),
        ("occluded", lambda: rt.occluded(o, d), (N_RAYS, 1), N_RAYS),
        ("get_ray_colours_into", lambda: rt.get_ray_colours_into(to, td, col), (N_RAYS, 1), N_RAYS),
        ("intersect_rays_into", lambda: rt.intersect_rays_into(to, td, five), (N_RAYS, 1), N_RAYS),
        ("occluded_into", lambda: rt.occluded_into(to, td, occ), (N_RAYS, 1), N_RAYS),
    ]
    assert 0 < region_rays < frame_rays
    for what, call, size, rays in table:
        call()
        torch.cuda.synchronize()
        s = rt.last_stats()
        print(f"{what}: {s['width']} x {s['height']}, {s['rays_primary']} primary rays, variant {s['filter_variant']}, {s['kernel_ms']:.4f} ms")
        assert (s["width"], s["height"]) == size, what
        assert s["rays_primary"] == rays, (what, s["rays_primary"], rays)
        assert s["filter_variant"] == 0, what
        assert s["kernel_ms"] > 0, what


# ------------------------------------------------------------------ 2
@pytest.fixture(scope="module")
def fresh_frames(rrt, model):
    """(w, h) -> the frame of a raytracer that has rendered nothing else; computed once per size, never modified."""
    frames = {}
    for w, h in ((W, H), (W2, H2)):
        frames[(w, h)] = rrt.RayTracer(model, rrt.default_lights()).render(w, h)
        frames[(w, h)].setflags(write=False)
        assert (frames[(w, h)][traced_rows(h)] != 0).any(), "an empty frame proves nothing"
    return frames


def test_the_kept_framebuffer_grows_and_is_reused(rrt, model, fresh_frames):
    rt = rrt.RayTracer(model, rrt.default_lights())
    for w, h in ((W, H), (W2, H2), (W, H)):
        assert np.array_equal(rt.render(w, h), fresh_frames[(w, h)]), (w, h)


def test_the_kept_planes_grow_and_are_reused(rrt, torch, model):
    """ONE raytracer (`host`) runs the host forms of all five users of the kept allocation in turn, so that it grows, is used in part and changes its layout
    between calls; every result against the device form of the same call on another raytracer (`rt`), which never touches a kept allocation."""
    rt = rrt.RayTracer(model, rrt.default_lights())
    tensors = device_planes(torch, rrt, W2, H2)
    rt.visibility_into(tensors, W2, H2)
    full = planes_to_host(torch, rrt, tensors)
    assert full["hit"].any(), "an empty frame proves nothing"
    x0, y0, w, h = REGION
    crop = lambda planes: {n: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for n, a in planes.items()}
    host = rrt.RayTracer(model, rrt.default_lights())
    assert_same_arrays(host.visibility(W2, H2, region=REGION), crop(full), what="a small region first")
    assert_same_arrays(host.visibility(W2, H2), full, what="then the whole frame")
    # surface of the whole frame, all ten planes: the largest layout
    surf_t = device_surface_planes(torch, rrt, W2, H2, rrt.PLANES)
    rt.surface_into(surf_t, W2, H2)
    surf = planes_to_host(torch, rrt, surf_t)
    assert_same_arrays({n: surf[n] for n in rrt.PLANES}, full, what="the visibility planes of the surface launch")
    assert (surf["lights"] != 0).any() and (surf["material"] != 0xFFFFFFFF).any(), "an empty frame proves nothing"
    assert_same_arrays(host.surface(W2, H2, visibility=rrt.PLANES), surf, what="all ten planes of the whole frame")
    ys, xs = np.nonzero(full["hit"][:, :, 0])
    px, py = int(xs[0]), int(ys[0])
    got = host.pick(W2, H2, px, py)
    assert got["hit"] and got["tri"] == full["tri"][py, px, 0] and got["albedo"] == full["albedo"][py, px, 0], got
    assert all(bits(np.float64(got[n])) == bits(full[n][py, px, 0]) for n in "tuv"), got
    # shade of the region from those planes: five inputs up, a framebuffer down
    kept_r = crop(surf)
    kept_rt = {n: torch.tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device="cuda") for n, a in kept_r.items()}
    fb_t = torch.empty((h, w), dtype=torch.int32, device="cuda")
    rt.shade_into(fb_t, kept_rt, W2, H2, region=REGION)
    torch.cuda.synchronize()
    fb = fb_t.cpu().numpy().view(np.uint32)
    assert (fb != 0).any() and (fb != 0x00FFFFFF).any(), "an empty region proves nothing"
    assert_same_arrays(dict(fb=host.shade(W2, H2, kept_r, region=REGION)), dict(fb=fb), what="shade of the region after the pick")
    # ambient occlusion of the whole frame, both outputs: three inputs up, two outputs of different sizes down
    amb_t = device_ambient_outputs(torch, W2, H2)
    rt.ambient_into(amb_t, surf_t, T8, T8_MAX_T, W2, H2)
    torch.cuda.synchronize()
    amb = {n: t.cpu().numpy().view(np.uint32) for n, t in amb_t.items()}
    assert (amb["occluded"] != 0).any() and (amb["grey"] != 0).any(), "an empty frame proves nothing"
    assert_same_arrays(host.ambient(W2, H2, surf, T8, T8_MAX_T), amb, what="ambient occlusion of the whole frame")
    assert_same_arrays(host.visibility(W2, H2, region=REGION, planes=("t", "tri")),
                       {n: full[n][y0:y0 + h, x0:x0 + w] for n in ("t", "tri")}, what="a small region after the rest")


def test_tune_rays_below_and_above_the_sample(rrt, torch, model):
    """20 000 rays, then 70 000 (more than the 65 536 the measurement traces): the variant it returns is the one the device forms then run, and their
    answers are the host form's."""
    rt = rrt.RayTracer(model, rrt.default_lights())
    kinds = dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, tri=torch.int32)
    for n in (20000, 70000):
        o, d = random_rays(n, n)
        to, td = torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda")
        variant = rt.tune_rays(to, td)
        assert variant in (0, 1, 2), variant
        occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        rt.occluded_into(to, td, occ)
        torch.cuda.synchronize()
        assert rt.last_stats()["filter_variant"] == variant, n
        five = {k: torch.empty(n, dtype=dt, device="cuda") for k, dt in kinds.items()}
        rt.intersect_rays_into(to, td, five)
        torch.cuda.synchronize()
        hit, t, u, v, tri = rt.intersect_rays(o, d)
        want = dict(hit=hit.astype(np.uint8), t=t, u=u, v=v, tri=tri)
        assert want["hit"].any(), "rays that all miss prove nothing"
        assert_same_arrays({k: x.cpu().numpy().view(want[k].dtype) for k, x in five.items()}, want, what=f"{n} rays")
        assert np.array_equal(occ.cpu().numpy(), want["hit"]), n


# ------------------------------------------------------------------ 3
def test_page_locked_and_pageable_planes_in_one_call(rrt, model):
    """rrt_render_visibility with the t and tri planes page-locked (one asynchronous copy each) and the other four pageable (the staging ring)."""
    rt = rrt.RayTracer(model, rrt.default_lights())
    want = rt.visibility(W2, H2)
    assert want["hit"].any(), "an empty frame proves nothing"
    L = rrt.lib()
    out = {n: np.zeros((H2, W2, 4), rrt.PLANE_DTYPES[n]) for n in rrt.PLANES}
    locked = []
    try:
        for n in ("t", "tri"):
            assert L.rrt_host_buffer_register(C.c_void_p(out[n].ctypes.data), out[n].nbytes) == rrt.OK, n
            locked.append(n)
        cv = rrt.CVisibility(**{n: a.ctypes.data for n, a in out.items()})
        assert L.rrt_render_visibility(rt._h, W2, H2, None, C.byref(cv)) == rrt.OK, L.rrt_last_error_detail()
    finally:
        for n in locked:
            assert L.rrt_host_buffer_unregister(C.c_void_p(out[n].ctypes.data)) == rrt.OK, n
    assert_same_arrays(out, want, what="t and tri page-locked")


# ------------------------------------------------------------------ 4
def test_a_ranks_share_through_the_measurement(rrt, torch, model, fresh_frames):
    """world = 2, one raytracer per rank, no forced variant, three rounds: the first launch of a rank runs the rule's variant, the second is the one on
    which the variants are timed (three streams at once: tune_variant), the third runs what that kept."""
    world = 2
    rts = [rrt.RayTracer(model, rrt.default_lights()) for _ in range(world)]
    gathered = torch.zeros((world, rrt.tiles_per_rank(W2, H2, world) * 64), dtype=torch.int32, device="cuda")
    fb = torch.empty((H2, W2), dtype=torch.int32, device="cuda")
    variants = []
    for round_ in range(3):
        gathered.zero_()
        for r, rt in enumerate(rts):
            rt.render_tiles_into(gathered[r], W2, H2, r, world)
        rts[0].detile_into(gathered, fb, W2, H2, world)
        torch.cuda.synchronize()
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), fresh_frames[(W2, H2)]), round_
        variants.append([rt.last_stats()["filter_variant"] for rt in rts])
        assert all(v in (0, 1, 2) for v in variants[-1]), variants
    print(f"variants per round and rank: {variants}")
    assert variants[1] == variants[2], variants
