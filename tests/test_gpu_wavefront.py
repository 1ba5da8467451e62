"""The two ends of the per-ray pipeline and the frame by ray generations (include/rrt.h: rrt_frame_rays, rrt_mix_rays, rrt_mix_pixels, rrt_render_wavefront and
their _device forms) on the GPU.

The statements under test: the generated batch IS the primary rays a frame traces, in both entry orders -- against the numpy restatement the other tests use
(tests/wavefront_checks.py) and against the library's own frame kernels (rrt_surface_rays of the batch equals rrt_render_surface's planes); one level of the unwind and
the pixels are the restated arithmetic; and the frame traced as compacted ray generations IS rrt_render's frame.  Every comparison is bit for bit, f64 through its
integer bits.
"""
import numpy as np
import pytest

from bitwise import assert_same_bits, bits, same
from gpu_checks import ALL_MODES, chain_rrt_lights, chain_scene
from ray_surface_checks import WHITE
from scenes import MOVED_EYE, TARGET, pose, room_without_oracle as room, teapot_arrays  # noqa: F401  (fixtures: room, teapot_arrays)
from shade_checks import MIRROR_ROOM_LIGHTS, soup_scene
from surface_checks import traced_pixels_in
from wavefront_checks import (ARRAYS, DEAD_BOUND, FRAMES, ORDERS, REGIONS, ROWS, SENTINEL, TILES, WIDTHS, alive_entries, assert_wavefront_is_render, expected_pixels,
                              expected_rays, host, mix_case, mix_level, ray_count, region_of)

pytestmark = pytest.mark.gpu

RW, RH = 32, 24                                                  # the mirror room's and the soup's frame
RECORDS = ("hit", "t", "u", "v", "tri", "albedo", "point", "normal", "material", "lights")   # what rrt_render_surface gives with its visibility planes


def device(torch, a):
    """A host array as a flat device tensor of the same bits (uint32 travels as int32)"""
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device="cuda").reshape(-1)


# ------------------------------------------------------------------ 1: the generator
@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_the_frame_rays_are_the_restated_ones(rrt, teapot, w, h, k):
    """Both orders, the whole frame and two regions cut off the tile boundaries: every element of every requested array is written with the restatement's bits, dead
    entries hold exactly the dead values, an array that is not passed stays as it was, the host form gives the device form's bits, and twice the same."""
    torch = pytest.importorskip("torch")
    cam = pose(rrt, k)
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.set_camera(**cam)
    rt.render(w, h)
    stats = rt.last_stats()
    stream = torch.cuda.Stream()
    for order in ORDERS:
        for region in REGIONS[(w, h)]:
            what = f"{w}x{h}, pose {k}, order {order}, region {region}"
            n = rrt.frame_ray_count(w, h, region, order)
            assert n == ray_count(w, h, region, order) > 0, what
            want = expected_rays(cam, w, h, region, order)
            alive = alive_entries(w, h, region, order)
            x0, y0, rw, rh = region_of(w, h, region)
            assert int(alive.sum()) == 4 * traced_pixels_in((x0, y0, rw, rh), w, h), what
            assert order == ROWS or region is None or not alive.all(), f"{what}: no tile of the region reaches over its edge"
            out = {name: torch.full((WIDTHS[name] * n,), SENTINEL, dtype=torch.float64, device="cuda") for name in ARRAYS}
            with torch.cuda.stream(stream):
                rt.frame_rays_into(out, w, h, region=region, order=order, stream=stream.cuda_stream)
            stream.synchronize()
            got = {name: host(out[name], np.float64, want[name].shape) for name in ARRAYS}
            for name in ARRAYS:
                assert_same_bits(got[name], want[name], f"{what}: {name}")
            dead = ~alive
            assert (bits(got["max_t"])[dead] == DEAD_BOUND).all() and (bits(got["origins"])[dead] == 0).all() and (bits(got["dirs"])[dead] == 0).all(), what
            assert np.isposinf(got["max_t"][alive]).all() and same(got["origins"][alive], np.broadcast_to(np.asarray(cam["eye"], np.float64), (int(alive.sum()), 3)).copy())
            again = rt.frame_rays(w, h, region=region, order=order)
            for name in ARRAYS:
                assert_same_bits(again[name], got[name], f"{what}: host form vs device form, {name}")
            for name in ARRAYS:                                    # one array at a time, from an address that is only 8-byte aligned: the others are not touched
                buf = {m: torch.full((WIDTHS[m] * n + 1,), SENTINEL, dtype=torch.float64, device="cuda") for m in ARRAYS}
                rt.frame_rays_into({name: buf[name][1:]}, w, h, region=region, order=order)
                torch.cuda.synchronize()
                assert_same_bits(host(buf[name][1:], np.float64, want[name].shape), want[name], f"{what}: {name} alone, 8-byte aligned")
                assert float(buf[name][0]) == SENTINEL and all(bool((buf[m] == SENTINEL).all()) for m in ARRAYS if m != name), f"{what}: {name} alone wrote elsewhere"
    assert rt.last_stats() == stats, "rrt_frame_rays touched rrt_last_stats"


@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_the_frame_rays_are_the_rays_the_frame_kernels_trace(rrt, teapot, w, h, k):
    """rrt_surface_rays of the generated rows-order batch, max_t included, equals the flattened planes of rrt_render_surface with its visibility planes, pixels the
    reference never traces included, in every walk.  (albedo of such a pixel is 0 in a plane and the miss value 0x00FFFFFF in a ray record: rrt.h.)"""
    cam = pose(rrt, k)
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        rt.set_camera(**cam)
        planes = rt.surface(w, h, visibility=RECORDS[:6])
        rays = rt.frame_rays(w, h)
        got = rt.surface_rays(rays["origins"], rays["dirs"], rays["max_t"], planes=RECORDS)
        alive = alive_entries(w, h, None, ROWS)
        hit = planes["hit"].reshape(-1).astype(bool)
        if (w, h) in ((64, 48), (97, 61)):
            assert hit[alive].mean() >= 0.5, f"{w}x{h}, pose {k}: only {hit[alive].mean():.3f} of the traced rays hit by the planes' own hit"
        assert not hit[~alive].any()
        for name in RECORDS:
            flat = planes[name].reshape(got[name].shape)
            sel = alive if name == "albedo" else slice(None)
            assert_same_bits(got[name][sel], flat[sel], f"{w}x{h}, pose {k}, walk {mode}: {name} of surface_rays(frame_rays) vs the surface planes")
        assert (got["albedo"][~alive] == WHITE).all() and (planes["albedo"].reshape(-1)[~alive] == 0).all()


def test_the_frame_rays_beyond_4_GiB(rrt, teapot):
    """A frame whose `dirs` array is 4.4 GB: the elements behind byte 2^32 are written where they belong, in both orders.  The last four rows of the array are
    compared with the restatement and with the batch of those rows as a region."""
    torch = pytest.importorskip("torch")
    from gpu_checks import pose_dirs
    from wavefront_checks import entries
    w, h = 8192, 5600
    cam = pose(rrt, 1)
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.set_camera(**cam)
    n = rrt.frame_ray_count(w, h, None, ROWS)
    assert n == rrt.frame_ray_count(w, h, None, TILES) == 4 * w * h and 24 * n > 2 ** 32 + 2 ** 26
    rows = np.arange(h - 4, h)
    tail = pose_dirs(cam, w, h, rows, np.arange(w)).transpose(0, 2, 1, 3)          # [4][w][4][3]
    m = 16 * w
    dirs = torch.empty(3 * n, dtype=torch.float64, device="cuda")
    for order in ORDERS:
        dirs[3 * (n - m):] = SENTINEL
        rt.frame_rays_into({"dirs": dirs}, w, h, order=order)
        part = torch.full((3 * m,), SENTINEL, dtype=torch.float64, device="cuda")
        rt.frame_rays_into({"dirs": part}, w, h, region=(0, h - 4, w, 4), order=order)
        torch.cuda.synchronize()
        got = host(dirs[3 * (n - m):], np.float64, (m, 3))
        px, py, sub, inside = entries(w, h, (0, h - 4, w, 4), order)
        assert inside.all() and len(px) == m
        assert_same_bits(got, tail[py - (h - 4), px, sub], f"order {order}: the last four rows of a 4.4 GB array vs the restatement")
        assert_same_bits(host(part, np.float64, (m, 3)), got, f"order {order}: the last four rows as a region vs the tail of the whole frame")


# ------------------------------------------------------------------ 2: one level of the unwind


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129, 4097))
def test_one_level_of_the_unwind(rrt, teapot, n):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    n_mats = len(teapot.materials())
    rt.render(16, 12)
    stats = rt.last_stats()
    local, kr, reflected, material = mix_case(n, n_mats)
    assert n < 9 or ((material >= n_mats).any() and ((material < n_mats) & (kr > 0.0)).any() and ((material < n_mats) & ~(kr > 0.0)).any())
    stream = torch.cuda.Stream()
    for what, (k, r, m) in {"all arrays": (kr, reflected, material), "no material": (kr, reflected, None), "no kr": (None, reflected, material),
                            "no reflected": (kr, None, material), "local alone": (None, None, None)}.items():
        want = mix_level(local, k, r, m, n_mats)
        got = rt.mix_rays(local, kr=k, reflected=r, material=m)
        assert_same_bits(got, want, f"n = {n}, {what}: host form vs the restatement")
        out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(stream):
            t = [None if a is None else device(torch, a) for a in (k, r, m)]
            rt.mix_rays_into(out, device(torch, local), kr_t=t[0], reflected_t=t[1], material_t=t[2], stream=stream.cuda_stream)
        stream.synchronize()
        assert_same_bits(host(out, np.uint32, (n,)), got, f"n = {n}, {what}: device form vs host form")
    assert rt.last_stats() == stats, "rrt_mix_rays touched rrt_last_stats"


# ------------------------------------------------------------------ 3: the pixels
@pytest.mark.parametrize("w,h", FRAMES)
def test_the_pixels(rrt, teapot, w, h):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.render(w, h)
    stats = rt.last_stats()
    rng = np.random.default_rng(w * h)
    for order in ORDERS:
        for region in REGIONS[(w, h)]:
            what = f"{w}x{h}, order {order}, region {region}"
            n = rrt.frame_ray_count(w, h, region, order)
            colours = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
            want = expected_pixels(colours, w, h, region, order)
            got = rt.mix_pixels(colours, w, h, region=region, order=order)
            assert_same_bits(got, want, f"{what}: host form vs the restatement")
            for shift in (0, 1):                                   # colours at a 16-byte aligned address, and at one that is only 4-byte aligned
                fb = torch.full((want.size,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                c = torch.zeros(n + shift, dtype=torch.int32, device="cuda")
                c[shift:] = device(torch, colours)
                rt.mix_pixels_into(fb, c[shift:], w, h, region=region, order=order)
                torch.cuda.synchronize()
                assert_same_bits(host(fb, np.uint32, want.shape), want, f"{what}: device form, colours shifted by {shift}")
    assert rt.last_stats() == stats, "rrt_mix_pixels touched rrt_last_stats"


# ------------------------------------------------------------------ 4: the frame by generations is rrt_render's frame
def tracer(rrt, sd, lights, mode, depth=5, **kw):
    rt = rrt.RayTracer(sd, lights, box_filter=mode, max_reflection_depth=depth, **kw)
    rt.max_reflection_depth = depth
    return rt


@pytest.mark.parametrize("depth", (0, 1, 5))
def test_the_mirror_room_by_generations(rrt, room, depth):
    torch = pytest.importorskip("torch")
    A, lights, sd = room
    frames = [assert_wavefront_is_render(rrt, torch, tracer(rrt, sd, lights, mode, depth), RW, RH, (5, 3, 18, 14), f"mirror room, depth {depth}, walk {mode}", mode)
              for mode in ALL_MODES]
    assert all((f == frames[0]).all() for f in frames)
    if depth == 5:                                                 # the chain is not vacuous: test_the_pieces_compose counts the rays alive per level of this frame
        shallow = tracer(rrt, sd, lights, None, 1).render(RW, RH)
        assert int((frames[0] != shallow).sum()) >= 100, "depth 5 and depth 1 give the same mirror room"


@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h,region", [(64, 48, (6, 9, 21, 18)), (97, 61, (90, 1, 7, 58))])
def test_the_teapot_by_generations(rrt, teapot, w, h, region, k):
    torch = pytest.importorskip("torch")
    cam = pose(rrt, k)
    for mode in ALL_MODES:
        rt = tracer(rrt, teapot, rrt.default_lights(), mode)
        rt.set_camera(**cam)
        frame = assert_wavefront_is_render(rrt, torch, rt, w, h, region, f"teapot {w}x{h}, pose {k}, walk {mode}", mode)
        assert (frame != 0).sum() >= w * h // 2


def test_a_soup_with_group_records_by_generations(rrt, teapot_arrays):
    torch = pytest.importorskip("torch")
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode in ALL_MODES:
        rt = tracer(rrt, sd, rrt.default_lights(), mode)
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records"
        assert_wavefront_is_render(rrt, torch, rt, 64, 48, (3, 5, 13, 7), f"soup, walk {mode}", mode)


def test_the_chain_scene_by_generations(rrt):
    torch = pytest.importorskip("torch")
    A, names = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode in ALL_MODES:
        rt = tracer(rrt, sd, chain_rrt_lights(rrt), mode, origin=rrt.Vector3d(*eye))
        rt.set_camera(**cam)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        assert_wavefront_is_render(rrt, torch, rt, 64, 48, (30, 2, 31, 41), f"chain scene, walk {mode}", mode)


# ------------------------------------------------------------------ 5: the pieces compose without the driver
@pytest.mark.parametrize("order", ORDERS)
def test_the_pieces_compose(rrt, room, order):
    """On one stream: frame_rays_into -> per level surface_rays_into, shade_rays_into (local and kr), compact_rays_into (mirror) -> back up scatter_rays_into and
    mix_rays_into -> mix_pixels_into: the mirror room ends in render's frame, with at least 1000 rays alive at level 5."""
    torch = pytest.importorskip("torch")
    A, lights, sd = room
    rt = rrt.RayTracer(sd, lights)
    want = rt.render(RW, RH)
    depth_max = 5
    n = rrt.frame_ray_count(RW, RH, None, order)
    f8 = lambda k: torch.full((k * n,), SENTINEL, dtype=torch.float64, device="cuda")
    i4 = lambda k=n: torch.full((k,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        rays = dict(origins=f8(3), dirs=f8(3), max_t=f8(1))
        rt.frame_rays_into(rays, RW, RH, order=order, stream=s)
        scratch = torch.zeros(max(1, rt.compact_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
        levels = []
        for k in range(depth_max + 1):
            rec = dict(albedo=i4(), point=f8(3), normal=f8(3), material=i4(), lights=i4())
            if k < depth_max:
                rec.update(next_origin=f8(3), next_dir=f8(3))
            rt.surface_rays_into(rays["origins"], rays["dirs"], rec, max_t_t=rays["max_t"], stream=s)
            out = dict(local=f8(3), kr=f8(1))
            rt.shade_rays_into(out, rays["dirs"], rec, depth=k, stream=s)
            index, count = i4(), i4(1)
            if k < depth_max:
                nxt = dict(origins=f8(3), dirs=f8(3), max_t=f8(1))
                rt.compact_rays_into(nxt, dict(origins=rec["next_origin"], dirs=rec["next_dir"], material=rec["material"]), "mirror", index, count, scratch, stream=s)
                rays = nxt
            levels.append((rec["material"], out, index, count))
        colour = None
        for k in reversed(range(depth_max + 1)):
            material, out, index, count = levels[k]
            reflected = None
            if k < depth_max:
                reflected = i4()
                rt.scatter_rays_into(index, colour, reflected, stream=s)
            colour = i4()
            rt.mix_rays_into(colour, out["local"], kr_t=out["kr"], reflected_t=reflected, material_t=material, stream=s)
        fb = i4(RW * RH)
        rt.mix_pixels_into(fb, colour, RW, RH, order=order, stream=s)
    stream.synchronize()
    assert_same_bits(host(fb, np.uint32, (RH, RW)), want, f"order {order}: the pipeline from library calls vs render")
    alive = [4 * traced_pixels_in((0, 0, RW, RH), RW, RH)] + [int(c.cpu().numpy().view(np.uint32)[0]) for _, _, _, c in levels[:-1]]
    print(f"order {order}: rays alive per level {alive}")
    assert alive[0] == 2944 and alive[5] >= 1000 and all(a >= b for a, b in zip(alive, alive[1:])), alive


# ------------------------------------------------------------------ 6: scene changes are followed
def test_scene_changes_are_followed(rrt, room):
    A, lights, sd = room
    rt = rrt.RayTracer(sd, lights)
    seen = [rt.render(RW, RH)]

    def check(what):
        want = rt.render(RW, RH)
        for order in ORDERS:
            assert_same_bits(rt.render_wavefront(RW, RH, order=order), want, f"after {what}, order {order}: render_wavefront vs render")
            assert_same_bits(rt.render_wavefront(RW, RH, region=(5, 3, 18, 14), order=order), want[3:17, 5:23], f"after {what}, order {order}, a region")
        assert not any((want == f).all() for f in seen), f"{what} did not change the frame"
        seen.append(want)
    check_first = [assert_same_bits(rt.render_wavefront(RW, RH, order=o), seen[0], f"before any change, order {o}") for o in ORDERS]
    assert len(check_first) == 2
    rt.look_at((2.0, 3.0, -9.0), TARGET)
    check("set_camera")
    rt.set_lights([rrt.Light(k, i * 0.8, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS[:3]])
    check("set_lights")
    mats = [dict(m) for m in A["materials"]]
    mats[0]["kr"], mats[1]["kr"] = 0.25, 0.5                       # a kr edit: the walls reflect less, the block becomes a mirror
    rt.set_materials(mats)
    check("set_materials")
    pos = np.array(A["pos"], np.float64)
    pos[A["mat"] == 1] += np.array([0.75, 0.0, -0.5])             # the block moves
    rt.set_triangles(pos, A["uv"], A["nrm"], A["mat"])
    check("set_triangles")
