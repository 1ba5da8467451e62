"""Shading of arbitrary ray batches from kept surface records (include/rrt.h: rrt_shade_rays, rrt_shade_rays_device) on the GPU.

The statement under test: with the records rrt_surface_rays wrote for the rays (o, d), `colour` at depth 0 IS what rrt_get_ray_colours returns for (o, d) with the
lights and materials in force now, bit for bit -- with the kept mask of lit lights and, without it, with the shadow rays of the records' hits walked again; at depth
k it is the colour of a raytracer whose max_reflection_depth is k smaller; and `local` / `kr` are what a level of the reference's recursion mixes the level below
into, so that the recursion can be followed level by level from library calls alone.

Comparisons of the library with itself are bit for bit; comparisons with the oracle are within COLOUR_TOL (the project's +-1 for pow) and assert their conditions
BY THE ORACLE'S ANSWERS, so an empty batch cannot pass; the thresholds sit below counts made on the CPU with the oracle alone.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from bitwise import assert_same_bits, bits, same
from conftest import channels
from gpu_checks import (ALL_MODES, CHAIN_CAMERA, CHAIN_LIGHTS, COLOUR_TOL, FORCED_MODES, ORIGIN, POOL, assert_frame_close, chain_main_rays, chain_rrt_lights,
                        chain_scene, oracle_for)
from ray_surface_checks import VECTORS, WHITE, clamp_u8, expected_ray_planes, kr_of, local_colour, pack
from scenes import CREATION, MOVED_EYE, TARGET, pose, posed, rays_of, room, teapot_arrays, teapot_osc  # noqa: F401  (fixtures: room, teapot_arrays, teapot_osc)
from shade_checks import soup_scene
from shade_rays_checks import (INPUTS, OUT_DTYPES, OUT_SENTINEL, OUTPUTS, chain_levels, mixed, oracle_colours, reflecting, unwind, without_mask)
from surface_checks import frame_dirs

pytestmark = pytest.mark.gpu

W, H = 64, 48
RW, RH = 32, 24                                                  # the mirror room's and the soup's frame
M = 5                                                            # the default max_reflection_depth


def assert_shade_is_get_ray_colours(rt, O, D, what, planes=None):
    """shade_rays at depth 0 of the records rt's surface_rays call returns (or of `planes`), with the mask and without it, is rt's get_ray_colours bit for bit.
    Returns (the colours, the records)."""
    planes = rt.surface_rays(O, D) if planes is None else planes
    want = rt.get_ray_colours(O, D)
    assert_same_bits(rt.shade_rays(D, planes)["colour"], want, f"{what}: shade_rays with the mask vs get_ray_colours", np.uint32)
    stats = rt.last_stats()
    assert (stats["width"], stats["height"], stats["rays_primary"]) == (len(D), 1, len(D)) and stats["kernel_ms"] > 0, stats
    assert_same_bits(rt.shade_rays(D, without_mask(planes))["colour"], want, f"{what}: shade_rays without the mask vs get_ray_colours", np.uint32)
    return want, planes


@pytest.fixture(scope="module")
def teapot_level1(rrt, teapot_arrays, teapot_osc):
    """The level-1 rays of the teapot's moved pose by the ORACLE's level 0 (read-only): next_origin / next_dir of its hits on a mirror, their expected arrays and
    the oracle's colours of them."""
    cam = pose(rrt, 1)
    O, D = rays_of(cam, W, H)
    ref0 = expected_ray_planes(teapot_osc, teapot_arrays, rrt.default_lights(), cam["eye"], D)
    on = reflecting(teapot_arrays, ref0, 0, M)
    o1, d1 = np.ascontiguousarray(ref0["next_origin"][on]), np.ascontiguousarray(ref0["next_dir"][on])
    ref1 = expected_ray_planes(teapot_osc, teapot_arrays, rrt.default_lights(), o1, d1)
    cols = oracle_colours(teapot_osc, o1, d1)
    for a in (o1, d1, cols):
        a.setflags(write=False)
    return o1, d1, ref1, cols


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h", [(64, 48), (97, 61)])
def test_depth_0_is_get_ray_colours(rrt, teapot, teapot_osc, w, h, k):
    cam = pose(rrt, k)
    O, D = rays_of(cam, w, h)
    ref = oracle_colours(teapot_osc, O, D)
    by_oracle = np.fromiter(POOL.map(lambda i: teapot_osc.intersect(O[i], D[i])[0], range(len(D))), bool, len(D))
    assert len(D) == {(64, 48): 12032, (97, 61): 22656}[(w, h)]
    assert by_oracle.mean() >= 0.5 and not by_oracle.all(), f"{by_oracle.mean():.3f} of the rays hit by the oracle: want at least 0.5 and some miss"
    for mode in ALL_MODES:
        rt = posed(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), cam)
        got, planes = assert_shade_is_get_ray_colours(rt, O, D, f"{w}x{h}, pose {k}, walk {mode}")
        hit, m = planes["hit"].astype(bool), planes["lights"]
        assert same(hit, by_oracle), f"walk {mode}: hit differs from the oracle's on {int((hit != by_oracle).sum())} rays"
        behind_break = int((hit & ((m >> 1) & 1 == 0) & ((m >> 2) & 1 == 1)).sum())
        before_break = int((hit & ((m >> 1) & 1 == 1) & ((m >> 2) & 1 == 0)).sum())
        assert behind_break >= 40 and before_break >= 15, (behind_break, before_break)
        assert_frame_close(got, ref, f"{w}x{h}, pose {k}, walk {mode}: shade_rays vs the oracle's get_ray_colour")


def test_depth_0_is_get_ray_colours_in_the_mirror_room(rrt, room):
    A, lights, sd, osc = room
    O, D = rays_of(CREATION, RW, RH)
    ref = oracle_colours(osc, O, D)
    by_oracle = np.fromiter(POOL.map(lambda i: osc.intersect(O[i], D[i])[0], range(len(D))), bool, len(D))
    assert len(D) == 2944 and by_oracle.all(), (len(D), int(by_oracle.sum()))                  # (a closed room: every ray hits a wall or the block)
    for mode in ALL_MODES:
        got, planes = assert_shade_is_get_ray_colours(rrt.RayTracer(sd, lights, box_filter=mode), O, D, f"mirror room, walk {mode}")
        assert reflecting(A, planes, 0, M).sum() >= 2500
        assert_frame_close(got, ref, f"mirror room, walk {mode}: shade_rays vs the oracle's get_ray_colour")


# ------------------------------------------------------------------ 2
def test_rays_that_do_not_start_at_the_eye(rrt, teapot, teapot_arrays, teapot_level1):
    o1, d1, ref1, cols = teapot_level1
    hit1 = ref1["hit"].astype(bool)
    n_mirror = int(reflecting(teapot_arrays, ref1, 0, M).sum())
    print(f"teapot, moved pose: level 1 {len(d1)} rays, {int(hit1.sum())} hit by the oracle, {n_mirror} of them on a mirror again")
    assert len(d1) >= 1500 and hit1.sum() >= 800 and n_mirror >= 700, (len(d1), int(hit1.sum()), n_mirror)
    for mode in ALL_MODES:
        rt = posed(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), pose(rrt, 1))
        got, planes = assert_shade_is_get_ray_colours(rt, o1, d1, f"teapot level 1, walk {mode}")
        assert same(planes["hit"].astype(bool), hit1)
        assert_frame_close(got, cols, f"teapot level 1, walk {mode}: shade_rays vs the oracle's get_ray_colour")


def test_level_1_of_the_mirror_room(rrt, room):
    A, lights, sd, osc = room
    O, D = rays_of(CREATION, RW, RH)
    ref0 = expected_ray_planes(osc, A, lights, ORIGIN, D)
    on = reflecting(A, ref0, 0, M)
    o1, d1 = np.ascontiguousarray(ref0["next_origin"][on]), np.ascontiguousarray(ref0["next_dir"][on])
    cols = oracle_colours(osc, o1, d1)
    hit1 = np.fromiter(POOL.map(lambda i: osc.intersect(o1[i], d1[i])[0], range(len(d1))), bool, len(d1))
    assert len(d1) >= 2500 and hit1.sum() >= 2500, (len(d1), int(hit1.sum()))
    for mode in ALL_MODES:
        got, _ = assert_shade_is_get_ray_colours(rrt.RayTracer(sd, lights, box_filter=mode), o1, d1, f"mirror room level 1, walk {mode}")
        assert_frame_close(got, cols, f"mirror room level 1, walk {mode}: shade_rays vs the oracle's get_ray_colour")


# ------------------------------------------------------------------ 3
@pytest.fixture(scope="module")
def room_chain(rrt, room):
    """The mirror room's raytracer and the levels of its 32 x 24 frame's reflection chain (shade_rays_checks.chain_levels), read-only."""
    A, lights, sd, _ = room
    rt = rrt.RayTracer(sd, lights)
    O, D = rays_of(CREATION, RW, RH)
    levels = chain_levels(rt, A, O, D, M)
    alive = [len(l[1]) for l in levels]
    print(f"mirror room: rays alive per level {alive}")
    assert len(levels) == M + 1 and alive[1] >= 2500 and alive[5] >= 1000, alive
    return rt, levels


def test_depth(rrt, room, room_chain):
    """The rays of level k, shaded at depth k, have the colours a raytracer with max_reflection_depth M - k gives them from depth 0."""
    A, lights, sd, _ = room
    _, levels = room_chain
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(sd, lights, box_filter=mode)
        for k in (1, 2, 5):
            o, d, planes, _ = levels[k]
            want = rrt.RayTracer(sd, lights, max_reflection_depth=M - k, box_filter=mode).get_ray_colours(o, d)
            for what, p in (("with the mask", planes), ("without the mask", without_mask(planes))):
                assert_same_bits(rt.shade_rays(d, p, depth=k)["colour"], want, f"walk {mode}, level {k} at depth {k} {what} vs max_reflection_depth {M - k}", np.uint32)
            if k < 5:
                assert (want != rt.get_ray_colours(o, d)).sum() >= 500, f"level {k}: depth {k} and depth 0 give the same colours: depth is not read"
        o, d, planes, _ = levels[5]
        out5, out7, big = (rt.shade_rays(d, planes, depth=dep, outputs=OUTPUTS) for dep in (5, 7, 0xFFFFFFFF))
        for n in OUTPUTS:
            assert same(out7[n], out5[n]) and same(big[n], out5[n]), f"walk {mode}: {n} at depth 7 or 2^32 - 1 is not {n} at depth 5"
        assert (out5["kr"] == 0.0).all() and same(out5["colour"], np.where(planes["hit"].astype(bool), pack(clamp_u8(out5["local"])), WHITE).astype(np.uint32))


# ------------------------------------------------------------------ 4
def check_local_and_kr(rt, A, lights, levels, what):
    """Every level of a chain: kr, local and colour by the rules of rrt.h, colour of the reflecting rays from the colours of the level below."""
    below = None
    for k in reversed(range(len(levels))):
        o, d, planes, go = levels[k]
        out = rt.shade_rays(d, planes, depth=k, outputs=OUTPUTS)
        hit = planes["hit"].astype(bool)
        assert same(out["kr"], np.where(go, kr_of(A, planes["material"]), 0.0)), f"{what}, level {k}: kr is not the table's where the reference reflects and 0.0 elsewhere"
        with np.errstate(invalid="ignore", divide="ignore"):
            want = pack(clamp_u8(local_colour(A, lights, d, planes)))
        assert_frame_close(pack(clamp_u8(out["local"])), want, f"{what}, level {k}: local, clamped, vs ray_surface_checks.local_colour", tol=COLOUR_TOL)
        assert (bits(out["local"][~hit]) == 0).all() and (out["colour"][~hit] == WHITE).all(), f"{what}, level {k}: a miss is not WHITE / (0, 0, 0)"
        matte = hit & ~go
        assert_same_bits(out["colour"][matte], pack(clamp_u8(out["local"][matte])), f"{what}, level {k}: colour where kr == 0", np.uint32)
        if go.any():
            assert_same_bits(out["colour"][go], mixed(out["local"][go], out["kr"][go], below), f"{what}, level {k}: colour where kr > 0 from the level below", np.uint32)
        below = out["colour"]
    return below


def test_local_and_kr(rrt, teapot, teapot_arrays, room, room_chain):
    A, lights, sd, _ = room
    rt, levels = room_chain
    top = check_local_and_kr(rt, A, lights, levels, "mirror room")
    assert_same_bits(top, rt.get_ray_colours(levels[0][0], levels[0][1]), "mirror room: level 0 vs get_ray_colours", np.uint32)
    cam = pose(rrt, 1)
    trt = posed(rrt.RayTracer(teapot, rrt.default_lights()), cam)
    O, D = rays_of(cam, W, H)
    tl = chain_levels(trt, teapot_arrays, O, D, M)
    alive = [len(l[1]) for l in tl]
    n_matte = int((tl[0][2]["hit"].astype(bool) & ~tl[0][3]).sum())
    print(f"teapot, moved pose: rays alive per level {alive}, {n_matte} matte hits at level 0")
    assert len(alive) >= 3 and alive[1] >= 1500 and alive[2] >= 700 and n_matte >= 5000, (alive, n_matte)
    check_local_and_kr(trt, teapot_arrays, rrt.default_lights(), tl, "teapot, moved pose")


def test_the_recursion_from_library_calls_alone(rrt, room, room_chain):
    """Level by level with `local` and `kr` only -- colour is never asked for -- on the host, then entirely on the device: both end in get_ray_colours' colours."""
    torch = pytest.importorskip("torch")
    A, lights, sd, _ = room
    rt, levels = room_chain
    O, D = levels[0][0], levels[0][1]
    want = rt.get_ray_colours(O, D)

    def host_level(k, d, planes):
        out = rt.shade_rays(d, planes, depth=k, outputs=("local", "kr"))
        return out["local"], out["kr"]
    assert_same_bits(unwind(levels, host_level), want, "the recursion followed on the host", np.uint32)
    # on the device: surface_rays_into and shade_rays_into per level on a stream of the test's own; the rays of a level are the reflecting rays of the level above
    stream = torch.cuda.Stream()
    kinds = {np.uint8: torch.uint8, np.float64: torch.float64, np.uint32: torch.int32}
    f64 = dict(dtype=torch.float64, device="cuda")
    kept = []
    with torch.cuda.stream(stream):
        o_t, d_t = torch.tensor(O, device="cuda").reshape(-1), torch.tensor(D, device="cuda").reshape(-1)
        for k in range(M + 1):
            n = d_t.numel() // 3
            rec = {name: torch.empty(n * (3 if name in VECTORS else 1), dtype=kinds[dt], device="cuda")
                   for name, dt in dict(albedo=np.uint32, point=np.float64, normal=np.float64, material=np.uint32, lights=np.uint32, next_origin=np.float64, next_dir=np.float64).items()}
            rt.surface_rays_into(o_t, d_t, rec, stream=stream.cuda_stream)
            out = {name: torch.full((n * (3 if name == "local" else 1),), OUT_SENTINEL[name], dtype=kinds[OUT_DTYPES[name]], device="cuda") for name in OUTPUTS}
            rt.shade_rays_into({name: out[name] for name in ("local", "kr")}, d_t, rec, depth=k, stream=stream.cuda_stream)
            go = out["kr"] > 0.0
            kept.append((rec, out, go))
            if k == M:
                break
            o_t, d_t = rec["next_origin"].reshape(-1, 3)[go].reshape(-1), rec["next_dir"].reshape(-1, 3)[go].reshape(-1)
        q = lambda x: torch.where(x > 0.0, torch.clamp(x, max=255.0), torch.zeros_like(x)).to(torch.int64)   # clamp(0.0, 255.0) as u8
        packed = lambda c: (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
        below = None
        for rec, out, go in reversed(kept):
            local = out["local"].reshape(-1, 3)
            c = torch.where((rec["material"].to(torch.int64) & 0xFFFFFFFF) < len(A["materials"]), packed(q(local)), torch.full_like(go, WHITE, dtype=torch.int64))
            if below is not None:
                kr = out["kr"][go]
                ch = torch.stack([(below >> 16) & 255, (below >> 8) & 255, below & 255], -1).to(torch.float64)
                c[go] = packed(q(local[go] * (1.0 - kr)[:, None] + ch * kr[:, None]))                      # raytracer.rs:89-101
            below = c
    stream.synchronize()
    assert [int(go.sum()) for _, _, go in kept[:-1]] == [len(l[1]) for l in levels[1:]] and not bool(kept[-1][2].any())
    assert_same_bits(below.cpu().numpy().astype(np.uint32), want, "the recursion followed on the device", np.uint32)
    for rec, out, go in kept:
        assert bool((out["colour"] == OUT_SENTINEL["colour"]).all()), "colour was not passed and was written"


# ------------------------------------------------------------------ 5
def test_without_colour_and_with_a_mask_only_what_is_asked_is_written(rrt, room, room_chain):
    torch = pytest.importorskip("torch")
    rt, levels = room_chain
    o, d, planes, go = levels[0]
    n = len(d)
    want = rt.shade_rays(d, planes, outputs=OUTPUTS)
    kinds = {np.float64: torch.float64, np.uint32: torch.int32}
    rec = {name: torch.tensor(np.ascontiguousarray(planes[name]).view(np.int32 if planes[name].dtype == np.uint32 else np.float64), device="cuda").reshape(-1) for name in INPUTS}
    d_t = torch.tensor(d, device="cuda").reshape(-1)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for asked in (("local", "kr"), ("kr",), ("local",), ("colour",), OUTPUTS):
        for masked in (True, False):
            out = {name: torch.full((n * (3 if name == "local" else 1),), OUT_SENTINEL[name], dtype=kinds[OUT_DTYPES[name]], device="cuda") for name in OUTPUTS}
            torch.cuda.synchronize()
            rt.shade_rays_into({name: out[name] for name in asked}, d_t, rec if masked else without_mask(rec), stream=stream.cuda_stream)
            stats = rt.last_stats()                                                        # (waits for the launch's second event)
            stream.synchronize()
            assert (stats["width"], stats["height"], stats["rays_primary"]) == (n, 1, n) and stats["kernel_ms"] > 0, (asked, masked, stats)
            for name in OUTPUTS:
                got = out[name].cpu().numpy().view(OUT_DTYPES[name]).reshape(want[name].shape)
                if name in asked:
                    assert same(got, want[name]), f"asked for {asked}, mask {masked}: {name} differs from the host form's"
                    if len(asked) == 1:                                                    # the host form with ONE output asked for and two NULL, against the device form's
                        one = rt.shade_rays(d, planes if masked else without_mask(planes), outputs=asked)
                        assert set(one) == set(asked)
                        assert same(one[name], got), f"{name} alone, mask {masked}: the host form differs from the device form"
                else:
                    assert (out[name].cpu().numpy() == np.array(OUT_SENTINEL[name]).astype(out[name].cpu().numpy().dtype)).all(), f"asked for {asked}: {name} was written"


# ------------------------------------------------------------------ 6
def edited_table(materials):
    new = copy.deepcopy(materials)
    new[0]["kr"], new[0]["ns"], new[0]["ka"] = 0.4, 20.0, (0.8, 0.9, 1.0)
    new[3]["kr"], new[3]["kd"], new[3]["ks"] = 0.0, (0.2, 0.5, 0.8), (0.3, 0.3, 0.3)
    return new


@pytest.fixture(scope="module")
def rays6(teapot_level1):
    """Every fourth primary ray of the teapot's 64 x 48 frame in the creation pose and the level-1 rays of its moved pose (plain rays from here on), read-only."""
    o1, d1, _, _ = teapot_level1
    d0 = frame_dirs(CREATION, W, H).reshape(-1, 3)[::4]
    O, D = np.concatenate([np.broadcast_to(np.asarray(ORIGIN), d0.shape), o1]), np.concatenate([d0, d1])
    O.setflags(write=False); D.setflags(write=False)
    return O, D


def apart(a, b):
    return int((np.abs(channels(a) - channels(b)).max(-1) > 1).sum())


def test_relighting_and_material_edits(rrt, ob, teapot, teapot_arrays, teapot_osc, rays6):
    """The records are kept, the lights and the materials change: shade_rays of the OLD records is get_ray_colours of the edited raytracer."""
    O, D = rays6
    A = teapot_arrays
    L, V = rrt.Light, rrt.Vector3d
    lights = rrt.default_lights()
    dimmed = [L.Ambient(0.2), L.Point(0.7, V(-7.0, 1.0, -15.0)), L.Point(0.1, V(0.0, 1.0, -41.0)), L.Directional(0.6, V(3.0, -1.0, 10.0))]
    moved = rrt.default_lights()
    moved[1] = L.Point(0.4, V(6.0, 8.0, -12.0))
    new = edited_table(A["materials"])
    base = oracle_colours(teapot_osc, O, D)
    refs = dict(dimmed=oracle_colours(oracle_for(ob, A, dimmed), O, D), moved=oracle_colours(oracle_for(ob, A, moved), O, D),
                materials=oracle_colours(oracle_for(ob, dict(A, materials=new), lights), O, D))
    counts = {k: apart(v, base) for k, v in refs.items()}
    print(f"{len(D)} rays; the oracle's colours move by more than 1 on {counts}")
    assert len(D) >= 4500 and counts["dimmed"] >= MIN_APART["dimmed"] and counts["moved"] >= MIN_APART["moved"] and counts["materials"] >= MIN_APART["materials"], counts
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, lights, box_filter=mode)
        old = rt.surface_rays(O, D)
        before = rt.get_ray_colours(O, D)
        # intensities and the directional light's vector: the kept mask is still the mask
        rt.set_lights(dimmed)
        fresh = rt.get_ray_colours(O, D)
        assert_same_bits(rt.shade_rays(D, old)["colour"], fresh, f"walk {mode}: dimmed lights, the old records with their mask", np.uint32)
        assert_frame_close(fresh, refs["dimmed"], f"walk {mode}: get_ray_colours with the dimmed lights vs the oracle")
        # a camera change in between leaves ray records valid
        rt.look_at(MOVED_EYE, TARGET)
        assert_same_bits(rt.shade_rays(D, old)["colour"], fresh, f"walk {mode}: the same after set_camera", np.uint32)
        rt.reset_camera()
        # a moved point light: the mask is stale, the other arrays are not
        rt.set_lights(moved)
        fresh = rt.get_ray_colours(O, D)
        assert_same_bits(rt.shade_rays(D, without_mask(old))["colour"], fresh, f"walk {mode}: a moved point light, the old records without their mask", np.uint32)
        assert_frame_close(fresh, refs["moved"], f"walk {mode}: get_ray_colours with the moved light vs the oracle")
        assert (rt.shade_rays(D, old)["colour"] != fresh).any(), f"walk {mode}: shading with the stale mask gives the fresh colours: the mask is not read"
        rt.set_lights(lights)
        assert_same_bits(rt.shade_rays(D, old)["colour"], before, f"walk {mode}: the first lights again", np.uint32)
        # ka, kd, ks, ns, kr
        rt.set_materials(new)
        fresh = rt.get_ray_colours(O, D)
        for what, p in (("with their mask", old), ("without their mask", without_mask(old))):
            assert_same_bits(rt.shade_rays(D, p)["colour"], fresh, f"walk {mode}: new materials, the old records {what}", np.uint32)
        assert_frame_close(fresh, refs["materials"], f"walk {mode}: get_ray_colours with the new materials vs the oracle")
        out = rt.shade_rays(D, old, outputs=("kr",))
        assert same(out["kr"], np.where(old["hit"].astype(bool), kr_of(dict(A, materials=new), old["material"]), 0.0)), f"walk {mode}: kr is not the new table's"


MIN_APART = dict(dimmed=2000, moved=1300, materials=1600)        # of 4765 rays (the oracle counts 2177, 1493 and 1828)


def test_the_options_are_followed(rrt, ob, teapot, teapot_arrays, teapot_osc, room, rays6):
    O, D = rays6
    lights = rrt.default_lights()
    base = oracle_colours(teapot_osc, O, D)
    for opt, least in ((dict(surface_offset=1e-2), MIN_OPTION["surface_offset"]), (dict(max_reflection_depth=0), MIN_OPTION["depth 0"]), (dict(max_reflection_depth=1), MIN_OPTION["depth 1"])):
        ref = oracle_colours(oracle_for(ob, teapot_arrays, lights, **opt), O, D)
        n = int((ref != base).sum())
        print(f"{opt}: the oracle's colours differ from the default's on {n} rays")
        assert n >= least, (opt, n)
        for mode in FORCED_MODES:
            got, _ = assert_shade_is_get_ray_colours(rrt.RayTracer(teapot, lights, box_filter=mode, **opt), O, D, f"{opt}, walk {mode}")
            assert_frame_close(got, ref, f"{opt}, walk {mode}: shade_rays vs the oracle")
    A, rl, sd, _ = room
    o, d = rays_of(CREATION, RW, RH)
    for depth in (0, 1, 3):
        got, _ = assert_shade_is_get_ray_colours(rrt.RayTracer(sd, rl, max_reflection_depth=depth), o, d, f"mirror room, max_reflection_depth {depth}")
        assert_frame_close(got, oracle_colours(oracle_for(ob, A, rl, max_reflection_depth=depth), o, d), f"mirror room, max_reflection_depth {depth}: shade_rays vs the oracle")


MIN_OPTION = {"surface_offset": 400, "depth 0": 600, "depth 1": 80}   # rays of the 4765 whose colour the option changes (the oracle counts 503, 671 and 94)


# ------------------------------------------------------------------ 7
def test_a_soup_with_long_own_lists(rrt, ob, teapot_arrays):
    A = soup_scene(teapot_arrays)
    lights = rrt.default_lights()
    osc = oracle_for(ob, A, lights)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    O, D = rays_of(CREATION, RW, RH)
    ref = oracle_colours(osc, O, D)
    by_oracle = np.fromiter(POOL.map(lambda i: osc.intersect(O[i], D[i])[0], range(len(D))), bool, len(D))
    print(f"soup: {len(D)} rays, {int(by_oracle.sum())} hit by the oracle")
    assert len(D) == 2944 and by_oracle.sum() >= SOUP_MIN_HITS, int(by_oracle.sum())
    for mode in ALL_MODES:
        rt = rrt.RayTracer(sd, lights, box_filter=mode)
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records (clusters.cpp)"
        got, planes = assert_shade_is_get_ray_colours(rt, O, D, f"soup, walk {mode}")
        assert same(planes["hit"].astype(bool), by_oracle)
        assert_frame_close(got, ref, f"soup, walk {mode}: shade_rays vs the oracle")


SOUP_MIN_HITS = 2800                                             # (the oracle counts 2944: the soup fills the 32 x 24 frame)


def test_the_chain_scene(rrt, ob):
    A, names = chain_scene("main")
    osc = oracle_for(ob, A, CHAIN_LIGHTS, CHAIN_CAMERA)
    R = chain_main_rays()
    sets = ("on_c1", "on_c2", "band")                                                     # (the rays without a bound: get_ray_colours takes none)
    O = np.ascontiguousarray(np.concatenate([R[k][0] for k in sets])); D = np.ascontiguousarray(np.concatenate([R[k][1] for k in sets]))
    ans = [osc.intersect(O[i], D[i]) for i in range(len(O))]
    by_oracle = np.array([a[0] for a in ans], bool)
    seen = {names[a[4]] for a in ans if a[0]}
    ref = oracle_colours(osc, O, D)
    print(f"chain scene: {len(O)} rays, {int(by_oracle.sum())} hit by the oracle ({sorted(seen)})")
    assert len(O) >= CHAIN_MIN[0] and by_oracle.sum() >= CHAIN_MIN[1] and {"c1", "c2", "graze", "lo2"} <= seen, (len(O), int(by_oracle.sum()), seen)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode, shortcut in [(m, True) for m in FORCED_MODES] + [("bundle", False)]:
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*CHAIN_CAMERA), box_filter=mode, chain_shortcut=shortcut)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        got, planes = assert_shade_is_get_ray_colours(rt, O, D, f"chain scene, walk {mode}, shortcut {shortcut}")
        assert same(planes["hit"].astype(bool), by_oracle)
        assert_frame_close(got, ref, f"chain scene, walk {mode}, shortcut {shortcut}: shade_rays vs the oracle")


CHAIN_MIN = (500, 200)                                           # rays and hits (the oracle counts 512 and 225)


# ------------------------------------------------------------------ 8
def test_edges_of_the_batch(rrt, teapot, teapot_arrays):
    O, D = rays_of(CREATION, W, H)
    o, d = O[5500:5800], D[5500:5800]                                                     # (the teapot's silhouette crosses these rays: the oracle counts 205 hits, 68 on the mirror)
    n_mats = len(teapot_arrays["materials"])
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        planes = rt.surface_rays(o, d)
        whole = rt.shade_rays(d, planes, outputs=OUTPUTS)
        hit = planes["hit"].astype(bool)
        assert 150 <= hit.sum() <= 250 and (whole["kr"] > 0.0).sum() >= 50, (int(hit.sum()), int((whole["kr"] > 0.0).sum()))
        assert_same_bits(whole["colour"], rt.get_ray_colours(o, d), f"walk {mode}: the slice of the frame", np.uint32)
        for n in (1, 63, 64, 65):
            for start in (0, 300 - n):
                sl = slice(start, start + n)
                part = rt.shade_rays(d[sl], {name: planes[name][sl] for name in INPUTS}, outputs=OUTPUTS)
                for name in OUTPUTS:
                    assert same(part[name], whole[name][sl]), f"walk {mode}: {n} rays from {start}: {name} is not the batch's slice"
        # n = 0: RRT_OK, nothing enqueued, the statistics stay
        stats = rt.last_stats()
        empty = rt.shade_rays(np.zeros((0, 3)), {name: planes[name][:0] for name in INPUTS}, outputs=OUTPUTS)
        assert set(empty) == set(OUTPUTS) and all(len(a) == 0 for a in empty.values())
        L = rrt.lib()
        assert L.rrt_shade_rays(rt._h, 0, None, C.byref(rrt.CRaySurface()), 0, C.byref(rrt.CRayShade())) == rrt.OK
        assert L.rrt_shade_rays_device(rt._h, 0, None, C.byref(rrt.CRaySurface()), 3, C.byref(rrt.CRayShade()), None) == rrt.OK
        assert rt.last_stats() == stats, "n = 0 changed the statistics"
        # dead rays: the records of rays with max_t = 0.0, and material indices at and beyond the table
        dead = rt.surface_rays(o, d, np.where(np.arange(300) % 2 == 0, 0.0, np.inf))
        assert (dead["material"][::2] == 0xFFFFFFFF).all() and same(dead["material"][1::2], planes["material"][1::2])
        out = rt.shade_rays(d, dead, outputs=OUTPUTS)
        edited = dict(planes, material=planes["material"].copy())
        edited["material"][0:300:3] = n_mats
        edited["material"][1:300:3] = 0x80000000
        out2 = rt.shade_rays(d, edited, outputs=OUTPUTS)
        for what, got, gone in (("max_t = 0.0", out, np.arange(300) % 2 == 0), ("a material index beyond the table", out2, np.arange(300) % 3 != 2)):
            assert (got["colour"][gone] == WHITE).all() and (bits(got["local"][gone]) == 0).all() and (bits(got["kr"][gone]) == 0).all(), f"walk {mode}: {what} is not WHITE / zeros / 0.0"
            for name in OUTPUTS:
                assert same(got[name][~gone], whole[name][~gone]), f"walk {mode}: {what} moves {name} of the other rays"
        assert (hit & (np.arange(300) % 3 != 2)).sum() >= 100
        # the top byte of albedo is ignored
        loud = dict(planes, albedo=planes["albedo"] | np.uint32(0xA5000000))
        out3 = rt.shade_rays(d, loud, outputs=OUTPUTS)
        for name in OUTPUTS:
            assert same(out3[name], whole[name]), f"walk {mode}: the top byte of albedo moves {name}"


# ------------------------------------------------------------------ 9
def test_refusals_leave_everything_as_it_was(rrt, teapot):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = [rt.render(W, H) for _ in range(2)][-1]                                         # (twice: the size's variant is measured)
    variant = rt.last_stats()["filter_variant"]
    O, D = rays_of(CREATION, W, H)
    o, d = O[:256], D[:256]
    rt.intersect_rays(o[:64], d[:64])
    ray_variant = rt.last_stats()["filter_variant"]
    planes = rt.surface_rays(o, d)
    want = rt.get_ray_colours(o, d)
    # neither form measures or alters the tuning state: a batch large enough to be measured by the other host forms runs in the variant small batches run
    big_o, big_d = O[:8192].repeat(3, 0), D[:8192].repeat(3, 0)
    big = rt.surface_rays(O[:8192], D[:8192])
    rt.shade_rays(big_d, {name: big[name].repeat(3, 0) for name in INPUTS})
    stats = rt.last_stats()
    assert (stats["width"], stats["filter_variant"]) == (24576, ray_variant), stats
    kinds = {np.float64: torch.float64, np.uint32: torch.int32}
    rec = {name: torch.tensor(np.ascontiguousarray(planes[name]).view(np.int32 if planes[name].dtype == np.uint32 else np.float64), device="cuda").reshape(-1) for name in INPUTS}
    d_t = torch.tensor(d, device="cuda").reshape(-1)
    out = {name: torch.full((256 * (3 if name == "local" else 1),), OUT_SENTINEL[name], dtype=kinds[OUT_DTYPES[name]], device="cuda") for name in OUTPUTS}
    torch.cuda.synchronize()
    rt.shade_rays_into({"colour": out["colour"]}, d_t, rec)
    torch.cuda.synchronize()
    assert rt.last_stats()["filter_variant"] == ray_variant
    assert_same_bits(out["colour"].cpu().numpy().view(np.uint32), want, "the device form", np.uint32)
    out["colour"].fill_(OUT_SENTINEL["colour"])
    torch.cuda.synchronize()
    frame_again = rt.render(W, H)
    assert np.array_equal(frame_again, frame) and rt.last_stats()["filter_variant"] == variant
    stats = rt.last_stats()
    s = rrt.CRaySurface(**{name: t.data_ptr() for name, t in rec.items()})
    so = rrt.CRayShade(**{name: t.data_ptr() for name, t in out.items()})
    buf = np.full(256, -12345.5)
    hs = rrt.CRaySurface(**{name: np.ascontiguousarray(planes[name]).ctypes.data for name in INPUTS})
    ho = rrt.CRayShade(kr=buf.ctypes.data)
    dp = lambda a: a.ctypes.data_as(rrt._dp)
    less = lambda st, name: type(st)(**{n: getattr(st, n) for n, _ in st._fields_ if n != name and getattr(st, n)})
    calls = [("all three outputs NULL", lambda: rt.shade_rays(d, planes, outputs=())),
             ("all three outputs NULL, device form", lambda: rt.shade_rays_into({}, d_t, rec)),
             ("a NULL record struct", lambda: rrt._call("rrt_shade_rays", rt._h, 256, dp(d), None, 0, C.byref(ho))),
             ("a NULL output struct", lambda: rrt._call("rrt_shade_rays", rt._h, 256, dp(d), C.byref(hs), 0, None)),
             ("NULL structs, device form", lambda: rrt._call("rrt_shade_rays_device", rt._h, 256, d_t.data_ptr(), None, 0, None, None)),
             ("NULL structs with n = 0", lambda: rrt._call("rrt_shade_rays", rt._h, 0, None, None, 0, None)),
             ("NULL dirs", lambda: rrt._call("rrt_shade_rays", rt._h, 256, None, C.byref(hs), 0, C.byref(ho))),
             ("NULL dirs, device form", lambda: rrt._call("rrt_shade_rays_device", rt._h, 256, None, C.byref(s), 0, C.byref(so), None)),
             ("a NULL raytracer", lambda: rrt._call("rrt_shade_rays_device", None, 256, d_t.data_ptr(), C.byref(s), 0, C.byref(so), None))]
    for name in ("albedo", "point", "normal", "material"):
        calls.append((f"NULL {name}", lambda name=name: rrt._call("rrt_shade_rays", rt._h, 256, dp(d), C.byref(less(hs, name)), 0, C.byref(ho))))
        calls.append((f"NULL {name}, device form", lambda name=name: rrt._call("rrt_shade_rays_device", rt._h, 256, d_t.data_ptr(), C.byref(less(s, name)), 0, C.byref(so), None)))
    for what, call in calls:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert rt.last_stats() == stats, f"{what}: the statistics changed"
    assert np.array_equal(rt.render(W, H), frame), "the next frame differs"
    assert rt.last_stats()["filter_variant"] == variant
    torch.cuda.synchronize()
    assert (buf == -12345.5).all()
    for name, t in out.items():
        a = t.cpu().numpy()
        assert (a == np.array(OUT_SENTINEL[name]).astype(a.dtype)).all(), f"a refused call wrote {name}"
    # ... and the call still works
    assert_same_bits(rt.shade_rays(d, planes)["colour"], want, "after the refusals", np.uint32)
