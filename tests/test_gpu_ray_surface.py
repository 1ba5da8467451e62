"""Surface attributes and bounce rays of arbitrary ray batches (include/rrt.h: rrt_surface_rays, rrt_surface_rays_device) on the GPU: per ray the full surface
record of its first hit -- hit, t, u, v, triangle, albedo, point, shading normal, material, light mask -- and the reference's own next ray.

The expected arrays are the host restatement of tests/ray_surface_checks.py (the reference's arithmetic in numpy around the oracle's intersector).  The arrays are
also checked against the library's own frame planes, its other per-ray calls and its own colours (the reference's recursion followed level by level from the
arrays), batches against slices of larger ones, the device form against the host form, and the calls' behaviour after scene changes, towards the tuning state
and when they refuse.

All comparisons of arrays are bit for bit: f64 through its integer bits.  Every comparison with the oracle asserts its conditions BY THE ORACLE'S ANSWERS, so an
empty batch cannot pass; the thresholds sit below counts made on the CPU with the oracle alone.
"""
import ctypes as C

import numpy as np
import pytest

from bitwise import assert_same_arrays, same
from gpu_checks import (ALL_MODES, CHAIN_CAMERA, CHAIN_LIGHTS, FORCED_MODES, ORIGIN, assert_frame_close, chain_main_rays, chain_rrt_lights, chain_scene, mix4,
                        oracle_for, sample_rays, traced_rows)
from ray_surface_checks import (NAMES, SENTINEL, VECTORS, HostChain, assert_miss_values, device_arrays, expected_ray_planes, follow_chain, kr_of, kr_table, reflected,
                                rows, to_host)
from scenes import CREATION, MOVED_EYE, pose, posed, room, teapot_arrays, teapot_osc  # noqa: F401  (fixtures: room, teapot_arrays, teapot_osc)
from shade_checks import soup_scene
from surface_checks import frame_dirs, length, light_vec, traced_cols, traced_part

pytestmark = pytest.mark.gpu

W, H = 64, 48
RW, RH = 32, 24                                                  # the mirror room's frame
SHARED = ("hit", "t", "u", "v", "tri", "albedo", "point", "normal", "material", "lights")   # what rrt_surface_rays shares with the frame planes


def flat(planes):
    """[...] and [...][3] arrays as [n] and [n][3]"""
    return {n: np.asarray(a).reshape((-1, 3) if n in VECTORS else (-1,)) for n, a in planes.items()}


def only(planes, names=NAMES):
    return {n: planes[n] for n in names}


def mirrors(A, planes):
    return planes["hit"].astype(bool) & (kr_of(A, planes["material"]) > 0.0)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h", [(64, 48), (97, 61)])
def test_primary_rays_of_a_frame_are_the_surface_planes(rrt, teapot, w, h, k):
    cam = pose(rrt, k)
    d = frame_dirs(cam, w, h)
    for mode in ALL_MODES:
        rt = posed(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), cam)
        want = traced_part(rt.surface(w, h, visibility=rrt.PLANES), w, h)
        hit, m = want["hit"].astype(bool), want["lights"]
        behind_break = int((hit & ((m >> 1) & 1 == 0) & ((m >> 2) & 1 == 1)).sum())
        before_break = int((hit & ((m >> 1) & 1 == 1) & ((m >> 2) & 1 == 0)).sum())
        assert hit.size == {(64, 48): 12032, (97, 61): 22656}[(w, h)]
        assert hit.mean() >= 0.5, f"only {hit.mean():.3f} of the compared rays hit (< 0.5)"
        assert behind_break >= 40 and before_break >= 15, (behind_break, before_break)
        got = rt.surface_rays(np.broadcast_to(np.asarray(cam["eye"]), d.shape), d)
        assert set(got) == set(NAMES)
        assert_same_arrays(flat(only(got, SHARED)), flat(only(want, SHARED)), SHARED, f"{w}x{h}, pose {k}, walk {mode}")
        stats = rt.last_stats()
        assert (stats["width"], stats["height"], stats["rays_primary"]) == (hit.size, 1, hit.size) and stats["kernel_ms"] > 0, stats


# ------------------------------------------------------------------ 2
def check_two_levels(rrt, make_rt, osc, A, lights, eye, d, what, min_rays, min_hits, min_mirror):
    """Level 0 = the rays (eye, d); level 1 = the next_origin / next_dir the library wrote for the level-0 hits on a mirror.  All twelve arrays of both levels equal
    expected_ray_planes in every mode; the conditions on level 1 are asserted by the oracle's answers."""
    d = d.reshape(-1, 3)
    ref0 = ref1 = None
    for mode in ALL_MODES:
        rt = make_rt(mode)
        l0 = rt.surface_rays(np.broadcast_to(np.asarray(eye, np.float64), d.shape), d)
        if ref0 is None:
            ref0 = expected_ray_planes(osc, A, lights, eye, d)
        assert_same_arrays(l0, ref0, NAMES, f"{what}, level 0, walk {mode}")
        on = mirrors(A, ref0)
        o1, d1 = l0["next_origin"][on], l0["next_dir"][on]
        assert same(d1, reflected(d[on], l0["normal"][on])) and same(o1, l0["point"][on] + l0["normal"][on] * 1e-4), f"{what}, walk {mode}: the next ray is not the restatement"
        l1 = rt.surface_rays(o1, d1)
        if ref1 is None:
            ref1 = expected_ray_planes(osc, A, lights, o1, d1)
            hit1 = ref1["hit"].astype(bool)
            n_mirror = int(mirrors(A, ref1).sum())
            print(f"{what}: level 0 {len(d)} rays, {int(ref0['hit'].sum())} hit, {int(on.sum())} on a mirror; level 1 {len(d1)} rays, {int(hit1.sum())} hit by the oracle, "
                  f"{n_mirror} of them on a mirror again, masks {np.unique(ref1['lights'][hit1]).tolist()}")
            assert len(d1) >= min_rays and hit1.sum() >= min_hits and n_mirror >= min_mirror, (len(d1), int(hit1.sum()), n_mirror)
        assert_same_arrays(l1, ref1, NAMES, f"{what}, level 1, walk {mode}")


def test_rays_that_do_not_start_at_the_eye_equal_the_oracle(rrt, teapot, teapot_arrays, teapot_osc):
    cam = pose(rrt, 1)
    check_two_levels(rrt, lambda mode: posed(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), cam), teapot_osc, teapot_arrays, rrt.default_lights(),
                     cam["eye"], frame_dirs(cam, W, H), "teapot, moved pose", 1500, 800, 700)


def test_the_mirror_room_equals_the_oracle(rrt, room):
    A, lights, sd, osc = room
    check_two_levels(rrt, lambda mode: rrt.RayTracer(sd, lights, box_filter=mode), osc, A, lights, ORIGIN, frame_dirs(CREATION, RW, RH), "mirror room", 2500, 2500, 0)


# ------------------------------------------------------------------ 3
def test_it_is_the_other_per_ray_calls(rrt, teapot, teapot_osc):
    """No oracle answer is compared: hit / t / u / v / tri against rrt_intersect_rays, the mask against rrt_occluded_rays on the shadow rays formed from next_origin
    and point, for primary, shadow-shaped and reflection-shaped rays under every kind of bound."""
    lights = rrt.default_lights()
    O1, D1, _ = sample_rays(teapot_osc, W, H, 256, np.random.default_rng(7), lights)
    n1 = len(O1)
    t_ref = np.array([teapot_osc.intersect(O1[i], D1[i])[1] for i in range(n1)])
    # every ray under every bound: +inf, |dir|, half of the oracle's t (|dir| for a miss), 0.0, -1.0, NaN
    bounds = (np.full(n1, np.inf), length(D1), np.where(t_ref > 0.0, 0.5 * t_ref, length(D1)), np.zeros(n1), np.full(n1, -1.0), np.full(n1, np.nan))
    O, D, B = np.tile(O1, (6, 1)), np.tile(D1, (6, 1)), np.concatenate(bounds)
    kind = np.repeat(np.arange(6), n1)
    dead = kind >= 3
    by_oracle = np.array([teapot_osc.intersect(O[i], D[i], B[i])[0] for i in range(len(O))])
    print(f"{n1} rays under 6 bounds; hits by the oracle per bound {[int(by_oracle[kind == j].sum()) for j in range(6)]}")
    assert n1 >= 600 and by_oracle[kind == 0].sum() >= 200 and by_oracle[kind == 1].sum() >= 50 and not by_oracle[dead].any(), [int(by_oracle[kind == j].sum()) for j in range(6)]
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, lights, box_filter=mode)
        got = rt.surface_rays(O, D, B)
        hit, t, u, v, tri = rt.intersect_rays(O, D, B)
        assert_same_arrays(got, dict(hit=hit.astype(np.uint8), t=t, u=u, v=v, tri=tri), ("hit", "t", "u", "v", "tri"), f"walk {mode}: against intersect_rays")
        assert same(hit, by_oracle), f"walk {mode}: hit differs from the oracle's on {int((hit != by_oracle).sum())} rays"
        assert_miss_values(rows(got, dead), slice(None), f"walk {mode}: a NaN or non-positive bound")
        assert_miss_values(rows(got, ~hit), slice(None), f"walk {mode}: a miss")
        assert same(got["point"][hit], O[hit] + D[hit] * got["t"][hit][:, None]), f"walk {mode}: point is not origin + dir * t"
        P, Q, m = got["point"][hit], got["next_origin"][hit], got["lights"][hit]
        n_occluded = 0
        for k, l in enumerate(lights):
            if l.kind != 1:
                assert ((m >> k) & 1 == 1).all(), f"walk {mode}: bit {k} of an Ambient / Directional light is not set on every hit"
                continue
            Ld = light_vec(l) - P
            occ = rt.occluded(Q, Ld, length(Ld))
            n_occluded += int(occ.sum())
            assert same(((m >> k) & 1).astype(np.uint8), (~occ).astype(np.uint8)), f"walk {mode}: bit {k} is not the negation of occluded_rays on {int((((m >> k) & 1) == occ).sum())} hits"
        assert n_occluded >= 100, n_occluded
        assert (m >> len(lights) == 0).all()


# ------------------------------------------------------------------ 4
def check_chain(rt, A, lights, cam, w, h, what, min_alive):
    """min_alive = (level, rays): at least that many rays are alive at that level."""
    d = frame_dirs(cam, w, h)
    O = np.ascontiguousarray(np.broadcast_to(np.asarray(cam["eye"], np.float64), d.shape)).reshape(-1, 3)
    chain = HostChain(rt, O, d)
    cols, alive = follow_chain(chain, A, lights)
    print(f"{what}: rays alive per level {alive}")
    assert chain.calls <= 6 and len(alive) > min_alive[0] and alive[min_alive[0]] >= min_alive[1], (chain.calls, alive)
    assert_frame_close(cols, rt.get_ray_colours(O, d.reshape(-1, 3)), f"{what}: the followed chain vs get_ray_colours")
    frame = rt.render(w, h)[np.ix_(traced_rows(h), traced_cols(w))]
    assert_frame_close(mix4(cols.reshape(-1, 4)).reshape(frame.shape), frame, f"{what}: the followed chain, mixed per pixel, vs render")
    return cols


def test_the_outputs_suffice_to_follow_the_recursion(rrt, teapot, teapot_arrays, room):
    """get_ray_colour_recursive from the arrays alone: at most six calls (max_reflection_depth 5), each fed the next_origin / next_dir of the hits whose material has
    kr > 0; every level shaded on the host, the unwind quantised at every level.

    Tolerance: COLOUR_TOL per channel, and it does not grow with depth.  numpy's pow and the GPU's may differ by an ulp, which moves a level's own colour by at
    most 1 after truncation.  Going up one level, the reflected input therefore differs by at most 1, is weighted by kr <= 1 and added to a local term that is
    the same on both sides up to that ulp: the sum differs by at most 1 before its own truncation, hence the level's colour by at most 1 again."""
    A, lights, sd, _ = room
    check_chain(rrt.RayTracer(sd, lights), A, lights, CREATION, RW, RH, "mirror room", (5, 1000))
    cam = pose(rrt, 1)
    check_chain(posed(rrt.RayTracer(teapot, rrt.default_lights()), cam), teapot_arrays, rrt.default_lights(), cam, W, H, "teapot, moved pose", (2, 700))


# ------------------------------------------------------------------ 5


class DeviceChain:
    """Feeds follow_chain from RayTracer.surface_rays_into: the rays of every level stay on the device, a level's arrays come to the host for shading only."""
    def __init__(self, torch, rt, A, O, D, stream):
        self.torch, self.rt, self.stream = torch, rt, stream
        self.kr = torch.tensor(kr_table(A), device="cuda")
        self.o, self.d, self.m = torch.tensor(O, device="cuda").reshape(-1), torch.tensor(D, device="cuda").reshape(-1), None
        self.calls = 0

    def level(self):
        torch = self.torch
        n = self.o.numel() // 3
        self.calls += 1
        with torch.cuda.stream(self.stream):
            self.out = device_arrays(torch, n)
            self.rt.surface_rays_into(self.o, self.d, self.out, self.m, stream=self.stream.cuda_stream)
        self.stream.synchronize()
        return self.d.cpu().numpy().reshape(n, 3), to_host(self.out, n)

    def descend(self, go, compact):
        torch = self.torch
        with torch.cuda.stream(self.stream):
            material = (self.out["material"].to(torch.int64) & 0xFFFFFFFF).clamp(max=len(self.kr) - 1)
            on = (self.out["hit"] == 1) & (self.kr[material] > 0.0)                       # the same decision, taken on the device
            assert bool((on.cpu().numpy() == go).all())
            if compact:
                self.o, self.d, self.m = self.out["next_origin"].reshape(-1, 3)[on].reshape(-1), self.out["next_dir"].reshape(-1, 3)[on].reshape(-1), None
            else:
                self.o, self.d = self.out["next_origin"], self.out["next_dir"]
                self.m = torch.where(on, torch.full_like(self.kr[material], float("inf")), torch.zeros_like(self.kr[material]))


def test_the_device_form(rrt, room):
    torch = pytest.importorskip("torch")
    A, lights, sd, _ = room
    d = frame_dirs(CREATION, RW, RH).reshape(-1, 3)
    O = np.ascontiguousarray(np.broadcast_to(np.asarray(ORIGIN), d.shape))
    n = len(d)
    rt = rrt.RayTracer(sd, lights)
    before = [rt.render(RW, RH) for _ in range(2)][-1]                                      # (twice: the size's variant is measured)
    variant = rt.last_stats()["filter_variant"]
    rt.intersect_rays(O[:64], d[:64])
    ray_variant = rt.last_stats()["filter_variant"]
    want = rt.surface_rays(O, d)
    stream = torch.cuda.Stream()
    o_t, d_t = torch.tensor(O, device="cuda").reshape(-1), torch.tensor(d, device="cuda").reshape(-1)
    torch.cuda.synchronize()
    # a subset of the outputs: the others are not written
    out = device_arrays(torch, n)
    subset = ("normal", "lights", "next_dir")
    rt.surface_rays_into(o_t, d_t, {name: out[name] for name in subset}, stream=stream.cuda_stream)
    stats = rt.last_stats()                                                                # (waits for the launch's second event)
    stream.synchronize()
    got = to_host(out, n)
    assert_same_arrays(got, want, subset, "surface_rays_into, three outputs")
    for name in set(NAMES) - set(subset):
        assert (out[name].cpu().numpy() == np.array(SENTINEL[name]).astype(out[name].cpu().numpy().dtype)).all(), f"array {name} was not passed and was written"
    assert (stats["width"], stats["height"], stats["rays_primary"], stats["filter_variant"]) == (n, 1, n, ray_variant) and stats["kernel_ms"] > 0, stats
    # all twelve, with a bound per ray
    bound = np.where(np.arange(n) % 3 == 0, 0.0, np.inf)
    out = device_arrays(torch, n)
    rt.surface_rays_into(o_t, d_t, out, torch.tensor(bound, device="cuda"), stream=stream.cuda_stream)
    stream.synchronize()
    assert_same_arrays(to_host(out, n), rt.surface_rays(O, d, bound), NAMES, "surface_rays_into, twelve outputs and max_t")
    # the host form with ONE array asked for and eleven NULL, against the device form's twelve
    out = device_arrays(torch, n)
    rt.surface_rays_into(o_t, d_t, out, stream=stream.cuda_stream)
    stream.synchronize()
    twelve = to_host(out, n)
    for name in NAMES:
        one = rt.surface_rays(O, d, planes=(name,))
        assert set(one) == {name}
        assert_same_arrays(one, twelve, (name,), f"array {name} alone, host form vs surface_rays_into")
    # the chain of part 4 on the device, joined by a boolean index and by a max_t of 0.0 for the dead rays
    host_cols, host_alive = follow_chain(HostChain(rt, O, d), A, lights)
    for compact in (True, False):
        chain = DeviceChain(torch, rt, A, O, d, stream)
        cols, alive = follow_chain(chain, A, lights, compact=compact)
        assert chain.calls <= 6 and alive == host_alive and alive[5] >= 1000, (chain.calls, alive, host_alive)
        assert same(cols, host_cols), f"the chain on the device (compact {compact}) ends in other colours than the chain on the host"
    assert_frame_close(host_cols, rt.get_ray_colours(O, d), "the chain vs get_ray_colours")
    # the tuning state is as before the device calls: the same frame from the same variant, small batches in the same variant, nothing measured
    rt.intersect_rays(O[:64], d[:64])
    assert rt.last_stats()["filter_variant"] == ray_variant
    after = rt.render(RW, RH)
    assert np.array_equal(after, before) and rt.last_stats()["filter_variant"] == variant


# ------------------------------------------------------------------ 6
@pytest.fixture(scope="module")
def rays4096(rrt, teapot):
    """2048 primary rays of the teapot frame and 2048 reflection-shaped rays from its hits (plain rays from here on), read-only."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    d = frame_dirs(CREATION, W, H).reshape(-1, 3)[::5][:2048]
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(ORIGIN), d.shape))
    l0 = rt.surface_rays(o, d)
    hit = np.flatnonzero(l0["hit"])
    assert len(hit) >= 1024
    pick = hit[np.arange(2048) % len(hit)]
    O, D = np.concatenate([o, l0["next_origin"][pick]]), np.concatenate([d, l0["next_dir"][pick]])
    O.setflags(write=False); D.setflags(write=False)
    return O, D


def assert_follows(rt, fresh, O, D, what):
    got, want = rt.surface_rays(O, D), fresh.surface_rays(O, D)
    assert_same_arrays(got, want, NAMES, what)
    return got


def test_scene_changes_are_followed(rrt, teapot, teapot_arrays, rays4096):
    O, D = rays4096
    L, V = rrt.Light, rrt.Vector3d
    A = teapot_arrays
    lights = rrt.default_lights()
    for mode in (None, "ray"):
        rt = rrt.RayTracer(teapot, lights, box_filter=mode)
        base = rt.surface_rays(O, D)
        hit = base["hit"].astype(bool)
        assert hit[:2048].sum() >= 1024 and hit[2048:].sum() >= 100, (int(hit[:2048].sum()), int(hit[2048:].sum()))
        # lights: a moved point light, then a shorter list
        moved = [lights[0], L.Point(0.4, V(6.0, 8.0, -12.0)), lights[2], lights[3]]
        for new, what in ((moved, "a moved point light"), (lights[:2], "a shorter list")):
            rt.set_lights(new)
            got = assert_follows(rt, rrt.RayTracer(teapot, new, box_filter=mode), O, D, f"walk {mode}: {what}")
            assert (got["lights"] != base["lights"]).sum() >= 100, f"{what} changes the mask on {int((got['lights'] != base['lights']).sum())} rays only"
            assert_same_arrays(got, base, [n for n in NAMES if n != "lights"], f"walk {mode}: {what} changes the mask only")
        rt.set_lights(lights)
        # materials: a bump map removed, a colour texture changed
        mats = [dict(m) for m in A["materials"]]                                          # (the rays see materials 0, 2 and 3 of the teapot's four)
        assert mats[0]["bump"] >= 0 and mats[2]["tex"] != mats[0]["tex"], mats
        mats[0]["bump"] = -1
        mats[2]["tex"] = mats[0]["tex"]
        rt.set_materials(mats)
        fresh = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], mats, A["textures"]), lights, box_filter=mode)
        got = assert_follows(rt, fresh, O, D, f"walk {mode}: new materials")
        assert (got["albedo"] != base["albedo"]).sum() >= 50 and (got["normal"] != base["normal"]).any(1).sum() >= 50
        assert_same_arrays(got, base, ("hit", "t", "u", "v", "tri", "point", "material"), f"walk {mode}: new materials leave the geometry alone")
        rt.set_materials(A["materials"])
        assert_same_arrays(rt.surface_rays(O, D), base, NAMES, f"walk {mode}: the first materials again")
        # triangles: the teapot shifted
        shifted = A["pos"] + np.array([0.25, -0.125, 0.5])
        rt.set_triangles(shifted, A["uv"], A["nrm"], A["mat"])
        fresh = rrt.RayTracer(rrt.SceneData.from_arrays(shifted, A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), lights, box_filter=mode)
        got = assert_follows(rt, fresh, O, D, f"walk {mode}: the teapot shifted")
        assert (got["t"] != base["t"]).sum() >= 1024


def test_the_surface_offset_option_is_followed(rrt, teapot, rays4096):
    O, D = rays4096
    lights = rrt.default_lights()
    base = rrt.RayTracer(teapot, lights).surface_rays(O, D)
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, lights, surface_offset=1e-2, box_filter=mode)
        got = rt.surface_rays(O, D)
        hit = got["hit"].astype(bool)
        assert_same_arrays(got, base, [n for n in NAMES if n not in ("lights", "next_origin")], f"walk {mode}: the offset moves next_origin and the shadow rays only")
        assert same(got["next_origin"][hit], got["point"][hit] + got["normal"][hit] * 1e-2), f"walk {mode}: next_origin is not point + normal * 1e-2"
        assert (got["lights"] != base["lights"]).sum() >= 1, "the larger offset changes no mask"
        P, Q, m = got["point"][hit], got["next_origin"][hit], got["lights"][hit]
        for k, l in enumerate(lights):
            if l.kind == 1:
                Ld = light_vec(l) - P
                assert same(((m >> k) & 1).astype(np.uint8), (~rt.occluded(Q, Ld, length(Ld))).astype(np.uint8)), f"walk {mode}: bit {k} is not the shadow query from the offset origin"


# ------------------------------------------------------------------ 7
def test_a_soup_with_long_own_lists_equals_the_oracle(rrt, ob, teapot_arrays):
    A = soup_scene(teapot_arrays)
    lights = rrt.default_lights()
    osc = oracle_for(ob, A, lights)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])

    def make(mode):
        rt = rrt.RayTracer(sd, lights, box_filter=mode)
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records (clusters.cpp)"
        return rt
    check_two_levels(rrt, make, osc, A, lights, ORIGIN, frame_dirs(CREATION, RW, RH), "soup", SOUP_MIN[0], SOUP_MIN[1], SOUP_MIN[2])


SOUP_MIN = (300, 300, 0)                                          # level 1 of the 32 x 24 soup frame: rays and hits (the oracle counts 366 and 344)


def test_the_chain_scene_equals_the_oracle(rrt, ob):
    A, names = chain_scene("main")
    osc = oracle_for(ob, A, CHAIN_LIGHTS, CHAIN_CAMERA)
    R = chain_main_rays()
    O = np.concatenate([r[0] for r in R.values()]); D = np.concatenate([r[1] for r in R.values()]); M = np.concatenate([r[2] for r in R.values()])
    ref0 = expected_ray_planes(osc, A, CHAIN_LIGHTS, O, D, M)
    hit0 = ref0["hit"].astype(bool)
    o1, d1 = ref0["next_origin"][hit0], ref0["next_dir"][hit0]                              # (one material, kr 0.4: every hit reflects)
    ref1 = expected_ray_planes(osc, A, CHAIN_LIGHTS, o1, d1)
    hit1 = ref1["hit"].astype(bool)
    seen = {names[i] for i in np.unique(ref0["tri"][hit0])}
    lit = int(((ref0["lights"][hit0] >> 1) & 1).sum())
    print(f"chain scene: {len(O)} rays, {int(hit0.sum())} hit ({sorted(seen)}), the point light reaches {lit}; level 1: {len(o1)} rays, {int(hit1.sum())} hit")
    assert len(O) >= CHAIN_MIN[0] and hit0.sum() >= CHAIN_MIN[1] and {"c1", "c2", "graze", "lo2"} <= seen and len(o1) == hit0.sum(), (len(O), int(hit0.sum()), seen)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode, shortcut in [(m, True) for m in FORCED_MODES] + [("bundle", False)]:
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*CHAIN_CAMERA), box_filter=mode, chain_shortcut=shortcut)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        l0 = rt.surface_rays(O, D, M)
        assert_same_arrays(l0, ref0, NAMES, f"chain scene, level 0, walk {mode}, shortcut {shortcut}")
        assert_same_arrays(rt.surface_rays(l0["next_origin"][hit0], l0["next_dir"][hit0]), ref1, NAMES, f"chain scene, level 1, walk {mode}, shortcut {shortcut}")


CHAIN_MIN = (600, 300)                                            # rays and level-0 hits (the oracle counts 644 and 309; the level-1 rays leave the scene: 309 misses)


# ------------------------------------------------------------------ 8
def test_edges_of_the_batch(rrt, teapot):
    torch = pytest.importorskip("torch")
    d = frame_dirs(CREATION, W, H).reshape(-1, 3)[5500:5800]                             # (the teapot's silhouette crosses these rays: both ends of the slice are mixed)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(ORIGIN), d.shape))
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        whole = rt.surface_rays(o, d)
        hit = whole["hit"].astype(bool)
        assert 60 <= hit.sum() <= 240 and 0 < hit[:129].sum() < 129 and 0 < hit[-129:].sum() < 129, (int(hit.sum()), int(hit[:129].sum()), int(hit[-129:].sum()))
        for n in (1, 63, 64, 65, 129):
            for start in (0, 300 - n):
                part = rt.surface_rays(o[start:start + n], d[start:start + n])
                assert_same_arrays(part, rows(whole, slice(start, start + n)), NAMES, f"walk {mode}: {n} rays from {start}")
        # misses only
        up = np.tile([0.0, 1.0, 0.0], (130, 1))
        away = rt.surface_rays(o[:130], up)
        assert_miss_values(away, slice(None), f"walk {mode}: a batch of misses")
        # n = 0: RRT_OK, nothing enqueued, nothing written
        empty = rt.surface_rays(np.zeros((0, 3)), np.zeros((0, 3)))
        assert set(empty) == set(NAMES) and all(len(a) == 0 for a in empty.values())
        stats = rt.last_stats()
        out = device_arrays(torch, 4)
        s = rrt.CRaySurface(**{name: t.data_ptr() for name, t in out.items()})
        L = rrt.lib()
        rays = torch.zeros(24, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert L.rrt_surface_rays_device(rt._h, 0, rays.data_ptr(), rays.data_ptr() + 96, None, C.byref(s), None) == rrt.OK
        assert L.rrt_surface_rays_device(rt._h, 0, None, None, None, C.byref(rrt.CRaySurface()), None) == rrt.OK
        assert L.rrt_surface_rays(rt._h, 0, None, None, None, C.byref(rrt.CRaySurface())) == rrt.OK
        torch.cuda.synchronize()
        for name, t in out.items():
            a = t.cpu().numpy()
            assert (a == np.array(SENTINEL[name]).astype(a.dtype)).all(), f"n = 0 wrote array {name}"
        assert rt.last_stats() == stats, "n = 0 changed the statistics"


# ------------------------------------------------------------------ 9
def test_refusals_leave_the_raytracer_as_it_was(rrt, teapot):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = rt.render(W, H)
    stats = rt.last_stats()
    L = rrt.lib()
    d = frame_dirs(CREATION, W, H).reshape(-1, 3)[:256]
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(ORIGIN), d.shape))
    o_t, d_t = torch.tensor(o, device="cuda").reshape(-1), torch.tensor(d, device="cuda").reshape(-1)
    out = device_arrays(torch, 256)
    torch.cuda.synchronize()
    s = rrt.CRaySurface(**{name: t.data_ptr() for name, t in out.items()})
    buf = np.full(256, -12345.5)
    hs = rrt.CRaySurface(t=buf.ctypes.data)
    dp = lambda a: a.ctypes.data_as(rrt._dp)
    for what, call in (("all twelve pointers NULL", lambda: rt.surface_rays(o, d, planes=())),
                       ("all twelve pointers NULL, device form", lambda: rt.surface_rays_into(o_t, d_t, {})),
                       ("a NULL struct", lambda: rrt._call("rrt_surface_rays", rt._h, 256, dp(o), dp(d), None, None)),
                       ("a NULL struct, device form", lambda: rrt._call("rrt_surface_rays_device", rt._h, 256, o_t.data_ptr(), d_t.data_ptr(), None, None, None)),
                       ("a NULL struct with n = 0", lambda: rrt._call("rrt_surface_rays", rt._h, 0, None, None, None, None)),
                       ("NULL origins", lambda: rrt._call("rrt_surface_rays", rt._h, 256, None, dp(d), None, C.byref(hs))),
                       ("NULL dirs", lambda: rrt._call("rrt_surface_rays", rt._h, 256, dp(o), None, None, C.byref(hs))),
                       ("NULL origins, device form", lambda: rrt._call("rrt_surface_rays_device", rt._h, 256, None, d_t.data_ptr(), None, C.byref(s), None)),
                       ("NULL dirs, device form", lambda: rrt._call("rrt_surface_rays_device", rt._h, 256, o_t.data_ptr(), None, None, C.byref(s), None)),
                       ("a NULL raytracer", lambda: rrt._call("rrt_surface_rays_device", None, 256, o_t.data_ptr(), d_t.data_ptr(), None, C.byref(s), None))):
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert rt.last_stats() == stats, f"{what}: the statistics changed"
        assert np.array_equal(rt.render(W, H), frame), f"{what}: the next frame differs"
        stats = rt.last_stats()
    torch.cuda.synchronize()
    assert (buf == -12345.5).all()
    for name, t in out.items():
        a = t.cpu().numpy()
        assert (a == np.array(SENTINEL[name]).astype(a.dtype)).all(), f"a refused call wrote array {name}"
    # ... and the call still works
    got = rt.surface_rays(o, d, planes=("hit", "next_dir"))
    assert set(got) == {"hit", "next_dir"} and got["hit"].sum() >= 1
