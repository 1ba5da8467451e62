"""Device-resident ray batches and the batched occlusion query (include/rrt.h: rrt_occluded_rays, rrt_occluded_rays_device, rrt_intersect_rays_device,
rrt_get_ray_colours_device, rrt_tune_rays_device) on the GPU, against the CPU oracle's intersector and against the library's host forms.

occluded[i] is Some/None of Ray::intersect_with_octant_with_max_t(octree, 0, max_t) (ray.rs:104-168), not "any triangle on the segment": max_t bounds the
root's own list and the final comparison only.  Part 1 uses the scene of tests/test_gpu_shadow_exit.py, whose shadow rays tell the two rules apart; the
numbers of rays that must be occluded with and without max_t are asserted FROM THE ORACLE'S ANSWERS, so no test passes on an empty or trivial batch.
All comparisons are bit for bit.  Oracle answers are computed once per module and never modified.
"""
import numpy as np
import pytest

from bitwise import bits
from gpu_checks import ALL_MODES, FORCED_MODES, POOL, oracle_for, row_dirs, sample_rays, traced_rows
from lighting_scenes import (SHADOW_EXIT_CAMERA as CAMERA, SHADOW_EXIT_LIGHT_ABOVE as LIGHT_ABOVE, SHADOW_EXIT_LIGHT_ON_FLOOR as LIGHT_ON_FLOOR,
                             SHADOW_EXIT_OFFSET as OFFSET, shadow_exit_arrays as _arrays, shadow_exit_lights as _lights, shadow_exit_rays as _primary_rays)

pytestmark = pytest.mark.gpu

NO_TRI = 0xFFFFFFFF
# rays of part 1, counted with the CPU oracle: light -> (rays, occluded with max_t, occluded with +inf)
CLASS_COUNTS = {LIGHT_ABOVE: (109, 54, 109), LIGHT_ON_FLOOR: (109, 27, 32)}


def oracle_hits(osc, O, D, M=None):
    M = np.full(len(O), np.inf) if M is None else np.broadcast_to(np.asarray(M, np.float64), (len(O),))
    return np.fromiter(POOL.map(lambda i: osc.intersect(O[i], D[i], M[i])[0], range(len(O))), bool, len(O))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def shadow_scene(rrt, ob):
    A, _ = _arrays()
    return A, rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])


@pytest.fixture(scope="module")
def shadow_batches(ob, shadow_scene):
    """light -> (ro, dirv, max_t, oracle's occluded with max_t, oracle's occluded with +inf): the shadow ray of every primary ray of the shadow-exit
    scene, formed in numpy as test_gpu_shadow_exit._classify forms it."""
    A, _ = shadow_scene
    O, D = _primary_rays()
    out = {}
    for light in (LIGHT_ABOVE, LIGHT_ON_FLOOR):
        osc = oracle_for(ob, A, _lights(None, light), CAMERA)
        L = np.array(light)
        ro, dirv, max_t = np.empty_like(O), np.empty_like(O), np.empty(len(O))
        for i, (o, d) in enumerate(zip(O, D)):
            hit, t, _, _, _ = osc.intersect(o, d)
            assert hit, f"primary ray {i} misses"
            p = o + d * t
            ro[i] = p + np.array([0.0, 1.0, 0.0]) * OFFSET
            dirv[i] = L - p
            max_t[i] = float(np.sqrt(dirv[i][0] * dirv[i][0] + dirv[i][1] * dirv[i][1] + dirv[i][2] * dirv[i][2]))
        out[light] = frozen(ro, dirv, max_t, oracle_hits(osc, ro, dirv, max_t), oracle_hits(osc, ro, dirv)) + (osc,)
    return out


@pytest.fixture(scope="module")
def teapot_rays(rrt, teapot_oracle):
    """4068 rays on the teapot (primary, shadow-shaped with their max_t, reflection-shaped) and the oracle's hit for each."""
    O, D, M = sample_rays(teapot_oracle, 160, 120, 1500, np.random.default_rng(1), rrt.default_lights())
    return frozen(O, D, M, oracle_hits(teapot_oracle, O, D, M))


def on_device(torch, *arrays):
    return [torch.tensor(a, device="cuda") for a in arrays]


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("light", [LIGHT_ABOVE, LIGHT_ON_FLOOR], ids=["light_above_floor", "light_on_floor"])
def test_occlusion_follows_the_references_rule_not_any_hit(rrt, shadow_scene, shadow_batches, light):
    _, sd = shadow_scene
    ro, dirv, max_t, want, want_inf, osc = shadow_batches[light]
    n, n_occ, n_occ_inf = CLASS_COUNTS[light]
    print(f"\n[ray queries] light {light}: {len(ro)} rays, {int(want.sum())} occluded with max_t, {int(want_inf.sum())} with +inf (oracle)")
    assert (len(ro), int(want.sum()), int(want_inf.sum())) == (n, n_occ, n_occ_inf)
    for bad in (np.nan, 0.0, -1.0):
        assert not oracle_hits(osc, ro, dirv, bad).any(), f"oracle: max_t = {bad} must give None"
    for mode in ALL_MODES:
        rt = rrt.RayTracer(sd, _lights(rrt, light), rrt.Vector3d(*CAMERA), box_filter=mode)
        got = rt.occluded(ro, dirv, max_t)
        assert got.dtype == bool and np.array_equal(got, want), f"walk {mode}: rays {np.flatnonzero(got != want).tolist()} differ from the oracle"
        assert np.array_equal(got, rt.intersect_rays(ro, dirv, max_t)[0]), f"walk {mode}: occluded differs from intersect_rays' hit"
        got = rt.occluded(ro, dirv)
        assert np.array_equal(got, want_inf), f"walk {mode}, max_t = None: rays {np.flatnonzero(got != want_inf).tolist()} differ from the oracle"
        assert np.array_equal(got, rt.intersect_rays(ro, dirv)[0]), f"walk {mode}, max_t = None: occluded differs from intersect_rays' hit"
        for bad in (np.nan, 0.0, -1.0):
            assert not rt.occluded(ro, dirv, bad).any(), f"walk {mode}: max_t = {bad} must give 0 for every ray"


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("n", (1, 63, 64, 65, 109))
def test_tail_lanes_write_nothing_beyond_n(rrt, shadow_scene, shadow_batches, n):
    torch = pytest.importorskip("torch")
    _, sd = shadow_scene
    ro, dirv, max_t, want, _, _ = shadow_batches[LIGHT_ABOVE]
    d_o, d_d, d_m = on_device(torch, ro[:n], dirv[:n], max_t[:n])
    stream = torch.cuda.Stream()
    for mode in ALL_MODES:
        rt = rrt.RayTracer(sd, _lights(rrt, LIGHT_ABOVE), rrt.Vector3d(*CAMERA), box_filter=mode)
        full_hit, _, _, _, full_tri = rt.intersect_rays(ro, dirv, max_t)
        assert np.array_equal(full_hit, want)
        occ = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        hit = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        tri = torch.full((n + 64,), 0x1234567, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rt.occluded_into(d_o, d_d, occ[:n], d_m, stream=stream.cuda_stream)
        rt.intersect_rays_into(d_o, d_d, {"hit": hit[:n], "tri": tri[:n]}, d_m, stream=stream.cuda_stream)
        stream.synchronize()
        occ, hit, tri = occ.cpu().numpy(), hit.cpu().numpy(), tri.cpu().numpy().view(np.uint32)
        assert np.array_equal(occ[:n], want[:n].astype(np.uint8)), f"walk {mode}, n = {n}: occluded_into"
        assert np.array_equal(hit[:n], full_hit[:n].astype(np.uint8)) and np.array_equal(tri[:n], full_tri[:n]), f"walk {mode}, n = {n}: intersect_rays_into"
        assert (occ[n:] == 0xA5).all() and (hit[n:] == 0x5A).all() and (tri[n:] == 0x1234567).all(), f"walk {mode}, n = {n}: memory beyond the batch was written"


# ------------------------------------------------------------------ 3
def test_occlusion_in_a_deep_tree(rrt, teapot, teapot_rays):
    O, D, M, want = teapot_rays
    shadow = np.isfinite(M)
    print(f"\n[ray queries] teapot: {len(O)} rays, {int(want.sum())} hit; {int(shadow.sum())} shadow-shaped, {int(want[shadow].sum())} of them occluded (oracle)")
    assert int(want[shadow].sum()) >= 100 and int((~want[shadow]).sum()) >= 1000 and int(want.sum()) >= 1000
    for mode in ALL_MODES:
        got = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode).occluded(O, D, M)
        assert np.array_equal(got, want), f"walk {mode}: {int((got != want).sum())} of {len(O)} rays differ from the oracle, first {np.flatnonzero(got != want)[:8].tolist()}"


# ------------------------------------------------------------------ 4
def test_device_forms_equal_host_forms(rrt, teapot, teapot_rays):
    torch = pytest.importorskip("torch")
    O, D, M, want = teapot_rays
    n = len(O)
    d_o, d_d, d_m = on_device(torch, O, D, M)
    kinds = dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, tri=torch.int32)
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        host = dict(zip(kinds, rt.intersect_rays(O, D, M)))
        host["hit"] = host["hit"].astype(np.uint8)
        assert np.array_equal(host["hit"], want.astype(np.uint8))
        out = {k: torch.empty(n, dtype=dt, device="cuda") for k, dt in kinds.items()}
        rt.intersect_rays_into(d_o, d_d, out, d_m)
        torch.cuda.synchronize()
        for k in kinds:
            got = out[k].cpu().numpy().view(host[k].dtype)
            assert np.array_equal(bits(got), bits(host[k])), f"walk {mode}: plane {k} of intersect_rays_into differs on {int((bits(got) != bits(host[k])).sum())} rays"
        two = {k: torch.full((n,), 77, dtype=kinds[k], device="cuda") for k in ("t", "tri")}
        rt.intersect_rays_into(d_o, d_d, two, d_m)
        torch.cuda.synchronize()
        for k in two:
            assert np.array_equal(bits(two[k].cpu().numpy().view(host[k].dtype)), bits(host[k])), f"walk {mode}: plane {k} of intersect_rays_into with t and tri only"
        colours = torch.empty(n, dtype=torch.int32, device="cuda")
        rt.get_ray_colours_into(d_o, d_d, colours)
        occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        rt.occluded_into(d_o, d_d, occ, d_m)
        torch.cuda.synchronize()
        assert np.array_equal(colours.cpu().numpy().view(np.uint32), rt.get_ray_colours(O, D)), f"walk {mode}: get_ray_colours_into"
        assert np.array_equal(occ.cpu().numpy().astype(bool), rt.occluded(O, D, M)), f"walk {mode}: occluded_into"


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("mode", ("bundle", None))
def test_shadow_mask_of_a_frame_without_leaving_the_device(rrt, ob, shadow_scene, mode):
    torch = pytest.importorskip("torch")
    A, sd = shadow_scene
    w, h = 97, 61
    osc = oracle_for(ob, A, _lights(None, LIGHT_ABOVE), CAMERA)
    rt = rrt.RayTracer(sd, _lights(rrt, LIGHT_ABOVE), rrt.Vector3d(*CAMERA), box_filter=mode)
    rows, xs = traced_rows(h), np.arange(2 * (w // 2))
    dirs = np.zeros((h, w, 4, 3))
    for r in rows:
        dirs[r, :len(xs)] = row_dirs(w, h, r, xs).transpose(1, 0, 2)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = torch.from_numpy(dirs).to("cuda", non_blocking=False)
        planes = dict(hit=torch.empty((h, w, 4), dtype=torch.uint8, device="cuda"), t=torch.empty((h, w, 4), dtype=torch.float64, device="cuda"))
        rt.visibility_into(planes, w, h, stream=stream.cuda_stream)
        seen = planes["hit"].bool()                                            # pixels the reference never traces read as misses
        eye = torch.tensor(CAMERA, dtype=torch.float64, device="cuda"); light = torch.tensor(LIGHT_ABOVE, dtype=torch.float64, device="cuda")
        p = eye + d[seen] * planes["t"][seen][:, None]
        ro = (p + torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device="cuda") * OFFSET).contiguous()
        dirv = (light - p).contiguous()
        max_t = torch.sqrt((dirv * dirv).sum(1)).contiguous()
        mask = torch.empty(len(ro), dtype=torch.uint8, device="cuda")
        mask_inf = torch.empty(len(ro), dtype=torch.uint8, device="cuda")
        rt.occluded_into(ro, dirv, mask, max_t, stream=stream.cuda_stream)
        rt.occluded_into(ro, dirv, mask_inf, stream=stream.cuda_stream)
    stream.synchronize()                                                         # the one synchronisation
    n_traced = 4 * len(rows) * len(xs)
    ro, dirv, max_t, mask, mask_inf = ro.cpu().numpy(), dirv.cpu().numpy(), max_t.cpu().numpy(), mask.cpu().numpy().astype(bool), mask_inf.cpu().numpy().astype(bool)
    want, want_inf = oracle_hits(osc, ro, dirv, max_t), oracle_hits(osc, ro, dirv)    # of exactly the rays torch produced: its rounding is not under test
    print(f"\n[ray queries] walk {mode}: {n_traced} traced rays, {len(ro)} hit, {int(want.sum())} occluded, {int(want_inf.sum())} occluded at +inf (oracle)")
    assert n_traced == 22656 and len(ro) >= 6000 and int(want.sum()) >= 1500 and int((~want).sum()) >= 3000
    assert np.array_equal(mask, want), f"{int((mask != want).sum())} of {len(ro)} rays differ from the oracle"
    assert np.array_equal(mask_inf, want_inf), f"max_t = None: {int((mask_inf != want_inf).sum())} of {len(ro)} rays differ from the oracle"


# ------------------------------------------------------------------ 6
def test_tuning_on_a_device_batch(rrt, teapot, teapot_rays):
    torch = pytest.importorskip("torch")
    O, D, M, want = teapot_rays
    n = len(O)
    d_o, d_d, d_m = on_device(torch, O, D, M)
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    before = rt.render(160, 120)
    picked = rt.tune_rays(d_o, d_d, d_m)
    assert picked in (0, 1, 2)
    rt.occluded_into(d_o, d_d, occ, d_m)
    torch.cuda.synchronize()
    st = rt.last_stats()
    assert (st["filter_variant"], st["width"], st["height"]) == (picked, n, 1) and st["kernel_ms"] > 0, st
    assert np.array_equal(occ.cpu().numpy().astype(bool), want)
    assert np.array_equal(rt.render(160, 120), before), "tune_rays changed a frame"
    for k, mode in enumerate(FORCED_MODES):
        forced = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        assert forced.tune_rays(d_o, d_d, d_m) == k, mode
        forced.occluded_into(d_o, d_d, occ, d_m)
        torch.cuda.synchronize()
        assert forced.last_stats()["filter_variant"] == k, mode
