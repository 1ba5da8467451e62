"""Visibility buffers of a frame (include/rrt.h: rrt_render_visibility, rrt_render_visibility_device, rrt_pick) on the GPU: hit, t, u, v and triangle of every
primary ray against the oracle's intersector, the albedo plane against the oracle's shader, the planes against the library's own per-ray entry point, regions
and picks against the whole frame, the chain shortcut and the exactness guard of a moved eye, and the refusals.

Layout: every plane is [row][column][sub-sample]; `frame_dirs` gives the directions in the same shape, built by `pose_dirs` (the contract of rrt.h: rrt_camera).
All comparisons are bit for bit: the f64 planes are compared through their integer bits.

Albedo method: an oracle scene of the same arrays in which every material has ka = (1, 1, 1) and kr = 0, lit by Ambient(1.0) alone.  There
get_ray_colour is  texel * 1.0  clamped to u8 -- the texel itself -- for a hit and 0xFFFFFF for a miss (raytracer.rs:43-55, 67-111), so the oracle's own
shader states what rrt.h calls the albedo; the GPU raytracer keeps the real materials and lights.

Every comparison with the oracle asserts the fraction of rays that hit BY THE ORACLE'S ANSWERS, so an empty frame cannot pass.
"""
import numpy as np
import pytest

from bitwise import assert_same_arrays, same
from gpu_checks import CHAIN_LIGHTS, FORCED_MODES, POOL, chain_rrt_lights, chain_scene, oracle_for, plane_scene, plane_scene_data
from scenes import EYE3, H3, REGIONS, TARGET, W3, pose, posed, teapot_arrays, teapot_osc, visibility_frame3 as frame3  # noqa: F401  (fixtures: frame3, teapot_arrays, teapot_osc)
from surface_checks import assert_untraced_pixels, frame_dirs, traced_part, traced_pixels_in

pytestmark = pytest.mark.gpu

EYES = ((6.0, 3.0, -8.0), (9.0, 2.0, 1.0), (0.0, 9.0, -4.0))
GEOMETRY = ("hit", "t", "u", "v", "tri")
NO_TRI = 0xFFFFFFFF


def oracle_planes(osc, cam, w, h):
    """The oracle's intersector on every traced sub-sample ray: dict of [rows][cols][4] arrays."""
    d = frame_dirs(cam, w, h)
    flat = d.reshape(-1, 3)
    eye = cam["eye"]
    ans = list(POOL.map(lambda x: osc.intersect(eye, x), flat))
    shape = d.shape[:3]
    return dict(hit=np.array([a[0] for a in ans], np.uint8).reshape(shape), t=np.array([a[1] for a in ans], np.float64).reshape(shape),
                u=np.array([a[2] for a in ans], np.float64).reshape(shape), v=np.array([a[3] for a in ans], np.float64).reshape(shape),
                tri=np.array([a[4] for a in ans], np.uint32).reshape(shape))

_answers = {}


@pytest.fixture(scope="module")
def teapot_answers(rrt, teapot_osc):
    """(pose index, w, h) -> the oracle's planes, computed once per pose and size and shared by the tests; never modified."""
    def get(k, w, h):
        if (k, w, h) not in _answers:
            ref = oracle_planes(teapot_osc, pose(rrt, k, EYES), w, h)
            for a in ref.values():
                a.setflags(write=False)
            _answers[(k, w, h)] = ref
        return _answers[(k, w, h)]
    return get


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", range(4), ids=["creation pose"] + [f"eye {e}" for e in EYES])
@pytest.mark.parametrize("w,h", [(64, 48), (97, 61)])
def test_geometry_planes_equal_the_oracles_intersector(rrt, teapot, teapot_answers, w, h, k):
    cam = pose(rrt, k, EYES)
    ref = teapot_answers(k, w, h)
    n_rays = ref["hit"].size
    assert n_rays == {(64, 48): 12032, (97, 61): 22656}[(w, h)]
    frac = ref["hit"].mean()
    print(f"{w}x{h}, pose {k}: {n_rays} rays, {frac:.3f} of them hit by the oracle")
    assert frac >= 0.5, f"only {frac:.3f} of the compared rays hit (< 0.5)"
    for mode in FORCED_MODES + (None,):
        rt = posed(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), cam)
        planes = rt.visibility(w, h)
        assert set(planes) == set(rrt.PLANES) and all(a.shape == (h, w, 4) for a in planes.values())
        assert_same_arrays(traced_part(planes, w, h), ref, GEOMETRY, f"{w}x{h}, pose {k}, walk {mode}")
        assert_untraced_pixels(planes, w, h, f"{w}x{h}, pose {k}, walk {mode}")


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("k", (1, 0), ids=[f"eye {EYES[0]}", "creation pose"])
def test_albedo_plane_equals_the_oracles_shader(rrt, ob, teapot, teapot_arrays, teapot_answers, k):
    w, h = 64, 48
    cam = pose(rrt, k, EYES)
    flat_mats = [dict(m, ka=(1.0, 1.0, 1.0), kr=0.0) for m in teapot_arrays["materials"]]
    osc = oracle_for(ob, dict(teapot_arrays, materials=flat_mats), [rrt.Light.Ambient(1.0)])
    d = frame_dirs(cam, w, h)
    eye = cam["eye"]
    want = np.fromiter(POOL.map(lambda x: osc.get_ray_colour(eye, x), d.reshape(-1, 3)), np.uint32, d.size // 3).reshape(d.shape[:3])
    hit = teapot_answers(k, w, h)["hit"].astype(bool)
    assert (want[~hit] == 0xFFFFFF).all(), "the flat-lit oracle scene gives the background on every miss"
    frac, n_colours = hit.mean(), len(np.unique(want[hit]))
    print(f"pose {k}: {hit.size} rays, {frac:.3f} hit, {n_colours} distinct texels over materials {sorted(set(teapot_arrays['mat'][teapot_answers(k, w, h)['tri'][hit]].tolist()))}")
    assert frac >= 0.5 and n_colours >= 100, (frac, n_colours)
    for mode in FORCED_MODES:
        rt = posed(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), cam)            # the real materials, the default lights
        planes = rt.visibility(w, h, planes=("albedo", "hit"))
        assert_same_arrays(traced_part(planes, w, h), dict(albedo=want, hit=hit.astype(np.uint8)), ("albedo", "hit"), f"pose {k}, walk {mode}")
        assert_untraced_pixels(planes, w, h, f"pose {k}, walk {mode}")


# ------------------------------------------------------------------ 3


def test_whole_frame_equals_the_per_ray_entry_point(rrt, frame3):
    rt, full = frame3
    cam = rt.camera()
    d = frame_dirs(cam, W3, H3)
    hit, t, u, v, tri = rt.intersect_rays(np.tile(cam["eye"], (d.size // 3, 1)), d.reshape(-1, 3))
    own = dict(hit=hit.astype(np.uint8), t=t, u=u, v=v, tri=tri)
    assert own["hit"].mean() >= 0.5, own["hit"].mean()
    assert_same_arrays(traced_part(full, W3, H3), {n: a.reshape(d.shape[:3]) for n, a in own.items()}, GEOMETRY, "visibility vs intersect_rays")
    assert_untraced_pixels(full, W3, H3, "whole frame")
    seen = traced_part(full, W3, H3)
    assert (seen["albedo"][seen["hit"] == 0] == 0xFFFFFF).all(), "a traced ray that misses has the background's albedo"


@pytest.mark.parametrize("region", REGIONS)
def test_a_region_is_a_slice_of_the_frame(frame3, region):
    rt, full = frame3
    x0, y0, w, h = region
    part = rt.visibility(W3, H3, region=region)
    stats = rt.last_stats()
    assert_same_arrays(part, {n: a[y0:y0 + h, x0:x0 + w] for n, a in full.items()}, full.keys(), f"region {region}")
    assert (stats["width"], stats["height"]) == (W3, H3)
    assert stats["rays_primary"] == 4 * traced_pixels_in(region, W3, H3), (region, stats["rays_primary"])
    assert stats["kernel_ms"] > 0
    two = rt.visibility(W3, H3, region=region, planes=("t", "tri"))
    assert set(two) == {"t", "tri"}
    assert_same_arrays(two, part, ("t", "tri"), f"region {region}, t and tri only")


def test_pick_is_sub_sample_0_of_the_pixel(frame3):
    rt, full = frame3
    rng = np.random.default_rng(2024)
    pixels = [(int(x), int(y)) for x, y in zip(rng.integers(0, W3, 32), rng.integers(0, H3, 32))] + [(0, 0), (202, 116), (202, 5)]
    n_hit = 0
    for px, py in pixels:
        got = rt.pick(W3, H3, px, py)
        want = {n: full[n][py, px, 0] for n in full}
        assert got["hit"] == bool(want["hit"]) and got["tri"] == want["tri"] and got["albedo"] == want["albedo"], ((px, py), got, want)
        assert all(same(np.float64(got[n]), want[n]) for n in "tuv"), ((px, py), got, want)
        n_hit += got["hit"]
    assert rt.pick(W3, H3, 202, 5) == dict(hit=False, tri=NO_TRI, t=0.0, u=0.0, v=0.0, albedo=0)       # a column the reference never traces
    assert n_hit >= 8, n_hit


def test_device_tensors_equal_the_host_form(rrt, frame3):
    torch = pytest.importorskip("torch")
    rt, full = frame3
    kinds = dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, tri=torch.int32, albedo=torch.int32)
    for region in (None, REGIONS[4]):
        x0, y0, w, h = region or (0, 0, W3, H3)
        tensors = {n: torch.empty((h, w, 4), dtype=k, device="cuda") for n, k in kinds.items()}
        rt.visibility_into(tensors, W3, H3, region=region)
        torch.cuda.synchronize()
        got = {n: t.cpu().numpy().view(full[n].dtype) for n, t in tensors.items()}
        assert_same_arrays(got, {n: a[y0:y0 + h, x0:x0 + w] for n, a in full.items()}, full.keys(), f"visibility_into, region {region}")
    for name in kinds:                                                             # the host form with ONE plane asked for and five NULL, against the device form's
        one = rt.visibility(W3, H3, region=region, planes=(name,))
        assert set(one) == {name}
        assert_same_arrays(one, got, (name,), f"region {region}: plane {name} alone, host form vs visibility_into")


@pytest.mark.parametrize("frames_before", (0, 1, 2))
def test_the_tuning_state_is_untouched(rrt, teapot, frame3, frames_before):
    """render before and after visibility and pick calls: the same frame from the same variant, on a raytracer that has rendered this size once (the next
    frame is the measured one) and on one that has rendered it twice (measured already); on one that has rendered nothing, the visibility launch runs the
    variant the first frame then runs."""
    _, full = frame3
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.look_at(EYE3, TARGET)
    before, variant = None, None
    for _ in range(frames_before):
        before = rt.render(W3, H3)
        variant = rt.last_stats()["filter_variant"]
    got = rt.visibility(W3, H3)
    vis_variant = rt.last_stats()["filter_variant"]
    assert_same_arrays(got, full, full.keys(), f"after {frames_before} frames")
    rt.visibility(W3, H3, region=REGIONS[3], planes=("hit",))
    rt.pick(W3, H3, 100, 60)
    rt.visibility(64, 48)                                                          # another size must not become "the" size either
    after = rt.render(W3, H3)
    if frames_before:
        assert vis_variant == variant, (vis_variant, variant)
        assert np.array_equal(after, before)
        assert rt.last_stats()["filter_variant"] == variant, (rt.last_stats()["filter_variant"], variant)
    else:
        assert rt.last_stats()["filter_variant"] == vis_variant, "a visibility call before any frame runs the first frame's variant"


# ------------------------------------------------------------------ 4
def test_chain_shortcut_scene_equals_the_oracle(rrt, ob):
    w, h = 64, 48
    A, names = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    osc = oracle_for(ob, A, CHAIN_LIGHTS, eye)
    ref = oracle_planes(osc, cam, w, h)
    frac = ref["hit"].mean()
    hit_names = {names[i] for i in np.unique(ref["tri"][ref["hit"] == 1])}
    print(f"chain scene: {ref['hit'].size} rays, {frac:.3f} hit, triangles {sorted(hit_names)}")
    assert ref["hit"].size == 12032 and frac >= 0.2, frac
    assert {"c1", "c2", "big"} <= hit_names, hit_names
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode, shortcut in [(m, True) for m in FORCED_MODES] + [("bundle", False)]:
        rt = posed(rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*eye), box_filter=mode, chain_shortcut=shortcut), cam)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        planes = rt.visibility(w, h)
        assert_same_arrays(traced_part(planes, w, h), ref, GEOMETRY, f"chain scene, walk {mode}, shortcut {shortcut}")
        assert_untraced_pixels(planes, w, h, f"chain scene, walk {mode}")


# ------------------------------------------------------------------ 5
def test_the_guard_of_a_moved_eye(rrt):
    """The construction of test_the_guard_works_after_a_move (tests/test_gpu_camera.py): 60 triangles in planes through an eye that is not the creation
    origin, the view along the first plane.  With the guard the index walks agree with the reference-order (no_cull) walk on every ray."""
    w, h = 256, 192
    rng = np.random.default_rng(5)
    E = np.array([1.5, 1.0, -8.0])
    lights = rrt.default_lights()
    tris, planes = plane_scene(rng, E, 6, 10, 3000)
    sd = plane_scene_data(rrt, tris)
    cam = rrt.look_at(tuple(E), tuple(E + planes[0][0]))
    exact_rt = posed(rrt.RayTracer(sd, lights, no_cull=True), cam)
    exact = exact_rt.visibility(w, h)
    print(f"guard scene: {exact['hit'][1:].mean():.3f} of the rays hit")
    assert exact["hit"].any()
    for mode in (None,) + FORCED_MODES:
        rt = rrt.RayTracer(sd, lights, box_filter=mode)
        assert rt.last_stats()["origin_plane_triangles"] == 0
        rt.set_camera(**cam)
        assert rt.last_stats()["origin_plane_triangles"] == 60
        assert_same_arrays(rt.visibility(w, h), exact, exact.keys(), f"guard scene, walk {mode} vs no_cull")


# ------------------------------------------------------------------ 6
def test_refusals_leave_the_raytracer_as_it_was(rrt, teapot):
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = rt.render(W3, H3)
    for what, call in (("empty region", lambda: rt.visibility(W3, H3, region=(0, 0, 0, 1))),
                       ("region beyond the last column", lambda: rt.visibility(W3, H3, region=(200, 0, 8, 1))),
                       ("no plane", lambda: rt.visibility(W3, H3, planes=())),
                       ("pick outside the frame", lambda: rt.pick(64, 48, 64, 0))):
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert np.array_equal(rt.render(W3, H3), frame), what
