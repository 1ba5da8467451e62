"""Shading a frame from its kept surface buffers (include/rrt.h: rrt_shade_surface, rrt_shade_surface_device) and the material update of a living raytracer
(rrt_raytracer_set_materials, rrt_raytracer_get_materials) on the GPU.

The statement under test: shade of the planes rrt_render_surface wrote IS the frame rrt_render produces with the lights and materials in force now, bit for bit
-- with the kept mask of lit lights and, without it, with the depth-0 shadow rays walked again.  Frames are compared with each other bit for bit and with the
oracle's frames within COLOUR_TOL (the project's +-1 for pow).  Every comparison asserts its conditions BY THE ORACLE'S ANSWERS, so an empty frame cannot pass.
"""
import copy

import numpy as np
import pytest

from bitwise import assert_same_arrays, assert_same_bits
from gpu_checks import (ALL_MODES, CHAIN_LIGHTS, FORCED_MODES, ORIGIN, assert_frame_close, chain_rrt_lights, chain_scene, mix4, oracle_for, traced_rows)
from scenes import CREATION, EYE3, H3, MOVED_EYE, REGIONS, TARGET, W3, pose, shade_frame3 as frame3, teapot_arrays, teapot_osc  # noqa: F401  (fixtures: frame3, teapot_arrays, teapot_osc)
from shade_checks import MIRROR_ROOM_LIGHTS, assert_shade_is_render, mirror_room, oracle_frame, pixels_apart, soup_scene, without
from surface_checks import NO_MATERIAL, expected_planes, frame_dirs, shade, traced_cols, traced_part, traced_pixels_in

pytestmark = pytest.mark.gpu

W, H = 64, 48


@pytest.fixture(scope="module")
def default_frame(teapot_osc):
    """The oracle's 64x48 teapot frame in the creation pose with the default lights and materials (read-only)."""
    fb, _ = teapot_osc.render(W, H)
    fb.setflags(write=False)
    return fb


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h", [(64, 48), (97, 61)])
def test_the_frame_from_its_buffers(rrt, teapot, teapot_arrays, teapot_osc, w, h, k):
    cam = pose(rrt, k)
    ref, hit, mat = oracle_frame(teapot_osc, teapot_arrays, cam, w, h)
    n_mirror = int((mat == 3).sum())
    print(f"{w}x{h}, pose {k}: {hit.size} rays, {hit.mean():.3f} hit by the oracle, {n_mirror} of them the mirror (material 3, kr {teapot_arrays['materials'][3]['kr']})")
    assert teapot_arrays["materials"][3]["kr"] > 0.0
    assert n_mirror >= 1000, f"only {n_mirror} mirror sub-samples (< 1000)"
    assert hit.mean() >= 0.5 and not hit.all(), f"{hit.mean():.3f} of the rays hit: want at least 0.5 and some miss"
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        rt.set_camera(**cam)
        frame, _ = assert_shade_is_render(rt, w, h, f"{w}x{h}, pose {k}, walk {mode}")
        assert_frame_close(frame, ref, f"{w}x{h}, pose {k}, walk {mode}: render vs the oracle")


# ------------------------------------------------------------------ 2
def test_deep_reflection_chains(rrt, ob):
    """Mirrors in mirrors: the teapot's frames never get beyond one bounce at these sizes, a room of half mirrors does at every depth."""
    A = mirror_room()
    lights = [rrt.Light(k, i, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS]
    refs = {d: oracle_for(ob, A, lights, max_reflection_depth=d).render(W, H)[0] for d in (0, 1, 4, 5)}
    deep = int((refs[4] != refs[5]).sum())
    print(f"mirror room: the oracle's depth-0 and depth-1 frames differ on {int((refs[0] != refs[1]).sum())} pixels, depth 4 and depth 5 on {deep}")
    assert deep >= 500, f"the oracle's depth-4 and depth-5 frames differ on {deep} pixels only (< 500)"
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for depth in (0, 1, 5):
        for mode in FORCED_MODES:
            rt = rrt.RayTracer(sd, lights, max_reflection_depth=depth, box_filter=mode)
            frame, _ = assert_shade_is_render(rt, W, H, f"mirror room, depth {depth}, walk {mode}")
            assert_frame_close(frame, refs[depth], f"mirror room, depth {depth}, walk {mode}: render vs the oracle")


# ------------------------------------------------------------------ 3
def test_relighting_with_a_kept_mask(rrt, ob, teapot, teapot_arrays, default_frame):
    """Intensities and the direction of the directional light change, the point lights stay where they were: the kept mask is still the mask."""
    L, V = rrt.Light, rrt.Vector3d
    new = [L.Ambient(0.2), L.Point(0.7, V(-7.0, 1.0, -15.0)), L.Point(0.1, V(0.0, 1.0, -41.0)), L.Directional(0.6, V(3.0, -1.0, 10.0))]
    ref = oracle_for(ob, teapot_arrays, new).render(W, H)[0]
    apart = pixels_apart(default_frame, ref)
    print(f"relighting: the oracle's frames differ by more than 1 on {apart} of {ref.size} pixels")
    assert apart >= 600, f"the oracle's two frames differ by more than 1 on {apart} pixels only (< 600)"
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        old = rt.surface(W, H, visibility=("albedo",))
        rt.set_lights(new)
        fresh = rt.render(W, H)
        assert_same_bits(rt.shade(W, H, old), fresh, f"walk {mode}: shade of the old planes, mask included, vs a fresh render")
        assert_frame_close(fresh, ref, f"walk {mode}: render with the new lights vs the oracle")


# ------------------------------------------------------------------ 4
def test_a_moved_point_light(rrt, ob, teapot, teapot_arrays, teapot_osc, default_frame):
    """The mask is stale, the other four planes are not: shading without it walks the depth-0 shadow rays and gives the frame; shading with it does not."""
    new = rrt.default_lights()
    new[1] = rrt.Light.Point(0.4, rrt.Vector3d(6.0, 8.0, -12.0))
    osc = oracle_for(ob, teapot_arrays, new)
    ref = osc.render(W, H)[0]
    d = frame_dirs(CREATION, W, H)
    before, after = expected_planes(teapot_osc, teapot_arrays, rrt.default_lights(), ORIGIN, d), expected_planes(osc, teapot_arrays, new, ORIGIN, d)
    n_mask = int((before["hit"].astype(bool) & (before["lights"] != after["lights"])).sum())
    apart = pixels_apart(default_frame, ref)
    print(f"moved light: the mask changes on {n_mask} hit samples, the oracle's frames differ by more than 1 on {apart} pixels")
    assert n_mask >= 100 and apart >= 300, (n_mask, apart)
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        old = rt.surface(W, H, visibility=("albedo",))
        rt.set_lights(new)
        fresh = rt.render(W, H)
        assert_same_bits(rt.shade(W, H, without(old, "lights")), fresh, f"walk {mode}: shade of the old planes without the mask vs a fresh render")
        assert_frame_close(fresh, ref, f"walk {mode}: render with the moved light vs the oracle")
        stale = rt.shade(W, H, old)
        print(f"walk {mode}: shading with the stale mask differs from the frame on {int((stale != fresh).sum())} pixels")
        assert (stale != fresh).any(), f"walk {mode}: shading with the stale mask gives the fresh frame: the mask is not read"


# ------------------------------------------------------------------ 5
def test_the_planes_are_read_not_walked_again(rrt, teapot, teapot_arrays):
    lights = rrt.default_lights()
    n_mats = len(teapot_arrays["materials"])
    rt = rrt.RayTracer(teapot, lights)
    frame, planes = assert_shade_is_render(rt, W, H, "teapot")
    # two blocks of material indices beyond the table: WHITE there, nothing else moves
    edited = dict(planes, material=planes["material"].copy())
    assert (planes["material"][8:16, 8:16] != NO_MATERIAL).any() or (planes["material"][24:32, 24:32] != NO_MATERIAL).any(), "both blocks are misses already"
    edited["material"][8:16, 8:16] = 0xFFFFFFFF
    edited["material"][24:32, 24:32] = n_mats
    want = frame.copy()
    want[8:16, 8:16] = 0x00FFFFFF
    want[24:32, 24:32] = 0x00FFFFFF
    assert (want != frame).sum() >= 32, "the blocks lie on background pixels: the edit shows nothing"
    for what, p in (("with the mask", edited), ("without the mask", without(edited, "lights"))):
        assert_same_bits(rt.shade(W, H, p), want, f"material 0xFFFFFFFF and n_mats in two 8x8 blocks, {what}")
    # bits of the mask at and above n_lights are not lights
    noisy = dict(planes, lights=planes["lights"] | np.uint32((0xFFFFFFFF << len(lights)) & 0xFFFFFFFF))
    assert_same_bits(rt.shade(W, H, noisy), frame, "bits at and above n_lights set in the mask")
    # another albedo: the numpy shader of surface_checks on the same planes, wherever no sub-sample hits a mirror
    flat = dict(planes, albedo=np.full_like(planes["albedo"], 0x00C86432))
    got = rt.shade(W, H, flat)
    seen = traced_part(flat, W, H)
    kr = np.array([m["kr"] for m in teapot_arrays["materials"]] + [0.0])                  # (the last entry: a miss)
    mirror = kr[np.minimum(seen["material"], len(kr) - 1)] > 0.0
    ok = ~mirror.any(-1)
    n_hit_px = int((ok & (seen["material"] != NO_MATERIAL).any(-1)).sum())
    print(f"{int(ok.sum())} of {ok.size} traced pixels have no mirror sub-sample, {n_hit_px} of them with a hit")
    assert ok.sum() >= 512 and n_hit_px >= 256, (int(ok.sum()), n_hit_px)
    cols = shade(teapot_arrays, lights, frame_dirs(CREATION, W, H), seen, seen["albedo"])
    assert_frame_close(got[np.ix_(traced_rows(H), traced_cols(W))][ok], mix4(cols[ok]), "a constant albedo: shade vs the numpy shader on the same planes")
    assert (got[np.ix_(traced_rows(H), traced_cols(W))][ok] != frame[np.ix_(traced_rows(H), traced_cols(W))][ok]).sum() >= 128, "the albedo plane is not read"


# ------------------------------------------------------------------ 6


@pytest.mark.parametrize("region", REGIONS)
def test_a_region_is_a_slice_of_the_frame(rrt, frame3, region):
    torch = pytest.importorskip("torch")
    rt, frame, full = frame3
    x0, y0, w, h = region
    want = frame[y0:y0 + h, x0:x0 + w]
    if region == REGIONS[0]:
        miss = traced_part(full, W3, H3)["material"] == NO_MATERIAL
        assert 0.2 <= miss.mean() <= 0.8, miss.mean()
        assert (frame[0] == 0).all() and (frame[1] == 0).all() and (frame[:, -1] == 0).all() and (frame[2:, :-1] != 0).any(), "row 0, row 1 and the last column of an odd-sized frame are 0"
    part = rt.surface(W3, H3, region=region, visibility=("albedo",))
    assert_same_arrays(part, {n: a[y0:y0 + h, x0:x0 + w] for n, a in full.items()}, part.keys(), f"region {region}: planes")
    for what, p in (("with the mask", part), ("without the mask", without(part, "lights"))):
        assert_same_bits(rt.shade(W3, H3, p, region=region), want, f"region {region}, {what}")
        stats = rt.last_stats()
        assert (stats["width"], stats["height"], stats["rays_primary"]) == (W3, H3, 4 * traced_pixels_in(region, W3, H3)) and stats["kernel_ms"] > 0, (region, stats)
    # device form: exactly region.h x region.w elements are written, and every one of them
    G, SENTINEL = 64, -1515870811
    whole = torch.full((G + w * h + G,), SENTINEL, dtype=torch.int32, device="cuda")
    tensors = {n: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda().reshape(-1) for n, a in part.items()}
    rt.shade_into(whole[G:-G], tensors, W3, H3, region=region)
    torch.cuda.synchronize()
    a = whole.cpu().numpy()
    assert (a[:G] == SENTINEL).all() and (a[-G:] == SENTINEL).all(), f"region {region}: an element outside the output was written"
    assert not (a[G:-G] == SENTINEL).any(), f"region {region}: {int((a[G:-G] == SENTINEL).sum())} pixels were not written"
    assert_same_bits(a[G:-G].view(np.uint32).reshape(h, w), want, f"region {region}: shade_into vs the slice of the frame")


# ------------------------------------------------------------------ 7
def test_the_surface_offset_option_is_followed(rrt, ob, teapot, teapot_arrays, default_frame):
    ref = oracle_for(ob, teapot_arrays, rrt.default_lights(), surface_offset=1e-2).render(W, H)[0]
    n_diff = int((ref != default_frame).sum())
    print(f"surface_offset 1e-2: the oracle's frame differs from the default's on {n_diff} pixels")
    assert n_diff >= 1
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), surface_offset=1e-2, box_filter=mode)
        frame, _ = assert_shade_is_render(rt, W, H, f"surface_offset 1e-2, walk {mode}")
        assert_frame_close(frame, ref, f"surface_offset 1e-2, walk {mode}: render vs the oracle")


def test_a_soup_with_long_own_lists(rrt, ob, teapot_arrays):
    A = soup_scene(teapot_arrays)
    lights = rrt.default_lights()
    ref, hit, mat = oracle_frame(oracle_for(ob, A, lights), A, CREATION, W, H)
    print(f"soup: {hit.mean():.3f} of {hit.size} rays hit by the oracle, {int((mat == 3).sum())} of them the mirror")
    assert hit.mean() >= 0.5 and (mat == 3).sum() >= 500, (hit.mean(), int((mat == 3).sum()))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode, no_cull in [(m, False) for m in ALL_MODES] + [(None, True)]:
        rt = rrt.RayTracer(sd, lights, box_filter=mode, no_cull=no_cull)
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert len(supers) > 0
        if not no_cull:
            assert (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records (clusters.cpp): the kernels' group instantiation did not run"
        frame, _ = assert_shade_is_render(rt, W, H, f"soup, walk {mode}, no_cull {no_cull}")
        assert_frame_close(frame, ref, f"soup, walk {mode}, no_cull {no_cull}: render vs the oracle")


def test_the_chain_shortcut_scene(rrt, ob):
    A, names = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    ref, hit, _ = oracle_frame(oracle_for(ob, A, CHAIN_LIGHTS, eye), A, cam, W, H)
    print(f"chain scene: {hit.mean():.3f} of {hit.size} rays hit by the oracle; every triangle is a mirror (kr {A['materials'][0]['kr']})")
    assert hit.mean() >= 0.2 and A["materials"][0]["kr"] > 0.0, hit.mean()
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode, shortcut in [(m, True) for m in FORCED_MODES] + [("bundle", False)]:
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*eye), box_filter=mode, chain_shortcut=shortcut)
        rt.set_camera(**cam)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        frame, _ = assert_shade_is_render(rt, W, H, f"chain scene, walk {mode}, shortcut {shortcut}")
        assert_frame_close(frame, ref, f"chain scene, walk {mode}, shortcut {shortcut}: render vs the oracle")


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("frames_before", (0, 1, 2))
def test_the_tuning_state_is_untouched(rrt, teapot, frame3, frames_before):
    """render before and after shade calls: the same frame from the same variant, on a raytracer that has rendered this size once (the next frame is the measured
    one) and on one that has rendered it twice (measured already); on one that has rendered nothing, the shade launch runs the variant the first frame then runs."""
    _, frame, full = frame3
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.look_at(EYE3, TARGET)
    before, variant = None, None
    for _ in range(frames_before):
        before = rt.render(W3, H3)
        variant = rt.last_stats()["filter_variant"]
    got = rt.shade(W3, H3, full)
    stats = rt.last_stats()
    assert_same_bits(got, frame, f"after {frames_before} frames")
    assert (stats["width"], stats["height"], stats["rays_primary"]) == (W3, H3, 4 * traced_pixels_in(REGIONS[0], W3, H3)) and stats["kernel_ms"] > 0, stats
    x0, y0, w, h = REGIONS[3]
    rt.shade(W3, H3, {n: a[y0:y0 + h, x0:x0 + w] for n, a in full.items()}, region=REGIONS[3])
    small = rt.surface(64, 48, visibility=("albedo",))
    rt.shade(64, 48, small)                                                        # another size must not become "the" size either
    after = rt.render(W3, H3)
    assert_same_bits(after, frame, f"render after the shade calls, {frames_before} frames before them")
    if frames_before:
        assert stats["filter_variant"] == variant, (stats["filter_variant"], variant)
        assert np.array_equal(after, before)
        assert rt.last_stats()["filter_variant"] == variant, (rt.last_stats()["filter_variant"], variant)
    else:
        assert rt.last_stats()["filter_variant"] == stats["filter_variant"], "a shade call before any frame runs the first frame's variant"


# ------------------------------------------------------------------ 9
def test_refusals_leave_the_raytracer_as_it_was(rrt, frame3, teapot):
    import ctypes as C
    _, frame, full = frame3
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.look_at(EYE3, TARGET)
    region = REGIONS[4]
    x0, y0, w, h = region
    part = {n: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for n, a in full.items()}
    tiny = {n: np.ascontiguousarray(a[:1, :1]) for n, a in full.items()}
    L = rrt.lib()
    cs = rrt.CSurface(**{n: part[n].ctypes.data for n in ("point", "normal", "material", "lights")})
    cv = rrt.CVisibility(albedo=part["albedo"].ctypes.data)
    creg = rrt.CRegion(*region)
    fb = np.full((h, w), 0xA5A5A5A5, np.uint32)

    def raw(vis, planes, out):
        status = L.rrt_shade_surface(rt._h, W3, H3, C.byref(creg), vis, planes, out)
        if status != rrt.OK:
            raise rrt.RrtError(status, "rrt_shade_surface", (L.rrt_last_error_detail() or b"").decode())

    calls = [(f"plane {name} missing", (lambda name=name: rt.shade(W3, H3, without(part, name), region=region))) for name in ("point", "normal", "material", "albedo")]
    calls += [("a NULL output", lambda: raw(C.byref(cv), C.byref(cs), None)),
              ("a NULL visibility struct", lambda: raw(None, C.byref(cs), fb.ctypes.data_as(C.POINTER(C.c_uint32)))),
              ("a NULL surface struct", lambda: raw(C.byref(cv), None, fb.ctypes.data_as(C.POINTER(C.c_uint32)))),
              ("region beyond the last column", lambda: rt.shade(W3, H3, {n: np.repeat(a, 8, 1) for n, a in tiny.items()}, region=(200, 0, 8, 1))),
              ("region beyond the last row", lambda: rt.shade(W3, H3, {n: np.repeat(a, 2, 0) for n, a in tiny.items()}, region=(0, 116, 1, 2))),
              ("w == 0", lambda: rt.shade(W3, H3, {n: a[:, :0] for n, a in tiny.items()}, region=(0, 0, 0, 1))),
              ("a frame of no width", lambda: rt.shade(0, H3, tiny, region=(0, 0, 1, 1))),
              ("a frame of 2^31 pixels", lambda: rt.shade(65536, 32768, tiny, region=(0, 0, 1, 1)))]
    for what, call in calls:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert (fb == 0xA5A5A5A5).all(), f"{what}: the output of a refused call was written"
        assert_same_bits(rt.shade(W3, H3, part, region=region), frame[y0:y0 + h, x0:x0 + w], f"after the refusal of: {what}")
    assert_same_bits(rt.render(W3, H3), frame, "render after the refusals")


# ------------------------------------------------------------------ 10
def edited_table(materials):
    new = copy.deepcopy(materials)
    new[0]["kr"], new[0]["ns"] = 0.4, 20.0
    new[3]["kr"], new[3]["kd"] = 0.0, (0.2, 0.5, 0.8)
    return new


def from_arrays(rrt, A, materials, mode):
    return rrt.RayTracer.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], materials, A["textures"], rrt.default_lights(), box_filter=mode)


def test_a_new_material_table(rrt, ob, teapot, teapot_arrays, default_frame):
    A = teapot_arrays
    new = edited_table(A["materials"])
    ref = oracle_for(ob, dict(A, materials=new), rrt.default_lights()).render(W, H)[0]
    apart = pixels_apart(default_frame, ref)
    print(f"materials: the oracle's old and new frames differ by more than 1 on {apart} of {ref.size} pixels")
    assert apart >= 400, f"the oracle's old and new frames differ by more than 1 on {apart} pixels only (< 400)"
    swapped = copy.deepcopy(new)
    for a, b in ((0, 1), (1, 0)):
        swapped[a]["tex"], swapped[a]["bump"] = new[b]["tex"], new[b]["bump"]
    assert (swapped[0]["tex"], swapped[0]["bump"]) != (new[0]["tex"], new[0]["bump"])
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        assert rt.materials() == A["materials"]
        old_frame = rt.render(W, H)
        before = rt.surface(W, H, visibility=("albedo",))
        rt.set_materials(new)
        assert rt.materials() == new
        frame = rt.render(W, H)
        assert pixels_apart(frame, old_frame) >= 400, f"walk {mode}: the new table changes {pixels_apart(frame, old_frame)} pixels only"
        assert_same_bits(frame, from_arrays(rrt, A, new, mode).render(W, H), f"walk {mode}: render after set_materials vs a raytracer created with the new table")
        assert_frame_close(frame, ref, f"walk {mode}: render after set_materials vs the oracle")
        after = rt.surface(W, H, visibility=("albedo",))
        assert_same_arrays(after, before, before.keys(), f"walk {mode}: ka, kd, ks, ns and kr leave the planes as they were")
        assert_same_bits(rt.shade(W, H, before), frame, f"walk {mode}: shade of the planes taken before the edit vs the new frame")
        assert_same_bits(rt.shade(W, H, without(before, "lights")), frame, f"walk {mode}: the same without the mask")
        # tex and bump: albedo and normal planes follow, as on a raytracer created with that table
        rt.set_materials(swapped)
        assert rt.materials() == swapped
        fresh = from_arrays(rrt, A, swapped, mode)
        assert_same_bits(rt.render(W, H), fresh.render(W, H), f"walk {mode}: render after swapping tex and bump of materials 0 and 1")
        planes, want = rt.surface(W, H, visibility=("albedo",)), fresh.surface(W, H, visibility=("albedo",))
        assert_same_arrays(planes, want, want.keys(), f"walk {mode}: planes after swapping tex and bump of materials 0 and 1")
        assert not np.array_equal(planes["albedo"], before["albedo"]) and not np.array_equal(planes["normal"], before["normal"]), "the swap shows in neither albedo nor normal"


def test_a_refused_material_table_changes_nothing(rrt, teapot, teapot_arrays):
    new = edited_table(teapot_arrays["materials"])
    n_tex = len(teapot_arrays["textures"])
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.set_materials(new)
    frame = rt.render(W, H)
    bad_tex, bad_bump = copy.deepcopy(new), copy.deepcopy(new)
    bad_tex[2]["tex"] = n_tex
    bad_bump[1]["bump"] = -2
    calls = (("a table of three", lambda: rt.set_materials(new[:3])), ("a table of five", lambda: rt.set_materials(new + new[:1])),
             ("tex = n_tex", lambda: rt.set_materials(bad_tex)), ("bump = -2", lambda: rt.set_materials(bad_bump)),
             ("a NULL list", lambda: rrt._check(rrt.lib().rrt_raytracer_set_materials(rt._h, None, len(new)), "rrt_raytracer_set_materials")))
    for what, call in calls:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert rt.materials() == new, f"after the refusal of {what}"
        assert_same_bits(rt.render(W, H), frame, f"render after the refusal of {what}")
    n = rrt.lib().rrt_raytracer_get_materials(rt._h, (rrt.CMaterial * 2)(), 2, None)
    assert n == rrt.ERR_INVALID_ARG, "a capacity below the count with a non-NULL array"


def test_materials_of_a_host_setup_raytracer(rrt, teapot, teapot_arrays):
    new = edited_table(teapot_arrays["materials"])
    rt = rrt.RayTracer(teapot, rrt.default_lights(), host_setup=True)
    old = rt.render(W, H)
    rt.set_materials(new)
    assert rt.materials() == new
    frame = rt.render(W, H)
    assert pixels_apart(frame, old) >= 400
    assert_same_bits(frame, from_arrays(rrt, teapot_arrays, new, None).render(W, H), "host_setup: render after set_materials vs a raytracer created with the new table")
