"""The kernels written after the fused frame kernel -- visibility, surface, shade, ambient, their per-ray forms, frame rays, the mix kernels and the frame by ray
generations (include/rrt.h) -- at the limits of the options: a viewport that is not (1, 1, 1), sixteen lights with every bit of the kept mask in use, reflection
depths 6 to 8, everything at once, and ambient occlusion at surface offsets other than 1e-4.

Comparisons of the library with itself are bit for bit.  point, normal, material, lights, hit, t, u, v and tri are compared bit for bit with
surface_checks.expected_planes (the reference's arithmetic in numpy around the oracle's intersector), frames with the oracle's frames within COLOUR_TOL (the
project's +-1 for pow), with the count of unequal pixels printed.  Every case first asserts, BY THE ORACLE'S ANSWERS, that it exercises what it names; the
minimums sit below counts made on the CPU with the oracle alone, which are written beside them.
"""
import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T, Rays, by_oracle as plane_by_oracle
from ambient_rays_checks import Fan, by_oracle as fan_by_oracle, open_of, standard_rot
from bitwise import assert_same_arrays, assert_same_bits, same
from gpu_checks import ALL_MODES, N_THREADS, POOL, assert_frame_close, mix4, oracle_for, oracle_pixels, traced_rows
from lighting_scenes import (CORRIDOR_ORIGIN, SHADOW_ORIGIN, SIXTEEN, _corridor_lights, _corridor_scene, _shadow_box_mirror_scene, _shadow_box_scene, lights_of)
from scenes import CREATION, IDENTITY, TARGET, rays_of, teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import assert_shade_is_render
from shade_rays_checks import OUTPUTS, chain_levels, oracle_colours, without_mask
from surface_checks import EXPECTED, NO_MATERIAL, assert_untraced_pixels, expected_planes, frame_dirs, lights_added_up, shade, traced_cols, traced_part
from wavefront_checks import ARRAYS, ORDERS, ROWS, alive_entries, assert_wavefront_is_render, expected_rays

pytestmark = pytest.mark.gpu

W, H = 64, 48
DEFAULT_VIEWPORT = (1.0, 1.0, 1.0)
VISIBLE = ("hit", "t", "u", "v", "tri")                          # the visibility planes expected_planes states
RECORDS = ("hit", "t", "u", "v", "tri", "albedo", "point", "normal", "material", "lights")   # what rrt_render_surface gives with its visibility planes
REGION = {(64, 48): (6, 9, 21, 18), (97, 61): (90, 1, 7, 58), (32, 24): (5, 3, 18, 14)}      # cut off the 4x4 tile boundaries, a tile straddling each edge


def traced_region(w, h):
    """The pixels the reference traces, as a region: its rows-order ray batch is the traced sub-samples in the planes' index order, none of them dead."""
    return (0, int(traced_rows(h)[0]), 2 * (w // 2), h - int(traced_rows(h)[0]))


def oracle_frame(osc, cam, w, h, what, viewport=DEFAULT_VIEWPORT, neighbour=False):
    """The oracle's frame in any pose and viewport from gpu_checks.oracle_pixels (which asserts that half the pixels see something): 0 where the reference never
    traces.  neighbour: a frame that is only counted against another one -- the same colours and Color::mix without oracle_pixels' second pass.  Read-only."""
    frame = np.zeros((h, w), np.uint32)
    if neighbour:
        d = frame_dirs(cam, w, h, viewport)
        frame[np.ix_(traced_rows(h), traced_cols(w))] = mix4(oracle_colours(osc, cam["eye"], d).reshape(-1, 4)).reshape(d.shape[:2])
    else:
        frame[np.ix_(traced_rows(h), traced_cols(w))] = oracle_pixels(osc, cam, w, h, traced_rows(h), traced_cols(w), what, viewport)
    frame.setflags(write=False)
    return frame


def unequal(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def tracer(rrt, sd, lights, mode, cam=None, **opt):
    """A raytracer in the walk `mode` and the pose `cam`; max_reflection_depth is kept as an attribute for wavefront_checks.assert_wavefront_is_render."""
    rt = rrt.RayTracer(sd, lights, rrt.Vector3d(*(cam or CREATION)["eye"]), box_filter=mode, **opt)
    rt.max_reflection_depth = opt.get("max_reflection_depth", 5)
    if cam is not None:
        rt.set_camera(**cam)
    return rt


def check_planes(rt, want, w, h, what):
    """rt's surface planes, with the hit plane, are `want` on the traced pixels and the never-traced values elsewhere.  Returns the planes."""
    got = rt.surface(w, h, visibility=("hit",))
    assert_same_arrays(traced_part(got, w, h), want, EXPECTED, what)
    assert_untraced_pixels(got, w, h, what)
    return got


def check_frame_rays_are_the_planes(rt, w, h, what, names=RECORDS):
    """rrt_surface_rays of the rows-order frame batch, max_t included, equals the flattened planes of rrt_render_surface, as
    test_gpu_wavefront.py::test_the_frame_rays_are_the_rays_the_frame_kernels_trace states it.  Returns (the rays, the records)."""
    planes = rt.surface(w, h, visibility=RECORDS[:6])
    rays = rt.frame_rays(w, h)
    got = rt.surface_rays(rays["origins"], rays["dirs"], rays["max_t"], planes=RECORDS)
    alive = alive_entries(w, h, None, ROWS)
    hit = planes["hit"].reshape(-1).astype(bool)
    assert not hit[~alive].any(), f"{what}: a pixel the reference never traces has a hit"
    for name in names:
        flat = planes[name].reshape(got[name].shape)
        sel = alive if name == "albedo" else slice(None)         # (albedo of a never-traced pixel: 0 in a plane, the miss value in a ray record, rrt.h)
        assert_same_arrays({name: got[name][sel]}, {name: flat[sel]}, (name,), f"{what}: surface_rays(frame_rays) vs the surface planes")
    return rays, got


def wavefront_frames(rt, w, h, frame, what):
    for order in ORDERS:
        assert_same_bits(rt.render_wavefront(w, h, order=order), frame, f"{what}, order {order}: render_wavefront vs render")
        x0, y0, rw, rh = REGION[(w, h)]
        assert_same_bits(rt.render_wavefront(w, h, region=REGION[(w, h)], order=order), frame[y0:y0 + rh, x0:x0 + rw], f"{what}, order {order}, region {REGION[(w, h)]}")


# ------------------------------------------------------------------ A: the viewport in every kernel that forms a primary ray
VIEWPORTS = ((1.5, 1.0, 1.25), (1.3, 0.7, 1.1))
TEAPOT_EYE = (9.0, 2.0, 1.0)
SIZES = ((64, 48), (97, 61))
POSE_IDS = ["creation pose", f"eye {TEAPOT_EYE}"]
VIEWPORT_IDS = [f"viewport {v}" for v in VIEWPORTS]
_teapot = {}


def teapot_pose(rrt, k):
    return CREATION if k == 0 else rrt.look_at(TEAPOT_EYE, TARGET)


@pytest.fixture(scope="module")
def teapot_oracle_answers(rrt, ob, teapot_arrays):
    """(what, viewport, pose index, w, h) -> the oracle's answer, computed once and shared by the tests (read-only): "planes" = expected_planes of the frame's
    rays, "hit" = hit or miss of those rays alone, "frame" = the oracle's frame."""
    def get(what, vp, k, w, h):
        key = (what, vp, k, w, h)
        if key not in _teapot:
            cam = teapot_pose(rrt, k)
            osc = oracle_for(ob, teapot_arrays, rrt.default_lights(), cam["eye"])
            if what == "planes":
                _teapot[key] = expected_planes(osc, teapot_arrays, rrt.default_lights(), cam["eye"], frame_dirs(cam, w, h, vp))
            elif what == "hit":
                d = frame_dirs(cam, w, h, vp)
                _teapot[key] = np.fromiter(POOL.map(lambda v: osc.intersect(cam["eye"], v)[0], d.reshape(-1, 3)), bool, d.size // 3).reshape(d.shape[:-1])
            elif k == 0:
                _teapot[key] = osc.render(w, h, viewport=vp, n_threads=N_THREADS)[0]
                _teapot[key].setflags(write=False)
            else:
                _teapot[key] = oracle_frame(osc, cam, w, h, f"teapot {w}x{h}, pose {k}, viewport {vp}", vp)
        return _teapot[key]
    return get


@pytest.mark.parametrize("k", (0, 1), ids=POSE_IDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("vp", VIEWPORTS, ids=VIEWPORT_IDS)
def test_viewport_rays_and_planes(rrt, teapot, teapot_oracle_answers, vp, w, h, k):
    """frame_rays in both orders, of the frame and of a region, is the restated batch; surface_rays of it is the surface planes; visibility, surface and pick are
    expected_planes of the restated directions."""
    cam = teapot_pose(rrt, k)
    ref = teapot_oracle_answers("planes", vp, k, w, h)
    hit = ref["hit"].astype(bool)
    moved = unequal(hit, teapot_oracle_answers("hit", DEFAULT_VIEWPORT, k, w, h))
    print(f"{w}x{h}, pose {k}, viewport {vp}: {hit.size} rays, {int(hit.sum())} hit by the oracle; hit differs from the default viewport's on {moved} rays")
    assert hit.mean() >= MIN_HIT_FRACTION and not hit.all(), f"{hit.mean():.3f} of the rays hit: want at least {MIN_HIT_FRACTION} and some miss"
    assert moved >= hit.size // 10, f"hit differs from the default viewport's on {moved} of {hit.size} rays only: the viewport shows nothing"
    rows, rng = traced_rows(h), np.random.default_rng(w * h + k)
    pixels = [(int(x), int(y)) for x, y in zip(rng.integers(0, 2 * (w // 2), 24), rng.integers(rows[0], h, 24))]
    assert sum(bool(ref["hit"][y - rows[0], x, 0]) for x, y in pixels) >= 6, "fewer than 6 of the picked pixels see anything"
    for mode in ALL_MODES:
        what = f"{w}x{h}, pose {k}, viewport {vp}, walk {mode}"
        rt = tracer(rrt, teapot, rrt.default_lights(), mode, cam, viewport=vp)
        for order in ORDERS:
            for region in (None, REGION[(w, h)]):
                assert_same_arrays(rt.frame_rays(w, h, region=region, order=order), expected_rays(cam, w, h, region, order, viewport=vp), ARRAYS,
                                    f"{what}, order {order}, region {region}: frame_rays vs the restatement")
        check_frame_rays_are_the_planes(rt, w, h, what)
        check_planes(rt, ref, w, h, what)
        assert_same_arrays(traced_part(rt.visibility(w, h, planes=VISIBLE), w, h), ref, VISIBLE, f"{what}: visibility")
        for px, py in pixels:
            got, want = rt.pick(w, h, px, py), {n: ref[n][py - rows[0], px, 0] for n in VISIBLE}
            assert got["hit"] == bool(want["hit"]) and got["tri"] == want["tri"] and all(same(np.float64(got[n]), want[n]) for n in "tuv"), \
                f"{what}: pick of pixel ({px}, {py}) gives {got}, the oracle {want}"


MIN_HIT_FRACTION = 0.5                                           # (the oracle counts 0.600 to 0.659 over the eight cases, and 0.135 to 0.167 of the rays with another hit/miss)


@pytest.mark.parametrize("k", (0, 1), ids=POSE_IDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("vp", VIEWPORTS, ids=VIEWPORT_IDS)
def test_viewport_frames(rrt, teapot, teapot_oracle_answers, vp, w, h, k):
    """render is the oracle's frame of that viewport (creation pose: oracle.render(viewport=); moved: oracle_pixels(viewport=)), and shading the surface planes,
    the frame by ray generations, the progressive frame and the gathered tiles of 2 and 3 ranks are render's frame."""
    torch = pytest.importorskip("torch")
    cam = teapot_pose(rrt, k)
    ref = teapot_oracle_answers("frame", vp, k, w, h)
    teeth = unequal(ref, teapot_oracle_answers("frame", DEFAULT_VIEWPORT, k, w, h))
    print(f"{w}x{h}, pose {k}: the oracle's frame of viewport {vp} differs from the default viewport's on {teeth} of {w * h} pixels")
    assert 4 * teeth >= w * h, f"the oracle's frame of viewport {vp} differs from the default viewport's on {teeth} of {w * h} pixels (less than a quarter)"
    for mode in ALL_MODES:
        what = f"{w}x{h}, pose {k}, viewport {vp}, walk {mode}"
        rt = tracer(rrt, teapot, rrt.default_lights(), mode, cam, viewport=vp)
        frame, _ = assert_shade_is_render(rt, w, h, what)
        d = assert_frame_close(frame, ref, f"{what}: render vs the oracle")
        print(f"{what}: {int((d > 0).sum())} pixels not bit-equal to the oracle")
        wavefront_frames(rt, w, h, frame, what)
        assert_same_bits(rt.render_progressive(w, h, chunk_rows=13), frame, f"{what}: render_progressive vs render")
        for world in (2, 3):
            gathered = torch.empty((world, rrt.tiles_per_rank(w, h, world) * 64), dtype=torch.int32, device="cuda")
            for r in range(world):
                rt.render_tiles_into(gathered[r], w, h, r, world)
            fb = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rt.detile_into(gathered, fb, w, h, world)
            torch.cuda.synchronize()
            assert_same_bits(fb.cpu().numpy().view(np.uint32), frame, f"{what}: the tiles of {world} ranks, detiled, vs render")


# ------------------------------------------------------------------ B: sixteen lights through the kept masks
SHADOW_TARGET = (0.0, 1.0, 2.0)
SHADOW_EYE = (5.0, 6.0, -9.0)                                    # off every triangle's plane (x = -6, 2, 4; y = 0, 2, 7; z = 3, 5, 8)
SHADOW_IDS = ["creation pose", f"eye {SHADOW_EYE}"]
# minimums of the kept masks of SIXTEEN on the shadow box at 64x48, by the oracle.         it counts:    creation pose   eye (5, 6, -9)
MIN_FULL = 300                                                   # hits with mask 0xFFFF                   664             708
MIN_ALL_BUT_LAST = 15                                            # hits with mask 0x7FFF                   36              59
MIN_CTZ_VALUES, MIN_PER_CTZ_VALUE = 8, 30                        # values of ctz(~mask) with 30 hits each  10              10
MIN_DISTINCT = 40                                                # distinct masks                          77              81
MIN_PIXELS_OF_LIGHT_15 = 100                                     # pixels the sixteenth light changes      213             215
_shadow = {}


def shadow_pose(rrt, k):
    return dict(eye=SHADOW_ORIGIN, **IDENTITY) if k == 0 else rrt.look_at(SHADOW_EYE, SHADOW_TARGET)


def assert_mask_minimums(ref, what):
    """The masks of the oracle's answers `ref` use all sixteen bits: see the constants.  Prints the counts."""
    hit = ref["hit"].astype(bool)
    m = ref["lights"][hit]
    values, counts = np.unique(lights_added_up(m), return_counts=True)
    n_full, n_last, n_values, n_distinct = int((m == 0xFFFF).sum()), int((m == 0x7FFF).sum()), int((counts >= MIN_PER_CTZ_VALUE).sum()), len(np.unique(m))
    print(f"{what}: {hit.size} rays, {int(hit.sum())} hits; mask 0xFFFF on {n_full}, 0x7FFF on {n_last}, {n_distinct} distinct masks; ctz(~mask): "
          f"{dict(zip(values.tolist(), counts.tolist()))}")
    assert n_full >= MIN_FULL, f"{what}: mask 0xFFFF on {n_full} hits (< {MIN_FULL})"
    assert n_last >= MIN_ALL_BUT_LAST, f"{what}: mask 0x7FFF on {n_last} hits (< {MIN_ALL_BUT_LAST})"
    assert n_values >= MIN_CTZ_VALUES, f"{what}: {n_values} values of ctz(~mask) occur on {MIN_PER_CTZ_VALUE} hits or more (< {MIN_CTZ_VALUES})"
    assert n_distinct >= MIN_DISTINCT, f"{what}: {n_distinct} distinct masks (< {MIN_DISTINCT})"


@pytest.fixture(scope="module")
def shadow_box(rrt, ob):
    """(SceneData, arrays, the sixteen lights, get): get(what, pose index, n_lights = 16) -> the oracle's answer for the shadow box with the first n_lights of
    SIXTEEN at 64x48, computed once (read-only): "planes" = expected_planes of the frame's rays, "frame" = the oracle's frame."""
    sd, A = _shadow_box_scene(rrt)
    lights = lights_of(rrt, SIXTEEN)

    def get(what, k, n_lights=16):
        key = (what, k, n_lights)
        if key not in _shadow:
            cam = shadow_pose(rrt, k)
            osc = oracle_for(ob, A, lights[:n_lights], cam["eye"])
            if what == "planes":
                _shadow[key] = expected_planes(osc, A, lights[:n_lights], cam["eye"], frame_dirs(cam, W, H))
            elif k == 0:
                _shadow[key] = osc.render(W, H, n_threads=N_THREADS)[0]
                _shadow[key].setflags(write=False)
            else:
                _shadow[key] = oracle_frame(osc, cam, W, H, f"shadow box, pose {k}, {n_lights} lights")
        return _shadow[key]
    return sd, A, lights, get


def assert_sixteen_has_teeth(get, k):
    assert_mask_minimums(get("planes", k), f"shadow box, pose {k}")
    n = unequal(get("frame", k), get("frame", k, 15))
    print(f"shadow box, pose {k}: the oracle's frames of 16 and of the first 15 lights differ on {n} pixels")
    assert n >= MIN_PIXELS_OF_LIGHT_15, f"shadow box, pose {k}: the oracle's frames of 16 and of the first 15 lights differ on {n} pixels (< {MIN_PIXELS_OF_LIGHT_15})"


@pytest.mark.parametrize("k", (0, 1), ids=SHADOW_IDS)
def test_sixteen_lights_in_the_kept_masks(rrt, shadow_box, k):
    """The lights plane of surface and the lights array of surface_rays(frame_rays) are the oracle's masks, with the other planes."""
    sd, A, lights, get = shadow_box
    assert_sixteen_has_teeth(get, k)
    ref = get("planes", k)
    for mode in ALL_MODES:
        what = f"shadow box, 16 lights, pose {k}, walk {mode}"
        rt = tracer(rrt, sd, lights, mode, shadow_pose(rrt, k))
        check_planes(rt, ref, W, H, what)
        _, rec = check_frame_rays_are_the_planes(rt, W, H, what)
        alive = alive_entries(W, H, None, ROWS)
        assert_same_arrays({"lights": rec["lights"][alive]}, {"lights": ref["lights"].reshape(-1)}, ("lights",), f"{what}: lights of surface_rays(frame_rays) vs the oracle")


@pytest.mark.parametrize("k", (0, 1), ids=SHADOW_IDS)
def test_sixteen_lights_shaded_from_the_kept_masks(rrt, shadow_box, k):
    """render is the oracle's frame; shade with and without the mask, shade_rays with and without it (mixed by mix_pixels) and the frame by ray generations are
    render's frame; the numpy shader on the planes reproduces it (no mirror in this scene); junk in bits 16 to 31 of the mask changes nothing."""
    sd, A, lights, get = shadow_box
    assert_sixteen_has_teeth(get, k)
    cam, ref = shadow_pose(rrt, k), get("frame", k)
    ix = np.ix_(traced_rows(H), traced_cols(W))
    for mode in ALL_MODES:
        what = f"shadow box, 16 lights, pose {k}, walk {mode}"
        rt = tracer(rrt, sd, lights, mode, cam)
        frame, planes = assert_shade_is_render(rt, W, H, what)
        d = assert_frame_close(frame, ref, f"{what}: render vs the oracle")
        print(f"{what}: {int((d > 0).sum())} pixels not bit-equal to the oracle")
        wavefront_frames(rt, W, H, frame, what)
        # per ray: the records of the frame's rays, shaded with and without their masks, mixed per pixel
        rays = rt.frame_rays(W, H)
        rec = rt.surface_rays(rays["origins"], rays["dirs"], rays["max_t"])
        for name, p in (("with the mask", rec), ("without the mask", without_mask(rec))):
            colours = rt.shade_rays(rays["dirs"], p)["colour"]
            assert_same_bits(rt.mix_pixels(colours, W, H), frame, f"{what}: mix_pixels(shade_rays {name}) vs render")
        # bits 16 to 31 are no lights, in a plane and in a ray record
        junk = np.uint32(0xFFFF0000) & (np.arange(planes["lights"].size, dtype=np.uint32).reshape(planes["lights"].shape) * np.uint32(0x9E3779B1))
        junk |= np.uint32(0x00010000)                                                             # (bit 16, the one above the last light, everywhere)
        assert_same_bits(rt.shade(W, H, dict(planes, lights=planes["lights"] | junk)), frame, f"{what}: shade with junk in bits 16 to 31 of the mask")
        colours = rt.shade_rays(rays["dirs"], dict(rec, lights=rec["lights"] | junk.reshape(-1)))["colour"]
        assert_same_bits(rt.mix_pixels(colours, W, H), frame, f"{what}: shade_rays with junk in bits 16 to 31 of the mask")
        # the planes suffice: numpy Phong over the lights [0, ctz(~mask)) is the frame
        seen = traced_part(planes, W, H)
        assert not any(m["kr"] > 0.0 for m in A["materials"]), "the shadow box has a mirror: the numpy shader does not follow reflections"
        cols = shade(A, lights, frame_dirs(cam, W, H), seen, seen["albedo"])
        assert (seen["material"] != NO_MATERIAL).sum() >= 6000, f"{what}: only {int((seen['material'] != NO_MATERIAL).sum())} hits in the planes"
        assert_frame_close(mix4(cols.reshape(-1, 4)).reshape(cols.shape[:2]), frame[ix], f"{what}: the numpy shader on the planes vs render")


@pytest.mark.parametrize("k", (0, 1), ids=SHADOW_IDS)
def test_set_lights_between_sixteen_fifteen_and_none(rrt, shadow_box, k):
    """One handle through SIXTEEN, its first 15, [] and SIXTEEN again: every frame and every mask plane is a fresh raytracer's, shade of the planes is render, and
    without lights every mask is 0."""
    sd, A, lights, get = shadow_box
    assert_sixteen_has_teeth(get, k)
    cam = shadow_pose(rrt, k)
    for mode in ALL_MODES:
        rt = tracer(rrt, sd, lights[:3], mode, cam)
        seen = []
        for n in (16, 15, 0, 16):
            what = f"shadow box, pose {k}, walk {mode}, set_lights to {n} lights"
            rt.set_lights(lights[:n])
            fresh = tracer(rrt, sd, lights[:n], mode, cam)
            frame, planes = assert_shade_is_render(rt, W, H, what)
            assert_same_bits(frame, fresh.render(W, H), f"{what}: render vs a fresh raytracer's")
            want = fresh.surface(W, H, visibility=("albedo",))
            assert_same_arrays(planes, want, want.keys(), f"{what}: planes vs a fresh raytracer's")
            if n:
                assert_same_arrays(traced_part(planes, W, H), get("planes", k, n), ("lights",), f"{what}: the lights plane vs the oracle")
                assert_frame_close(frame, get("frame", k, n), f"{what}: render vs the oracle")
            else:
                assert (planes["lights"] == 0).all(), f"{what}: {int((planes['lights'] != 0).sum())} masks are not 0"
                hit = traced_part(planes, W, H)["material"] != NO_MATERIAL
                assert ((frame[np.ix_(traced_rows(H), traced_cols(W))] == 0) == hit.all(-1)).all(), f"{what}: without lights exactly the pixels whose four rays hit are black"
            seen.append(frame)
        assert (seen[0] == seen[3]).all() and (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any(), f"walk {mode}: the light lists do not show in the frames"


# ------------------------------------------------------------------ C: depths 6, 7 and 8 beyond the fused kernel
DEPTH_SIZES = ((64, 48), (32, 24))
MIN_DEPTH_TEETH = 20                                             # pixels of 64x48 between depths 5/6, 6/7, 7/8 (the oracle counts 100, 59, 41; at 32x24: 26, 20, 15)
MIN_ALIVE_AT_LEVEL_8 = 100                                       # rays of the 64x48 frame still reflecting at level 8 (the oracle counts 147)
CORRIDOR_CAM = dict(eye=CORRIDOR_ORIGIN, **IDENTITY)
_corridor = {}


@pytest.fixture(scope="module")
def corridor(rrt, ob):
    """(SceneData, arrays, lights, get): get(depth, w, h) -> (the oracle scene at that depth, its frame), computed once; the frame is read-only."""
    sd, A = _corridor_scene(rrt)
    lights = _corridor_lights(rrt)

    def get(depth, w, h):
        if (depth, w, h) not in _corridor:
            osc = oracle_for(ob, A, lights, CORRIDOR_ORIGIN, max_reflection_depth=depth)
            frame = osc.render(w, h, n_threads=N_THREADS)[0]
            frame.setflags(write=False)
            _corridor[(depth, w, h)] = (osc, frame)
        return _corridor[(depth, w, h)]
    return sd, A, lights, get


def assert_depth_teeth(get):
    teeth = [unequal(get(d, W, H)[1], get(d + 1, W, H)[1]) for d in (5, 6, 7)]
    print(f"corridor {W}x{H}: the oracle's frames of depths 5/6, 6/7 and 7/8 differ on {teeth} pixels")
    assert min(teeth) >= MIN_DEPTH_TEETH, f"corridor {W}x{H}: the oracle's frames of depths 5/6, 6/7 and 7/8 differ on {teeth} pixels (< {MIN_DEPTH_TEETH})"


@pytest.mark.parametrize("w,h", DEPTH_SIZES)
@pytest.mark.parametrize("depth", (6, 7, 8))
def test_deep_reflections_from_kept_buffers_and_by_generations(rrt, corridor, depth, w, h):
    torch = pytest.importorskip("torch")
    sd, A, lights, get = corridor
    assert_depth_teeth(get)
    osc, ref = get(depth, w, h)
    shallower = unequal(ref, get(depth - 1, w, h)[1])
    print(f"corridor {w}x{h}: the oracle's frames of depths {depth - 1} and {depth} differ on {shallower} pixels")
    assert shallower >= 10, f"corridor {w}x{h}: the oracle's frames of depths {depth - 1} and {depth} differ on {shallower} pixels (< 10)"
    O, D = rays_of(CORRIDOR_CAM, w, h)
    ray_ref = oracle_colours(osc, O, D)
    for mode in ALL_MODES:
        what = f"corridor {w}x{h}, depth {depth}, walk {mode}"
        rt = tracer(rrt, sd, lights, mode, CORRIDOR_CAM, max_reflection_depth=depth)
        frame, _ = assert_shade_is_render(rt, w, h, what)
        d = assert_frame_close(frame, ref, f"{what}: render vs the oracle")
        print(f"{what}: {int((d > 0).sum())} pixels not bit-equal to the oracle")
        assert_frame_close(rt.get_ray_colours(O, D), ray_ref, f"{what}: get_ray_colours of the frame's rays vs the oracle's get_ray_colour")
        assert_same_bits(assert_wavefront_is_render(rrt, torch, rt, w, h, REGION[(w, h)], what, mode), frame, f"{what}: the frame of assert_wavefront_is_render")


def test_every_level_of_a_depth_8_chain(rrt, corridor):
    """M = 8.  The rays of level k, shaded at depth k, have the colours a raytracer with max_reflection_depth 8 - k gives them, for k = 0..8; local and kr of
    every level unwind with mix_rays, and mix_pixels, to render's frame."""
    sd, A, lights, get = corridor
    assert_depth_teeth(get)
    M = 8
    region = traced_region(W, H)
    x0, y0, rw, rh = region
    for mode in ALL_MODES:
        rt = tracer(rrt, sd, lights, mode, CORRIDOR_CAM, max_reflection_depth=M)
        frame = rt.render(W, H)
        rays = rt.frame_rays(W, H, region=region)                                                 # rows order: the traced sub-samples, all alive
        assert np.isposinf(rays["max_t"]).all(), "the traced region's batch has a dead entry"
        levels = chain_levels(rt, A, rays["origins"], rays["dirs"], max_depth=M)
        alive = [len(l[1]) for l in levels]
        print(f"corridor {W}x{H}, walk {mode}: rays alive per level {alive}")
        assert len(levels) == M + 1 and alive[M] >= MIN_ALIVE_AT_LEVEL_8, f"walk {mode}: rays alive per level {alive}: want {M + 1} levels, {MIN_ALIVE_AT_LEVEL_8} rays at the last"
        shallow = {k: tracer(rrt, sd, lights, mode, CORRIDOR_CAM, max_reflection_depth=M - k) for k in range(M + 1)}
        below = None
        for k in reversed(range(M + 1)):
            o, d, planes, go = levels[k]
            want = shallow[k].get_ray_colours(o, d)
            out = {}
            for name, p in (("with the mask", planes), ("without the mask", without_mask(planes))):
                out = rt.shade_rays(d, p, depth=k, outputs=OUTPUTS)
                bad = out["colour"] != want
                assert not bad.any(), f"walk {mode}, level {k} at depth {k} {name} vs max_reflection_depth {M - k}: {int(bad.sum())} of {bad.size} colours differ"
            assert ((out["kr"] > 0.0) == go).all(), f"walk {mode}, level {k}: kr > 0 on {int((out['kr'] > 0.0).sum())} rays, the reference reflects at {int(go.sum())}"
            reflected = None
            if below is not None:
                reflected = np.zeros(len(d), np.uint32)
                reflected[go] = below                                                             # the scatter of the level below into this level's order
            colour = rt.mix_rays(out["local"], kr=out["kr"], reflected=reflected, material=planes["material"])
            bad = colour != want
            assert not bad.any(), f"walk {mode}, level {k}: mix_rays of local, kr and the level below differs from get_ray_colours on {int(bad.sum())} of {bad.size} rays"
            below = colour
        assert_same_bits(rt.mix_pixels(below, W, H, region=region), frame[y0:y0 + rh, x0:x0 + rw], f"walk {mode}: the unwind by mix_rays and mix_pixels vs render")
        if mode is None:                                                                          # depth is read: level 1 at depth 1 is not level 1 at depth 0
            o, d, planes, _ = levels[1]
            n = unequal(rt.shade_rays(d, planes, depth=1)["colour"], rt.shade_rays(d, planes, depth=0)["colour"])
            assert n >= 100, f"level 1 shaded at depth 1 and at depth 0 differs on {n} rays only"


# ------------------------------------------------------------------ D: everything at once
ALL_VIEWPORT, ALL_OFFSET, ALL_DEPTH = (1.3, 0.7, 1.1), 1e-2, 8
ALL_EYE, ALL_TARGET = (6.0, 5.0, -6.0), (0.0, 1.0, 2.0)                 # off every triangle's plane, in front of the mirror
# by the oracle, for this pose, viewport and offset at 64x48: mask 0xFFFF on 645 hits, 0x7FFF on 129, 10 values of ctz(~mask) with 30 hits, 100 distinct
# masks, the sixteenth light changes 227 pixels.  One flat mirror never sees itself, so the frames of depths 0 and 1 differ (on 701 pixels) and those of depths 1
# to 8 do not: what depth 8 adds here is its stack and its work memory beside the other options, the deep levels themselves are part C's.
MIN_MIRROR_PIXELS = 400


def test_everything_at_once(rrt, ob):
    torch = pytest.importorskip("torch")
    sd, A = _shadow_box_mirror_scene(rrt)
    lights = lights_of(rrt, SIXTEEN)
    cam = rrt.look_at(ALL_EYE, ALL_TARGET)
    opt = dict(surface_offset=ALL_OFFSET, max_reflection_depth=ALL_DEPTH)
    what = f"shadow box with a mirror, 16 lights, depth {ALL_DEPTH}, viewport {ALL_VIEWPORT}, offset {ALL_OFFSET}, eye {ALL_EYE}"
    osc = oracle_for(ob, A, lights, cam["eye"], **opt)
    planes_ref = expected_planes(osc, A, lights, cam["eye"], frame_dirs(cam, W, H, ALL_VIEWPORT), surface_offset=ALL_OFFSET)
    assert_mask_minimums(planes_ref, what)
    ref = oracle_frame(osc, cam, W, H, what, ALL_VIEWPORT)
    frames = {name: oracle_frame(oracle_for(ob, A, ls, cam["eye"], **dict(opt, **o)), cam, W, H, f"{what}, {name}", ALL_VIEWPORT, neighbour=True)
              for name, ls, o in (("15 lights", lights[:15], {}), ("depth 0", lights, dict(max_reflection_depth=0)))}
    teeth = {name: unequal(ref, f) for name, f in frames.items()}
    print(f"{what}: the oracle's frame differs from that of {teeth}")
    assert teeth["15 lights"] >= MIN_PIXELS_OF_LIGHT_15, f"the sixteenth light changes {teeth['15 lights']} pixels (< {MIN_PIXELS_OF_LIGHT_15})"
    assert teeth["depth 0"] >= MIN_MIRROR_PIXELS, f"the frames of depths 0 and 8 differ on {teeth['depth 0']} pixels (< {MIN_MIRROR_PIXELS})"
    for mode in ALL_MODES:
        rt = tracer(rrt, sd, lights, mode, cam, viewport=ALL_VIEWPORT, **opt)
        check_planes(rt, planes_ref, W, H, f"{what}, walk {mode}")
        frame, _ = assert_shade_is_render(rt, W, H, f"{what}, walk {mode}")
        d = assert_frame_close(frame, ref, f"{what}, walk {mode}: render vs the oracle")
        print(f"walk {mode}: {int((d > 0).sum())} pixels not bit-equal to the oracle")
        assert_same_bits(assert_wavefront_is_render(rrt, torch, rt, W, H, REGION[(W, H)], f"{what}, walk {mode}", mode), frame, f"walk {mode}: the frame of assert_wavefront_is_render")


# ------------------------------------------------------------------ E: ambient occlusion at another surface offset
MIN_AMBIENT_MOVED = 50                                           # samples whose T8 mask is not the offset-1e-4 mask; the oracle counts 629 at offset 1e-2, 2876 at offset 0.0
MIN_AMBIENT_TURNED = 1000                                        # samples whose rotated mask is not the unrotated one; the oracle counts 5870 and 5466 of 7142 hits


AMBIENT_INPUTS = ("point", "normal", "material")
_ambient = {}


def ambient_answers(osc, planes, n_mats, offset, rotated):
    """The oracle's T8 masks of the hits of `planes` -- rt.surface's, [h][w][4] -- at `offset`, without or with the standard rotation per record, computed once
    per (offset, rotated) and shared by the cases (read-only).  The offset option moves no plane the rays are formed from: every call's planes are the first's."""
    kept = _ambient.setdefault("planes", {n: planes[n].copy() for n in AMBIENT_INPUTS})
    assert_same_arrays(planes, kept, AMBIENT_INPUTS, f"the planes at offset {offset} vs the planes of the first case")
    if (offset, rotated) not in _ambient:
        if rotated:
            rec = {n: kept[n].reshape((-1, 3) if n != "material" else (-1,)) for n in AMBIENT_INPUTS}
            mask = fan_by_oracle(osc, Fan(rec, n_mats, T8, standard_rot(len(rec["material"])), surface_offset=offset), T8_MAX_T).reshape(kept["material"].shape)
        else:
            mask = plane_by_oracle(osc, Rays(kept, n_mats, T8, surface_offset=offset), T8_MAX_T)
        mask.setflags(write=False)
        _ambient[(offset, rotated)] = mask
    return _ambient[(offset, rotated)]


@pytest.mark.parametrize("rotated", (False, True), ids=["no rotation", "a rotation per record"])
@pytest.mark.parametrize("offset", (1e-2, 0.0))
def test_ambient_occlusion_at_another_offset(rrt, ob, teapot, teapot_arrays, offset, rotated):
    """ambient of the frame's planes and ambient_rays of the same records -- and ambient_rays with a rotation per record -- are the masks the oracle's intersector
    gives for the restated rays at that offset; the two unrotated forms are each other's."""
    n_mats = len(teapot_arrays["materials"])
    osc = oracle_for(ob, teapot_arrays, rrt.default_lights(), surface_offset=offset)
    want = None
    for mode in ALL_MODES:
        what = f"teapot, surface_offset {offset}, walk {mode}"
        rt = tracer(rrt, teapot, rrt.default_lights(), mode, surface_offset=offset)
        planes = rt.surface(W, H, planes=AMBIENT_INPUTS)
        rec = {n: planes[n].reshape((-1, 3) if n != "material" else (-1,)) for n in AMBIENT_INPUTS}
        hit = planes["material"] < n_mats
        if want is None:                                                                          # the oracle's part, before any comparison
            want = ambient_answers(osc, planes, n_mats, offset, rotated)
            other = ambient_answers(osc, planes, n_mats, 1e-4, False) if not rotated else ambient_answers(osc, planes, n_mats, offset, False)
            moved = unequal(want, other)
            least = MIN_AMBIENT_TURNED if rotated else MIN_AMBIENT_MOVED
            print(f"surface_offset {offset}: {int(hit.sum())} hit samples; by the oracle the mask differs from the {'unrotated' if rotated else 'offset-1e-4'} mask on {moved} samples")
            assert hit.mean() >= 0.5, f"only {hit.mean():.3f} of the samples hit"
            assert moved >= least, f"by the oracle the mask differs from the {'unrotated' if rotated else 'offset-1e-4'} mask on {moved} samples (< {least})"
        if rotated:
            got = rt.ambient_rays(rec, T8, T8_MAX_T, rot=standard_rot(len(rec["material"])))
            assert_same_bits(got["occluded"], want.reshape(-1), f"{what}: ambient_rays with a rotation vs the oracle's intersector")
        else:
            got = rt.ambient(W, H, planes, T8, T8_MAX_T, outputs=("occluded",))["occluded"]
            assert_same_bits(got, want, f"{what}: ambient vs the oracle's intersector")
            got = rt.ambient_rays(rec, T8, T8_MAX_T)
            assert_same_bits(got["occluded"], want.reshape(-1), f"{what}: ambient_rays of the flattened planes vs the oracle's intersector, and so ambient")
        assert_same_bits(got["open"], open_of(want.reshape(-1), hit.reshape(-1), len(T8)), f"{what}: open")
