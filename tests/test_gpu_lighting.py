"""Light lists, reflection depth and surface offset on the GPU against the CPU oracle.

Every other GPU test renders with default_lights() (Ambient, Point, Point, Directional), depth 5 and offset 1e-4.  This module runs the light-loop
state machine of render.hip (trace_colour: shadow ray per point light, the `break` of raytracer.rs:235-237 as n_eval, the lighting sum formed after
the last shadow ray, the reflection stack) on other light lists and options, each case checked three ways:
  (a) the reference-order frame (RRT_FLAG_NO_CULL) is within COLOUR_TOL per channel of the oracle's frame with the same lights and options (the
      count of pixels that are not bit-equal is printed);
  (b) the default, lane-filter, bundle-filter and ray-walk frames are bit-identical to it;
  (c) the case has teeth: the oracle's frame differs from the frame of a neighbouring configuration (other lights, depth -/+ 1, another offset) on
      at least a stated number of pixels, so the case really exercises what it names.
Where (b) could fail by contract (secondary rays inside the exactness band of include/rrt.h, RRT_FLAG_NO_CULL), the differing rays are rebuilt and
checked one by one against the band criterion; a difference outside the band fails the test.
"""
import numpy as np
import pytest

from conftest import channels
from gpu_checks import FORCED_MODES, N_THREADS, ORIGIN, assert_frame_close, assert_walks_match, in_noise_band, oracle_for, row_dirs, sample_rays
from lighting_scenes import CORRIDOR_ORIGIN, SHADOW_ORIGIN, _corridor_lights, _corridor_scene, _shadow_box_scene
from scenes import teapot_arrays_with_root as teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)

pytestmark = pytest.mark.gpu
SIZES = ((160, 120), (97, 61))


def _oracle_frame(ob, A, lights, origin, w, h, **opt):
    return oracle_for(ob, A, lights, origin, **opt).render(w, h, n_threads=N_THREADS)[0]


def _shade_normal(A, tri, u, v):
    """get_normal_at_intersection (raytracer.rs:114-162) and the texel indices, in numpy (for rebuilding secondary rays)."""
    w = 1.0 - u - v
    m = A["materials"][int(A["mat"][tri])]
    tex = A["textures"][m["tex"]]
    uv = A["uv"][tri]
    tx = uv[1, 0] * u + uv[2, 0] * v + uv[0, 0] * w; ty = uv[1, 1] * u + uv[2, 1] * v + uv[0, 1] * w
    as_usize = lambda x: int(x) if x > 0 and np.isfinite(x) else 0
    xi = as_usize(tx * tex.shape[1]) % tex.shape[1]; yi = as_usize(ty * tex.shape[0]) % tex.shape[0]
    nr = A["nrm"][tri]
    n = (nr[1] * u + nr[2] * v) + nr[0] * w
    if m["bump"] >= 0:
        bm = A["textures"][m["bump"]]
        bv = bm[yi, xi].astype(np.float64)           # colour-texture indices into the bump map (raytracer.rs:127-128)
        bv = bv / np.linalg.norm(bv) * 2.0 - 1.0
        t = np.cross(n, [0.0, 1.0, 0.0])
        if np.linalg.norm(t) == 0.0:
            t = np.cross(n, [0.0, 0.0, 1.0])
        t /= np.linalg.norm(t)
        b = np.cross(n, t); b /= np.linalg.norm(b)
        n = np.array([bv @ t, bv @ b, bv @ n])
    return n / np.linalg.norm(n), m


def _secondary_rays(osc, A, lights, o, d, offset, max_depth):
    """The shadow and reflection rays that RayTracer::get_ray_colour (raytracer.rs:29-112, 164-188) traces for the primary ray (o, d)."""
    out = []
    for depth in range(max_depth + 1):
        hit, t, u, v, tri = osc.intersect(o, d)
        if not hit:
            break
        p = np.asarray(o) + np.asarray(d) * t
        n, m = _shade_normal(A, tri, u, v)
        for l in lights:
            if l.kind == 1:
                L = np.array([l.v.x, l.v.y, l.v.z])
                out.append((p + n * offset, L - p))
                if osc.intersect(p + n * offset, L - p, np.linalg.norm(L - p))[0]:
                    break                                        # occluded: the loop ends (raytracer.rs:235-237)
        if not (m["kr"] > 0.0 and depth < max_depth):
            break
        r = d - n * 2.0 * np.dot(d, n)
        o, d = p + n * offset, r / np.linalg.norm(r)
        out.append((o, d))
    return out


def _pixel_in_band(osc, A, lights, origin, opt, w, h, r, c):
    """Whether one of the pixel's four sub-sample rays casts a shadow or reflection ray inside the exactness band of some triangle (the criterion
    of test_gpu_configs.py case C): only such a pixel may differ from the reference-order frame."""
    pad = max(abs(x) for x in A["root"]) / 32768.0                         # clusters.cpp: 2^-15 of the scene magnitude
    rays = [ray for d in row_dirs(w, h, r, [c])[:, 0]
            for ray in _secondary_rays(osc, A, lights, np.array(origin), d, opt.get("surface_offset", 1e-4), opt.get("max_reflection_depth", 5))]
    return any(in_noise_band(A["pos"], o, d, pad) for o, d in rays)


def run_case(rrt, ob, sd, A, name, lights, origin, neighbour, min_teeth, band_ok=False, sizes=SIZES, **opt):
    """(a), (b) and (c) for one configuration; returns the reference-order frames.  neighbour = (lights, opt) of the neighbouring configuration.
    With band_ok, (b) lets a pixel differ where _pixel_in_band holds, and the count of such pixels is printed."""
    exact = rrt.RayTracer(sd, lights, rrt.Vector3d(*origin), no_cull=True, **opt)
    osc = oracle_for(ob, A, lights, origin, **opt)
    frames, refs, report = [], [], []
    for w, h in sizes:
        gpu = exact.render(w, h)
        ref = osc.render(w, h, n_threads=N_THREADS)[0]
        d = assert_frame_close(gpu, ref, f"{name} {w}x{h}")
        report.append(f"{w}x{h}: {(d > 0).sum()} px not bit-equal to the oracle")
        frames.append(gpu); refs.append(ref)
    in_band = (lambda w, h, r, c: _pixel_in_band(osc, A, lights, origin, opt, w, h, r, c)) if band_ok else None
    n_band = assert_walks_match(lambda mode: rrt.RayTracer(sd, lights, rrt.Vector3d(*origin), box_filter=mode, **opt), frames, sizes, name,
                                in_band=in_band)
    teeth = int((_oracle_frame(ob, A, neighbour[0], origin, *sizes[0], **neighbour[1]) != refs[0]).sum())
    assert teeth >= min_teeth, f"{name}: differs from its neighbouring configuration on only {teeth} pixels (< {min_teeth})"
    print(f"\n[lighting] {name}: {'; '.join(report)}; teeth {teeth} px (min {min_teeth})" + (f"; band pixels {n_band}" if band_ok else ""))
    return frames


# ------------------------------------------------------------------ light lists on the teapot
def _teapot_lights(rrt, teapot_arrays):
    L, V = rrt.Light, rrt.Vector3d
    pos, mat = teapot_arrays["pos"], teapot_arrays["mat"]
    front = pos[mat == 0].reshape(-1, 3)
    vertex = front[int(np.argmin(front[:, 2]))]                  # the teapot's nearest vertex to the camera
    rng = np.random.default_rng(0x11647)
    sixteen = []
    for k in range(16):
        kind = int(rng.integers(0, 3))
        v = V(*rng.uniform([-15, -2, -25], [15, 15, 5])) if kind else V(0.0, 0.0, 0.0)
        sixteen.append(L(kind, float(rng.uniform(0.02, 0.3)), v))
    return {
        # name: (lights, neighbour lights or None = default lights, minimum teeth in pixels)
        "empty": ([], None, 9000),
        "ambient_only": ([L.Ambient(0.7)], None, 9000),
        "directional_only": ([L.Directional(0.8, V(-5.0, 4.0, -10.0))], None, 9000),
        "default_reversed": (rrt.default_lights()[::-1], None, 2000),
        "break_drops_ambient": ([L.Point(0.4, V(0.0, -3.0, 0.0)), L.Ambient(0.5), L.Point(0.5, V(4.0, 8.0, -12.0))],
                                [L.Ambient(0.5), L.Point(0.4, V(0.0, -3.0, 0.0)), L.Point(0.5, V(4.0, 8.0, -12.0))], 4000),
        "opposite_points": ([L.Ambient(0.2), L.Point(0.5, V(-12.0, 4.0, -2.0)), L.Point(0.5, V(12.0, 4.0, 2.0))], None, 5000),
        "point_at_origin": ([L.Ambient(0.3), L.Point(0.6, V(*ORIGIN))], None, 5000),
        "point_at_vertex": ([L.Ambient(0.3), L.Point(0.6, V(*map(float, vertex)))], None, 5000),
        "point_inside_teapot": ([L.Ambient(0.3), L.Point(0.6, V(0.0, 1.5, 0.0)), L.Point(0.4, V(-7.0, 1.0, -15.0))], None, 5000),
        "point_outside_root": ([L.Ambient(0.3), L.Point(0.6, V(25.0, 10.0, -25.0))], None, 5000),
        "point_inside_cull_limit": ([L.Ambient(0.3), L.Point(0.6, V(0.0, 40.0, -70.0))], None, 5000),
        "point_beyond_cull_limit": ([L.Ambient(0.3), L.Point(0.6, V(0.0, 50.0, -95.0))], None, 5000),
        "point_at_1e4": ([L.Ambient(0.3), L.Point(0.6, V(1e4, 1e4, -1e4))], None, 5000),
        "zero_directional": ([L.Ambient(0.3), L.Directional(0.6, V(0.0, 0.0, 0.0))], [L.Ambient(0.3), L.Directional(0.6, V(-5.0, 4.0, -10.0))], 5000),
        "negative_and_saturating": ([L.Ambient(-0.3), L.Point(3.0, V(-7.0, 1.0, -15.0)), L.Directional(-1.0, V(-5.0, 0.0, 20.0))], None, 5000),
        "sixteen_lights": (sixteen, None, 5000),
    }


CASES = ("empty", "ambient_only", "directional_only", "default_reversed", "break_drops_ambient", "opposite_points", "point_at_origin", "point_at_vertex",
         "point_inside_teapot", "point_outside_root", "point_inside_cull_limit", "point_beyond_cull_limit", "point_at_1e4", "zero_directional",
         "negative_and_saturating", "sixteen_lights")
BAND_CASES = ("point_at_vertex",)    # a light on a mesh vertex: shadow rays of the triangles round it run in their planes


@pytest.mark.parametrize("case", CASES)
def test_teapot_light_lists(rrt, ob, teapot, teapot_arrays, case):
    lights, neighbour, min_teeth = _teapot_lights(rrt, teapot_arrays)[case]
    neighbour = rrt.default_lights() if neighbour is None else neighbour
    frames = run_case(rrt, ob, teapot, teapot_arrays, case, lights, ORIGIN, (neighbour, {}), min_teeth, band_ok=case in BAND_CASES)
    f = frames[0][1:]
    if case == "empty":                                          # no light: every hit is black, every miss white, mixed per pixel
        c = channels(f)
        assert (c[..., 0] == c[..., 1]).all() and (c[..., 1] == c[..., 2]).all()
        assert (f == 0).sum() > 5000 and (f == 0xFFFFFF).sum() > 5000
    elif case == "zero_directional":                             # |l| = 0: n.l = 0 gives no diffuse, r = 0 no specular -- the ambient-only frame
        w, h = SIZES[0]
        assert np.array_equal(frames[0], _oracle_frame(ob, teapot_arrays, lights[:1], ORIGIN, w, h))
    elif case == "negative_and_saturating":
        assert (f == 0xFFFFFF).sum() > 9000 and (f == 0).sum() > 1000   # lit hits clamp to white (misses alone: ~7800), shadowed ones to black
    elif case == "break_drops_ambient":                          # the light under the table is occluded for most of the frame: black there
        assert (f == 0).sum() > 4000


def test_sixteen_lights_ray_colours(rrt, ob, teapot, teapot_arrays):
    """get_ray_colours against oracle.get_ray_colour with the 16-light list: primary sub-sample rays plus shadow- and reflection-shaped rays
    (gpu_checks.sample_rays), in all three walk variants."""
    lights = _teapot_lights(rrt, teapot_arrays)["sixteen_lights"][0]
    osc = oracle_for(ob, teapot_arrays, lights)
    O, D, _ = sample_rays(osc, 160, 120, 1500, np.random.default_rng(1616), lights)
    assert len(O) > 5000
    ref = np.fromiter((osc.get_ray_colour(O[i], D[i]) for i in range(len(O))), np.uint32, len(O))
    for mode in FORCED_MODES:
        assert_frame_close(rrt.RayTracer(teapot, lights, box_filter=mode).get_ray_colours(O, D), ref, f"walk {mode}: ray colours")


def test_invalid_lights_and_depth_are_rejected(rrt, teapot):
    L, V = rrt.Light, rrt.Vector3d
    for lights, opt in (([L.Ambient(0.01)] * 17, {}), ([L.Ambient(0.5), L(3, 0.5, V(0.0, 1.0, 0.0))], {}), (rrt.default_lights(), dict(max_reflection_depth=9))):
        with pytest.raises(rrt.RrtError) as e:
            rrt.RayTracer(teapot, lights, **opt)
        assert e.value.status == -1                              # RRT_ERR_INVALID_ARG
    rrt.RayTracer(teapot, [L.Ambient(0.01)] * 16, max_reflection_depth=8)   # the limits themselves are accepted


# ------------------------------------------------------------------ hand-built scenes
@pytest.fixture(scope="module")
def shadow_box(rrt):
    return _shadow_box_scene(rrt)


SHADOW_CASES = {
    # lights between the blocker and the floor: the blocker lies beyond max_t for floor points and before it for points above
    "between_blocker_and_floor": lambda L, V: [L.Ambient(0.2), L.Point(0.6, V(0.0, 1.0, 1.2)), L.Point(0.4, V(-3.0, 5.0, -2.0))],
    # a light just above the blocker: floor points under it are occluded just before max_t
    "just_beyond_occluder": lambda L, V: [L.Ambient(0.2), L.Point(0.7, V(0.0, 2.05, 1.2)), L.Point(0.3, V(4.0, 6.0, -3.0))],
    # a light inside the closed box: occluded everywhere, the `break` drops the lights after it
    "inside_closed_box": lambda L, V: [L.Ambient(0.25), L.Point(0.6, V(3.0, 1.0, 4.0)), L.Point(0.5, V(0.0, 1.0, 1.2))],
}
SHADOW_NEIGHBOURS = {
    "between_blocker_and_floor": lambda L, V: [L.Ambient(0.2), L.Point(0.4, V(-3.0, 5.0, -2.0))],
    "just_beyond_occluder": lambda L, V: [L.Ambient(0.2), L.Point(0.3, V(4.0, 6.0, -3.0))],
    "inside_closed_box": lambda L, V: [L.Ambient(0.25), L.Point(0.5, V(0.0, 1.0, 1.2))],
}


@pytest.mark.parametrize("case", list(SHADOW_CASES))
def test_shadow_box(rrt, ob, shadow_box, case):
    sd, A = shadow_box
    L, V = rrt.Light, rrt.Vector3d
    run_case(rrt, ob, sd, A, f"shadow_box/{case}", SHADOW_CASES[case](L, V), SHADOW_ORIGIN, (SHADOW_NEIGHBOURS[case](L, V), {}), 1000)


@pytest.fixture(scope="module")
def corridor(rrt):
    return _corridor_scene(rrt)


@pytest.mark.parametrize("depth", range(9))
def test_mirror_corridor_depth(rrt, ob, corridor, depth):
    """Every reflection depth 0..8 against the oracle at the same depth; teeth: depth d differs from depth d + 1 (d = 8: from d - 1, the stack is full)."""
    sd, A = corridor
    lights = _corridor_lights(rrt)
    nd = depth + 1 if depth < 8 else 7
    run_case(rrt, ob, sd, A, f"corridor/depth{depth}", lights, CORRIDOR_ORIGIN, (lights, dict(max_reflection_depth=nd)), 50,
             sizes=((96, 72), (61, 45)), max_reflection_depth=depth)


OFFSETS = (0.0, 1e-12, 1e-6, 1e-4, 1e-2, 0.3)
NEIGHBOUR_OFFSET = {0.0: 1e-4, 1e-12: 1e-4, 1e-6: 1e-4, 1e-4: 1e-2, 1e-2: 1e-4, 0.3: 1e-4}
# teeth against the neighbouring offset.  The teapot's bump-mapped, curved surfaces and its mirror react to every offset (0: self-shadowing); the
# shadow box's flat faces only to offsets that lift a shadow or reflection ray past geometry, so its small offsets carry no minimum of their own.
OFFSET_TEETH = {"teapot": {0.0: 3000, 1e-12: 20, 1e-6: 20, 1e-4: 200, 1e-2: 200, 0.3: 500},
                "shadow_box": {0.0: 0, 1e-12: 0, 1e-6: 0, 1e-4: 0, 1e-2: 0, 0.3: 100}}


@pytest.mark.parametrize("offset", OFFSETS)
def test_surface_offset_teapot(rrt, ob, teapot, teapot_arrays, offset):
    lights = rrt.default_lights()
    run_case(rrt, ob, teapot, teapot_arrays, f"teapot/offset {offset:g}", lights, ORIGIN, (lights, dict(surface_offset=NEIGHBOUR_OFFSET[offset])),
             OFFSET_TEETH["teapot"][offset], band_ok=offset == 0.0, surface_offset=offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_surface_offset_shadow_box(rrt, ob, shadow_box, offset):
    sd, A = shadow_box
    lights = SHADOW_CASES["just_beyond_occluder"](rrt.Light, rrt.Vector3d)
    run_case(rrt, ob, sd, A, f"shadow_box/offset {offset:g}", lights, SHADOW_ORIGIN, (lights, dict(surface_offset=NEIGHBOUR_OFFSET[offset])),
             OFFSET_TEETH["shadow_box"][offset], band_ok=offset == 0.0, surface_offset=offset)
