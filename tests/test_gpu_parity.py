"""Parity tests proper: the HIP path, called through the C ABI (librrt_hip.so), against the CPU oracle on identical inputs.

Bar (BASELINE.json north_star): every pixel within +-1 per RGB channel of the CPU renderer.  Tolerances are written where used:
  * geometry (hit/miss, triangle id, t, u, v): BIT-EXACT -- f64 op for op, -ffp-contract=off, correctly rounded / and sqrt.
  * colours: <= 1 per channel (only pow(), raytracer.rs:295, may differ by an ulp between glibc and OCML before u8 truncation).
"""
import os

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, channels, oracle_scene_for
from gpu_checks import (N_THREADS, ORIGIN, assert_frame_close, assert_rays_match_oracle, assert_walks_match, check_rows_against_oracle,
                        oracle_for)

pytestmark = pytest.mark.gpu


def _free_port():
    """A port nobody listens on right now, with room above it: bench.py's children rendezvous on MASTER_PORT + 11 + k, and a fixed number taken from the pid
    met the lingering socket of an earlier test's killed group once in a while."""
    import socket
    for _ in range(50):
        with socket.socket() as a:
            a.bind(("127.0.0.1", 0)); p = a.getsockname()[1]
        if p > 60000:
            continue
        try:
            for q in (p + 1, p + 11, p + 12):
                with socket.socket() as b:
                    b.bind(("127.0.0.1", q))
            return p
        except OSError:
            continue
    return 29500


@pytest.fixture(scope="module")
def teapot_rt(rrt, teapot):
    return rrt.RayTracer(teapot, rrt.default_lights(), rrt.DEFAULT_ORIGIN, device=0)


@pytest.mark.parametrize("w,h", [(64, 48), (97, 61), (160, 120), (1, 1), (2, 2), (8, 3), (640, 480)])
def test_teapot_frames_match_oracle(teapot_rt, teapot_oracle, w, h):
    """configs[0] scene (model2.obj) incl. 640x480, odd sizes (unwritten last column / rows 0-1) and degenerate sizes."""
    gpu = teapot_rt.render(w, h)
    ref, _ = teapot_oracle.render(w, h, n_threads=N_THREADS)
    assert_frame_close(gpu, ref, f"{w}x{h}")
    assert (gpu[0] == 0).all()                                   # row 0 never written (engine.rs:146-158)
    assert np.array_equal(gpu == 0, ref == 0)


@pytest.mark.parametrize("name", ["model.obj", "model2.obj", "model3.obj"])
def test_golden_fixtures(rrt, name):
    """Committed oracle outputs (tests/golden/make_golden.py): frames, and 1024 fixed rays incl. secondary-like rays from inside the scene."""
    g = np.load(os.path.join(GOLDEN, name.replace(".obj", ".npz")))
    sd = rrt.parse_obj_file(os.path.join(ASSETS, name))
    rt = rrt.RayTracer(sd, rrt.default_lights())
    for key in [k for k in g.files if k.startswith("fb_")]:
        w, h = map(int, key[3:].split("x"))
        assert_frame_close(rt.render(w, h), g[key], f"{name} {key}")
    hit, t, u, v, tri = rt.intersect_rays(g["ray_o"], g["ray_d"])
    assert np.array_equal(hit, g["ray_hit"])
    m = g["ray_hit"]
    assert np.array_equal(tri[m], g["ray_tri"][m])
    assert np.array_equal(t[m], g["ray_t"][m]) and np.array_equal(u[m], g["ray_u"][m]) and np.array_equal(v[m], g["ray_v"][m])   # bit-exact
    col = rt.get_ray_colours(g["ray_o"], g["ray_d"])
    assert_frame_close(col, g["ray_col"], f"{name} ray colours")


def test_random_rays_with_max_t_bit_exact(teapot_rt, teapot_oracle):
    """Ray::intersect_with_octant_with_max_t on rays that start anywhere (on split planes too) with finite max_t (the shadow-ray form)."""
    rng = np.random.default_rng(7)
    n = 1500
    o = rng.uniform([-4, 0, -6], [4, 5, 4], (n, 3)); d = rng.normal(size=(n, 3))
    o[:200, 0] = 0.0; d[:100, 0] = 0.0          # on the root split plane x = 0, some with d.x = 0 (NaN slab path)
    o[200:300, 1] = 0.0; o[300:400, 2] = 0.0
    mt = rng.uniform(0.5, 30.0, n); mt[::5] = np.inf
    got = teapot_rt.intersect_rays(o, d, mt)
    assert_rays_match_oracle(got, teapot_oracle, o, d, mt, "random rays with max_t")
    assert 0.2 < got[0].mean() < 0.95


@pytest.mark.parametrize("mode", ["lane", "bundle", "ray"])
def test_extreme_ray_magnitudes_bit_exact(rrt, teapot, teapot_oracle, mode):
    """Rays whose components leave the range in which the walk may share one reciprocal per axis across its slab quotients (render.hip, RayRcp:
    |d| in [2^-500, 2^500], origin components 0 or in [2^-200, 2^200]) must take the ordinary divide and still agree bit for bit: directions scaled by
    2^+-600 (same line, t scaled the other way), denormal-small and zero origin components, in both kernel variants."""
    rng = np.random.default_rng(11)
    n = 600
    o = rng.uniform([-4, 0, -6], [4, 5, 4], (n, 3)); d = rng.normal(size=(n, 3))
    scale = np.ones(n); scale[:150] = 2.0 ** 600; scale[150:300] = 2.0 ** -600; scale[300:350] = 2.0 ** 499; scale[350:400] = 2.0 ** -499
    d *= scale[:, None]
    o[400:450, 0] = 1e-300; o[450:500, 1] = 5e-201 ; o[500:550, 2] = 0.0; o[550:, 0] = 2.0 ** -1060   # denormal
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    n_hit = assert_rays_match_oracle(rt.intersect_rays(o, d), teapot_oracle, o, d, what=f"extreme magnitudes, walk {mode}")
    assert n_hit > 100


def test_center_column_nan_path(teapot_rt, teapot_oracle):
    """Column w/2: d.x = 0 at origin.x = 0 == the root split plane -> (0-0)/0 = NaN in the slab test (ray.rs:22-23)."""
    w, h = 128, 96
    gpu = teapot_rt.render(w, h); ref, _ = teapot_oracle.render(w, h, n_threads=N_THREADS)
    assert_frame_close(gpu[:, w // 2 - 1:w // 2 + 2], ref[:, w // 2 - 1:w // 2 + 2], "centre columns")
    ys = np.linspace(-0.4, 0.4, 257)
    o = np.tile(ORIGIN, (len(ys), 1)); d = np.stack([np.zeros_like(ys), ys, np.ones_like(ys)], -1)
    assert_rays_match_oracle(teapot_rt.intersect_rays(o, d), teapot_oracle, o, d, what="centre column rays", uv=False)


def test_mirror_and_shadow_pixels_present(teapot_rt, teapot_oracle):
    """The frame exercises reflection (Kr 0.95 mirror, model2.obj:25977-25990) and the shadow `break`; both must match the oracle."""
    w, h = 320, 240
    gpu = teapot_rt.render(w, h); ref, cnt = teapot_oracle.render(w, h, n_threads=N_THREADS)
    assert cnt["rays_reflect"] > 1000 and cnt["rays_shadow"] > cnt["rays_primary"] // 2
    assert_frame_close(gpu, ref, "320x240")
    assert (ref == 0xFFFFFF).sum() > 100                         # miss pixels are WHITE


def test_options_viewport_offset_depth(rrt, teapot, ob):
    lights = rrt.default_lights()
    rt = rrt.RayTracer(teapot, lights, rrt.Vector3d(0.5, 2.5, -9.0), surface_offset=3e-3, max_reflection_depth=2, viewport=(1.5, 1.0, 1.25))
    osc = oracle_scene_for(ob, rrt, teapot, lights, (0.5, 2.5, -9.0))
    o = np.tile([0.5, 2.5, -9.0], (64, 1)); d = np.stack([np.linspace(-0.3, 0.6, 64), np.full(64, -0.12), np.ones(64)], -1)
    assert_rays_match_oracle(rt.intersect_rays(o, d), osc, o, d, what="viewport rays", uv=False)
    ref, _ = osc.render(96, 64, viewport=(1.5, 1.0, 1.25), n_threads=N_THREADS)
    gpu = rrt.RayTracer(teapot, lights, rrt.Vector3d(0.5, 2.5, -9.0), viewport=(1.5, 1.0, 1.25)).render(96, 64)
    assert_frame_close(gpu, ref, "viewport 1.5x1x1.25")
    # the whole frame of the depth-2, offset-3e-3 raytracer against the oracle with the same options; the options must change the frame
    pos, uv, nrm, mat = teapot.triangles()
    A = dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=teapot.materials(), textures=teapot.textures())
    osc2 = oracle_for(ob, A, lights, (0.5, 2.5, -9.0), surface_offset=3e-3, max_reflection_depth=2)
    ref2, _ = osc2.render(96, 64, viewport=(1.5, 1.0, 1.25), n_threads=N_THREADS)
    got = rt.render(96, 64)
    assert got.shape == (64, 96)
    assert_frame_close(got, ref2, "viewport 1.5x1x1.25, depth 2, offset 3e-3")
    assert (ref2 != ref).sum() > 20, "depth 2 / offset 3e-3 must change the frame"


@pytest.mark.parametrize("name,w,h", [("model2.obj", 640, 480), ("model2.obj", 1920, 1080), ("model3.obj", 480, 360), ("model.obj", 333, 211)])
def test_cluster_index_is_result_preserving(rrt, name, w, h):
    """Default mode (padded cluster boxes over every own list, clusters.cpp) vs RRT_FLAG_NO_CULL (every list walked in full, in list
    order, as ray.rs:119-129): frames must be IDENTICAL, at configs[0]/configs[1] sizes too; likewise t/u/v/triangle of random rays."""
    sd = rrt.parse_obj_file(os.path.join(ASSETS, name))
    fast = rrt.RayTracer(sd, rrt.default_lights()); exact = rrt.RayTracer(sd, rrt.default_lights(), no_cull=True)
    lane = rrt.RayTracer(sd, rrt.default_lights(), box_filter="lane"); bundle = rrt.RayTracer(sd, rrt.default_lights(), box_filter="bundle")
    ray = rrt.RayTracer(sd, rrt.default_lights(), box_filter="ray")
    ref = exact.render(w, h)
    assert np.array_equal(fast.render(w, h), ref) and np.array_equal(lane.render(w, h), ref) and np.array_equal(bundle.render(w, h), ref) and np.array_equal(ray.render(w, h), ref)
    assert lane.last_stats()["filter_variant"] == 0 and bundle.last_stats()["filter_variant"] == 1 and ray.last_stats()["filter_variant"] == 2
    rng = np.random.default_rng(11)
    n = 20000
    o = rng.uniform([-5, -0.5, -8], [5, 6, 5], (n, 3)); d = rng.normal(size=(n, 3)); d[:500, rng.integers(0, 3)] = 0.0
    mt = rng.uniform(0.5, 40.0, n); mt[::3] = np.inf
    b = exact.intersect_rays(o, d, mt)
    for other in (fast, lane, bundle, ray):                 # incoherent random rays: the bundle's interval test degenerates gracefully
        for x, y in zip(other.intersect_rays(o, d, mt), b):
            assert np.array_equal(x, y)
    for other in (bundle, ray): assert np.array_equal(other.get_ray_colours(o[:4096], d[:4096]), exact.get_ray_colours(o[:4096], d[:4096]))
    big = rrt.RayTracer(sd, rrt.default_lights(), rrt.Vector3d(1e4, 2.0, -10.0))       # origin beyond the fp32 filter's scale limit: filter must switch itself off
    big_exact = rrt.RayTracer(sd, rrt.default_lights(), rrt.Vector3d(1e4, 2.0, -10.0), no_cull=True)
    assert np.array_equal(big.render(64, 48), big_exact.render(64, 48))


def test_tile_partition_reassembles_frame(rrt, teapot_rt):
    """Multi-GPU path on one GPU: every rank's tile buffer rendered separately, gathered, de-tiled == single-launch frame (bit-exact)."""
    torch = pytest.importorskip("torch")
    w, h = 203, 117
    full = teapot_rt.render(w, h)
    for world in (1, 2, 3, 8):
        tpr = rrt.tiles_per_rank(w, h, world)
        gathered = torch.empty((world, tpr * 64), dtype=torch.int32, device="cuda")
        for r in range(world):
            teapot_rt.render_tiles_into(gathered[r], w, h, r, world)
        fb = torch.empty((h, w), dtype=torch.int32, device="cuda")
        teapot_rt.detile_into(gathered, fb, w, h, world)
        torch.cuda.synchronize()
        got = fb.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, full), world
        assert np.array_equal(rrt.detile_host(gathered.cpu().numpy().view(np.uint32), w, h, world), full)
    fb = torch.empty((h, w), dtype=torch.int32, device="cuda")
    teapot_rt.render_into(fb, w, h)
    torch.cuda.synchronize()
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), full)


def test_render_multi_world1_through_rccl(rrt, teapot, teapot_rt):
    """rrt_render_multi / rrt_multi_enqueue (the N-GPU frame behind ONE C call: tile partition, RCCL gather, de-tiling inside the library) with the one
    GPU of this box.  Loopback makes rank 0's own tiles travel through ncclSend/ncclRecv (ncclCommInitAll over one device), so the RCCL binding
    (dlopen), the grouped point-to-point gather, the slot ring and the de-tiling all run; the frame must equal the single-launch frame bit for bit,
    at an odd size too, with frames in flight, and through the one-process-per-GPU form (rrt_dist_create, world 1)."""
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    for (w, h) in ((203, 117), (640, 480)):
        full = teapot_rt.render(w, h)
        for loopback in (False, True):
            mg = rrt.MultiGpu([rt], frames_in_flight=3, loopback=loopback)
            assert np.array_equal(mg.render(w, h), full), (w, h, loopback)
            fbs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(5)]
            for fb in fbs:                                                     # five frames through a ring of three slots
                mg.bind_enqueue(fb, w, h)()
            mg.sync()
            for fb in fbs:
                assert np.array_equal(fb.cpu().numpy().view(np.uint32), full), (w, h, loopback)
            del mg
    dg = rrt.MultiGpu.dist(rt, 0, 1, None, frames_in_flight=2)
    assert np.array_equal(dg.render(203, 117), teapot_rt.render(203, 117))
    assert len(rrt.MultiGpu.unique_id()) == 128


def test_full_size_properties_1080p(teapot_rt, teapot_oracle):
    """configs[1] (model2.obj @1920x1080) is too slow to check pixel by pixel on the CPU in a test, so: (a) a 1080p frame is deterministic,
    (b) random 16-row bands of it equal the oracle's rows (the oracle renders a row independently of the frame), (c) frame invariants."""
    w, h = 1920, 1080
    a = teapot_rt.render(w, h); b = teapot_rt.render(w, h)
    assert np.array_equal(a, b) and (a[0] == 0).all() and (a[1:] != 0).all()
    st = teapot_rt.last_stats()
    assert st["rays_primary"] == 4 * 1920 * 1079 and st["kernel_ms"] > 0
    rng = np.random.default_rng(3)
    rows = sorted(set(rng.integers(1, h, 6).tolist()) | {1, h // 2, h - 1})
    check_rows_against_oracle(a, teapot_oracle, w, h, rows, 16)


def test_soup_scene_matches_oracle(rrt, ob):
    """configs[2]-shaped input at test size: a 20k-triangle random soup (deep, wide octree; every wave diverges)."""
    syn = __import__("importlib").import_module("rust-ray-tracer_amd.synthetic")
    path = syn.ensure_soup(ASSETS, 20000, 0x5EED0003)
    sd = rrt.parse_obj_file(path)
    lights = rrt.default_lights()
    rt = rrt.RayTracer(sd, lights)
    osc = oracle_scene_for(ob, rrt, sd, lights)
    gpu = rt.render(200, 150); ref, _ = osc.render(200, 150, n_threads=N_THREADS)
    assert_frame_close(gpu, ref, "soup 20k 200x150")
    assert ((ref != 0xFFFFFF) & (ref != 0)).mean() > 0.2


def test_tiny_scenes_edge_cases(rrt, ob):
    """Empty scene, a single triangle, and triangles outside the root box."""
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=240.0, kr=0.3, tex=0, bump=-1)]
    tex = [np.arange(48, dtype=np.uint8).reshape(4, 4, 3)]
    lights = rrt.default_lights()
    for tris in (np.zeros((0, 3, 3)), np.array([[[-3, 0, 2], [3, 0, 2], [0, 5, 2.5]]], np.float64),
                 np.array([[[-3, 0, 2], [3, 0, 2], [0, 5, 2.5]], [[50, 50, 50], [51, 50, 50], [50, 51, 50]], [[-2, 1, 1], [2, 1, 1], [0, 3, 1.2]]], np.float64)):
        n = len(tris)
        uv = np.tile([[0.1, 0.2, 0], [0.9, 0.1, 0], [0.5, 0.8, 0]], (n, 1, 1)).astype(np.float64); nrm = np.tile([0.0, 0.1, -1.0], (n, 3, 1))
        sd = rrt.SceneData.from_arrays(tris, uv, nrm, np.zeros(n, np.uint32), mats, tex)
        osc = oracle_for(ob, dict(pos=tris, uv=uv, nrm=nrm, mat=np.zeros(n, np.uint32), materials=mats, textures=tex), lights)
        gpu = rrt.RayTracer(sd, lights).render(40, 30); ref, _ = osc.render(40, 30, n_threads=N_THREADS)
        assert_frame_close(gpu, ref, f"{n} triangles")


def _random_scene(rng, kind):
    """Small adversarial scenes: axis-aligned quads sharing edges and vertices (exact ties in t), faces lying exactly in the camera's
    d.y = 0 / d.x = 0 ray planes (coplanar ray/triangle pairs: the reference's own Moller-Trumbore is rounding noise there), slivers,
    triangles through octree split planes, a mirror and a bump-mapped material."""
    tris = []
    if kind == "grid":                                   # a wall of quads at z = 3 split into triangles: shared edges everywhere
        n = 6
        xs = np.linspace(-3, 3, n + 1); ys = np.linspace(-1, 5, n + 1)
        for i in range(n):
            for j in range(n):
                a, b, c, d = (xs[i], ys[j], 3.0), (xs[i + 1], ys[j], 3.0), (xs[i + 1], ys[j + 1], 3.0), (xs[i], ys[j + 1], 3.0)
                tris += [[a, b, c], [a, c, d]]
    elif kind == "coplanar":                             # horizontal faces exactly at the camera height y = 2 and a vertical face at x = 0
        for z in (0.0, 1.0, 2.0, 4.0):
            tris += [[(-2, 2.0, z), (2, 2.0, z), (2, 2.0, z + 1)], [(-2, 2.0, z), (2, 2.0, z + 1), (-2, 2.0, z + 1)]]
        tris += [[(0.0, 0, 1), (0.0, 4, 1), (0.0, 4, 5)], [(0.0, 0, 1), (0.0, 4, 5), (0.0, 0, 5)]]
        tris += [[(-4, -0.5, -2), (4, -0.5, -2), (0, -0.5, 9)]]
    elif kind == "noise":                                # triangles built (in f64) INSIDE planes that contain the camera origin and one sub-sample ray each:
        o = np.array(ORIGIN)                             # that ray is coplanar with them up to rounding, a = e1.(d x e2) is pure noise of either sign
        for (px, py) in [(10, 7), (-21.5, 3), (5, -12.5), (0.5, 0.5), (33, -8)]:
            d0 = np.array([px / 128.0, py / 96.0, 1.0])
            for k in range(6):
                u = rng.normal(size=3)
                a0, a1, a2 = rng.uniform(6, 14, 3); b0, b1, b2 = rng.uniform(-3, 3, 3)
                tris.append([o + a0 * d0 + b0 * u, o + a1 * d0 + b1 * u, o + a2 * d0 + b2 * u])
        tris += [[(-6, -1, 8), (6, -1, 8), (0, 6, 8.5)]]
    elif kind == "slivers":
        for k in range(40):
            p = rng.uniform([-3, 0, 0], [3, 4, 6]); e = rng.normal(size=3) * 2
            tris.append([p, p + e, p + e * (1 + 1e-7) + rng.normal(size=3) * 1e-6])
        for k in range(40):
            p = rng.uniform([-3, 0, 0], [3, 4, 6]); tris.append([p, p + rng.normal(size=3), p + rng.normal(size=3)])
    else:                                                # "soup": random triangles of mixed sizes, some crossing the root split planes
        for k in range(300):
            p = rng.uniform([-4, -0.5, -3], [4, 5, 7]); s = 10 ** rng.uniform(-1.5, 0.5)
            tris.append([p, p + rng.normal(size=3) * s, p + rng.normal(size=3) * s])
    tris = np.asarray(tris, np.float64)
    n = len(tris)
    nrm = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    nrm3 = np.repeat(nrm[:, None, :], 3, 1) + rng.normal(size=(n, 3, 3)) * 0.05
    uv = np.concatenate([rng.uniform(-2, 3, (n, 3, 2)), np.zeros((n, 3, 1))], -1)
    tex = [rng.integers(0, 256, (8, 16, 3), dtype=np.uint8), rng.integers(0, 256, (8, 16, 3), dtype=np.uint8)]
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=240.0, kr=0.0, tex=0, bump=1),
            dict(ka=(0.1, 0.1, 0.1), kd=(0.1, 0.1, 0.1), ks=(1, 1, 1), ns=500.0, kr=0.95, tex=0, bump=-1),
            dict(ka=(0.5, 0.4, 0.3), kd=(0.9, 0.8, 0.7), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=1, bump=-1)]
    mat = rng.integers(0, 3, n).astype(np.uint32)
    return tris, uv, nrm3, mat, mats, tex


@pytest.mark.parametrize("kind", ["grid", "coplanar", "noise", "slivers", "soup"])
def test_adversarial_random_scenes(rrt, ob, kind):
    """Default (autotuned), lane-filter, bundle-filter and no-cull modes against the oracle on small adversarial scenes: frames within the colour
    tolerance of the oracle, and the three culling modes IDENTICAL to the no-cull mode (the cluster index's exactness caveat, DESIGN.md section 4,
    would show up exactly here: ties, coplanar ray/triangle pairs, slivers)."""
    rng = np.random.default_rng({"grid": 1, "coplanar": 2, "slivers": 3, "soup": 4, "noise": 5}[kind])
    tris, uv, nrm, mat, mats, tex = _random_scene(rng, kind)
    lights = rrt.default_lights()
    sd = rrt.SceneData.from_arrays(tris, uv, nrm, mat, mats, tex)
    osc = oracle_for(ob, dict(pos=tris, uv=uv, nrm=nrm, mat=mat, materials=mats, textures=tex), lights)
    w, h = 128, 96                                        # even sizes: the rows y = 0 (d.y = 0) and the column x = 0 (d.x = 0) are sampled
    ref, _ = osc.render(w, h, n_threads=N_THREADS)
    exact = rrt.RayTracer(sd, lights, no_cull=True).render(w, h)
    assert_frame_close(exact, ref, f"{kind} no_cull vs oracle")
    assert_walks_match(lambda mode: rrt.RayTracer(sd, lights, box_filter=mode), [exact], [(w, h)], kind)


def test_cpp_host_cli_matches_python_host(rrt, teapot_rt, tmp_path):
    """render_cli (C++ mirror of the reference's main.rs over the C ABI) writes the same frame the Python host gets."""
    import subprocess
    cli = os.path.join(os.path.dirname(ASSETS), "rust-ray-tracer_amd", "render_cli")
    out = tmp_path / "f.ppm"
    r = subprocess.run([cli, os.path.join(ASSETS, "model2.obj"), str(out), "200", "150"], capture_output=True, text=True)
    assert r.returncode == 0 and "draw finished" in r.stdout, r.stderr
    raw = out.read_bytes()
    assert raw.startswith(b"P6\n200 150\n255\n")
    rgb = np.frombuffer(raw[len(b"P6\n200 150\n255\n"):], np.uint8).reshape(150, 200, 3).astype(np.uint32)
    fb = (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]
    assert np.array_equal(fb, teapot_rt.render(200, 150))
    out2 = tmp_path / "g.ppm"
    r = subprocess.run([cli, os.path.join(ASSETS, "model2.obj"), str(out2), "200", "150", "--progressive"], capture_output=True, text=True)
    assert r.returncode == 0 and "canvas updates: 3" in r.stdout, r.stdout + r.stderr          # 150 scene rows in chunks of 50 (engine.rs:195-199)
    assert out2.read_bytes() == raw


@pytest.mark.parametrize("w,h,chunk", [(200, 150, 50), (97, 61, 50), (64, 48, 7), (33, 2, 50), (16, 1, 50)])
def test_progressive_draw_matches_reference_pacing(rrt, teapot_rt, w, h, chunk):
    """rrt_render_progressive: the reference's chunked draw_scene (engine.rs:196-253).  The finished canvas equals the one-launch frame; the
    chunks arrive bottom-up (scene rows y = -H/2 .. H/2-1 map to canvas rows H-1 .. 1), one update per chunk of `chunk` scene rows, and after
    each update exactly the rows of the chunks so far are present."""
    full = teapot_rt.render(w, h)
    seen = []
    def on_update(fb, r0, n):
        seen.append((r0, n, fb.copy()))
    fb = teapot_rt.render_progressive(w, h, on_update, chunk)
    assert np.array_equal(fb, full)
    half = h // 2
    assert len(seen) == len(range(-half, half, chunk))                  # engine.rs:198: one canvas.update() per chunk
    done = np.zeros(h, bool)
    y = -half
    for r0, n, snap in seen:
        ys = range(y, min(y + chunk, half)); y += chunk
        rows = sorted(r for r in (h - (yy + half) for yy in ys) if r < h)   # put_pixel rejects new_y == h (engine.rs:152-155)
        assert (n == len(rows)) and (n == 0 or r0 == rows[0])
        done[rows] = True
        assert np.array_equal(snap[done], full[done]) and not snap[~done].any()
    sc = rrt.Scene(w, h); sc.draw_scene(teapot_rt, progressive=True)
    assert np.array_equal(sc.canvas.buffer, full) and sc.canvas.updates == len(range(-half, half, 50))   # the reference's chunk size, engine.rs:195


@pytest.mark.parametrize("mode", ["lane", "bundle", "ray", "no_cull"])
def test_deep_octree_rays_bit_exact(rrt, ob, mode):
    """Clusters of many tiny triangles a hair apart: a leaf splits whenever a second triangle arrives (octree.rs:79-92), so the tree goes ~20 levels deep
    before it separates them -- long LDS stacks, long unwinds, leaf children at every level.  Rays aimed at the triangles (and just past them) must
    return the oracle's (hit, t, u, v, triangle) bit for bit in every kernel variant."""
    rng = np.random.default_rng(21)
    tris = []
    for k in range(6):                                           # (every arrival in an occupied leaf adds one level: the resident stays, octree.rs:82-104)
        c = rng.uniform([-2.5, 0.5, 1], [2.5, 4, 6]); size = 10.0 ** rng.uniform(-6.5, -4)
        for j in range(40):
            q = c + rng.normal(size=3) * size * 6.0
            tris.append([q + np.array([-0.5, -0.4, 0.0]) * size, q + np.array([0.5, -0.4, 0.03]) * size, q + np.array([0.0, 0.5, 0.01]) * size])
    tris.append([(-6, -1, 8), (6, -1, 8), (0, 6, 8.5)])
    tris = np.array(tris, np.float64); n = len(tris)
    uv = np.tile([[0.1, 0.2, 0], [0.9, 0.1, 0], [0.5, 0.8, 0]], (n, 1, 1)).astype(np.float64); nrm = np.tile([0.0, 0.1, -1.0], (n, 3, 1))
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=240.0, kr=0.0, tex=0, bump=-1)]
    tex = [np.arange(48, dtype=np.uint8).reshape(4, 4, 3)]
    sd = rrt.SceneData.from_arrays(tris, uv, nrm, np.zeros(n, np.uint32), mats, tex)
    assert sd.info["max_depth"] >= 18, sd.info
    lights = rrt.default_lights()
    osc = oracle_for(ob, dict(pos=tris, uv=uv, nrm=nrm, mat=np.zeros(n, np.uint32), materials=mats, textures=tex), lights)
    cam = np.array(ORIGIN)
    cen = tris[:-1].mean(1)
    ext = np.abs(tris[:-1] - cen[:, None, :]).max((1, 2))
    targets = np.concatenate([cen, cen + rng.normal(size=cen.shape) * ext[:, None] * 0.6, cen + rng.normal(size=cen.shape) * ext[:, None] * 3.0])
    o = np.tile(cam, (len(targets), 1)); d = targets - cam
    rt = rrt.RayTracer(sd, lights, no_cull=True) if mode == "no_cull" else rrt.RayTracer(sd, lights, box_filter=mode)
    hit, _, _, _, tri = got = rt.intersect_rays(o, d)
    assert_rays_match_oracle(got, osc, o, d, what=f"deep octree, walk {mode}")
    assert (hit & (tri != n - 1)).sum() > 100                    # the tiny triangles in the deep leaves are really being hit
    assert_frame_close(rt.render(64, 48), osc.render(64, 48, n_threads=N_THREADS)[0], "deep-octree frame")


def test_long_own_list_with_group_records(rrt, ob):
    """A node whose own list exceeds 24 super-clusters gets group records (clusters.cpp): 2600 small triangles that all straddle the root's x = 0 or
    y = 0 split plane stay in the root list (octree.rs:82-104).  Lane filter (skips groups), bundle filter (ignores group records) and the
    reference-order mode (no index at all) must give the oracle's frame and the oracle's hits."""
    rng = np.random.default_rng(33)
    n = 2600
    c = np.stack([np.zeros(n), rng.uniform(0.3, 4.5, n), rng.uniform(-2.0, 7.0, n)], -1)
    c[n // 2:, 0] = rng.uniform(-4.0, 4.0, n - n // 2); c[n // 2:, 1] = 0.0                      # second half: across the plane y = 0
    off = rng.uniform(-0.06, 0.06, (n, 3, 3))
    off[: n // 2, 0, 0] = -0.05; off[: n // 2, 1, 0] = 0.05                                       # make sure the box really crosses the plane
    off[n // 2:, 0, 1] = -0.05; off[n // 2:, 1, 1] = 0.05
    tris = c[:, None, :] + off
    uv = rng.random((n, 3, 3)); nrm = np.tile([0.0, 0.3, -1.0], (n, 3, 1))
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=50.0, kr=0.0, tex=0, bump=-1)]
    tex = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)]
    sd = rrt.SceneData.from_arrays(tris, uv, nrm, np.zeros(n, np.uint32), mats, tex)
    assert sd.info["root_own_count"] > 24 * 64, sd.info
    lights = rrt.default_lights()
    osc = oracle_for(ob, dict(pos=tris, uv=uv, nrm=nrm, mat=np.zeros(n, np.uint32), materials=mats, textures=tex), lights)
    ref, _ = osc.render(160, 120, n_threads=N_THREADS)
    assert ((ref != 0xFFFFFF) & (ref != 0)).mean() > 0.02
    exact = rrt.RayTracer(sd, lights, no_cull=True).render(160, 120)
    assert_frame_close(exact, ref, "long list, reference order")
    assert_walks_match(lambda mode: rrt.RayTracer(sd, lights, box_filter=mode), [exact], [(160, 120)], "long list")
    cam = np.array(ORIGIN)
    tgt = tris.mean(1)[::7] + rng.normal(size=(len(tris[::7]), 3)) * 0.02
    o = np.tile(cam, (len(tgt), 1)); d = tgt - cam
    got = rrt.RayTracer(sd, lights, box_filter="lane").intersect_rays(o, d)
    assert_rays_match_oracle(got, osc, o, d, what="long list, lane filter")
    assert got[0].mean() > 0.5


def test_bench_multi_gpu_choreography_single_rank():
    """bench.py's N > 1 step -- per-slot tile buffers and streams, asynchronous RCCL gather, de-tiling on a side stream, four frames in flight, and the
    plain one-frame-at-a-time fallback -- run with ONE rank over RCCL on this GPU (RRT_BENCH_FORCE_DIST=1): the gathered, de-tiled frame must be the
    single-launch frame (same checksum), and stdout must be exactly one JSON line."""
    import json, subprocess, sys
    root = os.path.dirname(ASSETS)
    def run(env_extra, *flags):
        env = dict(os.environ, MASTER_PORT=str(_free_port()), **env_extra)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--no-cpu-baseline", "--steps", "6", "--warmup", "2", "--width", "320", "--height", "240", *flags],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    single = run({}, "--full")                                                            # --full: host_fb and first_frame are asserted below
    both = run({"RRT_BENCH_FORCE_DIST": "1"})                                             # default (auto): K steps of each path, the faster one reported
    inlib = run({"RRT_BENCH_FORCE_DIST": "1"}, "--gather", "lib")                         # the library's own gather (rrt_dist_create / rrt_multi_enqueue)
    piped = run({"RRT_BENCH_FORCE_DIST": "1"}, "--gather", "torch")
    plain = run({"RRT_BENCH_FORCE_DIST": "1"}, "--gather", "torch", "--pipeline-depth", "0")
    assert single["frame_checksum"] == inlib["frame_checksum"] == piped["frame_checksum"] == plain["frame_checksum"] == both["frame_checksum"]
    assert set(both["gather_paths"]) == {"torch", "lib"} and both["gather_paths"]["lib"]["frame_checksum"] == both["gather_paths"]["torch"]["frame_checksum"] == single["frame_checksum"]
    assert both["gather"] in ("lib", "torch") and both["value"] == max(both["gather_paths"]["lib"]["value"], both["gather_paths"]["torch"]["value"])
    assert single["n_gpus"] == 1 and single["unit"] == "Mrays/s"
    assert inlib["gather"] == "lib" and piped["gather"] == "torch" and inlib["pipeline_fallback"] is False and inlib["gather_ms"] is not None
    assert "frame_ms_host_fb" in single and single["host_fb"]["identical_to_device_frame"] and "setup_ms" in single
    assert single["first_frame"]["identical_to_steady_frame"] and single["first_frame_ms"] > 0
    # A library path that never finishes (test hook: the child sleeps before rrt_dist_create): the GPU-free supervisor kills that child group at its
    # timeout, reports the stage it hung in, prints the torch path's line and exits 0 -- nothing is decided by a process that holds the GPU.
    hung = run({"RRT_BENCH_FORCE_DIST": "1", "RRT_BENCH_TEST_HANG": "lib"}, "--lib-timeout", "40")
    err = hung["gather_paths"]["lib"]["error"]
    assert hung["gather"] == "torch" and hung["frame_checksum"] == single["frame_checksum"] and "timed out" in err and "RRT_BENCH_TEST_HANG" in err, err
    text = open(os.path.join(root, "bench.py")).read()
    assert "os._exit" not in text and "watchdog()" not in text


@pytest.mark.gpu
def test_per_ray_entry_points_pick_their_own_variant(rrt, teapot):
    """rrt_intersect_rays / rrt_get_ray_colours measure the three traversal variants on the first large batch and keep the fastest (scattered rays:
    the ray walk, up to 3x faster than the node-coherent walks); whatever is picked, results are those of the exact mode, and a forced variant
    is used as is.  rrt_last_stats reports the kernel time and the variant of the per-ray launch."""
    rng = np.random.default_rng(23)
    n = 1 << 16
    o = rng.uniform([-5, -0.5, -8], [5, 6, 5], (n, 3)); d = rng.normal(size=(n, 3))
    exact = rrt.RayTracer(teapot, rrt.default_lights(), no_cull=True)
    ref = exact.intersect_rays(o, d)
    auto = rrt.RayTracer(teapot, rrt.default_lights())
    small = auto.intersect_rays(o[:1000], d[:1000])                      # below the tuning threshold: the frame variant (none measured yet: lane)
    assert auto.last_stats()["filter_variant"] == 0
    for x, y in zip(small, ref): assert np.array_equal(x, y[:1000])
    got = auto.intersect_rays(o, d)
    st = auto.last_stats()
    assert st["filter_variant"] in (0, 1, 2) and st["kernel_ms"] > 0 and st["width"] == n
    picked = st["filter_variant"]
    for x, y in zip(got, ref): assert np.array_equal(x, y)
    assert np.array_equal(auto.get_ray_colours(o[:20000], d[:20000]), exact.get_ray_colours(o[:20000], d[:20000]))
    assert auto.last_stats()["filter_variant"] == picked                 # measured once per raytracer
    forced = rrt.RayTracer(teapot, rrt.default_lights(), box_filter="bundle")
    for x, y in zip(forced.intersect_rays(o, d), ref): assert np.array_equal(x, y)
    assert forced.last_stats()["filter_variant"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e-13, 1e-9, 1e6, 1e9, 1e12])
def test_direction_magnitude_does_not_matter_to_the_index(rrt, teapot, scale):
    """The reference never normalises a direction (t simply scales inversely), so rays with tiny or huge direction vectors -- some with exactly zero
    components, which the fp32 filter treats as parallel to their slabs -- must give the same triangle and (u, v) with the index as without it, and
    the same as the unscaled rays; t scales by 1/scale up to rounding.  (Directions beyond the filter's working range run unfiltered.)"""
    rng = np.random.default_rng(31)
    n = 20000
    o = rng.uniform([-5, -0.5, -8], [5, 6, 5], (n, 3)); d = rng.normal(size=(n, 3))
    d[:3000, rng.integers(0, 3, 3000)] *= 0.0                              # (fancy indexing: zero one random component of the first 3000 rays)
    d[np.arange(3000), rng.integers(0, 3, 3000)] = 0.0
    exact = rrt.RayTracer(teapot, rrt.default_lights(), no_cull=True)
    ref = exact.intersect_rays(o, d * scale)
    base = exact.intersect_rays(o, d)
    assert np.array_equal(ref[0], base[0]) or scale in (1e-13, 1e12)        # (at the extremes t > eps / a within eps may flip a few borderline hits)
    for mode in ("lane", "bundle", "ray"):
        got = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode).intersect_rays(o, d * scale)
        for x, y in zip(got, ref): assert np.array_equal(x, y), (mode, scale)


@pytest.mark.gpu
def test_triangles_poking_out_of_the_root_box(rrt, ob):
    """The single-candidate shortcut of the bundle-filter kernel (render.hip: a ray that certainly crosses the child's shrunk SUBTREE box needs no f64 slab test
    of the OCTANT box) relies on subtree boxes lying inside their octants, which fails when a triangle of the tree reaches beyond the root box: such scenes
    must switch it off.  Scene: a small root, a wall of triangles inside it and slivers that stick out through its faces; rays that reach the slivers' outer
    parts pass the root (and their child octant) by, so the reference does not find them there.  Frames of all variants against the oracle, bit for bit, from two
    origins; the same scene shrunk to fit inside the root exercises the shortcut itself."""
    rng = np.random.default_rng(77)
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0.3, 0.3, 0.3), ns=40.0, kr=0.0, tex=0, bump=-1)]
    tex = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)]
    lights = rrt.default_lights()
    def scene(reach):
        tris = []
        for _ in range(400):                                            # a wall of small triangles inside the root
            c = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(-0.2, 0.9)])
            tris.append(c + rng.uniform(-0.08, 0.08, (3, 3)))
        for _ in range(60):                                             # slivers through the +x, -x and +y faces, each well inside one octant otherwise
            y, z = rng.uniform(0.2, 0.8) * rng.choice([-1, 1]), rng.uniform(0.2, 0.8) * rng.choice([-1, 1])
            side = rng.choice([-1.0, 1.0])
            tris.append(np.array([[side * 0.6, y, z], [side * reach, y + 0.05, z], [side * reach, y - 0.05, z + 0.05]]))
            x = rng.uniform(0.2, 0.8) * rng.choice([-1, 1])
            tris.append(np.array([[x, 0.6, z], [x + 0.05, reach, z], [x - 0.05, reach, z + 0.05]]))
        for sx, sy, sz in ((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, 1)):   # sails: inside one octant in y and z, far out of the root in x -- whole waves of rays cross only their outer part
            tris.append(np.array([[sx * 0.6, sy * 0.5, sz * 0.5], [sx * reach * 1.2, sy * 0.1, sz * 0.9], [sx * reach * 1.2, sy * 0.9, sz * 0.1]]))
        pos = np.ascontiguousarray(np.array(tris))
        n = len(pos)
        return pos, rng.random((n, 3, 3)), rng.normal(size=(n, 3, 3)), np.zeros(n, np.uint32)
    root = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
    for reach in (2.5, 0.95):
        pos, uv, nrm, mat = scene(reach)
        sd = rrt.SceneData.from_arrays(pos, uv, nrm, mat, mats, tex, root=root)
        for origin in ((0.0, 0.0, -3.5), (1.5, 0.4, -3.0)):                # (inside the filter's range of 4 x the scene magnitude: farther origins switch the fp32 filters off altogether)
            osc = oracle_for(ob, dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=mats, textures=tex, root=root), lights, origin)
            want, _ = osc.render(480, 360, n_threads=N_THREADS)
            assert_walks_match(lambda mode: rrt.RayTracer(sd, lights, rrt.Vector3d(*origin), box_filter=mode), [want], [(480, 360)],
                               f"reach {reach}, origin {origin}, against the oracle")
        assert ((want != 0xFFFFFF) & (want != 0)).mean() > 0.02


def test_bench_two_ranks_in_both_launch_modes_rehearsal():
    """bench.py --gpus 2 end to end with TWO rank processes (RRT_BENCH_REHEARSAL=1: both ranks on this box's one GPU, the collective over gloo -- RCCL refuses
    two ranks on one device; numbers from it are not results): (a) started plainly -- the GPU-free supervisor starts one torch.distributed.run per gather
    path; (b) started the way the driver does, as ranks under torch.distributed.run -- every rank supervises its own children, which rendezvous on a port of
    their own.  Either way: rc 0, exactly one JSON line, n_gpus 2, and the gathered, de-tiled frame is the single-GPU frame."""
    import json, subprocess, sys
    root = os.path.dirname(ASSETS)
    common = ["--no-cpu-baseline", "--steps", "4", "--warmup", "1", "--width", "320", "--height", "240", "--torch-timeout", "240", "--lib-timeout", "240"]
    def one_line(r):
        assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2500:])
        lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    port, port2 = _free_port(), _free_port()
    env = dict(os.environ, RRT_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    single = one_line(subprocess.run([sys.executable, os.path.join(root, "bench.py"), *common, "--no-first-frame", "--no-host-fb"], capture_output=True, text=True, env=dict(os.environ), timeout=600))
    plain = one_line(subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", *common], capture_output=True, text=True, env=env, timeout=900))
    launched = one_line(subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port2),
                                        os.path.join(root, "bench.py"), "--gpus", "2", *common], capture_output=True, text=True, env=dict(os.environ, RRT_BENCH_REHEARSAL="1"), timeout=900))
    for out in (plain, launched):
        assert out["n_gpus"] == 2 and out["frame_checksum"] == single["frame_checksum"] and "rehearsal" in out and set(out["gather_paths"]) == {"torch", "lib"}
        assert all("error" not in v for v in out["gather_paths"].values()), out["gather_paths"]


@pytest.mark.gpu
def test_gpu_frame_matches_the_references_screenshot(rrt, teapot, teapot_rt):
    """The GPU frame of model2.obj at 800 x 800 against the fixture derived from the reference's one image (example_output.png, a lossless screenshot of an
    older build's canvas; tests/golden/make_example_mask.py): on the teapot above its contact zone with the table -- geometry, material, lights and camera
    unchanged since -- the pixels the HIP kernels produce are the reference's own: >= 80 % bit-equal, >= 92 % within one unit per channel (measured 86 % /
    94.5 %, the same figures as the oracle's frame; the rest are grazing-shadow edges where the old build differed), and canvas row 0 is black in both.
    The teapot pixels are selected with rrt_intersect_rays (all four sub-sample rays hit a teapot triangle, lowest hit at height >= 0.6)."""
    from conftest import GOLDEN
    m = np.load(os.path.join(GOLDEN, "example_output_mask.npz"))
    W = H = 800
    fb = teapot_rt.render(W, H)
    mine = channels(fb)
    ref_mask = np.unpackbits(m["mask_bits"])[:W * H].reshape(H, W).astype(bool)
    assert (fb[0] == 0).all() and ref_mask[0].all()
    _, _, _, mat = teapot.triangles()
    teapot_mat = int(np.argmax(np.bincount(mat)))
    r0, r1, c0, c1 = map(int, m["teapot_box"])
    rows, cols = np.meshgrid(np.arange(r0, r1, 3), np.arange(c0, c1, 3), indexing="ij")
    rows, cols = rows.ravel(), cols.ravel()
    y, x = (H - H // 2) - rows, cols - W // 2
    ok = np.ones(len(rows), bool); low = np.full(len(rows), np.inf)
    for dx, dy in ((0, 0), (.5, 0), (0, .5), (.5, .5)):
        d = np.stack([(x + dx) * (1.0 / W), (y + dy) * (1.0 / H), np.ones(len(x))], -1)
        hit, t, _, _, tri = teapot_rt.intersect_rays(np.tile(ORIGIN, (len(x), 1)), d)
        ok &= hit & (mat[np.minimum(tri, len(mat) - 1)] == teapot_mat)
        low = np.minimum(low, np.where(hit, 2.0 + d[:, 1] * t, np.inf))
    sel = ok & (low >= 0.6)
    assert sel.sum() > 6000
    diff = np.abs(mine[rows[sel], cols[sel]] - m["teapot_rgb"].astype(np.int64)[rows[sel] - r0, cols[sel] - c0]).max(-1)
    assert (diff <= 1).mean() >= 0.92 and (diff == 0).mean() >= 0.80, ((diff <= 1).mean(), (diff == 0).mean())
