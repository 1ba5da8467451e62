"""Root boxes of other scales and positions than the reference's +-20 cube, against the CPU oracle built on the same root.

The root box is an argument of the ABI, and much of the set-up scales with scene_magnitude = max |root coordinate| (clusters.cpp, scene_build.hip): the
index pad 2^-15 mag and the outward rounding of every fp32 box, cull_limit = 4 mag and the working range of make_ray32 (render.hip), the shrink of the
chain records, alpha / delta of the exactness guard, DevScene::bounds_plain, and the absolute constants of mt_uniform (|a| < 1e100, 1e-200).

Every test takes a scene and maps it with p' = p s + shift, computed once in f64 (`Placement.pt`); the GPU and the oracle get the SAME arrays.  The root
box, the eye, the point lights' positions and surface_offset = 1e-4 s go through the same map; direction vectors and the Directional light do not.

    id                  s, shift / root                              regime it reaches
    small_pow2          2^-10                                        primary rays (d.z = 1 > limit = 4 mag) run unfiltered; only scene-sized directions are filtered
    small_dec           1e-3                                         no power of two: every coordinate is re-rounded
    near_eps            2^-18                                        a is close to f64 epsilon: the parallel rejection (ray.rs:66) decides many pairs
    large               2^40
    f32_denormal_scale  2^120                                        cull_limit ~ 1.06e38 is finite, 0.5 / limit is a denormal float
    f32_overflow        2^122                                        (float)(4 mag) = +inf
    a_beyond_1e100      2^180                                        mt_uniform's a_ok is false; node planes still inside 2^200
    bounds_not_plain    2^200                                        bounds_plain is false, and so is org_plain of the eye
    shifted             1, (1000.3, -517.7, 333.1)                   fp32 ulp 6e-5 against 0.1-sized triangles; the pad is 0.03
    scaled_shifted      0.37, (-55.5, 7.25, 90.1)
    far_shift           1, (1e9, 1e9, -1e9)                          the pad (3e4) exceeds the root: every box must pass; f64 ulp is 1.2e-7
    anisotropic         root (-20.1, 19.7, -3.3, 14.9, -12.7, 28.3)  non-cubic octants, rounded split planes
    cutting             root (-2.9, 6.3, -0.45, 7.7, -6.1, 3.2)      the reference drops the triangles that do not lie inside the root (octree.rs:71-73)

No pixel or ray is exempted: every indexed mode is compared bit for bit with the reference-order (no_cull) walk, and that one with the oracle (frames and
ray colours within COLOUR_TOL, assert_frame_close's default).

What these tests found (fixed with them): from s = 2^126 on a ray origin converts to +-inf in fp32, and make_ray32's n = -o * inv was inf * 0 = NaN for the
lane whose filter is off -- every box a miss, the ray hit nothing in any walk, no_cull included (a_beyond_1e100 and bounds_not_plain: every ray of
test_rays_match_the_oracle missed, 1725 pixels of the frame differed by up to 175); and rrt_stats.filter_pad was derived from the fp32 cull_limit (test 2,
every placement whose magnitude is no fp32 number).

Input conditions (test_placements_hold_on_the_cpu, from the oracle alone), threshold <- measured:
    frame 96 x 72, pixels of rows >= 1 that differ from the miss colour       >= 0.4       <- 0.603 for every placement
    ray batch, rays that hit                                                  >= 0.5       <- 0.647 (small_dec) .. 0.671 (shifted, cutting)
    `cutting` keeps fewer triangles than it was given                         < 6334       <- 6059 (275 dropped), depth 9
    `anisotropic` max_depth                                                   >= 9         <- 11
    `shifted`, in-plane triangles of the guard scene within delta of the apex >= 50 of 60  <- 60
"""
import numpy as np
import pytest

from bitwise import assert_same_arrays
from gpu_checks import (ALL_MODES, CHAIN_CAMERA, CHAIN_LIGHTS, FORCED_MODES, N_THREADS, ORIGIN, POOL, ROOT_BOX, PlainLight, assert_frame_close,
                        assert_rays_match_oracle, chain_main_rays, chain_scene, check_scene, coplanar_rays, oracle_for, oracle_pixels, origin_within_delta,
                        plane_scene, plane_scene_data, rrt_lights_of, traced_rows)
from placements import PLACEMENTS, Placement
from scenes import IDENTITY, TARGET

W, H = 96, 72
N_RAYS, N_COLOURS = 4096, 1024
RESULTS = ("hit", "t", "u", "v", "tri")                        # what intersect_rays returns, in its order
MIN_FRAME, MIN_HITS, MIN_DEPTH, MIN_GUARD = 0.4, 0.5, 9, 50      # measured: 0.603, 0.647 .. 0.671, 11, 60 (module docstring)


ALL_IDS = list(PLACEMENTS)
CAMERA_IDS = ("small_pow2", "shifted", "f32_denormal_scale")
SCENE_IDS = ("small_pow2", "large", "shifted")                    # the guard and the chains


# ------------------------------------------------------------------ the placed teapot, its oracle and its ray batch: built once per placement
_placed = {}


def cull_limit32(P):
    """DevScene::cull_limit: (float)(4 mag)."""
    with np.errstate(over="ignore"):
        return np.float32(4.0 * P.mag)


def filtered_half(P):
    """Which half of the batch is meant to lie in make_ray32's range: the rays of scene-sized directions (0) for a small scene, those of unit-sized ones (1)."""
    return 0 if P.mag < 1.0 else 1


def ray_batch(P, osc, seed=0):
    """N_RAYS rays: origins uniform in the inner half of the mapped +-20 cube, targets in its inner quarter (for the two placements that are given a root
    of their own, that cube lies around the scene and the root does not); even rays get directions of length mag 10^U(-1,0), odd rays of
    length 10^U(-1,0); every third ray carries max_t = the oracle's t x U(0.5, 1.5) (the shadow form, on both sides of the hit)."""
    rng = np.random.default_rng([seed, ALL_IDS.index(P.id)])
    r = np.asarray(P.box).reshape(3, 2); c = r.mean(1); hw = (r[:, 1] - r[:, 0]) * 0.5
    O = c + rng.uniform(-0.5, 0.5, (N_RAYS, 3)) * hw; T = c + rng.uniform(-0.25, 0.25, (N_RAYS, 3)) * hw
    u = T - O; u /= np.linalg.norm(u, axis=1)[:, None]
    length = 10.0 ** rng.uniform(-1.0, 0.0, N_RAYS); length[0::2] *= P.mag
    D = u * length[:, None]
    free = list(POOL.map(lambda i: osc.intersect(O[i], D[i]), range(N_RAYS)))
    hit = np.array([f[0] for f in free]); t = np.array([f[1] for f in free])
    M = np.full(N_RAYS, np.inf)
    k = np.arange(N_RAYS) % 3 == 0
    M[k & hit] = (t * rng.uniform(0.5, 1.5, N_RAYS))[k & hit]
    return O, D, M, hit


def placed(ob, rrt, teapot, pid):
    if pid not in _placed:
        P = PLACEMENTS[pid]
        pos, uv, nrm, mat = teapot.triangles()
        A = P.arrays(dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=teapot.materials(), textures=teapot.textures()))
        lights = P.lights(rrt.default_lights())
        eye = tuple(P.pt(ORIGIN))
        osc = oracle_for(ob, A, lights, origin=eye, surface_offset=P.offset)
        O, D, M, hit = ray_batch(P, osc)
        _placed[pid] = dict(P=P, A=A, lights=lights, eye=eye, osc=osc, frame=osc.render(W, H, n_threads=N_THREADS)[0], O=O, D=D, M=M, hit=hit)
    return _placed[pid]


def scene_data(rrt, A):
    return rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"], root=A["root"])


def raytracer(rrt, S, **kw):
    """A raytracer of the placed scene S (dict: sd, lights, eye, P)."""
    return rrt.RayTracer(S["sd"], rrt_lights_of(rrt, S["lights"]), rrt.Vector3d(*S["eye"]), surface_offset=S["P"].offset, **kw)


def gpu_scene(ob, rrt, teapot, pid):
    S = placed(ob, rrt, teapot, pid)
    if "sd" not in S:
        S["sd"] = scene_data(rrt, S["A"])
    return S


def in_filter_range(P, O, D):
    """make_ray32's range conditions (render.hip) in numpy's float32: |o| < limit, 1e-10 < max|d| < min(limit, 1e8), every component a number."""
    limit = cull_limit32(P)
    with np.errstate(over="ignore"):
        o, d = O.astype(np.float32), D.astype(np.float32)
    dmax = np.abs(d).max(1)
    return (np.abs(o) < limit).all(1) & ~np.isnan(d).any(1) & (dmax < limit) & (dmax > np.float32(1e-10)) & (dmax < np.float32(1e8))


# ------------------------------------------------------------------ 1: the inputs, from the oracle alone
def guard_scene(P):
    """plane_scene at the reference pose, mapped: 12 planes x 5 triangles through the eye, 300 others, a backdrop; 20 000 rays generated AFTER the map from
    the mapped triangles."""
    apex = np.array(ORIGIN)
    tris, planes = plane_scene(np.random.default_rng(77), apex, 12, 5, 300)
    tris, apex = P.pt(tris), P.pt(apex)
    O, D = coplanar_rays(np.random.default_rng(78), tris, planes, 60, apex, 20_000)
    return tris, apex, O, D


@pytest.mark.parametrize("pid", ALL_IDS)
def test_placements_hold_on_the_cpu(ob, rrt, teapot, pid):
    S = placed(ob, rrt, teapot, pid); P, osc = S["P"], S["osc"]
    away = (0.0, 0.0, -1.0)                                                      # the scene lies in front of the eye
    assert not osc.intersect(S["eye"], away)[0]
    miss = osc.get_ray_colour(S["eye"], away)
    frac = float((S["frame"][1:] != miss).mean())
    hits = float(S["hit"].mean())
    tree = osc.octree()
    print(f"\n[placement {pid}] mag {P.mag!r}, frame {frac:.3f} of the pixels not the miss colour, {hits:.3f} of the rays hit, "
          f"{int(tree['tri_count'][0])} of {len(S['A']['pos'])} triangles in the tree, depth {tree['max_depth']}")
    assert frac >= MIN_FRAME, f"{pid}: only {frac:.3f} of the frame's pixels show the scene (< {MIN_FRAME})"
    assert hits >= MIN_HITS, f"{pid}: only {hits:.3f} of the batch's rays hit (< {MIN_HITS})"
    assert len(S["O"]) == N_RAYS and np.isfinite(S["M"]).sum() >= N_RAYS // 8, "rays with a finite max_t"
    if np.isfinite(cull_limit32(P)):
        half = filtered_half(P)
        ok = in_filter_range(P, S["O"][half::2], S["D"][half::2])
        assert ok.all(), f"{pid}: {(~ok).sum()} of the {len(ok)} rays meant to be filtered lie outside make_ray32's range"
    else:
        assert pid in ("f32_overflow", "a_beyond_1e100", "bounds_not_plain"), pid
    if pid == "f32_denormal_scale":
        h = np.float32(0.5) / cull_limit32(P)
        assert 0.0 < h < np.finfo(np.float32).tiny, f"0.5 / limit = {h!r} is no denormal float"
    if pid == "cutting":
        assert int(tree["tri_count"][0]) < len(S["A"]["pos"]), "the root of `cutting` cuts no triangle off"
    if pid == "anisotropic":
        assert tree["max_depth"] >= MIN_DEPTH, f"anisotropic: depth {tree['max_depth']} (< {MIN_DEPTH})"
    if pid == "shifted":
        tris, apex, _, _ = guard_scene(P)
        n = int(origin_within_delta(tris[:60], apex, P.pad).sum())
        print(f"[placement {pid}] guard scene: {n} of the 60 in-plane triangles lie within delta of the mapped apex")
        assert n >= MIN_GUARD, f"shifted: only {n} of the 60 in-plane triangles lie within delta of the apex (< {MIN_GUARD})"


# ------------------------------------------------------------------ 2: set-up
@pytest.mark.gpu
@pytest.mark.parametrize("pid", ALL_IDS)
def test_setup_matches_host_and_oracle(rrt, ob, teapot, pid):
    S = gpu_scene(ob, rrt, teapot, pid)
    check_scene(rrt, S["sd"], f"placement {pid}", ob=ob, origin=rrt.Vector3d(*S["eye"]))


# ------------------------------------------------------------------ 3: frames
@pytest.mark.gpu
@pytest.mark.parametrize("pid", ALL_IDS)
def test_frames_match_no_cull_and_the_oracle(rrt, ob, teapot, pid):
    S = gpu_scene(ob, rrt, teapot, pid)
    exact = raytracer(rrt, S, no_cull=True).render(W, H)
    assert_frame_close(exact, S["frame"], f"placement {pid}, no_cull frame vs oracle")
    assert np.array_equal(exact == 0, S["frame"] == 0), f"placement {pid}: unwritten pixels differ from the oracle's"
    for mode in ALL_MODES:
        got = raytracer(rrt, S, box_filter=mode).render(W, H)
        bad = np.argwhere(got != exact)
        assert len(bad) == 0, f"placement {pid}, walk {mode}: {len(bad)} of {W * H} pixels differ from the no_cull frame (first {bad[:3].tolist()})"


# ------------------------------------------------------------------ 4: rays
@pytest.mark.gpu
@pytest.mark.parametrize("pid", ALL_IDS)
def test_rays_match_the_oracle(rrt, ob, teapot, pid):
    S = gpu_scene(ob, rrt, teapot, pid); osc, O, D, M = S["osc"], S["O"], S["D"], S["M"]
    if "colours" not in S:
        S["colours"] = np.fromiter(POOL.map(lambda i: osc.get_ray_colour(O[i], D[i]), range(N_COLOURS)), np.uint32, N_COLOURS)
    for mode in FORCED_MODES + ("no_cull",):
        rt = raytracer(rrt, S, no_cull=True) if mode == "no_cull" else raytracer(rrt, S, box_filter=mode)
        n_hit = assert_rays_match_oracle(rt.intersect_rays(O, D, M), osc, O, D, M, f"placement {pid}, walk {mode}", min_rays=N_RAYS)
        assert 0 < n_hit < int(S["hit"].sum()), f"placement {pid}: {n_hit} hits with max_t, {int(S['hit'].sum())} without: max_t cuts nothing off"
        assert_rays_match_oracle(rt.intersect_rays(O, D), osc, O, D, None, f"placement {pid}, walk {mode}, no max_t", min_hit_frac=MIN_HITS)
        assert_frame_close(rt.get_ray_colours(O[:N_COLOURS], D[:N_COLOURS]), S["colours"], f"placement {pid}, walk {mode}, ray colours")


# ------------------------------------------------------------------ 5: the camera
EYES = ((6.0, 3.0, -8.0), (-7.0, 4.0, -6.0))


@pytest.mark.gpu
@pytest.mark.parametrize("pid", CAMERA_IDS)
def test_a_moved_camera_equals_one_created_there(rrt, ob, teapot, pid):
    S = gpu_scene(ob, rrt, teapot, pid); P = S["P"]
    w, h = 64, 48
    rows, xs = traced_rows(h), np.arange(0, w, 2)
    for e in EYES:
        eye = tuple(P.pt(e))
        turned = rrt.look_at(eye, tuple(P.pt(TARGET)))
        ref_turned = oracle_pixels(S["osc"], turned, w, h, rows, xs, f"placement {pid}, eye {e} turned to the target")
        for mode in ALL_MODES:
            what = f"placement {pid}, eye {e}, walk {mode}"
            moved = raytracer(rrt, S, box_filter=mode)
            moved.set_camera(eye, **IDENTITY)
            fresh = raytracer(rrt, dict(S, eye=eye), box_filter=mode)
            assert_frame_close(moved.render(W, H), fresh.render(W, H), what + ": moved vs created there", tol=0)
            assert moved.last_stats()["origin_plane_triangles"] == fresh.last_stats()["origin_plane_triangles"], what
            assert np.array_equal(moved.buffer("suspects"), fresh.buffer("suspects")), what + ": suspect lists differ"
            moved.set_camera(**turned); fresh.set_camera(**turned)
            got = moved.render(w, h)
            assert_frame_close(got, fresh.render(w, h), what + ", turned: moved vs created there", tol=0)
            assert_frame_close(got[np.ix_(rows, xs)], ref_turned, what + ", turned: frame vs oracle rays")


# ------------------------------------------------------------------ 6: the guard
@pytest.mark.gpu
@pytest.mark.parametrize("pid", SCENE_IDS)
def test_the_guard_at_other_scales(rrt, pid):
    P = PLACEMENTS[pid]
    lights = rrt.default_lights()
    tris, apex, O, D = guard_scene(P)
    sd = plane_scene_data(rrt, tris, root=P.root)
    E = rrt.Vector3d(*apex)
    exact = rrt.RayTracer(sd, lights, E, no_cull=True).intersect_rays(O, D)
    assert 0.2 < exact[0].mean() <= 1.0
    inside = in_filter_range(P, O, D).mean()
    assert 0.2 < inside, f"placement {pid}: only {inside:.3f} of the guard's rays lie in the filter's range"
    counts = []
    for mode in ("lane", "bundle", None):
        rt = rrt.RayTracer(sd, lights, E, box_filter=mode)
        counts.append(rt.last_stats()["origin_plane_triangles"])
        assert_same_arrays(dict(zip(RESULTS, rt.intersect_rays(O, D))), dict(zip(RESULTS, exact)), what=f"placement {pid}, walk {mode} vs the reference-order walk")
    assert len(set(counts)) == 1, counts
    if P.pow2:                                                   # the construction scales exactly: unit normal, squared-sine threshold and alpha are scale-free, delta ~ s
        t0, a0, _, _ = guard_scene(Placement("reference"))
        plain = rrt.RayTracer(plane_scene_data(rrt, t0), lights, rrt.Vector3d(*a0), box_filter="lane")
        assert counts[0] == plain.last_stats()["origin_plane_triangles"] >= 60, (counts, plain.last_stats()["origin_plane_triangles"])
        assert np.array_equal(rt.buffer("suspects"), plain.buffer("suspects")), f"placement {pid}: the suspect list is not the unscaled scene's, byte for byte"
    else:
        n = int(origin_within_delta(tris[:60], apex, P.pad).sum())
        assert n >= MIN_GUARD, n
        assert counts[0] >= n, f"placement {pid}: {counts[0]} suspects, but {n} in-plane triangles lie within delta of the apex"


# ------------------------------------------------------------------ 7: the chains
def placed_chain_scene(ob, P):
    """The hand-built chain scene (gpu_checks.chain_scene), its rays and its camera, mapped.  Directions are scaled with a scene smaller than the
    reference's and kept for a larger one, so they stay inside the filter's range; max_t follows."""
    A, _ = chain_scene("main")
    A = P.arrays(A)
    R = chain_main_rays()
    O = P.pt(np.concatenate([R[k][0] for k in R])); D = np.concatenate([R[k][1] for k in R]) * min(P.s, 1.0); M = np.concatenate([R[k][2] for k in R]) * max(P.s, 1.0)
    lights, eye = P.lights(CHAIN_LIGHTS), tuple(P.pt(CHAIN_CAMERA))
    osc = oracle_for(ob, A, lights, origin=eye, surface_offset=P.offset)
    return dict(P=P, A=A, lights=lights, eye=eye, osc=osc, O=O, D=D, M=M)


@pytest.mark.gpu
@pytest.mark.parametrize("pid", SCENE_IDS)
def test_chains_at_other_scales(rrt, ob, pid):
    P = PLACEMENTS[pid]
    S = placed_chain_scene(ob, P); S["sd"] = scene_data(rrt, S["A"])
    osc, O, D, M = S["osc"], S["O"], S["D"], S["M"]
    ok = in_filter_range(P, O, D)
    assert ok.all(), f"placement {pid}: {(~ok).sum()} of the chain scene's rays lie outside the filter's range"
    plain = placed_chain_scene(ob, Placement("reference")); plain["sd"] = scene_data(rrt, plain["A"])
    want = raytracer(rrt, plain, box_filter="bundle").chain_info
    assert want["n_chains"] > 0, want
    colours = np.fromiter((osc.get_ray_colour(O[i], D[i]) for i in range(len(O))), np.uint32, len(O))
    frame = osc.render(160, 120, n_threads=N_THREADS)[0]
    assert (frame[1:] != frame[1, 0]).mean() > 0.01, "the chain scene's frame shows nothing"
    for mode in FORCED_MODES:
        for on in (True, False):
            what = f"placement {pid}, walk {mode}, shortcut {'on' if on else 'off'}"
            rt = raytracer(rrt, S, box_filter=mode, chain_shortcut=on)
            if P.pow2:
                assert rt.chain_info == want, (what, rt.chain_info, want)
            else:                                                # the pad is 50 times the reference's there and may empty the shrunk end box
                assert rt.chain_info["n_chains"] <= want["n_chains"] and rt.chain_info["n_chain_nodes"] <= want["n_chain_nodes"], (what, rt.chain_info, want)
            assert assert_rays_match_oracle(rt.intersect_rays(O, D, M), osc, O, D, M, what) > 0
            assert_frame_close(rt.get_ray_colours(O, D), colours, what + " (colours)")
            assert_frame_close(rt.render(160, 120), frame, what + ", frame")
    exact = raytracer(rrt, S, no_cull=True)
    assert exact.chain_info == {"n_chains": 0, "n_chain_nodes": 0}
    assert_rays_match_oracle(exact.intersect_rays(O, D, M), osc, O, D, M, f"placement {pid}, no_cull")
