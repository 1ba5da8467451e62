"""Constants, scene builders, ray generators and oracle checks shared by the GPU test modules (and tools/band_count.py).

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import channels, lights_tuple

COLOUR_TOL = 1                               # per RGB channel: only pow() (raytracer.rs:295) may differ by an ulp between glibc and OCML
ALL_MODES = (None, "lane", "bundle", "ray")  # the autotuned default and the three forced walk variants
FORCED_MODES = ("lane", "bundle", "ray")
ORIGIN = (0.0, 2.0, -10.0)                   # the reference's camera (main.rs)
ROOT_BOX = (-20.0, 20.0, -20.0, 20.0, -20.0, 20.0)
N_THREADS = 16                               # host threads for the oracle: its renders and POOL
POOL = ThreadPoolExecutor(N_THREADS)         # oracle calls from Python (ctypes releases the GIL)


# ------------------------------------------------------------------ the oracle
def oracle_for(ob, A, lights, origin=ORIGIN, **opt):
    """The oracle scene of the arrays dict A (pos, uv, nrm, mat, materials, textures, optional root); opt: surface_offset, max_reflection_depth."""
    return ob.OracleScene(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"], lights_tuple(lights), origin, A.get("root", ROOT_BOX),
                          **opt)


def assert_frame_close(gpu, ref, what, tol=COLOUR_TOL):
    """Packed RGB frames (or ray colours) within tol per channel (tol=0: bit-exact); returns the per-pixel max channel difference."""
    d = np.abs(channels(gpu) - channels(ref)).max(-1)
    assert d.max() <= tol, f"{what}: max channel diff {d.max()} (> {tol}) on {(d > tol).sum()} of {d.size} pixels"
    return d


def assert_rays_match_oracle(got, osc, O, D, M=None, what="rays", min_rays=0, min_hit_frac=0.0, uv=True):
    """got = (hit, t, u, v, tri) of intersect_rays(O, D, M): hit/miss, t, u, v and triangle bit for bit as osc.intersect (uv=False: hit/miss, t and
    triangle only).  At least min_rays rays, at least min_hit_frac of them hitting.  Returns the number of hits."""
    assert len(O) >= min_rays, f"{what}: {len(O)} rays (< {min_rays})"
    hit, t, u, v, tri = got
    M = np.full(len(O), np.inf) if M is None else M
    ref = list(POOL.map(lambda i: osc.intersect(O[i], D[i], M[i]), range(len(O))))
    n_hit = 0
    for i, (rh, rt_, ru, rv, rtri) in enumerate(ref):
        assert bool(hit[i]) == rh, f"{what}, ray {i}: hit {bool(hit[i])} vs oracle {rh}"
        if rh:
            n_hit += 1
            mine, want = ((t[i], u[i], v[i], tri[i]), (rt_, ru, rv, rtri)) if uv else ((t[i], tri[i]), (rt_, rtri))
            assert mine == want, f"{what}, ray {i}: {mine!r} vs oracle {want!r}"
    assert n_hit >= min_hit_frac * len(O), f"{what}: {n_hit} of {len(O)} rays hit (< {min_hit_frac} of them)"
    return n_hit


def assert_walks_match(make_rt, frames, sizes, what, modes=ALL_MODES, rays=None, in_band=None):
    """For each walk variant in modes, make_rt(mode)'s frame of each size equals the reference frame bit for bit, and with rays = (O, D, colours)
    its get_ray_colours(O, D) equals colours.  in_band(w, h, row, col) -> bool: a differing pixel is allowed where it returns True (the exactness
    band of include/rrt.h).  Returns the number of such band pixels."""
    n_band = 0
    for mode in modes:
        rt = make_rt(mode)
        for (w, h), ref in zip(sizes, frames):
            bad = np.argwhere(rt.render(w, h) != ref)
            assert in_band is not None or len(bad) == 0, f"{what}, walk {mode}, {w}x{h}: {len(bad)} of {w * h} pixels differ from the reference frame"
            for r, c in bad:
                assert in_band(w, h, r, c), f"{what}, walk {mode}, {w}x{h}: pixel ({r}, {c}) differs from the reference frame outside the exactness band"
                n_band += 1
        if rays is not None:
            O, D, colours = rays
            n = int((rt.get_ray_colours(O, D) != colours).sum())
            assert n == 0, f"{what}, walk {mode}: {n} of {len(D)} ray colours differ from the reference"
    return n_band


# ------------------------------------------------------------------ rays
def row_dirs(w, h, r, xs, viewport=(1.0, 1.0, 1.0)):
    """Directions of the 4 sub-sample rays (engine.rs:207-236) of the pixels `xs` (canvas columns) of canvas row r: [4, len(xs), 3].  viewport = (width,
    height, depth) of engine.rs:113-119: the scales are one division each (engine.rs:189-190), a component is one product with its scale, z is the depth."""
    vp_w, vp_h, vp_d = (float(v) for v in viewport)
    y = (h - h // 2) - r                                    # put_pixel: new_y = h - (y + h/2), engine.rs:147-150
    x = np.asarray(xs, np.float64) - (w // 2)
    d = np.empty((4, len(x), 3)); d[..., 2] = vp_d
    d[0, :, 0] = x * (vp_w / w); d[1, :, 0] = (x + 0.5) * (vp_w / w); d[2, :, 0] = d[0, :, 0]; d[3, :, 0] = d[1, :, 0]
    d[0, :, 1] = y * (vp_h / h); d[1, :, 1] = d[0, :, 1]; d[2, :, 1] = (y + 0.5) * (vp_h / h); d[3, :, 1] = d[2, :, 1]
    return d


def check_rows_against_oracle(frame, osc, w, h, rows, step):
    """Every step-th pixel of the frame's rows against oracle.get_ray_colour of its four sub-sample rays + Color::mix, within COLOUR_TOL."""
    xs = np.arange(0, 2 * (w // 2), step)
    for r in rows:
        d = row_dirs(w, h, r, xs).reshape(-1, 3)
        cols = np.fromiter(POOL.map(lambda v: osc.get_ray_colour(ORIGIN, v), d), np.uint32, len(d)).reshape(4, len(xs))
        mixed = channels(cols).sum(0) // 4                   # Color::mix, entities.rs:49-69
        got = channels(frame[r, xs])
        bad = np.abs(got - mixed).max(-1) > COLOUR_TOL
        assert not bad.any(), f"row {r}: {bad.sum()} of {len(xs)} sampled pixels differ from the oracle by more than {COLOUR_TOL}"


def sample_rays(osc, w, h, n_primary, rng, lights):
    """n_primary random sub-sample rays of the frame + for each one that hits: the shadow-shaped rays to the point lights (origin on the surface,
    un-normalised direction, max_t = |dir|: raytracer.rs:164-188) and one reflection-shaped ray (raytracer.rs:79-82) about a perturbed normal."""
    rows = rng.integers(1, h, n_primary); cols = rng.integers(0, 2 * (w // 2), n_primary); sub = rng.integers(0, 4, n_primary)
    d = np.stack([row_dirs(w, h, r, [c])[s, 0] for r, c, s in zip(rows, cols, sub)])
    o = np.tile(ORIGIN, (n_primary, 1))
    prim = list(POOL.map(lambda i: osc.intersect(o[i], d[i]), range(n_primary)))
    so, sdir, smax = [], [], []
    for i, (hit, t, u, v, tri) in enumerate(prim):
        if not hit:
            continue
        p = o[i] + d[i] * t
        n = -d[i] / np.linalg.norm(d[i]) + rng.normal(size=3) * 0.3
        n /= np.linalg.norm(n)
        for l in lights:
            if l.kind == 1:
                dirv = np.array([l.v.x, l.v.y, l.v.z]) - p
                so.append(p + n * 1e-4); sdir.append(dirv); smax.append(np.linalg.norm(dirv))
        rd = d[i] - n * 2.0 * np.dot(d[i], n)
        so.append(p + n * 1e-4); sdir.append(rd / np.linalg.norm(rd)); smax.append(np.inf)
    O = np.concatenate([o, np.array(so).reshape(-1, 3)]); D = np.concatenate([d, np.array(sdir).reshape(-1, 3)])
    M = np.concatenate([np.full(n_primary, np.inf), np.array(smax)])
    return O, D, M


def noise_band_terms(tris, o, pad):
    """The origin's part of the exactness criterion (clusters.cpp, find_origin_suspects), per triangle: (n, |n|, alpha, delta, rho) -- the plane normal,
    the angle and distance thresholds, and the distance of `o` from the plane."""
    e1 = tris[:, 1] - tris[:, 0]; e2 = tris[:, 2] - tris[:, 0]; s = o - tris[:, 0]
    n = np.cross(e1, e2); ln = np.linalg.norm(n, axis=1); l1 = np.linalg.norm(e1, axis=1); l2 = np.linalg.norm(e2, axis=1)
    R = np.linalg.norm(s, axis=1) + np.maximum(l1, l2); sinphi = ln / (l1 * l2); eps = 2.0 ** -53
    alpha = 8 * 64 * eps * R / (pad * sinphi); delta = 2 * (alpha * R + 64 * eps * R) / sinphi
    rho = np.abs((s * n).sum(1)) / ln
    return n, ln, alpha, delta, rho


def origin_within_delta(tris, o, pad):
    """Per triangle: does `o` lie within delta of its plane (the origin term of the criterion alone: what makes a triangle a suspect of the eye `o`)?"""
    _, _, _, delta, rho = noise_band_terms(tris, o, pad)
    return rho <= delta


def in_noise_band(tris, o, d, pad):
    """Host restatement of the exactness criterion (clusters.cpp, find_origin_suspects) for ONE ray against every triangle: is the ray's origin within
    delta of a triangle's plane AND its direction within alpha of parallel to it?  Outside that band the index is provably exact."""
    n, ln, alpha, delta, rho = noise_band_terms(tris, o, pad)
    sina = np.abs(n @ d) / (ln * np.linalg.norm(d))
    return bool(((rho <= delta) & (sina <= alpha)).any())


def plane_scene(rng, apex, n_planes, per, n_filler):
    """Triangles constructed in f64 INSIDE planes through `apex` (the generator of the `noise` scene of test_gpu_parity.py, scaled up) + random filler
    triangles + a backdrop.  Returns triangles, and per plane (d0, u): the in-plane directions are d0 + s*u."""
    tris, planes = [], []
    for k in range(n_planes):
        d0 = np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.3, 0.3), 1.0]); u = rng.normal(size=3)
        for j in range(per):
            a0, a1, a2 = rng.uniform(6, 14, 3); b0, b1, b2 = rng.uniform(-3, 3, 3)
            tris.append([apex + a0 * d0 + b0 * u, apex + a1 * d0 + b1 * u, apex + a2 * d0 + b2 * u])
        planes.append((d0, u))
    for k in range(n_filler):
        p = rng.uniform([-4, -0.5, -3], [4, 5, 7]); sz = 10 ** rng.uniform(-1.5, 0.0)
        tris.append([p, p + rng.normal(size=3) * sz, p + rng.normal(size=3) * sz])
    tris.append([(-8, -2, 16), (8, -2, 16), (0, 9, 16.5)])
    return np.asarray(tris, np.float64), planes


def coplanar_rays(rng, tris, planes, n_plane_tris, apex, N):
    """N rays from `apex`: in-plane directions (coplanar with that plane's triangles up to rounding), rays through vertices and through edge points of
    the in-plane triangles, each with and without a tiny perturbation (1e-16 .. 1e-9)."""
    pk = rng.integers(0, len(planes), N)
    d0s = np.array([p[0] for p in planes]); us = np.array([p[1] for p in planes])
    D = d0s[pk] + rng.uniform(-0.35, 0.35, N)[:, None] * us[pk]
    third = N // 3
    ti = rng.integers(0, n_plane_tris, third); vi = rng.integers(0, 3, third)
    D[:third] = tris[ti, vi] - apex
    w2 = rng.random((third, 1))
    D[third:2 * third] = (tris[ti, vi] * w2 + tris[ti, (vi + 1) % 3] * (1 - w2)) - apex
    eps = 10.0 ** rng.uniform(-16, -9, N) * (rng.random(N) < 0.5)
    D += rng.normal(size=(N, 3)) * eps[:, None]
    return np.tile(apex, (N, 1)), D


def plane_scene_data(rrt, tris, root=ROOT_BOX):
    """SceneData of plane_scene's triangles: one material, fixed uv and normals."""
    n = len(tris)
    nrm = np.tile([0.0, 0.1, -1.0], (n, 3, 1)); uv = np.tile([[0.1, 0.2, 0], [0.9, 0.1, 0], [0.5, 0.8, 0]], (n, 1, 1)).astype(np.float64)
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=240.0, kr=0.0, tex=0, bump=-1)]
    return rrt.SceneData.from_arrays(tris, uv, nrm, np.zeros(n, np.uint32), mats, [np.arange(48, dtype=np.uint8).reshape(4, 4, 3)], root=root)


# ------------------------------------------------------------------ hand-built geometry
def quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def closed_box(lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    p = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    faces = ((0, 1, 2, 3), (5, 4, 7, 6), (4, 0, 3, 7), (1, 5, 6, 2), (3, 2, 6, 7), (4, 5, 1, 0))
    return [t for f in faces for t in quad(*(p[i] for i in f))]


def flat_normals(tris, towards):
    """Per-triangle face normals, flipped to face the point `towards`."""
    t = np.asarray(tris, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); n /= np.linalg.norm(n, axis=1)[:, None]
    flip = ((np.asarray(towards) - t.mean(1)) * n).sum(1) < 0
    n[flip] *= -1
    return np.repeat(n[:, None], 3, 1)


def checker(c0, c1, k=8):
    yy, xx = np.mgrid[0:k, 0:k]
    t = np.where(((xx + yy) % 2 == 0)[..., None], np.array(c0, np.uint8), np.array(c1, np.uint8))
    return np.ascontiguousarray(t.astype(np.uint8))


# ------------------------------------------------------------------ set-up: GPU build vs host build vs oracle build
MATS = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=240.0, kr=0.0, tex=0, bump=-1)]
TEX = [np.full((2, 2, 3), 200, np.uint8)]
OCT_KEYS = ("aabb", "first_child", "tri_count", "own_off", "own_idx")
SCENE_BUFS = ("nodes", "geom", "attr", "supers", "cboxes", "child_boxes", "tboxes", "chains")


def scene_from(rrt, pos, root=None):
    pos = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    n = len(pos)
    rng = np.random.default_rng(n)
    uv = rng.random((n, 3, 3)); nrm = rng.normal(size=(n, 3, 3))
    return rrt.SceneData.from_arrays(pos, uv, nrm, np.zeros(n, np.uint32), MATS, TEX, **({} if root is None else {"root": root}))


def assert_same_octree(a, b, what):
    for k in OCT_KEYS:
        assert a[k].shape == b[k].shape, f"{what}: {k} shape {a[k].shape} vs {b[k].shape}"
        if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)):
            bad = np.flatnonzero((a[k] != b[k]).reshape(len(a[k]), -1).any(1))
            raise AssertionError(f"{what}: {k} differs in {len(bad)} rows, first {bad[:5]}: {a[k][bad[:3]]} vs {b[k][bad[:3]]}")
    assert a["max_depth"] == b["max_depth"], f"{what}: max_depth {a['max_depth']} vs {b['max_depth']}"


def assert_same_buffers(gpu, host, what, rec=32):
    for name in SCENE_BUFS:
        g, h = gpu.buffer(name), host.buffer(name)
        assert g.shape == h.shape, f"{what}: {name} is {g.shape[0]} bytes on the GPU path, {h.shape[0]} on the host path"
        if not np.array_equal(g, h):
            size = {"nodes": 96, "geom": 80, "attr": 128, "chains": 160}.get(name, rec)
            bad = np.flatnonzero((g.reshape(-1, size) != h.reshape(-1, size)).any(1))
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {len(g) // size} records, first {bad[:8]};\n gpu  {g.reshape(-1, size)[bad[0]].view(np.uint32)}\n host {h.reshape(-1, size)[bad[0]].view(np.uint32)}")
    ng, nh = gpu.last_stats()["origin_plane_triangles"], host.last_stats()["origin_plane_triangles"]
    assert ng == nh, f"{what}: {ng} origin-plane suspects on the GPU path, {nh} on the host path"
    if ng <= 64:                                              # beyond RRT_MAX_SUSPECTS the list is not read (every ray from the origin runs unfiltered)
        gs, hs = gpu.buffer("suspects").reshape(-1, 32), host.buffer("suspects").reshape(-1, 32)
        assert sorted(map(bytes, gs)) == sorted(map(bytes, hs)), f"{what}: origin-plane suspects differ ({len(gs)} vs {len(hs)})"


def check_scene(rrt, sd, what, ob=None, no_cull_too=True, origin=None):
    """The GPU set-up's octree equals the host build's (and with ob, the oracle's, built on the same root box); its scene buffers equal the host
    set-up's (and without the index); its index pad is 2^-15 of the root's largest |coordinate|."""
    lights = rrt.default_lights()
    kw = {} if origin is None else {"origin": origin}
    gpu = rrt.RayTracer(sd, lights, **kw)
    tree = gpu.octree()
    assert_same_octree(tree, sd.octree(), what + " (GPU build vs host build)")
    assert tree["info"] == sd.info, f"{what}: info {tree['info']} vs {sd.info}"
    lo, hi = sd.octree()["aabb"][0, :3], sd.octree()["aabb"][0, 3:]                     # node 0 is the root box the scene was given (min xyz, max xyz)
    if ob is not None:
        pos, uv, nrm, mat = sd.triangles()
        root = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
        osc = ob.OracleScene(pos, uv, nrm, mat, sd.materials(), sd.textures(), lights_tuple(lights), (0.0, 2.0, -10.0), root)
        assert_same_octree(tree, osc.octree(), what + " (GPU build vs oracle build)")
    pad, want = gpu.last_stats()["filter_pad"], float(np.abs(np.concatenate([lo, hi])).max()) / 32768.0
    assert pad == want, f"{what}: filter_pad {pad!r}, but 2^-15 of the root's magnitude is {want!r}"
    host = rrt.RayTracer(sd, lights, host_setup=True, **kw)
    assert_same_buffers(gpu, host, what)
    if no_cull_too:
        assert_same_buffers(rrt.RayTracer(sd, lights, no_cull=True, **kw), rrt.RayTracer(sd, lights, no_cull=True, host_setup=True, **kw), what + " [no_cull]")
    return gpu, host


# ------------------------------------------------------------------ the hand-built chain scenes (tests/test_gpu_chain_shortcut.py describes them)
CHAIN_PAD = 20.0 * 2.0 ** -15                             # the index pad of a +-20 root (clusters.cpp: kPadFraction of the scene magnitude)
CHAIN_CAMERA = (0.0, 2.0, -10.0)


class PlainLight:
    def __init__(self, kind, intensity, v):
        self.kind, self.intensity, self.v = kind, intensity, self
        self.x, self.y, self.z = v


CHAIN_LIGHTS = [PlainLight(0, 0.3, (0.0, 0.0, 0.0)), PlainLight(1, 0.6, (-4.0, 9.0, -6.0)), PlainLight(2, 0.2, (0.5, 1.0, -1.0))]


def rrt_lights_of(rrt, lights):
    """The package's Light objects of any lights with kind / intensity / v.x, v.y, v.z."""
    return [rrt.Light(int(l.kind), float(l.intensity), rrt.Vector3d(float(l.v.x), float(l.v.y), float(l.v.z))) for l in lights]


def chain_rrt_lights(rrt):
    return rrt_lights_of(rrt, CHAIN_LIGHTS)


CHAIN_ROOT_TRI = [(-15, -15, -15), (-14, -15, -15), (-15, -14, -15)]
CHAIN_C1 = [(2, 2, 1.5), (3, 2, 1.5), (2, 3, 1.5)]
CHAIN_C2 = [(7, 7, 7), (8, 7, 7), (7, 8, 7)]
CHAIN_D_TRIS = {"big": [(1, 1, 3), (4, 1, 3), (1, 4, 3)], "lo": [(1, 1, 2), (2, 1, 2), (1, 2, 2)], "hi": [(3, 3, 3.75), (4, 3, 3.75), (3, 4, 3.75)],
                "tie": [(2, 2, 1.5), (2.5, 2, 1.5), (2, 2.5, 1.5)], "behind": [(2, 2, 2.25), (3, 2, 2.25), (2, 3, 2.25)],
                "graze": [(5 - 2.0 ** -20, 1, 3.5), (5 - 2.0 ** -20, 4, 3.5), (3, 1, 3.5)], "lo2": [(0.25, 0.25, 0.5), (0.5, 0.25, 0.5), (0.25, 0.5, 0.5)]}


def chain_arrays(tris, scale=1.0, extra=()):
    pos = np.asarray(list(tris), np.float64) * scale
    if len(extra): pos = np.concatenate([pos, np.asarray(extra, np.float64)])
    n = len(pos)
    rng = np.random.default_rng(n)
    nrm = np.tile([0.0, 0.1, -1.0], (n, 3, 1)); uv = rng.random((n, 3, 3))
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.4, tex=0, bump=-1)]
    return dict(pos=pos, uv=uv, nrm=nrm, mat=np.zeros(n, np.uint32), materials=mats, textures=[checker((230, 200, 170), (120, 140, 160))], root=ROOT_BOX)


def chain_scene(which):
    """name -> (arrays, names of the triangles).  Push order matters: the first triangle that reaches a node stays in it."""
    d = list(CHAIN_D_TRIS.items())
    if which == "main":                       # root <- CHAIN_ROOT_TRI; d1 <- CHAIN_C1; d2 <- CHAIN_C2; D <- the rest
        names = ["root", "c1", "c2"] + [k for k, _ in d]
        return chain_arrays([CHAIN_ROOT_TRI, CHAIN_C1, CHAIN_C2] + [t for _, t in d]), names
    if which == "leaf_end":                   # the chain ends in a leaf that holds one triangle
        return chain_arrays([CHAIN_ROOT_TRI, CHAIN_C1, CHAIN_C2, CHAIN_D_TRIS["big"]]), ["root", "c1", "c2", "big"]
    if which == "long_lists":                 # d1 keeps six triangles: five of them straddle its split planes
        strad = [[(9, 9, 9 + 0.25 * i), (11, 9, 9 + 0.25 * i), (9, 11, 9 + 0.25 * i)] for i in range(5)]
        names = ["root", "c1"] + ["strad"] * 5 + ["c2"] + [k for k, _ in d]
        return chain_arrays([CHAIN_ROOT_TRI, CHAIN_C1] + strad + [CHAIN_C2] + [t for _, t in d]), names
    if which == "non_root_parent":            # the main scene at half size below P = [0,20]^3, whose child [10,20]^3 holds a triangle too
        names = ["root", "p_own", "other"] + ["c1", "c2"] + [k for k, _ in d]
        half = lambda t: [tuple(0.5 * c for c in v) for v in t]
        return chain_arrays([CHAIN_ROOT_TRI, [(9, 9, 12), (11, 9, 12), (9, 11, 12)], [(14, 14, 14), (15, 14, 14), (14, 15, 14)]] + [half(CHAIN_C1), half(CHAIN_C2)] + [half(t) for _, t in d]), names
    if which == "pokes_out":                  # a triangle that crosses the root's face: no "subtree box inside octant box" argument, no shortcut
        names = ["root", "c1", "c2"] + [k for k, _ in d] + ["poke"]
        return chain_arrays([CHAIN_ROOT_TRI, CHAIN_C1, CHAIN_C2] + [t for _, t in d] + [[(19, 1, 1), (21, 1, 1), (19, 2, 1)]]), names
    raise KeyError(which)


def chain_z_rays(xs, ys, z0=-5.0):
    O = np.array([(x, y, z0) for x in xs for y in ys], np.float64)
    return O, np.tile([0.0, 0.0, 1.0], (len(O), 1))


def chain_main_rays():
    """name -> (O, D, M).  Dyadic coordinates and axis-parallel directions keep every t exact."""
    R = {}
    g = np.arange(2.0625, 3.0, 0.0625)
    O, D = chain_z_rays(g, g); R["on_c1"] = (O, D, np.full(len(O), np.inf))                                   # case 1: over CHAIN_C1 (and TIE, BEHIND, BIG behind it)
    O, D = chain_z_rays(np.arange(7.0625, 8.0, 0.125), np.arange(7.0625, 8.0, 0.125)); R["on_c2"] = (O, D, np.full(len(O), np.inf))   # case 2: CHAIN_C2, outside D's subtree box
    Ob = np.array([(7.25 + 9.0, 7.25, 7.0 - 9.0), (7.5, 7.25 + 6.0, 7.0 - 6.0)]); Db = np.array([(-1.0, 0.0, 1.0), (0.0, -1.0, 1.0)])  # ... and slanted, through the head's box
    # ... and through an empty corner of D's subtree box first (points P), then into CHAIN_C2: only the triangle-box condition keeps these lanes on the chain
    P = np.array([(4.5 + 0.03125 * i, 3.875 - 0.03125 * j, 1.0) for i in range(6) for j in range(6)]); T = np.array([(7.25, 7.25, 7.0)]) - P
    R["on_c2"] = (np.concatenate([R["on_c2"][0], Ob, P - 3.0 * T]), np.concatenate([R["on_c2"][1], Db, T]), np.full(len(O) + 2 + len(P), np.inf))
    R["through_end"] = (P - 3.0 * T, T, np.full(len(P), np.inf))                                            # (the same rays on their own, for the CPU proof)
    s = np.array([-1.5, -1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5]) * CHAIN_PAD                # case 3: within a pad of the faces of D's subtree box
    band = [(5.0 + CHAIN_PAD + e, y, -5.0) for e in s for y in (1.5, 2.5, 3.5)] + [(x, 4.0 + CHAIN_PAD + e, -5.0) for e in s for x in (1.25, 2.0)] + \
           [(0.25 - CHAIN_PAD + e, y, -5.0) for e in s for y in (0.3, 0.4)]
    graze = [(x, y, -5.0) for x in (5.0, 5.0 - 2.0 ** -20, 5.0 - 2.0 ** -21, 5.0 - 2.0 ** -19, 5.0 + 2.0 ** -40, 10.0, 10.0 - 2.0 ** -40, 0.0, 2.0 ** -40) for y in np.arange(1.125, 4.0, 0.25)]
    O = np.array(band + graze); R["band"] = (O, np.tile([0.0, 0.0, 1.0], (len(O), 1)), np.full(len(O), np.inf))
    O, D = chain_z_rays(np.arange(7.0625, 7.7, 0.125), (7.125, 7.25))                                         # case 4: shadow queries that only CHAIN_C2 can occlude (t = 12)
    Os = np.concatenate([O, O, P - 3.0 * T, P - 3.0 * T]); Ds = np.concatenate([D, D, T, T])          # (CHAIN_C2 lies at t = 4 of the slanted rays)
    R["shadow"] = (Os, Ds, np.concatenate([np.full(len(O), 13.0), np.full(len(O), 11.0), np.full(len(P), 5.0), np.full(len(P), 3.5)]))
    return R


# ------------------------------------------------------------------ frames of a posed camera (include/rrt.h: rrt_camera) against the oracle
MIN_PIXELS = 512                                   # compared with the oracle per pose, at least


def pose_dirs(cam, w, h, rows, xs, viewport=(1.0, 1.0, 1.0)):
    """[len(rows), 4, len(xs), 3]: the four sub-sample directions of the pixels (row, x) of a w x h frame in the pose `cam`, in the contract's order."""
    R, U, F = (np.asarray(cam[k], np.float64) for k in ("right", "up", "forward"))
    out = np.empty((len(rows), 4, len(xs), 3))
    for i, r in enumerate(rows):
        abc = row_dirs(w, h, r, xs, viewport)      # (a, b, c) of engine.rs:207-236; with the default viewport c = 1.0
        a, b, c = abc[..., 0:1], abc[..., 1:2], abc[..., 2:3]
        out[i] = (R * a + U * b) + F * c
    return out


def mix4(cols):
    """Color::mix (entities.rs:49-69) over axis 1 (the four sub-samples): channel sums, truncating / 4 -> packed 0x00RRGGBB."""
    ch = channels(cols).sum(1) // 4
    return ((ch[..., 0] << 16) | (ch[..., 1] << 8) | ch[..., 2]).astype(np.uint32)


def traced_rows(h):
    return np.arange(h - 2 * (h // 2) + 1, h)     # rows the reference writes (engine.rs:146-158)


def oracle_pixels(osc, cam, w, h, rows, xs, what, viewport=(1.0, 1.0, 1.0)):
    """The oracle's pixels (rows, xs) of a w x h frame in the pose `cam`: get_ray_colour of the four sub-sample rays + Color::mix.  Asserts that there are at
    least MIN_PIXELS of them and that at least half have a sub-sample ray the oracle's intersector says hits."""
    eye = cam["eye"]
    d = pose_dirs(cam, w, h, rows, xs, viewport)
    flat = d.reshape(-1, 3)
    cols = np.fromiter(POOL.map(lambda v: osc.get_ray_colour(eye, v), flat), np.uint32, len(flat)).reshape(d.shape[:3])
    hits = np.fromiter(POOL.map(lambda v: osc.intersect(eye, v)[0], flat), bool, len(flat)).reshape(d.shape[:3])
    n_px = len(rows) * len(xs)
    frac = hits.any(1).mean()
    print(f"{what}: {n_px} pixels compared, {frac:.3f} of them with a hit, {hits.mean():.3f} of their rays hit")
    assert n_px >= MIN_PIXELS, f"{what}: {n_px} pixels compared (< {MIN_PIXELS})"
    assert frac >= 0.5, f"{what}: only {frac:.3f} of the compared pixels have a sub-sample ray that hits (< 0.5)"
    return mix4(cols)
