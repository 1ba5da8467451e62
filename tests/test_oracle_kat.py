"""Pins the CPU oracle (oracle/rrt_oracle.c) -- known-answer tests.

The reference has no live tests.  What it does hold are the data vectors of its commented-out octree
tests (src/collision/octree.rs:244-652); the ones still valid for today's code are used below as data: the child
boxes of a subdivided [-10,10]^3 root in the order BBL,BFL,BFR,BBR,TBL,TFL,TFR,TBR (octree.rs:434-529, second level
octree.rs:530-610) and the Aabb::from_triangle boxes (octree.rs:308-319, 410-432).  Everything else is hand-derived from
the cited reference lines.
"""
import math
import os

import numpy as np

from conftest import GOLDEN, channels

INF = float("inf")

# octree.rs:434-529 (children of the root [-10,10]^3) and 530-610 (children of [0,10]^3), min xyz + max xyz
REF_CHILD_BOXES_L1 = [(-10, -10, -10, 0, 0, 0), (-10, -10, 0, 0, 0, 10), (0, -10, 0, 10, 0, 10), (0, -10, -10, 10, 0, 0),
                      (-10, 0, -10, 0, 10, 0), (-10, 0, 0, 0, 10, 10), (0, 0, 0, 10, 10, 10), (0, 0, -10, 10, 10, 0)]
REF_CHILD_BOXES_L2 = [(0, 0, 0, 5, 5, 5), (0, 0, 5, 5, 5, 10), (5, 0, 5, 10, 5, 10), (5, 0, 0, 10, 5, 5),
                      (0, 5, 0, 5, 10, 5), (0, 5, 5, 5, 10, 10), (5, 5, 5, 10, 10, 10), (5, 5, 0, 10, 10, 5)]
MAT = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(1, 1, 1), ns=240.0, kr=0.0, tex=0, bump=-1)]
TEX = [np.full((2, 2, 3), 200, np.uint8)]
ROOT10 = (-10.0, 10.0, -10.0, 10.0, -10.0, 10.0)


def tiny_scene(ob, tris, root=ROOT10, lights=((0, 1.0, (0, 0, 0)),), mats=MAT, tex=TEX, mat_ids=None, uv=None, nrm=None, **options):
    pos = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    n = len(pos)
    uv = np.zeros((n, 3, 3)) if uv is None else np.asarray(uv, np.float64)
    nrm = np.tile([0.0, 0.0, -1.0], (n, 3, 1)) if nrm is None else np.asarray(nrm, np.float64)
    return ob.OracleScene(pos, uv, nrm, np.zeros(n, np.uint32) if mat_ids is None else mat_ids, mats, tex, list(lights), (0, 0, -5), root, **options)


# ------------------------------------------------------------------ Moller-Trumbore, ray.rs:56-94
def test_mt_known_answer(ob):
    tri = [(-1, -1, 0), (1, -1, 0), (0, 1, 0)]
    assert ob.intersect_triangle((0, 0, -1), (0, 0, 1), tri) == (True, 1.0, 0.25, 0.5)
    # no back-face culling: reversed winding still hits, with the barycentrics of the swapped vertices
    hit, t, u, v = ob.intersect_triangle((0, 0, -1), (0, 0, 1), [tri[0], tri[2], tri[1]])
    assert hit and t == 1.0 and (u, v) == (0.5, 0.25)


def test_mt_rejections(ob):
    tri = [(-1, -1, 0), (1, -1, 0), (0, 1, 0)]
    assert not ob.intersect_triangle((0, 0, -1), (1, 0, 0), tri)[0]          # parallel: |a| < eps (ray.rs:66)
    assert not ob.intersect_triangle((0, 0, 1), (0, 0, 1), tri)[0]           # behind: t = -1 (ray.rs:89)
    assert not ob.intersect_triangle((5, 0, -1), (0, 0, 1), tri)[0]          # u > 1
    assert not ob.intersect_triangle((0, 3, -1), (0, 0, 1), tri)[0]          # v/u+v out of range
    assert ob.intersect_triangle((-1, -1, -1), (0, 0, 1), tri)[0]            # exactly on vertex v1: u = v = 0 is inside (ray.rs:75,82 use strict <)
    assert not ob.intersect_triangle((0, 0, 0), (0, 0, 1), tri)[0]           # t = 0 is not > eps
    assert not ob.intersect_triangle((0, 0, -1), (float("nan"), 0, 1), tri)[0]   # NaN falls through every test to t > eps == false


# ------------------------------------------------------------------ slab test, ray.rs:21-54
def test_aabb_known_answers(ob):
    box = (-1, -1, -1, 1, 1, 1)
    assert ob.intersect_aabb((0, 0, -5), (0, 0, 1), box) == (True, 4.0)
    assert ob.intersect_aabb((0, 0, 0), (0, 0, 1), box) == (True, 1.0)       # origin inside -> tmax (ray.rs:49-51)
    assert ob.intersect_aabb((0, 0, 5), (0, 0, 1), box) == (False, None)     # behind (ray.rs:39-41)
    assert ob.intersect_aabb((3, 0, -5), (0, 0, 1), box) == (False, None)    # tmin > tmax with +-inf from d.x = 0
    assert ob.intersect_aabb((0, 0, -5), (0, 0, 2), box) == (True, 2.0)      # t is in units of |d|


def test_aabb_nan_on_split_plane(ob):
    """d.x = 0 with the origin ON a box face gives (0-0)/0 = NaN; Rust f64::min/max ignore NaN, so both x-halves of a
    node split at x = 0 are MISSED ('NaN/inf semantics are load-bearing')."""
    assert ob.intersect_aabb((0, 2, -10), (0, 0.1, 1), (0, -20, -20, 20, 20, 20)) == (False, None)
    assert ob.intersect_aabb((0, 2, -10), (0, 0.1, 1), (-20, -20, -20, 0, 20, 20)) == (False, None)
    assert ob.intersect_aabb((0, 2, -10), (1e-9, 0.1, 1), (0, -20, -20, 20, 20, 20))[0]   # any non-zero d.x hits


# ------------------------------------------------------------------ casts and colour packing
def test_rust_casts(ob):
    L = ob.lib()
    assert L.oracle_f64_as_usize(-3.7) == 0 and L.oracle_f64_as_usize(float("nan")) == 0 and L.oracle_f64_as_usize(-0.0) == 0
    assert L.oracle_f64_as_usize(3.99) == 3 and L.oracle_f64_as_usize(1e30) == 2**64 - 1 and L.oracle_f64_as_usize(INF) == 2**64 - 1
    assert L.oracle_clamp_u8(-5.0) == 0 and L.oracle_clamp_u8(255.9) == 255 and L.oracle_clamp_u8(254.999) == 254
    assert L.oracle_clamp_u8(float("nan")) == 0 and L.oracle_clamp_u8(1e9) == 255


def test_color_mix_truncates(ob):
    L = ob.lib()
    assert L.oracle_color_mix4(0x010203, 0x010203, 0x010203, 0x020304) == 0x010203      # (1+1+1+2)/4 = 1 (entities.rs:60-62)
    assert L.oracle_color_mix4(0xFFFFFF, 0xFFFFFF, 0xFFFFFF, 0xFFFFFF) == 0xFFFFFF      # u64 sums do not wrap
    assert L.oracle_color_mix4(0xFF0000, 0, 0, 0) == 0x3F0000                           # 0x00RRGGBB packing (entities.rs:32-36)


# ------------------------------------------------------------------ octree build, octree.rs:41-241
def test_octree_first_triangle_stays_in_root(ob):
    s = tiny_scene(ob, [[(2, 2, 2), (2, 5, 2), (5, 2, 2)]])
    t = s.octree()
    assert len(t["first_child"]) == 1 and t["own_idx"].tolist() == [0] and t["tri_count"].tolist() == [1]
    assert t["aabb"][0].tolist() == [-10, -10, -10, 10, 10, 10]


def test_octree_child_order_matches_reference_vectors(ob):
    # triangles of octree.rs:335-390: tri0 near (5.2..5.5), tri1 near (0.6..0.8); a third one forces a split of child TFR
    tris = [[(5.2, 5.2, 5.2), (5.2, 5.5, 5.2), (5.5, 5.2, 5.2)], [(0.6, 0.6, 0.6), (0.6, 0.8, 0.6), (0.8, 0.6, 0.6)],
            [(7.0, 7.0, 7.0), (7.0, 7.5, 7.0), (7.5, 7.0, 7.0)]]
    t = tiny_scene(ob, tris[:2]).octree()
    # today's insert leaves the first triangle in the parent: 1 + 8 nodes, tri0 in the root, tri1 alone in child TFR (node 7)
    assert len(t["first_child"]) == 9 and t["first_child"][0] == 1
    assert t["aabb"][1:9].tolist() == [list(map(float, b)) for b in REF_CHILD_BOXES_L1]
    own = {n: t["own_idx"][t["own_off"][n]:t["own_off"][n + 1]].tolist() for n in range(9)}
    assert own[0] == [0] and own[7] == [1] and sum(len(v) for v in own.values()) == 2
    assert t["tri_count"].tolist() == [2, 0, 0, 0, 0, 0, 0, 1, 0]
    t3 = tiny_scene(ob, tris).octree()
    assert len(t3["first_child"]) == 17 and t3["first_child"][7] == 9
    assert t3["aabb"][9:17].tolist() == [list(map(float, b)) for b in REF_CHILD_BOXES_L2]
    assert t3["max_depth"] == 3


def test_octree_straddlers_stay_and_outsiders_drop(ob):
    tris = [[(1, 1, 1), (1, 2, 1), (2, 1, 1)],            # root (first)
            [(-1, 1, 1), (1, 1.5, 1), (1, 1, 2)],          # straddles x = 0 -> touches 2 children -> stays in the root
            [(50, 50, 50), (51, 50, 50), (50, 51, 50)],    # outside the root box -> silently dropped (octree.rs:71-73)
            [(0, 3, 3), (0, 4, 3), (0, 3, 4)]]             # lies IN the plane x = 0: inclusive test touches both halves -> stays
    t = tiny_scene(ob, tris).octree()
    assert t["own_idx"][t["own_off"][0]:t["own_off"][1]].tolist() == [0, 1, 3]
    assert t["tri_count"][0] == 3 and len(t["own_idx"]) == 3


def test_duplicate_triangles_chain_downwards(ob):
    tri = [(1, 1, 1), (1, 2, 1), (2, 1, 1)]
    t = tiny_scene(ob, [tri] * 4).octree()
    # the resident triangle is never pushed down, every duplicate opens one more level (octree.rs:79-92)
    assert t["max_depth"] == 4 and len(t["first_child"]) == 1 + 8 * 3


# ------------------------------------------------------------------ the walk, ray.rs:104-168
def test_walk_is_not_exact_nearest(ob):
    """The walk returns the first child (stable sort by box distance) that has ANY hit (ray.rs:146-161).  With the origin inside
    child TFR the key of TFR is its EXIT distance (ray.rs:49-51), which ties with the ENTRY distance of the neighbour TFL; the
    stable sort keeps child order, TFL (index 5) goes first, and its hit at t = 3 beats the nearer hit at t = 0.5 in TFR."""
    dummy = [(-9, -9, -9), (-8, -9, -9), (-9, -8, -9)]           # first triangle always stays in the root leaf
    a = [(0.5, 0.5, 0.5), (0.5, 2, 0.5), (0.5, 0.5, 2)]          # inside TFR, plane x = 0.5
    b = [(-2, 0.5, 0.5), (-2, 2, 0.5), (-2, 0.5, 2)]             # inside TFL, plane x = -2
    s = tiny_scene(ob, [dummy, a, b])
    tr = s.octree()
    assert len(tr["first_child"]) == 9 and tr["tri_count"].tolist() == [3, 0, 0, 0, 0, 0, 1, 1, 0]
    o, d = (1.0, 1.0, 1.0), (-1.0, 0.0, 0.0)
    assert ob.intersect_aabb(o, d, tr["aabb"][7]) == (True, 1.0) and ob.intersect_aabb(o, d, tr["aabb"][6]) == (True, 1.0)
    assert ob.intersect_triangle(o, d, a)[:2] == (True, 0.5)
    hit, t, u, v, tri = s.intersect(o, d)
    assert (hit, t, tri) == (True, 3.0, 2)


def test_walk_child_vs_own_and_max_t(ob):
    a = [(-9, -9, 8), (9, -9, 8), (0, 9, 8)]              # root list (first triangle), z = 8
    b = [(6, 6, 1), (6, 7, 1), (7, 6, 1)]                 # child TFR, z = 1
    s = tiny_scene(ob, [a, b])
    o, d = (6.2, 6.2, -5), (0, 0, 1)
    hit, t, u, v, tri = s.intersect(o, d)
    assert hit and tri == 1 and t == 6.0                   # child hit nearer than own hit -> child (ray.rs:163-164)
    # max_t only filters the ROOT's own list (children restart at +inf, ray.rs:153): with max_t = 5 the own hit (t=13) is
    # rejected, the child hit t=6 is found, and 6 < 5 fails -> falls back to own = None
    assert s.intersect(o, d, 5.0)[0] is False
    assert s.intersect(o, d, 7.0)[:2] == (True, 6.0)
    # tie-break inside one list is first-wins (strict <, ray.rs:124)
    s2 = tiny_scene(ob, [a, [(-9, -9, 8), (9, -9, 8), (0, 9, 8.0)]])
    assert s2.intersect((0, 0, -5), (0, 0, 1))[4] == 0


def test_empty_scene_and_empty_children(ob):
    s = tiny_scene(ob, np.zeros((0, 3, 3)))
    assert s.intersect((0, 0, -5), (0, 0, 1))[0] is False          # triangle_count == 0 -> None (ray.rs:112-114)
    assert s.get_ray_colour((0, 0, -5), (0, 0, 1)) == 0xFFFFFF     # WHITE, raytracer.rs:109-111


# ------------------------------------------------------------------ shading, raytracer.rs
def test_texel_index_saturates_and_wraps(ob):
    tex = np.zeros((2, 2, 3), np.uint8); tex[0, 0] = (10, 20, 30); tex[0, 1] = (40, 50, 60); tex[1, 0] = (70, 80, 90); tex[1, 1] = (100, 110, 120)
    tri = [[(-4, -4, 0), (4, -4, 0), (0, 4, 0)]]
    amb = ((0, 1.0, (0, 0, 0)),)
    for uvval, want in (((-3.25, -0.1), (10, 20, 30)),      # negative -> `as usize` saturates to 0 (raytracer.rs:52-53)
                        ((0.75, 0.25), (40, 50, 60)),       # x = 1, y = 0
                        ((1.25, 2.75), (70, 80, 90)),       # (2.5 as usize) % 2 = 0, (5.5 as usize) % 2 = 1 -> wraps, no V flip
                        ((0.5, 0.5), (100, 110, 120))):
        uv = np.tile([uvval[0], uvval[1], 0.0], (1, 3, 1))
        s = tiny_scene(ob, tri, lights=amb, tex=[tex], uv=uv)
        c = s.get_ray_colour((0, 0, -5), (0, 0, 1))
        assert ((c >> 16) & 255, (c >> 8) & 255, c & 255) == want


def test_shadow_break_drops_later_lights(ob):
    """A blocked point light `break`s out of the WHOLE light loop (raytracer.rs:235-237): lights after it are lost."""
    floor = [(-8, -8, 5), (8, -8, 5), (0, 8, 5)]
    blocker = [(-1, -1, 2), (1, -1, 2), (0, 1, 2)]
    nrm = np.tile([0.0, 0.0, -1.0], (2, 3, 1))
    lights_blocked_first = [(1, 0.5, (0, 0, -3)), (0, 0.5, (0, 0, 0))]     # point (blocked at the probe), then ambient
    lights_ambient_first = [(0, 0.5, (0, 0, 0)), (1, 0.5, (0, 0, -3))]
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=0, bump=-1)]
    probe_o, probe_d = (6.0, 0.0, -5.0), (-0.6, -0.01, 1.0)                # passes beside the blocker, hits the floor at (0, -0.1, 5) under it
    s1 = tiny_scene(ob, [floor, blocker], lights=lights_blocked_first, mats=mats, nrm=nrm)
    s2 = tiny_scene(ob, [floor, blocker], lights=lights_ambient_first, mats=mats, nrm=nrm)
    assert s1.intersect(probe_o, probe_d)[4] == 0
    assert s1.get_ray_colour(probe_o, probe_d) == 0x000000                 # ambient never added
    assert s2.get_ray_colour(probe_o, probe_d) == 0x646464                 # 200 * 0.5 = 100


def test_mirror_recursion_depth_and_quantisation(ob):
    """Two facing mirrors: the recursion stops at max_reflection_depth (5 by default, raytracer.rs:20,76) and every level quantises to u8
    (raytracer.rs:85-101).  The mirrors' local colours differ (100 and 0) and kr = 0.75, so every extra bounce level changes the answer."""
    m1 = [(-8, -8, 5), (8, -8, 5), (0, 8, 5)]
    m2 = [(-8, -8, -8), (8, -8, -8), (0, 8, -8)]
    nrm = np.array([np.tile([0, 0, -1.0], (3, 1)), np.tile([0, 0, 1.0], (3, 1))])
    mats = [dict(ka=(1, 1, 1), kd=(0, 0, 0), ks=(0, 0, 0), ns=-1.0, kr=0.75, tex=0, bump=-1),
            dict(ka=(0, 0, 0), kd=(0, 0, 0), ks=(0, 0, 0), ns=-1.0, kr=0.75, tex=0, bump=-1)]
    local = (100, 0)                                       # texel 200 * ka * ambient 0.5: level d hits m1 (even d) or m2 (odd d)

    def want(depth):
        c = local[depth % 2]                               # level `depth` is terminal: its local colour, no reflection
        for d in range(depth - 1, -1, -1):                 # unwind: trunc(local * (1 - kr) + c * kr), exact in f64
            c = int(local[d % 2] * 0.25 + c * 0.75)
        return c

    wants = []
    for depth in [None] + list(range(9)):
        opts = {} if depth is None else dict(max_reflection_depth=depth)
        s = tiny_scene(ob, [m1, m2], lights=((0, 0.5, (0, 0, 0)),), mats=mats, mat_ids=np.array([0, 1], np.uint32), nrm=nrm, **opts)
        w = want(5 if depth is None else depth)
        assert s.get_ray_colour((0, 0, -5), (0, 0, 1)) == (w << 16 | w << 8 | w), depth
        if depth is not None:
            wants.append(w)
    assert wants == [100, 25, 81, 38, 70, 46, 64, 50, 61]                   # depth 0 is the first mirror's own colour; every level counts


def test_surface_offset_moves_the_shadow_ray_origin(ob):
    """light_reaches_point (raytracer.rs:164-188) starts the shadow ray at point + normal * SURFACE_OFFSET (raytracer.rs:17).  A floor at z = 5 (normal
    towards the light, -z), a thin occluder 0.5 above it over the probe point and a point light above both: with offset 1e-4 the shadow ray meets the
    occluder, the light `break`s the loop and [Point, Ambient] gives black; with offset 1.0 the ray starts above the occluder (z = 4) and the probe is lit."""
    floor = [(-8, -8, 5), (8, -8, 5), (0, 8, 5)]
    occluder = [(-0.2, -0.3, 4.5), (0.2, -0.3, 4.5), (0, 0.2, 4.5)]
    nrm = np.tile([0.0, 0.0, -1.0], (2, 3, 1))
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=0, bump=-1)]   # ns = -1: no specular term (raytracer.rs:286)
    tex = [np.full((2, 2, 3), 201, np.uint8)]
    lights = [(1, 0.5, (0, -0.1, 0)), (0, 0.25, (0, 0, 0))]
    probe_o, probe_d = (6.0, 0.0, -5.0), (-0.6, -0.01, 1.0)        # passes beside the occluder (x = 0.3 at z = 4.5), hits the floor at (0, -0.1, 5)
    near = tiny_scene(ob, [floor, occluder], lights=lights, mats=mats, tex=tex, nrm=nrm)
    far = tiny_scene(ob, [floor, occluder], lights=lights, mats=mats, tex=tex, nrm=nrm, surface_offset=1.0)
    hit, t, u, v, tri = near.intersect(probe_o, probe_d)
    assert hit and tri == 0 and abs(t - 10.0) < 1e-12
    assert near.intersect((0, -0.1, 4.9999), (0, 0, -5), 5.0)[4] == 1   # the offset-1e-4 shadow ray meets the occluder at t = 0.09998
    assert near.get_ray_colour(probe_o, probe_d) == 0x000000         # occluded point light first: the ambient term is never added
    # lit: 201 * (ambient 0.25 + diffuse 0.5 * cos) with cos = n.l / |l| = 5 / 5.000001 (light 5 above the probe, straight up the normal):
    # 201 * 0.7499999 = 150.74998 -> 150 per channel
    assert far.get_ray_colour(probe_o, probe_d) == 0x969696
    assert tiny_scene(ob, [floor, occluder], lights=lights, mats=mats, tex=tex, nrm=nrm, surface_offset=1e-4).get_ray_colour(probe_o, probe_d) == 0


# ------------------------------------------------------------------ frame driver, engine.rs:146-158, 186-255
def test_frame_row0_and_odd_sizes(teapot_oracle):
    fb, cnt = teapot_oracle.render(33, 21)
    assert (fb[0] == 0).all() and (fb[1] == 0).all()       # odd height: rows 0 and 1 are never written
    assert (fb[:, 32] == 0).all() and (fb[2:, :32] != 0).any()   # odd width: last column never written
    assert cnt["rays_primary"] == 4 * 32 * 20              # the loop still traces y = -h/2, whose pixels put_pixel rejects
    fb2, _ = teapot_oracle.render(32, 20)
    assert (fb2[0] == 0).all() and (fb2[1:] != 0).all()


def test_frame_is_schedule_independent(teapot_oracle):
    a, _ = teapot_oracle.render(48, 40, n_threads=1)
    b, _ = teapot_oracle.render(48, 40, n_threads=7)
    assert np.array_equal(a, b)


def test_teapot_octree_shape(teapot_oracle):
    t = teapot_oracle.octree()
    assert len(t["first_child"]) == 3265 and t["own_off"][1] == 1110 and len(t["own_idx"]) == 6334   # SURVEY.md 3.4 / BASELINE.md section 2
    assert int((t["tri_count"] > 0).sum()) == 490


def test_teapot_center_column_nan_path(teapot_oracle):
    """Column w/2 (x = 0): left sub-samples have d.x = 0 at origin.x = 0 = the root split plane; all 8 root children miss,
    so only the root list is tested -- the pixel must still agree with a ray nudged off the plane where it only sees root triangles."""
    o = (0.0, 2.0, -10.0)
    hit, t, u, v, tri = teapot_oracle.intersect(o, (0.0, -0.1, 1.0))
    tree = teapot_oracle.octree()
    root_list = set(tree["own_idx"][:1110].tolist())
    assert (not hit) or tri in root_list


def test_golden_frames_and_rays(ob, rrt, teapot_oracle):
    g = np.load(f"{GOLDEN}/model2.npz")
    for key in [k for k in g.files if k.startswith("fb_")]:
        w, h = map(int, key[3:].split("x"))
        fb, _ = teapot_oracle.render(w, h)
        assert np.array_equal(fb, g[key]), key
    for i in range(0, len(g["ray_o"]), 7):
        hit, t, u, v, tri = teapot_oracle.intersect(g["ray_o"][i], g["ray_d"][i])
        assert hit == bool(g["ray_hit"][i])
        if hit:
            assert (t, u, v, tri) == (g["ray_t"][i], g["ray_u"][i], g["ray_v"][i], g["ray_tri"][i])
        assert teapot_oracle.get_ray_colour(g["ray_o"][i], g["ray_d"][i]) == g["ray_col"][i]
    assert int(g["n_nodes"]) == 3265 and int(g["root_own"]) == 1110


def test_oracle_silhouette_matches_the_references_only_image(rrt, ob, teapot, teapot_oracle):
    """The one image the reference holds, example_output.png (README.md:9), shows an OLDER teapot scene (no mirror, untextured teapot) in an 800 x 800
    minifb window.  It cannot pin arithmetic, but it does pin the camera (main.rs:62-66), the viewport and pixel grid (engine.rs:186-255), the
    orientation of put_pixel (engine.rs:146-158: y up, no vertical flip, row 0 = top) and the white-miss convention: the oracle's frame of model2.obj
    at 800 x 800 must cover the same pixels as the screenshot's canvas everywhere outside the projection of the mirror, the one object the old scene
    lacks.  The fixture is the derived non-white mask (tests/golden/make_example_mask.py), not the image."""
    m = np.load(os.path.join(GOLDEN, "example_output_mask.npz"))
    W = H = 800
    ref = np.unpackbits(m["mask_bits"])[:W * H].reshape(H, W).astype(bool)
    fb, _ = teapot_oracle.render(W, H)
    mine = fb != 0xFFFFFF
    # the mirror: the triangles whose material reflects (model2.obj:25989-25990), projected with the reference's camera model
    pos, _, _, mat = teapot.triangles()
    mirror = np.flatnonzero(np.isin(mat, [i for i, mt in enumerate(teapot.materials()) if mt["kr"] > 0]))
    assert len(mirror) == 2
    o = np.array([0.0, 2.0, -10.0])
    yy, xx = np.mgrid[0:H, 0:W]
    excl = np.zeros((H, W), bool)
    for t in pos[mirror]:
        d = t - o
        px = d[:, 0] / d[:, 2] * W + W / 2; row = H - (d[:, 1] / d[:, 2] * H + H / 2)     # engine.rs:209-236 inverted; put_pixel engine.rs:147-150
        def side(a, b): return (xx - px[b]) * (row[a] - row[b]) - (px[a] - px[b]) * (yy - row[b])
        d1, d2, d3 = side(0, 1), side(1, 2), side(2, 0)
        excl |= ~(((d1 < 0) | (d2 < 0) | (d3 < 0)) & ((d1 > 0) | (d2 > 0) | (d3 > 0)))
    grown = excl.copy()
    for _ in range(3):                                                   # 3-pixel margin around the mirror's edge
        g = grown.copy(); g[1:] |= grown[:-1]; g[:-1] |= grown[1:]; g[:, 1:] |= grown[:, :-1]; g[:, :-1] |= grown[:, 1:]; grown = g
    keep = ~grown; keep[0] = False                                       # row 0 is never written (engine.rs:152-155)
    iou = ((ref & mine & keep).sum()) / (((ref | mine) & keep).sum())
    assert keep.sum() > 0.75 * W * H and iou >= 0.995, f"silhouette IoU outside the mirror {iou:.5f}"
    assert ref[600:740, :].mean() > 0.9 and not ref[1:100, 500:].any()     # the table low in the frame, empty background top right: the frame is not flipped
    assert ref[0].all() and (fb[0] == 0).all()                             # canvas row 0 is BLACK in the reference's own screenshot: put_pixel never writes it (engine.rs:146-158)


def test_oracle_colours_match_the_references_only_image(rrt, ob, teapot, teapot_oracle):
    """The same screenshot pins ARITHMETIC too, on the parts of the old scene that model2.obj still contains unchanged -- the teapot (material, lights
    and camera as today) and the table's front face.  Those canvas pixels are what the reference's own build computed with get_ray_colour
    (raytracer.rs:29-112: walk, barycentric normal and texel, Phong diffuse + specular `powf`, shadow rays, Color::mix of the four sub-samples,
    put_pixel); the PNG is lossless.  Of the sampled pixels whose four sub-sample rays all hit the teapot above its contact zone with the table
    (hit height >= 0.6), the oracle reproduces 86 % EXACTLY (all 24 bits) and 94.5 % within one unit per channel; the remaining 5 % sit on the lid
    knob, the inner edge of the handle and the top edge of the spout -- grazing shadow rays, where the screenshot's older build evidently offset or
    ordered its shadow test differently (it also predates the mirror and has another table top, which is why only these regions are compared).
    The table's front face (texture lookup, no highlight): 97.8 % within one unit, all within 8.  Thresholds leave a small margin below the measured
    figures; a wrong camera, normal interpolation, light loop, `powf` argument or sub-sample mix moves every one of these pixels."""
    from concurrent.futures import ThreadPoolExecutor
    m = np.load(os.path.join(GOLDEN, "example_output_mask.npz"))
    W = H = 800
    fb, _ = teapot_oracle.render(W, H)
    mine = channels(fb)
    _, _, _, mat = teapot.triangles()
    mats = teapot.materials()
    teapot_mat = int(np.argmax(np.bincount(mat)))                          # the teapot's 6320 triangles
    assert mats[teapot_mat]["kr"] == 0.0

    def lowest_hit(material):
        """Height of the lowest of the pixel's four primary hits if all four hit `material`, else None."""
        def f(rc):
            r, c = rc
            y, x = (H - H // 2) - r, c - W // 2                                # put_pixel inverted (engine.rs:147-150), pixel grid engine.rs:207-236
            ys = []
            for dx, dy in ((0, 0), (.5, 0), (0, .5), (.5, .5)):
                d = ((x + dx) * (1.0 / W), (y + dy) * (1.0 / H), 1.0)
                h = teapot_oracle.intersect((0.0, 2.0, -10.0), d)
                if not h[0] or int(mat[h[4]]) != material: return None
                ys.append(2.0 + d[1] * h[1])
            return min(ys)
        return f
    with ThreadPoolExecutor(8) as pool:
        r0, r1, c0, c1 = map(int, m["teapot_box"])
        pts = [(r, c) for r in range(r0, r1, 3) for c in range(c0, c1, 3)]
        low = list(pool.map(lowest_hit(teapot_mat), pts))
        sel = np.array([p for p, y in zip(pts, low) if y is not None and y >= 0.6])
        assert len(sel) > 6000
        d = np.abs(mine[sel[:, 0], sel[:, 1]] - m["teapot_rgb"].astype(np.int64)[sel[:, 0] - r0, sel[:, 1] - c0]).max(-1)
        assert (d <= 1).mean() >= 0.92 and (d == 0).mean() >= 0.80, ((d <= 1).mean(), (d == 0).mean())
        r0, r1, c0, c1 = map(int, m["front_box"])
        table_mat = int(mat[np.flatnonzero((mat != teapot_mat) & np.array([mats[k]["kr"] == 0.0 for k in mat]))[0]])
        pts = [(r, c) for r in range(r0, r1, 4) for c in range(c0, c1, 4)]
        low = list(pool.map(lowest_hit(table_mat), pts))
        sel = np.array([p for p, y in zip(pts, low) if y is not None])
        assert len(sel) > 2000
        d = np.abs(mine[sel[:, 0], sel[:, 1]] - m["front_rgb"].astype(np.int64)[sel[:, 0] - r0, sel[:, 1] - c0]).max(-1)
        assert d.max() <= 8 and (d <= 1).mean() >= 0.95, (d.max(), (d <= 1).mean(), (d == 0).mean())


# ------------------------------------------------------------------ texel addressing, bump maps and colour arithmetic at their edges
def _rust_as_usize(x):
    """Rust `f64 as usize` (64-bit): NaN and everything <= 0 give 0, >= 2^64 and +inf saturate to 2^64 - 1."""
    if not x > 0.0:
        return 0
    return 2**64 - 1 if x >= 2.0**64 else int(x)


def _texel_probe(ob, w, h, uv, o, d, tri=((-4, -4, 0), (4, -4, 0), (0, 4, 0))):
    """Colour of the texel the oracle reads for the ray (o, d) on one triangle with per-vertex uv, under ambient light 1 (texel colour = pixel colour),
    and the texel (x, y) derived in Python from the oracle's barycentrics with the reference's operation order (raytracer.rs:43-53)."""
    yy, xx = np.mgrid[0:h, 0:w]
    tex = np.stack([xx * 20 + 1, yy * 20 + 2, np.full_like(xx, 7)], -1).astype(np.uint8)    # texel (x, y) -> (20x + 1, 20y + 2, 7)
    mats = [dict(ka=(1, 1, 1), kd=(0, 0, 0), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=0, bump=-1)]
    s = tiny_scene(ob, [tri], lights=((0, 1.0, (0, 0, 0)),), mats=mats, tex=[tex], uv=np.asarray(uv, np.float64).reshape(1, 3, 3))
    hit, t, u, v, _ = s.intersect(o, d)
    assert hit
    wb = 1.0 - u - v
    tx = uv[1][0] * u + uv[2][0] * v + uv[0][0] * wb
    ty = uv[1][1] * u + uv[2][1] * v + uv[0][1] * wb
    xi, yi = _rust_as_usize(tx * float(w)) % w, _rust_as_usize(ty * float(h)) % h
    c = s.get_ray_colour(o, d)
    return ((c >> 16) & 255, (c >> 8) & 255, c & 255), (xi * 20 + 1, yi * 20 + 2, 7), (tx * w, ty * h, xi, yi)


NAN = float("nan")
V1_RAY = ((-4.0, -4.0, -5.0), (0.0, 0.0, 1.0))                 # hits vertex v1 exactly: u = v = 0, w = 1 (ray.rs:75,82 keep it)
MID_RAY = ((0.3, -1.1, -5.0), (0.0, 0.0, 1.0))                 # an interior point: u, v, w all in (0, 1)


def test_texel_index_non_power_of_two_sizes(ob):
    """raytracer.rs:52-53 on textures whose sides are not powers of two: (x as usize) % width for x below 2^32, in [2^32, 2^64), at and beyond 2^64
    (saturating: (2^64 - 1) % w), +inf, NaN, -inf and -0 (all 0).  At v1 the uv of v1 comes through exactly (w = 1, u = v = 0), except where another
    vertex's uv is infinite: inf * 0 = NaN there, so the index is 0."""
    sizes = ((1, 3), (3, 5), (5, 7), (7, 6), (6, 10), (10, 1))
    for w, h in sizes:
        cases = [  # (uv of v1, uv of v2, uv of v3), ray, expected (x index, y index) -- None: derived only
            ([(2.5 / w, 4.5 / h, 0), (0.1, 0.2, 0), (0.3, 0.4, 0)], V1_RAY, (2 % w, 4 % h)),                               # below 2^32
            ([((2**40 + 5) / w, (2**33 + 3) / h, 0), (0, 0, 0), (0, 0, 0)], V1_RAY, None),                                    # [2^32, 2^64)
            ([(float(2**40 + 5), float(2**50 + 7), 0), (0, 0, 0), (0, 0, 0)], V1_RAY, ((2**40 + 5) * w % w, (2**50 + 7) * h % h)),   # exact products
            ([(1e25, 2.0**64, 0), (0, 0, 0), (0, 0, 0)], V1_RAY, ((2**64 - 1) % w, (2**64 - 1) % h)),                         # >= 2^64: saturates
            ([(INF, INF, 0), (0, 0, 0), (0, 0, 0)], V1_RAY, ((2**64 - 1) % w, (2**64 - 1) % h)),                              # +inf: saturates
            ([(NAN, -INF, 0), (0, 0, 0), (0, 0, 0)], V1_RAY, (0, 0)),                                                         # NaN, -inf -> 0
            ([(-0.0, -3.25, 0), (0, 0, 0), (0, 0, 0)], V1_RAY, (0, 0)),                                                       # -0, negative -> 0
            ([(0.1, 0.1, 0), (INF, 2.0**70, 0), (0.2, INF, 0)], V1_RAY, (0, 0)),                                              # inf * u(=0) = NaN
            ([(0.1, 0.1, 0), (INF, 2.0**70, 0), (0.2, 0.3, 0)], MID_RAY, ((2**64 - 1) % w, (2**64 - 1) % h)),                 # interior: inf, 2^70 * u
            ([(3.7, 1.3, 0), (-2.2, 5.9, 0), (11.1, -0.4, 0)], MID_RAY, None),                                                # ordinary interpolation
            ([((2**36 + 0.5) / w, 1e10, 0), ((2**36 + 9.25) / w, 3e9, 0), (2**36 / w, 7e9, 0)], MID_RAY, None),               # interpolated, >= 2^32
        ]
        for uv, (o, d), want in cases:
            got, derived, (fx, fy, xi, yi) = _texel_probe(ob, w, h, uv, o, d)
            assert got == derived, (w, h, uv, fx, fy)
            if want is not None:
                assert (xi, yi) == want, (w, h, uv, fx, fy, xi, yi, want)
    assert (2**64 - 1) % 3 == 0 and (2**64 - 1) % 7 == 1            # the saturated index: 0 for w = 3, 1 for w = 7
    got, _, (fx, _, xi, _) = _texel_probe(ob, 7, 3, [((2**40 + 5) / 7, 0.5, 0), (0, 0, 0), (0, 0, 0)], *V1_RAY)
    assert 2**32 <= fx < 2**64 and xi == int(fx) % 7 and got[0] == xi * 20 + 1


def _bump_scene(ob, tex_wh, bump):
    """One triangle facing the camera (vertex normals (0, 0, -1)), uniform colour texture 200 of tex_wh = (w, h), bump map `bump` ([h, w, 3]), one
    directional light (0, 0, -1) of intensity 1 and kd = 1: the pixel is trunc(200 * n.l) for the bumped normal n."""
    tw, th = tex_wh
    mats = [dict(ka=(0, 0, 0), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=0, bump=1)]
    return tex_wh, lambda uv: tiny_scene(ob, [((-4, -4, 0), (4, -4, 0), (0, 4, 0))], lights=((2, 1.0, (0, 0, -1)),), mats=mats,
                                         tex=[np.full((th, tw, 3), 200, np.uint8), np.ascontiguousarray(bump, np.uint8)],
                                         uv=np.asarray(uv, np.float64).reshape(1, 3, 3))


def test_bump_map_of_another_width(ob):
    """raytracer.rs:127-128 addresses the bump map with the COLOUR texture's (x, y) and the BUMP map's width: index = bump.width * y + x.  Hand-derived
    normals (raytracer.rs:130-161) for n = (0, 0, -1): t = n x (0, 1, 0) = (1, -0, 0), b = n x t = (0, -1, 0), so bump texel c gives the normal
    (bv.x, -bv.y, -bv.z) with bv = 2 c / |c| - 1, and the light (0, 0, -1) sees n.l = bv.z / |bv|:
      (0, 0, 255): bv = (-1, -1, 1), n.l = 1 / sqrt(3) -> trunc(200 / sqrt(3)) = 115;
      (128, 128, 255): n.l = 0.92636 -> 185;   (40, 40, 255): n.l = 0.69660 -> 139;   (255, 0, 0): bv.z = -1, n.l < 0 -> no diffuse, 0."""
    right, wrong, other = (0, 0, 255), (128, 128, 255), (255, 0, 0)
    for (tw, th), (bw, bh), (x, y) in (((3, 2), (5, 2), (2, 1)),       # wider bump map: index 5 * 1 + 2 = 7 -> bump row 1, column 2
                                        ((3, 2), (5, 2), (1, 0)),
                                        ((3, 2), (2, 4), (2, 0)),       # narrower, taller: index 2 * 0 + 2 = 2 wraps to bump row 1, column 0
                                        ((3, 2), (2, 4), (2, 1)),       # index 2 * 1 + 2 = 4 -> bump row 2, column 0
                                        ((8, 3), (4, 4), (7, 2))):      # exactly fitting: index 4 * 2 + 7 = 15, the bump map's last texel
        bump = np.empty((bh, bw, 3), np.uint8); bump[:] = other
        k = bw * y + x
        own = (int((y + 0.5) / th * bh) % bh, int((x + 0.5) / tw * bw) % bw)    # the texel the bump map's OWN (x, y) would address: must not be read
        bump[own] = wrong                                               # (the exactly fitting case: both are the last texel)
        bump[k // bw, k % bw] = right
        _, mk = _bump_scene(ob, (tw, th), bump)
        s = mk([((x + 0.5) / tw, (y + 0.5) / th, 0), (0, 0, 0), (0, 0, 0)])
        assert s.get_ray_colour(*V1_RAY) == 0x737373, ((tw, th), (bw, bh), (x, y))              # 115
    for c, want in (((128, 128, 255), 185), ((40, 40, 255), 139), ((255, 0, 0), 0)):
        _, mk = _bump_scene(ob, (1, 1), np.array([[c]], np.uint8))
        assert mk([(0.5, 0.5, 0), (0, 0, 0), (0, 0, 0)]).get_ray_colour(*V1_RAY) == want * 0x010101, c


def test_colour_arithmetic_edges(ob):
    """clamp_u8 of NaN is 0 and of +inf 255 (raytracer.rs:97-108); kr = 1 over an infinite local colour blends inf * (1 - 1) = NaN -> black
    (raytracer.rs:95); ns = -1 is the 'no specular' sentinel (raytracer.rs:286) and nextafter(-1, 0) is not."""
    L = ob.lib()
    assert L.oracle_clamp_u8(INF) == 255 and L.oracle_clamp_u8(-INF) == 0 and L.oracle_clamp_u8(NAN) == 0 and L.oracle_clamp_u8(-0.0) == 0
    assert L.oracle_f64_as_usize(2.0**64) == 2**64 - 1 and L.oracle_f64_as_usize(2.0**64 - 2048) == 2**64 - 2048 and L.oracle_f64_as_usize(-INF) == 0
    tri = [((-4, -4, 0), (4, -4, 0), (0, 4, 0))]
    tex = [np.full((2, 2, 3), 200, np.uint8)]
    probe = ((0.0, -1.0, -5.0), (0.0, 0.0, 1.0))                     # reflects straight back (n = (0, 0, -1)) and misses: reflected colour white
    for kr, want in ((1.0, 0x000000), (0.5, 0xFFFFFF), (0.0, 0xFFFFFF)):
        mats = [dict(ka=(1, 1, 1), kd=(0, 0, 0), ks=(0, 0, 0), ns=-1.0, kr=kr, tex=0, bump=-1)]
        assert tiny_scene(ob, tri, lights=((0, INF, (0, 0, 0)),), mats=mats, tex=tex).get_ray_colour(*probe) == want, kr
    # specular only: n = v = l = (0, 0, -1), so r = l and r.v / (|r| |v|) = 1, pow(1, ns) = 1: 200 * ks 1 * intensity 0.5 = 100 unless ns == -1
    for ns, want in ((-1.0, 0), (math.nextafter(-1.0, 0.0), 100), (-5.0, 100), (0.0, 100), (INF, 100), (NAN, 100)):
        mats = [dict(ka=(0, 0, 0), kd=(0, 0, 0), ks=(1, 1, 1), ns=ns, kr=0.0, tex=0, bump=-1)]
        assert tiny_scene(ob, tri, lights=((2, 0.5, (0, 0, -1)),), mats=mats, tex=tex).get_ray_colour(*probe) == want * 0x010101, ns
