"""Wide boxes and simple waves of whole frames (csrc/coverage_rule.hpp "wide boxes", csrc/coverage.hip, render_kernel's wide_list_hit; RRT_FLAG_NO_WIDE_COVER =
wide_cover=False): a covered wave that only the listed boxes of the root's own list reach tests its primary rays against those few triangles instead of walking,
and no pixel may change.  (The bundle-filter kernel does; the lane-filter and ray-walk kernels are built without the path and walk every covered wave: their
frames, masks and counts are held to the same values all the same.)

Every frame is compared bit for bit among the default raytracer, RRT_FLAG_NO_WIDE_COVER, RRT_FLAG_NO_COVERAGE and the oracle, in the lane, bundle and ray walks (all
created with RRT_FLAG_COVERAGE_ALWAYS: the frames are small on purpose; test_scenes_on_the_cpu needs no GPU), and in the bundle walk also against a raytracer
built on the host (RRT_FLAG_HOST_SETUP: the other builder's root slot range), whose counts must be the GPU build's; the library's n_wide and n_simple_waves must equal the counts of tests/wide_cover_checks.py on
the box records read back from the device, and its mask the restated mask.  Materials have no specular term and no bump map: no pow, the oracle's bits.

 1. floor_cluster  a floor quad that straddles the root's planes and twelve small triangles inside one octant: simple, ordinary and empty waves in one frame
                   (256x192 and the odd 253x141);
 2. ties           two identical coplanar wide triangles with different materials -- ties on t: the first list position must win -- and a third, parallel, behind
                   them; in both push orders;
 3. strips         twenty wide slats, each two wave rows of the full width: the list overflows, and whichever four find it full must mark `fine` (the slats are
                   disjoint and of one size, so the count of simple waves is the same whichever they are);
 4. octant         a large triangle wholly inside one child octant: wide by size, not in the root's list, ordinary;
 5. mirror         a wide mirror triangle (kr > 0) facing a lit floor, two point lights: shadow and reflection walks follow a replaced primary walk;
 6. poses          scene 1 from a look_at pose with a roll, and from an eye for which the floor's box crosses the eye's plane (no simple wave);
 7. teapot         model2.obj at 256x144.
"""
import numpy as np
import pytest

import coverage_checks as cc
import wide_cover_checks as wc
from bitwise import assert_same_bits
from gpu_checks import FORCED_MODES, N_THREADS, ORIGIN, flat_normals, oracle_for, quad
from scenes import CREATION, arrays_of
from test_gpu_coverage_poses import oracle_frame

ON = "always"
WHITE = 0x00FFFFFF
VIEWPORT = (1.0, 1.0, 1.0)
PAD = 20.0 / 32768.0
TEXS = [np.full((2, 2, 3), (200, 60, 20), np.uint8), np.full((2, 2, 3), (30, 90, 210), np.uint8), np.full((2, 2, 3), (60, 200, 80), np.uint8)]   # (a hit is never WHITE)


def material(tex, kr=0.0):
    return dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=kr, tex=tex, bump=-1)


def arrays(pos, mat=None, materials=None):
    pos = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    n = len(pos)
    return dict(pos=pos, uv=np.zeros((n, 3, 3)), nrm=flat_normals(pos, ORIGIN), mat=np.zeros(n, np.uint32) if mat is None else np.asarray(mat, np.uint32),
                materials=materials or [material(0), material(1), material(2)], textures=TEXS)


FLOOR = quad((-6.0, -1.0, -4.0), (6.0, -1.0, -4.0), (6.0, -1.0, 8.0), (-6.0, -1.0, 8.0))          # straddles x = 0 and z = 0: the root's own list (and pushed first)


def cluster(seed=5, n=12):
    """n small triangles around (2.5, 1.5, 3), inside the octant x, y, z > 0."""
    rng = np.random.default_rng(seed)
    centre = np.array([2.5, 1.5, 3.0]) + rng.uniform(-0.8, 0.8, (n, 1, 3))
    return centre + rng.uniform(-0.25, 0.25, (n, 3, 3))


def scene_floor_cluster():
    return arrays(np.concatenate([np.asarray(FLOOR), cluster()]), mat=[0, 0] + [1] * 12)


def scene_ties(swapped):
    front = [(-5.0, -1.0, 4.0), (5.0, -1.0, 4.0), (0.0, 5.0, 4.0)]
    behind = [(-7.0, -1.5, 6.0), (7.0, -1.5, 6.0), (0.0, 7.0, 6.0)]
    return arrays([front, front, behind], mat=[1, 0, 2] if swapped else [0, 1, 2])


def scene_strips():
    """Twenty slats at depth 12 (z = 2) in a 256x192 frame: slat i covers the wave rows 4 + 2 i and 5 + 2 i (yd from top - 4 r0 - 6 to top - 4 r0 - 0.5) and reaches
    beyond both sides of the frame (x from -7 to 7; the frame ends at +-6)."""
    tris = []
    for i in range(20):
        r0 = 4 + 2 * i
        y_lo, y_hi = 2.0 + (96 - 4 * r0 - 6.0) * 12.0 / 192.0, 2.0 + (96 - 4 * r0 - 0.5) * 12.0 / 192.0
        tris.append([(-7.0, y_lo, 2.0), (7.0, y_lo, 2.0), (0.0, y_hi, 2.0)])
    return arrays(tris, mat=[i % 3 for i in range(20)])


def scene_octant():
    small = [(-0.5, -0.5, 15.0), (0.5, -0.5, 15.0), (0.0, 0.5, 15.0)]                             # pushed first: stays in the root (and straddles its planes)
    large = [(0.5, 0.5, 6.0), (9.0, 0.5, 6.0), (0.5, 8.0, 6.0)]                                   # wholly inside x, y, z > 0
    return arrays([small, large] + list(cluster(seed=9, n=4) + np.array([4.0, 3.0, 1.0])), mat=[0, 1, 2, 2, 2, 2])


def scene_mirror():
    mirror = [(-5.0, -0.5, 7.0), (5.0, -0.5, 7.0), (0.0, 6.0, 7.0)]                               # straddles x = 0 and y = 0
    mats = [material(0), material(1), material(2, kr=0.5)]
    return arrays(np.concatenate([np.asarray(FLOOR), [mirror], cluster()]), mat=[0, 0, 2] + [1] * 12, materials=mats)


def mirror_lights(rrt):
    return [rrt.Light.Ambient(0.2), rrt.Light.Point(0.5, rrt.Vector3d(-4.0, 6.0, -2.0)), rrt.Light.Point(0.4, rrt.Vector3d(5.0, 4.0, 1.0))]


# ------------------------------------------------------------------ the device's records and the restated counts
def root_slot_end(rt):
    """The end of the root's own slots from the device's records: node 0's super-clusters, each run padded to a multiple of 8 (a group record holds no slots)."""
    node0 = rt.buffer("nodes")[:96].view(np.uint32)
    sup_begin, sup_count = int(node0[19]), int(node0[20])
    sup = rt.buffer("supers").view(np.uint32).reshape(-1, 8)[sup_begin:sup_begin + sup_count]
    plain = sup[sup[:, 7] != 0]
    return int(((plain[:, 6] + plain[:, 7] + 7) & ~np.uint32(7)).max()) if len(plain) else 0


def restated(rt, w, h, cam):
    c, hh = cc.box_records(rt.buffer("tboxes"))
    F = cc.frame_of(w, h, VIEWPORT, cam["right"], cam["up"], cam["forward"], cam["eye"])
    return wc.classify(F, cc.rects_of(F, c, hh), root_slot_end(rt))


def four_way(rrt, ob, A, lights, w, h, what, cam=CREATION, key=None, expect_simple=True):
    """The frame of the default raytracer, of RRT_FLAG_NO_WIDE_COVER and of RRT_FLAG_NO_COVERAGE in every forced walk, against the oracle's; the library's mask and
    counts against the restatement.  Returns the restated classification."""
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    ref = oracle_frame(oracle_for(ob, A, lights), key or what, cam, w, h, VIEWPORT)
    traced = ref[h - 2 * (h // 2) + 1:, :2 * (w // 2)]
    assert (traced == WHITE).any() and (traced != WHITE).any(), f"{what}: the oracle's frame shows nothing"
    want = None
    for mode in FORCED_MODES:
        rts = [rrt.RayTracer(sd, lights, box_filter=mode, **kw) for kw in (dict(coverage=ON), dict(coverage=ON, wide_cover=False), dict(coverage=False))]
        for rt in rts:
            if cam is not CREATION:
                rt.set_camera(**cam)
        default, no_wide, no_cover = (rt.render(w, h) for rt in rts)
        assert_same_bits(default, no_wide, f"{what}, walk {mode}, {w}x{h}: default against RRT_FLAG_NO_WIDE_COVER")
        assert_same_bits(default, no_cover, f"{what}, walk {mode}, {w}x{h}: default against RRT_FLAG_NO_COVERAGE")
        assert_same_bits(default, ref, f"{what}, walk {mode}, {w}x{h}: default against the oracle")
        assert rts[0].coverage_info()["state"] == rts[1].coverage_info()["state"] == "on" and rts[2].coverage_info()["state"] == "flag", what
        want = restated(rts[0], w, h, cam)
        info, off = rts[0].wide_cover_info(), rts[1].wide_cover_info()
        assert off == rts[2].wide_cover_info() == {"n_wide": 0, "n_simple_waves": 0}, (what, mode, off)
        for rt in rts[:2]:                                                     # the mask keeps every bit, with and without the list
            assert np.array_equal(rt.coverage_mask(), want["mask"]), f"{what}, walk {mode}: the kernel's mask is not the rule's"
        whole = bool(want["fine"].all())                                       # a box reaches the whole frame: every wave is ordinary and the list is reported empty (rrt.h)
        assert info["n_simple_waves"] == want["n_simple"] and info["n_wide"] == (0 if whole else want["n_wide"]), \
            f"{what}, walk {mode}: the library lists {info}, the rule restated {want['n_wide']} wide boxes and {want['n_simple']} simple waves"
        if mode == "bundle":                                                   # the host builder reports the same root range: same list, same simple waves, same frame
            host = rrt.RayTracer(sd, lights, box_filter=mode, coverage=ON, host_setup=True)
            if cam is not CREATION:
                host.set_camera(**cam)
            assert_same_bits(host.render(w, h), default, f"{what}, walk {mode}, {w}x{h}: RRT_FLAG_HOST_SETUP against the default")
            assert root_slot_end(host) == root_slot_end(rts[0]) and host.wide_cover_info() == info, f"{what}: the host build lists {host.wide_cover_info()}, the GPU build {info}"
    print(f"\n[wide cover] {what} {w}x{h}: {want['n_wide']} listed of {int(want['wide'].sum())} wide boxes, {want['n_simple']} simple of {int(want['mask'].sum())} covered "
          f"of {want['mask'].size} waves; listed boxes per simple wave up to {int(want['per_simple'].max()) if want['n_simple'] else 0}")
    assert (want["n_simple"] > 0) == expect_simple, f"{what}: {want['n_simple']} simple waves restated"
    return want, ref


def test_scenes_on_the_cpu():
    """What the scenes are meant to show, from approximate boxes, without a GPU: chosen by these counts."""
    def count(A, w, h, root_own, cam=CREATION):
        F = cc.frame_of(w, h, VIEWPORT, cam["right"], cam["up"], cam["forward"], cam["eye"])
        return wc.classify(F, cc.rects_of(F, *wc.approx_boxes(A["pos"], PAD)), root_own)
    got = count(scene_floor_cluster(), 256, 192, 2)
    assert got["n_wide"] == 2 and got["n_simple"] > 0 and (got["mask"] & got["fine"]).any() and not got["mask"].all(), (got["n_wide"], got["n_simple"])
    got = count(scene_ties(False), 128, 96, 3)
    assert got["n_wide"] == 3 and got["n_simple"] > 0 and int(got["per_simple"].max()) == 3
    got = count(scene_strips(), 256, 192, 20)
    assert int(got["wide"].sum()) == 20 and got["n_wide"] == 16 and got["n_simple"] == 16 * 128 and int(got["mask"].sum()) == 20 * 128, (got["n_simple"], int(got["mask"].sum()))
    assert (wc.rect_waves(cc.rects_of(cc.frame_of(256, 192, VIEWPORT, **{k: CREATION[k] for k in ("right", "up", "forward", "eye")}), *wc.approx_boxes(scene_strips()["pos"], PAD))) == 128).all()
    got = count(scene_octant(), 128, 96, 1)
    assert got["n_wide"] == 0 and got["n_simple"] == 0 and wc.rect_waves(cc.rects_of(cc.frame_of(128, 96, VIEWPORT, **{k: CREATION[k] for k in ("right", "up", "forward", "eye")}),
                                                                                     *wc.approx_boxes(scene_octant()["pos"], PAD)))[1] >= 16 * 8
    got = count(scene_mirror(), 160, 120, 3)
    assert got["n_wide"] == 3 and got["n_simple"] > 0


# ------------------------------------------------------------------ the scenes on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(256, 192), (253, 141)])
def test_floor_and_cluster(rrt, ob, w, h):
    want, _ = four_way(rrt, ob, scene_floor_cluster(), rrt.default_lights(), w, h, "floor_cluster")
    assert want["n_wide"] == 2 and (want["mask"] & want["fine"]).any() and not want["mask"].all(), "the frame is meant to have simple, ordinary and empty waves"


@pytest.mark.gpu
@pytest.mark.parametrize("swapped", [False, True])
def test_ties_on_t_keep_the_first_list_position(rrt, ob, swapped):
    A = scene_ties(swapped)
    want, ref = four_way(rrt, ob, A, rrt.default_lights(), 128, 96, f"ties{'_swapped' if swapped else ''}")
    assert want["n_wide"] == 3 and int(want["per_simple"].max()) == 3
    # the scene shows the tie: with the front pair's materials exchanged the oracle's frame changes (where the pair is hit first), and nowhere else
    other = oracle_frame(oracle_for(ob, scene_ties(not swapped), rrt.default_lights()), f"ties{'' if swapped else '_swapped'}", CREATION, 128, 96, VIEWPORT)
    assert (other != ref).sum() > 500, "exchanging the materials of the coincident pair must change the frame"


@pytest.mark.gpu
def test_twenty_strips_overflow_the_list(rrt, ob):
    want, _ = four_way(rrt, ob, scene_strips(), rrt.default_lights(), 256, 192, "strips")
    assert int(want["wide"].sum()) == 20 and want["n_wide"] == wc.MAX_WIDE and want["n_simple"] == 16 * 128, (want["n_wide"], want["n_simple"])


@pytest.mark.gpu
def test_large_triangle_inside_one_octant_is_ordinary(rrt, ob):
    want, _ = four_way(rrt, ob, scene_octant(), rrt.default_lights(), 128, 96, "octant", expect_simple=False)
    assert want["n_wide"] == 0 and int(want["mask"].sum()) >= 128


@pytest.mark.gpu
def test_wide_mirror_with_two_point_lights(rrt, ob):
    want, ref = four_way(rrt, ob, scene_mirror(), mirror_lights(rrt), 160, 120, "mirror")
    assert want["n_wide"] == 3
    # the mirror shows the floor and the floor carries shadows: more than the three materials' flat colours
    assert len(np.unique(ref)) > 20, len(np.unique(ref))


@pytest.mark.gpu
def test_poses_of_the_floor_and_cluster(rrt, ob):
    A = scene_floor_cluster()
    rolled = rrt.look_at((7.0, 5.0, -9.0), (0.5, 0.0, 2.0), up=(0.3, 1.0, 0.1))
    want, _ = four_way(rrt, ob, A, rrt.default_lights(), 128, 80, "floor_cluster rolled", cam=rolled)
    assert want["n_wide"] >= 1
    over = dict(eye=(0.0, 1.5, 2.0), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0))      # above the floor, whose box crosses the plane z = 2 of this eye
    want, _ = four_way(rrt, ob, A, rrt.default_lights(), 128, 80, "floor_cluster eye over the floor", cam=over, expect_simple=False)
    assert want["fine"].all() and want["mask"].all()


@pytest.mark.gpu
def test_teapot_256x144(rrt, ob, teapot):
    A = arrays_of(teapot)
    lights = rrt.default_lights()
    w, h = 256, 144
    ref = oracle_for(ob, A, lights).render(w, h, n_threads=N_THREADS)[0]
    want = None
    for mode in FORCED_MODES:
        rts = [rrt.RayTracer(teapot, lights, box_filter=mode, **kw) for kw in (dict(coverage=ON), dict(coverage=ON, wide_cover=False), dict(coverage=False))]
        default, no_wide, no_cover = (rt.render(w, h) for rt in rts)
        assert_same_bits(default, no_wide, f"teapot, walk {mode}: default against RRT_FLAG_NO_WIDE_COVER")
        assert_same_bits(default, no_cover, f"teapot, walk {mode}: default against RRT_FLAG_NO_COVERAGE")
        assert_same_bits(default, ref, f"teapot, walk {mode}: default against the oracle")
        want = restated(rts[0], w, h, CREATION)
        assert rts[0].wide_cover_info() == {"n_wide": want["n_wide"], "n_simple_waves": want["n_simple"]}, (rts[0].wide_cover_info(), want["n_wide"], want["n_simple"])
        assert np.array_equal(rts[0].coverage_mask(), want["mask"])
        if mode == "bundle":                                                   # the host builder's root range, over a root list of many super-clusters
            host = rrt.RayTracer(teapot, lights, box_filter=mode, coverage=ON, host_setup=True)
            assert_same_bits(host.render(w, h), default, "teapot: RRT_FLAG_HOST_SETUP against the default")
            assert root_slot_end(host) == root_slot_end(rts[0]) > 1110 and host.wide_cover_info() == rts[0].wide_cover_info(), (root_slot_end(host), host.wide_cover_info())
    print(f"\n[wide cover] teapot {w}x{h}: {want['n_wide']} wide boxes, {want['n_simple']} simple of {int(want['mask'].sum())} covered waves")
    assert want["n_wide"] == 14 and want["n_simple"] > 0.4 * want["mask"].sum()


@pytest.mark.gpu
def test_largest_mask_under_the_default_lds_limit(rrt, teapot):
    """3700x2100: 463 x 263 tiles, 15 222 mask words -- among the largest frames whose copy of `fine` still goes into the kernel's default 64 KB of LDS beside its
    static queue (coverage.hip: kLdsWords = 15 296; the frames of tests/test_gpu_coverage.py lie beyond it, on the raised limit and on the path without LDS).  The
    launch must succeed, and the frame, the mask and the counts must be what they are without the pass and by the rule."""
    w, h = 3700, 2100
    assert 15100 < ((w + 7) // 8) * ((h + 7) // 8) // 8 + 1 <= 15296
    lights = rrt.default_lights()
    on, off = rrt.RayTracer(teapot, lights, box_filter="bundle"), rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False)
    assert_same_bits(on.render(w, h), off.render(w, h), f"teapot {w}x{h}: default against RRT_FLAG_NO_COVERAGE")
    assert on.coverage_info()["state"] == "on", on.coverage_info()
    want = restated(on, w, h, CREATION)
    assert np.array_equal(on.coverage_mask(), want["mask"]), "the kernel's mask is not the rule's"
    assert on.wide_cover_info() == {"n_wide": want["n_wide"], "n_simple_waves": want["n_simple"]} and want["n_wide"] == 14 and want["n_simple"] > 0, (on.wide_cover_info(), want["n_wide"], want["n_simple"])
