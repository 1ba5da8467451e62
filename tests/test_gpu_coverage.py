"""The coverage pass of whole frames (csrc/coverage.hip, csrc/coverage_rule.hpp; RRT_FLAG_NO_COVERAGE = coverage=False turns it off): a wave whose mask bit
is clear stores WHITE and walks nothing, and no pixel may change.  Every frame here is compared three ways, bit for bit, in the three forced walks: the default
raytracer, the raytracer without the pass, and the oracle.

 1. the teapot at 64x48, 37x23 (partial tiles, an untraced row, an odd last column) and 1x1; at 64x48 the pass must prove some waves empty;
 2. scenes of one to three triangles in a 64x32 frame of the creation pose, where every projection is exact in f64: corners of PADDED boxes that project onto the
    outermost sub-sample of a wave (the wave touches the box's rectangle in one point), corners on 4-pixel block boundaries, and a triangle edge that lies on the
    outermost sub-sample column of a wave, so that the oracle has hits in that boundary wave; the number of waves proved empty must be the one a restatement of
    the rule in numpy gives for the box records read back from the device;
 3. a triangle with a corner behind the eye: the mask is fully set;
 4. changes between frames -- set_camera (a move, a rotation), set_triangles -- and two frame sizes in flight on twelve streams, more than the pool has buffers, without
    synchronising in between;
 5. the mask is off, and the frames are equal, with an origin-plane triangle, with RRT_FLAG_NO_CULL, with the flag, for a progressive frame, and by default for a
    frame of fewer than 49 152 waves (the tests above create their raytracers with RRT_FLAG_COVERAGE_ALWAYS: their frames are small on purpose);
 6. frames whose mask is beyond the kernel's default LDS limit: 3840x2160 (raised limit) and 5128x3072 (no LDS).
"""
import numpy as np
import pytest

import coverage_checks
from bitwise import assert_same_bits
from gpu_checks import CHAIN_PAD, FORCED_MODES, MATS, ORIGIN, flat_normals, oracle_for

pytestmark = pytest.mark.gpu


ON = "always"              # RRT_FLAG_COVERAGE_ALWAYS: by default a frame of fewer than 49 152 waves runs without the pass, and the frames here are small on purpose

WHITE = 0x00FFFFFF
TEX = [np.full((2, 2, 3), (200, 60, 20), np.uint8)]          # (no lighting of the default lights brings its blue channel to 255: a hit is never WHITE)


def three_way(rrt, make, osc, w, h, what):
    """The frame of make(mode, coverage) for coverage on and off in every forced walk, against the oracle's frame; returns (oracle frame, last default raytracer)."""
    ref, _ = osc.render(w, h)
    rt_on = None
    for mode in FORCED_MODES:
        rt_on, rt_off = make(mode, ON), make(mode, False)
        on, off = rt_on.render(w, h), rt_off.render(w, h)
        assert rt_off.coverage_info()["state"] == "flag", (what, mode, rt_off.coverage_info())
        assert_same_bits(on, off, f"{what}, walk {mode}, {w}x{h}: default against RRT_FLAG_NO_COVERAGE")
        assert_same_bits(on, ref, f"{what}, walk {mode}, {w}x{h}: default against the oracle")
    return ref, rt_on


# ------------------------------------------------------------------ 1. the teapot
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23), (1, 1)])
def test_teapot_frames(rrt, teapot, teapot_oracle, w, h):
    make = lambda mode, cov: rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode, coverage=cov)
    ref, rt = three_way(rrt, make, teapot_oracle, w, h, "teapot")
    info = rt.coverage_info(count=True)
    print(f"\n[coverage] teapot {w}x{h}: {info}")
    assert info["state"] == "on" and info["n_waves"] == 4 * ((w + 7) // 8) * ((h + 7) // 8), info
    if (w, h) == (64, 48):
        assert 0 < info["n_proved_empty"] < info["n_waves"], info
        assert (ref[1:] == WHITE).any() and (ref[1:] != WHITE).any()


# ------------------------------------------------------------------ 2. block boundaries
W2, H2 = 64, 32            # creation pose, viewport 1: a point (X, Y, Z) projects to xd = 64 X / (Z + 10), yd = 32 (Y - 2) / (Z + 10) -- exact for the dyadic values below
TOP2 = H2 - H2 // 2


def rule_waves(tboxes, w, h, eye=ORIGIN):
    """csrc/coverage_rule.hpp restated (tests/coverage_checks.py, held to the header's bits by tests/test_coverage_restatement.py) for the identity basis and
    viewport (1, 1, 1): the [waves_y, waves_x] mask of the box records `tboxes` (bytes of RRT_BUF_TBOXES).  Comparing the library's count with this one checks
    how the kernel MARKS (its word patterns, the copy in LDS, the flush) against the rule; it does not check the rule, whose independent references are the
    oracle's frames here and the slab tests of tests/test_coverage_rule.py."""
    frame = coverage_checks.frame_of(w, h, (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), eye)
    return coverage_checks.mask_of(frame, coverage_checks.rects_of(frame, tboxes))


def at(xd, yd, z):
    """The point at depth z (scene z) that projects onto (xd, yd) of the 64x32 frame."""
    g = z + 10.0
    return (xd * g / 64.0, 2.0 + yd * g / 32.0, z)


def boundary_scenes():
    """name -> (triangles, pixels (px, py) where the oracle must not be WHITE).  p = the index pad: a vertex `p` inside a position puts its PADDED box corner on it."""
    p = CHAIN_PAD
    out = {}
    # one triangle at depth 4 (z = -6): its padded box spans xd in [-12.5, 8] and yd in [-3, 4.5], so it touches wave bx = 4 (xd in [-16, -12.5]) in its last
    # sub-sample column, wave bx = 10 (xd from 8) in its first, wave by = 4 (yd in [-3, 0.5]) in its lowest row and wave by = 3 (yd up to 4.5) in its top row
    x0, y0, _ = at(-12.5, -3.0, -6.0); x1, y1, _ = at(8.0, 4.5, -6.0)
    out["box_on_subsamples"] = ([[(x0 + p, y0 + p, -6.0), (x1 - p, y0 + p, -6.0), (x0 + p, y1 - p, -6.0)]], [(24, 16), (21, 18)])
    # two triangles: one at depth 8 whose padded box has its corners on 4-pixel block boundaries (xd = -8 and 12, yd = -4 and 8), one at depth 4 whose left EDGE lies on
    # the last sub-sample column of wave bx = 12 (xd = 19.5) from yd = -6 to 6: the rays of that column pass through the edge itself
    a0, b0, _ = at(-8.0, -4.0, -2.0); a1, b1, _ = at(12.0, 8.0, -2.0)
    e0 = at(19.5, -6.0, -6.0); e1 = at(19.5, 6.0, -6.0); e2 = at(27.0, 0.0, -6.0)
    out["blocks_and_edge"] = ([[(a0 + p, b0 + p, -2.0), (a1 - p, b0 + p, -2.0), (a1 - p, b1 - p, -2.0)], [e0, e2, e1]], [(51, 16), (51, 14), (40, 18)])
    # three triangles: the two above and one tilted in depth (z from -7 to 5), whose box has corners at two depths
    out["three_with_depth"] = (out["blocks_and_edge"][0] + [[(-3.0, -1.0, -7.0), (-1.0, -1.5, 5.0), (-2.5, 1.0, -1.0)]], [(51, 16), (40, 18)])
    return out


@pytest.mark.parametrize("name", ["box_on_subsamples", "blocks_and_edge", "three_with_depth"])
def test_block_boundary_triangles(rrt, ob, name):
    tris, must_hit = boundary_scenes()[name]
    pos = np.asarray(tris, np.float64)
    n = len(pos)
    A = dict(pos=pos, uv=np.zeros((n, 3, 3)), nrm=flat_normals(pos, ORIGIN), mat=np.zeros(n, np.uint32), materials=MATS, textures=TEX)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], MATS, TEX)
    lights = rrt.default_lights()
    osc = oracle_for(ob, A, lights)
    make = lambda mode, cov: rrt.RayTracer(sd, lights, box_filter=mode, coverage=cov)
    ref, rt = three_way(rrt, make, osc, W2, H2, name)
    for px, py in must_hit:
        assert ref[py, px] != WHITE, f"{name}: the oracle finds nothing in pixel ({px}, {py}): the scene does not put a hit where the test needs one"
    assert rt.last_stats()["filter_pad"] == CHAIN_PAD
    info = rt.coverage_info(count=True)
    want = rule_waves(rt.buffer("tboxes"), W2, H2)
    print(f"\n[coverage] {name}: {info}; the rule restated marks {int(want.sum())} of {want.size} waves")
    assert info["state"] == "on" and info["n_waves"] == want.size and info["n_proved_empty"] == want.size - int(want.sum()) > 0, (info, int(want.sum()))
    # every pixel of a wave the restated rule leaves clear is WHITE in the oracle's frame (row 0 is not traced)
    clear = np.repeat(np.repeat(~want, 4, 0), 4, 1)[:H2, :W2]
    clear[0] = False
    assert (ref[clear] == WHITE).all()
    if name == "box_on_subsamples":      # the four waves the box touches in one sub-sample column / row are marked, their outer neighbours are not
        assert want[3:5, 4].all() and want[3:5, 10].all() and not want[:, 3].any() and not want[:, 11].any() and not want[2].any() and not want[5].any(), want.astype(int)


# ------------------------------------------------------------------ 3. the eye plane
def test_corner_behind_the_eye_marks_the_whole_frame(rrt, ob):
    pos = np.asarray([[(-3.0, 0.0, -15.0), (3.0, 0.5, -4.0), (0.0, 4.0, 5.0)], [(4.0, 1.0, -3.0), (5.0, 1.0, -3.0), (4.0, 2.0, -3.0)]], np.float64)
    n = len(pos)
    A = dict(pos=pos, uv=np.zeros((n, 3, 3)), nrm=flat_normals(pos, ORIGIN), mat=np.zeros(n, np.uint32), materials=MATS, textures=TEX)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], MATS, TEX)
    lights = rrt.default_lights()
    make = lambda mode, cov: rrt.RayTracer(sd, lights, box_filter=mode, coverage=cov)
    ref, rt = three_way(rrt, make, oracle_for(ob, A, lights), 64, 48, "corner behind the eye")
    info = rt.coverage_info(count=True)
    assert info == {"state": "on", "n_waves": 192, "n_proved_empty": 0}, info
    assert (ref[1:] != WHITE).any() and (ref[1:] == WHITE).any()


# ------------------------------------------------------------------ 4. changes between frames
def test_next_frame_after_set_camera_and_set_triangles(rrt, teapot):
    lights = rrt.default_lights()
    w, h = 96, 64
    rt = rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=ON)
    first = rt.render(w, h)
    empty_first = rt.coverage_info(count=True)["n_proved_empty"]
    for what, cam in (("move", rrt.look_at((9.0, 2.0, 1.0), (0.0, 1.0, 0.0))), ("rotation", dict(rrt.look_at((9.0, 2.0, 1.0), (0.0, 3.0, 2.0))))):
        rt.set_camera(**cam)
        got = rt.render(w, h)
        info = rt.coverage_info(count=True)
        fresh = rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False)
        fresh.set_camera(**cam)
        assert_same_bits(got, fresh.render(w, h), f"after set_camera ({what})")
        assert info["state"] == "on" and info["n_proved_empty"] > 0, info
        assert (got != first).any()
    rt.reset_camera()
    assert_same_bits(rt.render(w, h), first, "back at the creation pose")
    assert rt.coverage_info(count=True)["n_proved_empty"] == empty_first
    # new triangles: the teapot's, moved and shrunk (another part of the frame is empty now)
    pos, uv, nrm, mat = teapot.triangles()
    pos2 = np.asarray(pos, np.float64).reshape(-1, 3, 3) * 0.5 + np.array([3.0, 2.0, 0.0])
    rt.set_triangles(pos2, uv, nrm, mat)
    got = rt.render(w, h)
    info = rt.coverage_info(count=True)
    fresh = rrt.RayTracer.from_arrays(pos2, uv, nrm, mat, teapot.materials(), teapot.textures(), lights, box_filter="bundle", coverage=False)
    assert_same_bits(got, fresh.render(w, h), "after set_triangles")
    assert info["state"] == "on" and info["n_proved_empty"] > empty_first, (info, empty_first)


def test_two_sizes_on_many_streams_without_synchronising(rrt, teapot):
    """Frames of two sizes of ONE raytracer in flight on twelve streams, more than the pool's eight mask buffers, with no synchronisation in between.  Part one: a new
    stream for every launch, so that no launch finds a buffer of its own stream and every pick after the eighth is decided by the event behind a buffer's last frame
    (or the frame renders without a mask).  Part two: the streams in turn again, each finding the pool in whatever state part one left.  A mask handed out while
    its frame is still in flight is cleared and refilled for a frame of the other size under the reading kernel."""
    import torch
    lights = rrt.default_lights()
    sizes = ((640, 480), (320, 200))
    want = {s: rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False).render(*s) for s in sizes}
    rt = rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=ON)  # (a forced walk: no measurement, which would synchronise the stream)
    streams = [torch.cuda.Stream() for _ in range(12)]
    n = 3 * len(streams)
    fbs = [torch.zeros(sizes[k % 2][0] * sizes[k % 2][1], dtype=torch.int32, device="cuda") for k in range(n)]
    torch.cuda.synchronize()
    states = []
    for k in range(n):
        rt.render_into(fbs[k], *sizes[k % 2], stream=streams[(k * 5) % len(streams)].cuda_stream)      # (5 and 12 are coprime: every stream, never the one before)
        states.append(rt.coverage_info()["state"])
    torch.cuda.synchronize()
    print(f"\n[coverage] states of the {n} launches: {states}")
    assert set(states) <= {"on", "pool"} and states.count("on") >= 8, states
    for k in range(n):
        s = sizes[k % 2]
        assert_same_bits(fbs[k].cpu().numpy().view(np.uint32).reshape(s[1], s[0]), want[s], f"launch {k} of {s[0]}x{s[1]}")


# ------------------------------------------------------------------ 5. where the mask is off
def test_mask_is_off_where_the_guarantee_is_not_in_force(rrt, ob, teapot, teapot_oracle):
    lights = rrt.default_lights()
    w, h = 64, 48
    # an origin-plane triangle: the plane y = 2 contains the eye (0, 2, -10)
    pos = np.asarray([[(-2.0, 2.0, -5.0), (2.0, 2.0, -5.0), (0.0, 2.0, -2.0)], [(-1.0, 0.0, -4.0), (1.0, 0.0, -4.0), (0.0, 3.5, -4.0)]], np.float64)
    n = len(pos)
    A = dict(pos=pos, uv=np.zeros((n, 3, 3)), nrm=flat_normals(pos, (0.0, 5.0, -10.0)), mat=np.zeros(n, np.uint32), materials=MATS, textures=TEX)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], MATS, TEX)
    ref, _ = oracle_for(ob, A, lights).render(w, h)
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(sd, lights, box_filter=mode, coverage=ON)
        assert rt.coverage_info() == {"state": "no_frame", "n_waves": 0}
        got = rt.render(w, h)
        assert rt.last_stats()["origin_plane_triangles"] > 0
        assert rt.coverage_info(count=True) == {"state": "suspects", "n_waves": 0, "n_proved_empty": 0}
        assert_same_bits(got, rrt.RayTracer(sd, lights, box_filter=mode, coverage=False).render(w, h), f"origin-plane triangle, walk {mode}")
        assert_same_bits(got, ref, f"origin-plane triangle, walk {mode}, against the oracle")
    # RRT_FLAG_NO_CULL, and the parts of a frame that are not a whole frame of one GPU
    tref, _ = teapot_oracle.render(w, h)
    rt = rrt.RayTracer(teapot, lights, no_cull=True, coverage=ON)
    assert_same_bits(rt.render(w, h), tref, "RRT_FLAG_NO_CULL against the oracle")
    assert rt.coverage_info(count=True) == {"state": "no_cull", "n_waves": 0, "n_proved_empty": 0}
    rt = rrt.RayTracer(teapot, lights, coverage=ON)
    assert_same_bits(rt.render(w, h), tref, "default against the oracle")
    assert rt.coverage_info()["state"] == "on"
    assert_same_bits(rt.render_progressive(w, h, chunk_rows=10), tref, "progressive frame")
    assert rt.coverage_info()["state"] == "not_whole"
    assert_same_bits(rt.render(w, h), tref, "a whole frame again")
    assert rt.coverage_info()["state"] == "on"


def test_default_bound_on_the_frame_size(rrt, teapot, teapot_oracle):
    """Without RRT_FLAG_COVERAGE_ALWAYS: 64x48 runs without the pass, 1024x768 (49 152 waves) and the headline's 1920x1080 run with it; same frames."""
    lights = rrt.default_lights()
    rt, off = rrt.RayTracer(teapot, lights, box_filter="bundle"), rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False)
    assert_same_bits(rt.render(64, 48), teapot_oracle.render(64, 48)[0], "64x48 against the oracle")
    assert rt.coverage_info(count=True) == {"state": "small_frame", "n_waves": 0, "n_proved_empty": 0}
    assert_same_bits(rt.render(1016, 768), off.render(1016, 768), "1016x768")
    assert rt.coverage_info()["state"] == "small_frame"                 # 127 x 96 tiles: 48 768 waves
    for w, h in ((1024, 768), (1920, 1080)):
        assert_same_bits(rt.render(w, h), off.render(w, h), f"{w}x{h}: default against RRT_FLAG_NO_COVERAGE")
        info = rt.coverage_info(count=True)
        print(f"\n[coverage] teapot {w}x{h}: {info}")
        assert info["state"] == "on" and info["n_waves"] == 4 * (w // 8) * (h // 8) and 0 < info["n_proved_empty"] < info["n_waves"], info


@pytest.mark.parametrize("w,h,path", [(3840, 2160, "16 200 words: the LDS limit raised for the kernel"), (5128, 3072, "30 768 words: beyond the raised limit, global atomics")])
def test_masks_beyond_the_default_lds_limit(rrt, teapot, w, h, path):
    """The coverage kernel's two other paths (coverage.hip: launch_coverage): default against RRT_FLAG_NO_COVERAGE, compared on the device."""
    import torch
    lights = rrt.default_lights()
    fb = [torch.zeros(w * h, dtype=torch.int32, device="cuda") for _ in range(2)]
    rt, off = rrt.RayTracer(teapot, lights, box_filter="bundle"), rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False)
    rt.render_into(fb[0], w, h); off.render_into(fb[1], w, h)
    torch.cuda.synchronize()
    info = rt.coverage_info(count=True)
    print(f"\n[coverage] teapot {w}x{h} ({path}): {info}")
    assert (info["n_waves"] // 4 + 7) // 8 == int(path.split(" words")[0].replace(" ", "")), info
    assert info["state"] == "on" and 0.3 * info["n_waves"] < info["n_proved_empty"] < 0.45 * info["n_waves"], info
    assert torch.equal(fb[0], fb[1]) and int((fb[0] != WHITE).sum()) > w * h // 4
