"""The fused frame of a region and of a device-resident tile list on the GPU (include/rrt.h: rrt_render_region, rrt_render_region_device,
rrt_render_tile_list_device).

The statement under test: what these calls write IS what rrt_render writes at the same pixels, bit for bit, in every traversal variant -- the 0 of the pixels
the reference never traces included -- and nothing else is touched.  Every comparison is bitwise.assert_same_bits; every frame compared holds at least
MIN_PIXELS pixels that are neither the background nor 0 (region_render_checks), so white against white cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

from bitwise import assert_same_bits
from gpu_checks import ALL_MODES, FORCED_MODES, assert_frame_close, chain_rrt_lights, chain_scene
from region_render_checks import (SENTINEL, assert_frame_has_content, assert_listed_tiles_only, assert_region_has_content, assert_region_is_crop, crop, listed_pixels,
                                  tiles_of, traced_count)
from scenes import CREATION, EYE3, H3, REGIONS, TARGET, W3, room, teapot_arrays  # noqa: F401  (fixtures: room, teapot_arrays)
from shade_checks import oracle_frame, soup_scene

pytestmark = pytest.mark.gpu

W, H = 64, 48
SMALL_REGIONS = (None, (5, 3, 50, 41))
IN_PLACE = (13, 50, 77, 31)
QUARTERS = ((0, 0, 100, 60), (100, 0, 103, 60), (0, 60, 100, 57), (100, 60, 103, 57))     # a partition of the 203 x 117 frame
VARIANT = dict(lane=0, bundle=1, ray=2)


def sentinels(torch, n):
    return torch.from_numpy(np.full(n, SENTINEL, np.uint32).view(np.int32)).cuda()


def words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def frame3(rrt, teapot):
    """(the 203 x 117 teapot frame at EYE3 of a raytracer with no forced variant, [h][w] bool: a sub-sample of the pixel hits).  Read-only."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.look_at(EYE3, TARGET)
    frame = rt.render(W3, H3)
    hit = rt.visibility(W3, H3, planes=("hit",))["hit"].astype(bool).any(-1)
    assert_frame_has_content(frame, f"teapot {W3}x{H3} at {EYE3}")
    frame.setflags(write=False); hit.setflags(write=False)
    return frame, hit


def at_eye3(rrt, teapot, mode=None, **kw):
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode, **kw)
    rt.look_at(EYE3, TARGET)
    return rt


# ------------------------------------------------------------------ 1: a region is the crop of the frame
@pytest.mark.parametrize("mode", ALL_MODES)
def test_a_region_is_the_crop_of_the_frame(rrt, teapot, frame3, mode):
    frame, hit = frame3
    rt = at_eye3(rrt, teapot, mode)
    assert_same_bits(rt.render(W3, H3), frame, f"walk {mode}: render vs the shared frame", np.uint32)
    assert (frame[0] == 0).all() and (frame[1] == 0).all() and (frame[:, -1] == 0).all(), "the untraced rows and column are not in play"
    for region in REGIONS:
        assert_region_has_content(frame, region, f"walk {mode}", hit)
        assert_same_bits(rt.render_region(W3, H3, region), crop(frame, region), f"walk {mode}: render_region {region} vs the crop of render", np.uint32)
    assert_same_bits(rt.render_region(W3, H3), frame, f"walk {mode}: render_region of no region vs render", np.uint32)


def test_a_region_is_the_crop_of_the_frame_in_the_creation_pose(rrt, teapot):
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = rt.render(W3, H3)
    assert_frame_has_content(frame, f"teapot {W3}x{H3}, creation pose")
    hit = rt.visibility(W3, H3, planes=("hit",))["hit"].astype(bool).any(-1)
    for region in REGIONS:
        assert_region_is_crop(rt, frame, W3, H3, region, "creation pose", hit)


# ------------------------------------------------------------------ 2: pitch, and in place
def test_in_place_and_with_a_pitch(rrt, teapot, frame3):
    torch = pytest.importorskip("torch")
    frame, hit = frame3
    rt = at_eye3(rrt, teapot)
    x0, y0, w, h = IN_PLACE
    assert_region_has_content(frame, IN_PLACE, "in place", hit)
    # in place in a whole frame buffer
    fb = sentinels(torch, W3 * H3)
    rt.render_region_into(fb, W3, H3, region=IN_PLACE, pitch=W3, offset=y0 * W3 + x0)
    torch.cuda.synchronize()
    want = np.full((H3, W3), SENTINEL, np.uint32)
    want[y0:y0 + h, x0:x0 + w] = crop(frame, IN_PLACE)
    assert_same_bits(words(fb).reshape(H3, W3), want, "in place, pitch = the frame's width", np.uint32)
    # rows of 96 with a gap of 19
    pitch = 96
    want = np.full((h, pitch), SENTINEL, np.uint32)
    want[:, :w] = crop(frame, IN_PLACE)
    buf = sentinels(torch, h * pitch)
    rt.render_region_into(buf, W3, H3, region=IN_PLACE, pitch=pitch)
    torch.cuda.synchronize()
    assert_same_bits(words(buf).reshape(h, pitch), want, "device form, pitch 96", np.uint32)
    # the host form, the same rows
    host = np.full((h, pitch), SENTINEL, np.uint32)
    rrt._call("rrt_render_region", rt._h, W3, H3, C.byref(rrt.CRegion(*IN_PLACE)), host.ctypes.data_as(C.POINTER(C.c_uint32)), pitch)
    assert_same_bits(host, want, "host form, pitch 96", np.uint32)
    # a tight device buffer, and a tensor that only just holds the last row
    tight = sentinels(torch, w * h + 3)
    rt.render_region_into(tight, W3, H3, region=IN_PLACE, offset=3)
    torch.cuda.synchronize()
    got = words(tight)
    assert (got[:3] == SENTINEL).all(), "the elements in front of the offset were written"
    assert_same_bits(got[3:].reshape(h, w), crop(frame, IN_PLACE), "tight rows behind an offset of 3", np.uint32)


def test_four_regions_make_the_frame(rrt, teapot, frame3):
    """Four rectangles that partition the frame, in place on one stream: the frame of render, which is also the frame a covered whole frame gives."""
    torch = pytest.importorskip("torch")
    frame, _ = frame3
    cover = np.zeros((H3, W3), int)
    for (x0, y0, w, h) in QUARTERS:
        cover[y0:y0 + h, x0:x0 + w] += 1
    assert (cover == 1).all(), "the four rectangles do not partition the frame"
    rt = at_eye3(rrt, teapot)
    fb = sentinels(torch, W3 * H3)
    stream = torch.cuda.Stream()
    for (x0, y0, w, h) in QUARTERS:
        rt.render_region_into(fb, W3, H3, region=(x0, y0, w, h), pitch=W3, offset=y0 * W3 + x0, stream=stream.cuda_stream)
    stream.synchronize()
    assert_same_bits(words(fb).reshape(H3, W3), frame, "four regions on one stream vs render", np.uint32)
    always = at_eye3(rrt, teapot, coverage="always")
    covered_frame = always.render(W3, H3)
    info = always.coverage_info(count=True)
    print(f"the covered frame: {info}")
    assert info["state"] == "on" and info["n_proved_empty"] > 0, info
    assert_same_bits(words(fb).reshape(H3, W3), covered_frame, "four regions vs a frame with the coverage pass", np.uint32)


# ------------------------------------------------------------------ 3: the other instantiations and depths
def assert_regions_in_forced_walks(rrt, make_rt, what, check=None):
    """Per forced walk: the whole-frame region and (5, 3, 50, 41) of a 64 x 48 frame are crops of render.  Returns the frame."""
    frame = None
    for mode in FORCED_MODES:
        rt = make_rt(mode)
        if check is not None:
            check(rt)
        frame = rt.render(W, H)
        assert_frame_has_content(frame, f"{what}, walk {mode}")
        for region in SMALL_REGIONS:
            assert_region_is_crop(rt, frame, W, H, region, f"{what}, walk {mode}")
        assert rt.last_stats()["filter_variant"] == VARIANT[mode]
    return frame


def test_mirror_room_at_three_depths(rrt, room):
    A, lights, sd, _ = room
    frames = {depth: assert_regions_in_forced_walks(rrt, lambda mode: rrt.RayTracer(sd, lights, max_reflection_depth=depth, box_filter=mode), f"mirror room, depth {depth}")
              for depth in (0, 1, 5)}
    deep = int((frames[5] != frames[0]).sum())
    print(f"mirror room: the depth-5 frame differs from the depth-0 frame on {deep} pixels")
    assert deep >= 64, f"the depth-5 and depth-0 frames differ on {deep} pixels only (< 64)"


def test_a_soup_with_group_records(rrt, teapot_arrays):
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])

    def has_groups(rt):
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records: the kernels' group instantiation did not run"
    assert_regions_in_forced_walks(rrt, lambda mode: rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode), "soup", has_groups)


def test_the_chain_scene(rrt):
    A, _ = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])

    def make(mode):
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), origin=rrt.Vector3d(*eye), box_filter=mode)
        rt.set_camera(**cam)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        return rt
    assert_regions_in_forced_walks(rrt, make, "chain scene")


# ------------------------------------------------------------------ 4: edits
def test_a_region_follows_the_edits(rrt, teapot, teapot_arrays):
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    region = (5, 3, 50, 41)
    seen = [rt.render(W, H)]

    def check(what):
        frame = rt.render(W, H)
        assert_frame_has_content(frame, what)
        changed = int((frame != seen[-1]).sum())
        print(f"{what}: {changed} pixels differ from the frame before the edit")
        assert changed >= 64, f"{what}: the edit changes {changed} pixels only (< 64)"    # (an edit that moves nothing tests nothing; 64 as for the mirror room's depths)
        seen.append(frame)
        assert_region_is_crop(rt, frame, W, H, region, what)
        assert_region_is_crop(rt, frame, W, H, None, what)

    rt.set_camera(**rrt.look_at((4.0, 3.0, -8.0), TARGET))
    check("after set_camera")
    L, V = rrt.Light, rrt.Vector3d
    rt.set_lights([L.Ambient(0.2), L.Point(0.7, V(-7.0, 1.0, -15.0)), L.Directional(0.6, V(3.0, -1.0, 10.0))])
    check("after set_lights")
    mats = [dict(m) for m in teapot_arrays["materials"]]
    for m in mats:
        m["kd"] = (0.3, 0.9, 0.5)
        m["kr"] = 0.25
    rt.set_materials(mats)
    check("after set_materials")
    pos = np.array(teapot_arrays["pos"], np.float64)
    pos[..., 0] += 1.5
    pos[..., 1] *= 0.75
    rt.set_triangles(pos, teapot_arrays["uv"], teapot_arrays["nrm"], teapot_arrays["mat"])
    check("after set_triangles")


# ------------------------------------------------------------------ 5: not a frame
def test_a_region_call_is_not_a_frame(rrt, teapot, frame3):
    frame, _ = frame3
    rt, twin = at_eye3(rrt, teapot), at_eye3(rrt, teapot)
    for region in (IN_PLACE, None):
        got = rt.render_region(W3, H3, region)
        s = rt.last_stats()
        r = region or (0, 0, W3, H3)
        assert_same_bits(got, crop(frame, r), f"before any frame: render_region {r}", np.uint32)
        want = 4 * traced_count(r, W3, H3)
        assert (s["width"], s["height"], s["rays_primary"]) == (W3, H3, want) and s["kernel_ms"] > 0, (s, want)
        assert rt.coverage_info()["state"] == "no_frame", rt.coverage_info()
    assert traced_count((0, 0, W3, H3), W3, H3) == (W3 - 1) * (H3 - 2) and traced_count(IN_PLACE, W3, H3) == 77 * 31
    rt.render_region(W, H)                                                          # another size must not become "the" size either
    for k in (1, 2):
        a, b = rt.render(W3, H3), twin.render(W3, H3)
        va, vb = rt.last_stats()["filter_variant"], twin.last_stats()["filter_variant"]
        assert_same_bits(a, b, f"frame {k} after two region calls vs frame {k} of a raytracer that made none", np.uint32)
        assert_same_bits(a, frame, f"frame {k} vs the shared frame", np.uint32)
        assert va == vb, f"frame {k}: variant {va} after two region calls, {vb} without them"
    # ... and afterwards a region runs the kept variant and leaves the coverage state of the last frame alone
    state = rt.coverage_info()
    rt.render_region(W3, H3, IN_PLACE)
    assert rt.last_stats()["filter_variant"] == va and rt.coverage_info() == state, (rt.last_stats(), rt.coverage_info(), state)


# ------------------------------------------------------------------ 6: the tile list
@pytest.mark.parametrize("mode", FORCED_MODES)
def test_a_tile_list(rrt, teapot, frame3, mode):
    torch = pytest.importorskip("torch")
    frame, _ = frame3
    tx_n, ty_n = tiles_of(W3, H3)
    n_tiles = tx_n * ty_n
    assert (tx_n, ty_n, n_tiles) == (26, 15, 390)
    rt = at_eye3(rrt, teapot, mode)

    def run(tiles, what):
        fb = sentinels(torch, W3 * H3)
        t = torch.from_numpy(np.asarray(tiles, np.uint32).view(np.int32)).cuda()
        rt.render_tile_list_into(fb, t, W3, H3)
        torch.cuda.synchronize()
        s = rt.last_stats()
        if len(tiles):
            assert (s["width"], s["height"], s["rays_primary"], s["filter_variant"]) == (W3, H3, 0, VARIANT[mode]) and s["kernel_ms"] > 0, s
        return assert_listed_tiles_only(words(fb), frame, tiles, f"walk {mode}: {what}")

    every = np.arange(n_tiles, dtype=np.uint32)
    assert run(every, "all tiles in order") == W3 * H3
    assert run(every[::-1].copy(), "all tiles reversed") == W3 * H3
    rng = np.random.default_rng(97)
    edge = np.array([tx_n - 1, 2 * tx_n - 1, n_tiles - 1, n_tiles - tx_n, n_tiles - 3], np.uint32)          # of the last tile column and the last tile row
    inner = np.setdiff1d(every, edge)
    subset = np.concatenate([edge, rng.choice(inner, 97 - len(edge), replace=False).astype(np.uint32)])
    assert len(np.unique(subset)) == 97
    listed = np.concatenate([subset, rng.choice(subset, 10, replace=False), np.array([390, 0xFFFFFFFF, 391, 0x80000000], np.uint32)]).astype(np.uint32)
    rng.shuffle(listed)
    assert len(listed) == 111 and len(np.unique(listed[listed < n_tiles])) == 97
    n_px = run(listed, "97 tiles, 10 of them twice, four ids that name no tile")
    assert 0 < n_px < W3 * H3 and n_px == int(listed_pixels(W3, H3, subset).sum())
    before = rt.last_stats()
    assert run(np.zeros(0, np.uint32), "an empty list") == 0
    assert rt.last_stats() == before, "an empty list changed the statistics"


# ------------------------------------------------------------------ 7: the bound
def test_the_bound_of_a_tile_list(rrt, teapot, frame3):
    torch = pytest.importorskip("torch")
    frame, _ = frame3
    tx_n, ty_n = tiles_of(W3, H3)
    rng = np.random.default_rng(64)
    tiles = rng.choice(tx_n * ty_n, 64, replace=False).astype(np.uint32)
    rt = at_eye3(rrt, teapot)
    t = torch.from_numpy(tiles.view(np.int32)).cuda()
    for bound in (0, 1, 63, 64, 65, 2 ** 32 - 1):
        fb = sentinels(torch, W3 * H3)
        b = torch.from_numpy(np.array([bound], np.uint32).view(np.int32)).cuda()
        rt.render_tile_list_into(fb, t, W3, H3, bound_t=b)
        torch.cuda.synchronize()
        m = min(64, bound)
        n_px = assert_listed_tiles_only(words(fb), frame, tiles[:m], f"bound {bound}: the tiles of [0, {m}) and nothing else")
        assert (n_px == 0) == (m == 0)
        assert words(b)[0] == bound and (words(t) == tiles).all(), "the bound or the list was written"
    # the bound written on the stream just before the call
    stream = torch.cuda.Stream()
    fb = sentinels(torch, W3 * H3)
    b = torch.zeros(1, dtype=torch.int32, device="cuda")
    flags = torch.zeros(64, dtype=torch.int32, device="cuda")
    flags[:23] = 1
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        b.copy_(flags.sum().to(torch.int32).reshape(1))
        rt.render_tile_list_into(fb, t, W3, H3, stream=stream.cuda_stream, bound_t=b)
    stream.synchronize()
    assert words(b)[0] == 23
    assert assert_listed_tiles_only(words(fb), frame, tiles[:23], "a bound of 23 written by a torch op on the same stream") > 0


# ------------------------------------------------------------------ 8: against the oracle, once
def test_the_whole_frame_region_against_the_oracle(rrt, room):
    A, lights, sd, osc = room
    ref, hit, _ = oracle_frame(osc, A, CREATION, W, H)
    assert_frame_has_content(ref, "the oracle's mirror room")
    assert hit.mean() >= 0.5, f"{hit.mean():.3f} of the oracle's rays hit (< 0.5)"
    rt = rrt.RayTracer(sd, lights)
    assert_frame_close(rt.render_region(W, H), ref, "mirror room: render_region of the whole frame vs the oracle")
