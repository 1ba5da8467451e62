"""Ambient occlusion for arbitrary ray records, with a rotation per record (include/rrt.h: rrt_ambient_rays, rrt_ambient_rays_device) on the GPU.

The statement under test: bit k of `occluded` of a record that holds a hit IS what rrt_occluded_rays returns for the ray the contract defines -- origin = point +
normal * surface_offset, direction = (tg*rx + bt*ry) + n*sz in the reference's tangent frame with (rx, ry) the sample's (sx, sy) turned by the record's (c, s), the
call's max_t -- bit for bit, in every traversal variant; `open` is n - popcount of it, and n for a miss.  The rays are restated in numpy from the arrays of
rt.surface_rays() (ambient_rays_checks.py).  Every comparison asserts its conditions BY THE REFERENCE ANSWERS, so an empty result cannot pass.

The oracle, run on the CPU with T8 and max_t 2.0, gave for the record sets of parts 1 and 2 (without rotation / with ROT):
  teapot, creation pose, level 1 of all level-0 hits of the 64x48 frame: 7142 records, 3320 hits (0.465), occluded fraction 0.205 / 0.250, per sample
      0.176-0.270 / 0.187-0.386 occluded, no fallback hit, the masks of 0.611 of the hits differ between the two (at max_t +inf: 0.279 / 0.314, per sample
      0.199-0.380 / 0.247-0.442, 0.524 differ);
  mirror room, level 1 of the 32x24 frame: 2944 records, 2913 hits, 512 of them in the length(tg) == 0 branch, occluded fraction 0.222 / 0.218.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T, popcount
from ambient_rays_checks import INPUTS, OUTPUTS, Fan, by_oracle, by_shadow_query, kept_records as kept, level1, mask_figures, open_of, rows, standard_rot  # noqa: F401  (fixtures: kept)
from bitwise import assert_same_arrays, assert_same_bits
from compact_checks import G
from gpu_checks import ALL_MODES, CHAIN_LIGHTS, FORCED_MODES, ORIGIN, chain_rrt_lights, chain_scene, oracle_for
from scenes import CREATION, rays_of, teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import MIRROR_ROOM_LIGHTS, mirror_room, soup_scene
from surface_checks import NO_MATERIAL

pytestmark = pytest.mark.gpu

INF = float("inf")
W, H = 64, 48
RW, RH = 32, 24                                                  # the mirror room's, the soup's and the chain scene's frame
SENTINEL = -1515870811                                           # 0xA5A5A5A5 as int32
PATTERN = 0xA5A5A5A5


def assert_ambient_is_the_shadow_query(rt, rec, fan, rot, max_t, what, dirs=T8):
    """Both outputs of rt.ambient_rays against rt.occluded on the restated rays, bit for bit, and `open` by its rule.  Returns the reference mask."""
    want = by_shadow_query(rt, fan, max_t)
    hits = int(fan.hit.sum())
    assert hits > 0 and (want != 0).any() and (popcount(want[fan.hit]) < fan.n).any(), f"{what}: the reference masks are all empty or all full"
    got = rt.ambient_rays(rec, dirs, max_t, rot=rot)
    stats = rt.last_stats()
    assert_same_bits(got["occluded"], want, f"{what}: occluded vs rrt_occluded_rays")
    assert_same_bits(got["open"], open_of(want, fan.hit, fan.n), f"{what}: open vs n - popcount on hits and n on misses")
    assert (stats["width"], stats["height"], stats["rays_primary"]) == (len(want), 1, len(want)) and stats["kernel_ms"] > 0, (what, stats)
    return want


def device_records(torch, rec):
    return {n: torch.tensor(np.ascontiguousarray(rec[n]).view(np.int32 if rec[n].dtype == np.uint32 else rec[n].dtype), device="cuda").reshape(-1) for n in INPUTS}


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("max_t", (T8_MAX_T, INF))
def test_the_mask_is_the_shadow_query_at_level_1(rrt, ob, teapot, teapot_arrays, kept, max_t):
    rec, rot, fans = kept["rec"], kept["rot"], kept["fans"]
    hit = fans[False].hit
    print(f"teapot level 1: {len(hit)} records, {int(hit.sum())} hits ({hit.mean():.3f}), {int(fans[False].fallback.sum())} fallback hits")
    assert hit.mean() >= 0.40 and not hit.all(), f"hit fraction {hit.mean():.3f}: want at least 0.40 and some miss"
    for mode in ALL_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        _, again = level1(rt, CREATION, W, H)
        assert_same_arrays(again, rec, INPUTS, f"walk {mode}: the records the rays were formed from")
        want = {}
        for r in (False, True):
            what = f"teapot level 1, walk {mode}, max_t {max_t}, {'ROT' if r else 'no rot'}"
            want[r] = assert_ambient_is_the_shadow_query(rt, rec, fans[r], rot if r else None, max_t, what)
            frac, per = mask_figures(want[r], fans[r])
            print(f"{what}, by rrt_occluded_rays: occluded fraction {frac:.3f}, per sample {per.min():.3f}-{per.max():.3f}")
            assert frac >= 0.15, f"{what}: occluded fraction {frac:.3f} (< 0.15)"
            assert per.min() >= 0.10, f"{what}: per sample {per.tolist()}: want each occluded on >= 10 % of the hits"
            assert (1.0 - per).min() >= 0.50, f"{what}: per sample {per.tolist()}: want each open on >= 50 % of the hits"
        moved = float((want[True][hit] != want[False][hit]).mean())
        print(f"walk {mode}, max_t {max_t}: ROT changes the mask of {moved:.3f} of the hit records")
        assert moved >= 0.40, f"walk {mode}: ROT changes the mask of {moved:.3f} of the hit records (< 0.40): the rotation shows nothing"
        if mode == "lane" and max_t == T8_MAX_T:
            ref = by_oracle(oracle_for(ob, teapot_arrays, rrt.default_lights()), fans[True], max_t)
            frac, per = mask_figures(ref, fans[True])
            print(f"by the oracle, ROT: occluded fraction {frac:.3f}, per sample {per.min():.3f}-{per.max():.3f}")
            assert frac >= 0.15 and per.min() >= 0.10 and (1.0 - per).min() >= 0.50, (frac, per.tolist())
            assert_same_bits(want[True], ref, f"walk {mode}, max_t {max_t}, ROT: rrt_occluded_rays (= occluded) vs the oracle's intersector")


# ------------------------------------------------------------------ 2
def test_the_fallback_branch_of_the_tangent_frame(rrt, ob):
    A = mirror_room()
    lights = [rrt.Light(k, i, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS]
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    n_mats = len(A["materials"])
    rec = None
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(sd, lights, box_filter=mode)
        _, again = level1(rt, CREATION, RW, RH)
        if rec is None:
            rec = again
            rot = standard_rot(len(rec["material"]))
            fans = {False: Fan(rec, n_mats, T8), True: Fan(rec, n_mats, T8, rot)}
            n_fb = int(fans[False].fallback.sum())
            print(f"mirror room level 1: {len(fans[False].hit)} records, {int(fans[False].hit.sum())} hits, {n_fb} in the length(tg) == 0 branch")
            assert n_fb >= 400, f"{n_fb} hits take the length(tg) == 0 branch (< 400)"
        assert_same_arrays(again, rec, INPUTS, f"mirror room, walk {mode}: the records the rays were formed from")
        for r in (False, True):
            what = f"mirror room level 1, walk {mode}, {'ROT' if r else 'no rot'}"
            want = assert_ambient_is_the_shadow_query(rt, rec, fans[r], rot if r else None, T8_MAX_T, what)
            frac, per = mask_figures(want, fans[r])
            print(f"{what}: occluded fraction {frac:.3f}, per sample {per.min():.3f}-{per.max():.3f}")
            assert frac >= 0.15, f"{what}: occluded fraction {frac:.3f} (< 0.15)"
            fb = np.zeros(len(want), bool)
            fb[fans[r].hit] = fans[r].fallback
            assert (want[fb] != 0).any() and (popcount(want[fb]) < 8).any(), f"{what}: the fallback hits' masks are all empty or all full"
            if mode == "lane" and r:
                assert_same_bits(want, by_oracle(oracle_for(ob, A, lights), fans[r], T8_MAX_T), f"{what}: rrt_occluded_rays (= occluded) vs the oracle's intersector")


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("bump", (True, False), ids=["as loaded", "bump maps off"])
def test_the_planes_of_a_frame_are_records(rrt, teapot, teapot_arrays, bump):
    A = teapot_arrays
    sd = teapot
    if not bump:
        flat = copy.deepcopy(A["materials"])
        assert sum(m["bump"] >= 0 for m in flat) >= 1
        for m in flat:
            m["bump"] = -1
        sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], flat, A["textures"])
    rt = rrt.RayTracer(sd, rrt.default_lights())
    planes = rt.surface(W, H, planes=INPUTS)
    frame = rt.ambient(W, H, planes, T8, T8_MAX_T, outputs=("occluded",))["occluded"]
    rec = {n: planes[n].reshape((-1, 3) if n != "material" else (-1,)) for n in INPUTS}
    fan = Fan(rec, len(A["materials"]), T8)
    n_set = int((frame != 0).sum())
    print(f"frame planes as records: {len(fan.hit)} records, {int(fan.hit.sum())} hits, {int(fan.fallback.sum())} fallback hits, {n_set} masks with a bit set")
    assert fan.hit.mean() >= 0.5 and n_set >= 1000, (fan.hit.mean(), n_set)
    if not bump:
        assert fan.fallback.sum() >= 1000, f"{int(fan.fallback.sum())} hits take the length(tg) == 0 branch (< 1000)"
    assert (planes["material"][0] == NO_MATERIAL).all(), "row 0 of the frame is never traced: its records are misses"
    got = rt.ambient_rays(rec, T8, T8_MAX_T)
    assert_same_bits(got["occluded"], frame.reshape(-1), "occluded of the flattened planes vs the occluded plane of rt.ambient")
    assert_same_bits(got["open"], open_of(frame.reshape(-1), fan.hit, 8), "open of the flattened planes")
    assert (got["occluded"][:4 * W] == 0).all() and (got["open"][:4 * W] == 8).all(), "the records of pixels the reference never traces: mask 0, open n"


# ------------------------------------------------------------------ 4
def test_sample_counts(kept):
    rt, rec, rot = kept["rt"], kept["rec"], kept["rot"]
    for r in (False, True):
        want, hit = kept["want"][r], kept["fans"][r].hit
        assert (want >> np.uint32(7)).any(), "sample 7 is never occluded: bit 31 would show nothing"
        assert (want & np.uint32(1)).any() and not (want[hit] & np.uint32(1)).all()
        one = rt.ambient_rays(rec, T8[:1], T8_MAX_T, rot=rot if r else None)
        assert_same_bits(one["occluded"], want & np.uint32(1), f"n = 1, rot {r}: bit 0 of the mask of T8")
        assert_same_bits(one["open"], open_of(want & np.uint32(1), hit, 1), f"n = 1, rot {r}: open")
        full = rt.ambient_rays(rec, np.tile(T8, (4, 1)), T8_MAX_T, rot=rot if r else None)
        assert_same_bits(full["occluded"], want * np.uint32(0x01010101), f"n = 32, T8 four times, rot {r}: the mask of T8 in every byte")
        assert_same_bits(full["open"], np.where(hit, 4 * open_of(want, hit, 8), 32).astype(np.uint32), f"n = 32, rot {r}: open is 4 x T8's")


# ------------------------------------------------------------------ 5
def test_edges_of_the_batch(rrt, teapot, kept):
    rec, rot, n_mats = kept["rec"], kept["rot"], kept["n_mats"]
    want, hit = kept["want"][True], kept["fans"][True].hit
    busy = hit & (want != 0)
    first = int(np.flatnonzero(busy)[0])
    misses, shadowed = np.flatnonzero(~hit), np.flatnonzero(busy)
    assert len(misses) >= 64 and len(shadowed) >= 64
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        whole = rt.ambient_rays(rec, T8, T8_MAX_T, rot=rot)
        assert_same_bits(whole["occluded"], want, f"walk {mode}: the whole batch")
        for n in (1, 63, 64, 65, 129):
            for start in (first, len(hit) - n):
                sl = slice(start, start + n)
                n_hit, n_bits = int(hit[sl].sum()), int(popcount(want[sl]).sum())
                assert start != first or (n_hit >= 1 and n_bits >= 1), f"{n} records from {start}: {n_hit} hits, {n_bits} occluded rays by the reference"
                part = rt.ambient_rays(rows(rec, sl), T8, T8_MAX_T, rot=rot[sl])
                stats = rt.last_stats()
                assert (stats["width"], stats["height"], stats["rays_primary"]) == (n, 1, n), stats
                for name in OUTPUTS:
                    assert_same_bits(part[name], whole[name][sl], f"walk {mode}: {n} records from {start}: {name} is not the batch's slice")
        # 64 misses, then one hit: the first wave walks nothing.  63 misses and a hit in lane 63.  Both with a hit whose reference mask has a bit set.
        for what, idx in (("64 misses, then one hit", np.concatenate([misses[:64], shadowed[5:6]])), ("a wave whose only hit is lane 63", np.concatenate([misses[:63], shadowed[7:8]]))):
            got = rt.ambient_rays(rows(rec, idx), T8, T8_MAX_T, rot=rot[idx])
            assert want[idx][-1] != 0 and (want[idx][:-1] == 0).all()
            assert_same_bits(got["occluded"], want[idx], f"walk {mode}: {what}: occluded")
            assert_same_bits(got["open"], open_of(want[idx], hit[idx], 8), f"walk {mode}: {what}: open")
        # material == n_mats and 0xFFFFFFFF in records that were hits: mask 0, open n, nothing else moves
        edited = {k: rec[k].copy() for k in INPUTS}
        a, b = shadowed[0:len(shadowed):3], shadowed[1:len(shadowed):3]
        edited["material"][a] = n_mats
        edited["material"][b] = NO_MATERIAL
        want_edit = want.copy()
        want_edit[a] = 0
        want_edit[b] = 0
        gone = hit.copy()
        gone[a] = False
        gone[b] = False
        got = rt.ambient_rays(edited, T8, T8_MAX_T, rot=rot)
        assert_same_bits(got["occluded"], want_edit, f"walk {mode}: material = n_mats and 0xFFFFFFFF in hit records: occluded")
        assert_same_bits(got["open"], open_of(want_edit, gone, 8), f"walk {mode}: material = n_mats and 0xFFFFFFFF in hit records: open")
        assert (got["open"][a] == 8).all() and (got["open"][b] == 8).all() and (want_edit != 0).sum() >= 100
        # n == 0: RRT_OK, nothing enqueued, the statistics stay
        stats = rt.last_stats()
        empty = rt.ambient_rays(rows(rec, slice(0, 0)), T8, T8_MAX_T, rot=rot[:0])
        assert set(empty) == set(OUTPUTS) and all(len(x) == 0 for x in empty.values())
        assert rt.last_stats() == stats, "n = 0 changed the statistics"


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_the_device_form(rrt, teapot, kept, mode):
    torch = pytest.importorskip("torch")
    rec, rot = kept["rec"], kept["rot"]
    n = len(rec["material"])
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    stream = torch.cuda.Stream()
    tensors = device_records(torch, rec)
    occluded = torch.full((G + n + G,), SENTINEL, dtype=torch.int32, device="cuda")
    open_ = torch.full((G + n + G,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for r in (True, False):
        want, hit = kept["want"][r], kept["fans"][r].hit
        occluded.fill_(SENTINEL); open_.fill_(SENTINEL)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):                           # the rotations go up on the stream the call is enqueued on
            rot_t = torch.tensor(rot, device="cuda").reshape(-1) if r else None
            rt.ambient_rays_into(dict(occluded=occluded[G:-G], open=open_[G:-G]), tensors, T8, T8_MAX_T, rot_t=rot_t, stream=stream.cuda_stream)
        stream.synchronize()
        stats = rt.last_stats()
        for name, t, ref in (("occluded", occluded, want), ("open", open_, open_of(want, hit, 8))):
            a = t.cpu().numpy()
            assert (a[:G] == SENTINEL).all() and (a[-G:] == SENTINEL).all(), f"{name}: an element outside the output was written"
            assert_same_bits(a[G:-G].view(np.uint32), ref, f"walk {mode}, rot {r}: {name} of the device form")
        assert (stats["width"], stats["height"], stats["rays_primary"]) == (n, 1, n), stats
        assert stats["filter_variant"] == rrt.VARIANT_NAMES.index(mode) and stats["kernel_ms"] > 0, stats
    # one output only: the other tensor is not touched
    want, hit = kept["want"][False], kept["fans"][False].hit
    for asked, other in (("open", "occluded"), ("occluded", "open")):
        out = dict(occluded=occluded, open=open_)
        occluded.fill_(SENTINEL); open_.fill_(SENTINEL)
        torch.cuda.synchronize()
        rt.ambient_rays_into({asked: out[asked][G:-G]}, tensors, T8, T8_MAX_T, stream=stream.cuda_stream)
        stream.synchronize()
        assert (out[other].cpu().numpy() == SENTINEL).all(), f"{asked} alone: {other} was written"
        ref = want if asked == "occluded" else open_of(want, hit, 8)
        assert_same_bits(out[asked].cpu().numpy()[G:-G].view(np.uint32), ref, f"walk {mode}: {asked} alone, device form")
        one = rt.ambient_rays(rec, T8, T8_MAX_T, outputs=(asked,))                  # the host form with ONE output asked for and the other NULL, against the device form's
        assert set(one) == {asked}
        assert_same_bits(one[asked], out[asked].cpu().numpy()[G:-G].view(np.uint32), f"walk {mode}: {asked} alone, host form vs device form")


# ------------------------------------------------------------------ 6
def assert_walks(make_rt, cam, n_mats, what, modes):
    """Level-0 records of the 32x24 frame in the pose `cam`, with ROT, in every (mode, options) of `modes`; yields the raytracers."""
    rec = None
    for mode, kw in modes:
        rt = make_rt(mode, kw)
        O, D = rays_of(cam, RW, RH)
        again = rt.surface_rays(O, D, planes=INPUTS)
        if rec is None:
            rec = again
            rot = standard_rot(len(rec["material"]))
            fan = Fan(rec, n_mats, T8, rot)
        assert_same_arrays(again, rec, INPUTS, f"{what}, walk {mode} {kw}: the records the rays were formed from")
        want = assert_ambient_is_the_shadow_query(rt, rec, fan, rot, T8_MAX_T, f"{what}, walk {mode} {kw}")
        n_bits = int(popcount(want).sum())
        print(f"{what}, walk {mode} {kw}: {int(fan.hit.sum())} hits, {n_bits} of {int(fan.hit.sum()) * 8} rays occluded by rrt_occluded_rays")
        assert 100 <= n_bits < int(fan.hit.sum()) * 8, f"{what}, walk {mode}: {n_bits} occluded rays by the reference"
        yield rt


def test_a_soup_with_long_own_lists(rrt, teapot_arrays):
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    make = lambda mode, kw: rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, **kw)
    modes = [(m, {}) for m in FORCED_MODES] + [(None, dict(no_cull=True))]
    for rt, (mode, kw) in zip(assert_walks(make, CREATION, len(A["materials"]), "soup", modes), modes):
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert len(supers) > 0
        if not kw:
            assert (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records (clusters.cpp): the group handling of the walk did not run"


def test_the_chain_shortcut_scene(rrt):
    A, names = chain_scene("main")
    assert "big" in names
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])

    def make(mode, kw):
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*eye), box_filter=mode, **kw)
        rt.set_camera(**cam)
        assert kw.get("no_cull") or rt.chain_info["n_chains"] >= 1, rt.chain_info      # (without the index the shortcut cannot apply: rrt.h)
        return rt
    assert len(CHAIN_LIGHTS) == 3
    modes = [(m, {}) for m in FORCED_MODES] + [(None, dict(no_cull=True))] + [(m, dict(chain_shortcut=False)) for m in FORCED_MODES]
    for _ in assert_walks(make, cam, len(A["materials"]), "chain scene", modes):
        pass


# ------------------------------------------------------------------ 7
def test_the_chain_from_library_calls_alone_on_the_device(rrt, teapot, kept):
    """surface_rays_into -> surface_rays_into on the next rays -> ambient_rays_into, on a stream of the test's own; nothing leaves the device until the masks do.
    The batch keeps its size: a ray whose level-0 ray missed is a dead ray (max_t = 0.0) at level 1, and a dead record for the ambient call."""
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    O, D = rays_of(CREATION, W, H)
    n = len(D)
    h0 = kept["l0"]["hit"].astype(bool)
    rot_full = np.zeros((n, 2))
    rot_full[h0] = kept["rot"]
    stream = torch.cuda.Stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    with torch.cuda.stream(stream):
        o_t, d_t, rot_t = (torch.tensor(a, device="cuda").reshape(-1) for a in (O, D, rot_full))
        l0 = dict(hit=torch.empty(n, dtype=torch.uint8, device="cuda"), next_origin=torch.empty(3 * n, **f64), next_dir=torch.empty(3 * n, **f64))
        rt.surface_rays_into(o_t, d_t, l0, stream=stream.cuda_stream)
        alive = torch.where(l0["hit"] != 0, torch.full((n,), INF, **f64), torch.zeros(n, **f64))
        rec = dict(point=torch.empty(3 * n, **f64), normal=torch.empty(3 * n, **f64), material=torch.empty(n, dtype=torch.int32, device="cuda"))
        rt.surface_rays_into(l0["next_origin"], l0["next_dir"], rec, max_t_t=alive, stream=stream.cuda_stream)
        out = {name: torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for name in OUTPUTS}
        rt.ambient_rays_into(out, rec, T8, T8_MAX_T, rot_t=rot_t, stream=stream.cuda_stream)
    stream.synchronize()
    got = {name: t.cpu().numpy().view(np.uint32) for name, t in out.items()}
    assert np.array_equal(l0["hit"].cpu().numpy().astype(bool), h0)
    want, hit1 = kept["want"][True], kept["fans"][True].hit
    assert_same_bits(got["occluded"][h0], want, "the chain on the device, with ROT: occluded of the level-0 hits vs the host forms'")
    assert_same_bits(got["open"][h0], open_of(want, hit1, 8), "the chain on the device, with ROT: open of the level-0 hits")
    assert (~h0).sum() >= 1000 and (got["occluded"][~h0] == 0).all() and (got["open"][~h0] == 8).all(), "a dead record: mask 0, open n"


# ------------------------------------------------------------------ 8
def test_refusals_leave_the_outputs_as_they_were(rrt, teapot, kept):
    rec, rot = kept["rec"], kept["rot"]
    n = 200
    first = int(np.flatnonzero(kept["fans"][True].hit & (kept["want"][True] != 0))[0])
    sl = slice(first, first + n)
    part, prot = rows(rec, sl), np.ascontiguousarray(rot[sl])
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    L = rrt.lib()
    occluded, open_ = np.full(n, PATTERN, np.uint32), np.full(n, PATTERN, np.uint32)
    dirs = np.ascontiguousarray(T8)
    cs = rrt.CRaySurface(**{k: part[k].ctypes.data for k in INPUTS})

    def samples(d=dirs, k=8, max_t=T8_MAX_T):
        return rrt.CAmbientSamples(dirs=None if d is None else d.ctypes.data_as(C.POINTER(C.c_double)), n=k, max_t=max_t)

    def out(o=occluded, g=open_):
        return rrt.CRayAmbient(occluded=None if o is None else o.ctypes.data, open=None if g is None else g.ctypes.data)

    def raw(rec_p, samples_p, out_p, count=n, handle=None):
        status = L.rrt_ambient_rays(rt._h if handle is None else handle[0], count, rec_p, prot.ctypes.data_as(rrt._dp), samples_p, out_p)
        if status != rrt.OK:
            raise rrt.RrtError(status, "rrt_ambient_rays", (L.rrt_last_error_detail() or b"").decode())

    def bad_dir(value):
        d = dirs.copy()
        d[5, 1] = value
        return d
    nan_dirs, inf_dirs, many = bad_dir(np.nan), bad_dir(-np.inf), np.ascontiguousarray(np.tile(dirs, (5, 1)))   # (kept alive here: the structs only point at them)

    def without_array(name):
        return rrt.CRaySurface(**{k: part[k].ctypes.data for k in INPUTS if k != name})

    calls = [("a NULL raytracer", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), handle=(None,))),
             ("a NULL record struct", lambda: raw(None, C.byref(samples()), C.byref(out()))),
             ("a NULL samples struct", lambda: raw(C.byref(cs), None, C.byref(out()))),
             ("a NULL output struct", lambda: raw(C.byref(cs), C.byref(samples()), None)),
             ("a NULL record struct with n == 0", lambda: raw(None, C.byref(samples()), C.byref(out()), count=0))]
    calls += [(f"array {name} missing", (lambda name=name: raw(C.byref(without_array(name)), C.byref(samples()), C.byref(out())))) for name in INPUTS]
    tables = [("n_samples 0", samples(k=0)), ("n_samples 33", samples(d=many, k=33)), ("NULL dirs", samples(d=None)), ("a NaN direction component", samples(d=nan_dirs)),
              ("an infinite direction component", samples(d=inf_dirs)), ("max_t NaN", samples(max_t=np.nan)), ("max_t 0", samples(max_t=0.0)),
              ("max_t -1", samples(max_t=-1.0)), ("max_t -inf", samples(max_t=-np.inf))]
    calls += [("both outputs NULL", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out(None, None))))]
    calls += [(what, (lambda s=s: raw(C.byref(cs), C.byref(s), C.byref(out())))) for what, s in tables]
    calls += [(f"{what}, with n == 0", (lambda s=s: raw(C.byref(cs), C.byref(s), C.byref(out()), count=0))) for what, s in tables]
    calls += [("the Python form, 33 directions", lambda: rt.ambient_rays(part, many[:33], T8_MAX_T, rot=prot)),
              ("the Python form, no output", lambda: rt.ambient_rays(part, dirs, T8_MAX_T, rot=prot, outputs=()))]
    stats = rt.last_stats()
    for what, call in calls:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert (L.rrt_last_error_detail() or b"") != b"", what
        assert (occluded == PATTERN).all() and (open_ == PATTERN).all(), f"{what}: an output of a refused call was written"
        assert rt.last_stats() == stats, f"{what}: the statistics changed"
    raw(C.byref(cs), C.byref(samples()), C.byref(out()), count=0)                  # n == 0 with valid structs: RRT_OK, nothing written
    assert (occluded == PATTERN).all() and (open_ == PATTERN).all() and rt.last_stats() == stats
    raw(C.byref(cs), C.byref(samples(max_t=INF)), C.byref(out()))                  # +inf is a valid max_t
    assert not (occluded == PATTERN).any() and not (open_ == PATTERN).any(), "an accepted call leaves elements of its outputs unwritten"
    assert ((open_ <= 8) & (occluded < 256)).all()
    raw(C.byref(cs), C.byref(samples()), C.byref(out()))
    assert_same_bits(occluded, kept["want"][True][sl], "after the refusals: occluded")
    assert_same_bits(open_, open_of(kept["want"][True][sl], kept["fans"][True].hit[sl], 8), "after the refusals: open")


# ------------------------------------------------------------------ 9
def test_state_is_untouched(rrt, teapot, kept):
    """An ambient_rays call is neither a frame nor a measured batch: the variant kept for a frame size, the variant kept for per-ray calls and the frames stay."""
    torch = pytest.importorskip("torch")
    rec, rot, want = kept["rec"], kept["rot"], kept["want"][True]
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = [rt.render(W, H) for _ in range(2)][-1]                                # (twice: the size's variant is measured)
    variant = rt.last_stats()["filter_variant"]
    O, D = rays_of(CREATION, W, H)
    rt.intersect_rays(O[:64], D[:64])
    small_variant = rt.last_stats()["filter_variant"]
    # a batch large enough for the other host forms to measure on runs in the variant small batches run, and measures nothing
    reps = 4
    assert reps * len(want) >= 16384
    big = rt.ambient_rays({k: np.tile(rec[k], (reps,) + (1,) * (rec[k].ndim - 1)) for k in INPUTS}, T8, T8_MAX_T, rot=np.tile(rot, (reps, 1)), outputs=("occluded",))
    stats = rt.last_stats()
    assert (stats["width"], stats["filter_variant"]) == (reps * len(want), small_variant), stats
    assert_same_bits(big["occluded"], np.tile(want, reps), "the batch four times over")
    rt.intersect_rays(O[:64], D[:64])
    assert rt.last_stats()["filter_variant"] == small_variant, "an ambient_rays call of 28568 records kept a per-ray variant"
    assert np.array_equal(rt.render(W, H), frame) and rt.last_stats()["filter_variant"] == variant
    # the variant rrt_tune_rays_device keeps: run by the call, and left alone by it
    o_t, d_t = torch.tensor(O, device="cuda").reshape(-1), torch.tensor(D, device="cuda").reshape(-1)
    tuned = rt.tune_rays(o_t, d_t)
    for form in ("host", "device"):
        if form == "host":
            got = rt.ambient_rays(rec, T8, T8_MAX_T, rot=rot, outputs=("occluded",))["occluded"]
        else:
            out = torch.full((len(want),), SENTINEL, dtype=torch.int32, device="cuda")
            rt.ambient_rays_into({"occluded": out}, device_records(torch, rec), T8, T8_MAX_T, rot_t=torch.tensor(rot, device="cuda").reshape(-1))
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
        assert rt.last_stats()["filter_variant"] == tuned, (form, rt.last_stats(), tuned)
        assert_same_bits(got, want, f"the {form} form in the tuned variant")
    rt.intersect_rays(O[:64], D[:64])
    assert rt.last_stats()["filter_variant"] == tuned, "the variant kept by tune_rays changed"
    assert np.array_equal(rt.render(W, H), frame) and rt.last_stats()["filter_variant"] == variant, "the next frame, or its variant, differs"
