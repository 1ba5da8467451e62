"""Stable compaction of ray batches and records on the device, and its inverse (include/rrt.h: rrt_compact_rays[_device], rrt_scatter_rays[_device]) on the GPU.

The statement under test: the result is the contract's stable partition -- count, index, the survivors gathered byte for byte, the tail filled with the dead
values -- as compact_checks.py restates it in numpy, and a batch compacted this way, KEPT AT ITS LENGTH n, feeds rrt_surface_rays_device and
rrt_ambient_rays_device unchanged: what they give for the padded batch, scattered back, is what they give for the original one.  Every comparison is byte for byte
(doubles through their integer bits); every part asserts by the model that its record set has both survivors and dead entries.

A count / place block of csrc/compact.hip covers a tile of 1024 entries and the one scan block takes 256 tile counts per pass: BIG below has 1029 tiles, so its
scan makes five passes with a carry, the last one partly filled.
"""
import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T
from ambient_rays_checks import INPUTS, OUTPUTS, Fan, by_shadow_query, kept_records as kept, level1, open_of, standard_rot  # noqa: F401  (fixtures: kept)
from bitwise import assert_same_bits, bits
from compact_checks import (ARRAYS, DEAD_INDEX, ELEM_BYTES, NAMES, RECORD_NAMES, Guarded, assert_compacted, ceil_div, compacted, dead, flag_patterns, mixed_waves,
                            scattered, selection, to_device)
from gpu_checks import FORCED_MODES, chain_rrt_lights, chain_scene
from ray_surface_checks import kr_of
from scenes import CREATION, rays_of, teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import MIRROR_ROOM_LIGHTS, mirror_room, soup_scene

pytestmark = pytest.mark.gpu

W, H = 64, 48
RW, RH = 32, 24

TILE, SCAN = 1024, 256                                           # csrc/device_scene.hpp: kCompactTile; csrc/compact.hip: kScanBlock
BIG = 2 ** 20 + 4097                                             # 1029 tiles: five passes of the scan block
EDGE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 4097, 70001, BIG)


def device_compact(torch, rt, n, select, src, out_names, stream, flag=None, index=True, count=True):
    """rt.compact_rays_into of the host arrays `src` ({name: array}; flag: uint8 [n]) into guarded outputs on `stream`: {"index", "count", name: array}."""
    src_t = {name: to_device(torch, a) for name, a in src.items()}
    flag_t = None if flag is None else to_device(torch, flag)
    out = {name: Guarded(torch, ARRAYS[name][0], ARRAYS[name][1] * n) for name in out_names}
    index_g, count_g = (Guarded(torch, np.uint32, n) if index else None), (Guarded(torch, np.uint32, 1) if count else None)
    scratch = Guarded(torch, np.uint8, rt.compact_scratch_bytes(n))
    torch.cuda.synchronize()
    rt.compact_rays_into({name: g.t for name, g in out.items()}, src_t, select, index_g and index_g.t, count_g and count_g.t, scratch.t, flag_t=flag_t,
                         stream=stream.cuda_stream)
    stream.synchronize()
    scratch.read("scratch")
    got = {name: g.read(name).reshape((n, ARRAYS[name][1]) if ARRAYS[name][1] > 1 else (n,)) for name, g in out.items()}
    if index:
        got["index"] = index_g.read("index")
    if count:
        got["count"] = int(count_g.read("count")[0])
    return got


# ------------------------------------------------------------------ 1
def test_hit_on_the_level_0_records_of_the_teapot(rrt, teapot, teapot_arrays):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    O, D = rays_of(CREATION, W, H)
    n = len(D)
    max_t = np.linspace(50.0, 60.0, n)
    src = dict(origins=O, dirs=D, max_t=max_t, rot=standard_rot(n), **rt.surface_rays(O, D, max_t))
    assert tuple(src) == NAMES
    sel = selection("hit", n_mats=len(teapot_arrays["materials"]), material=src["material"])
    want = compacted(sel, src)
    print(f"teapot level 0: {n} records, {want['count']} hits, {mixed_waves(sel)} waves with hits and misses")
    assert 0 < want["count"] < n and np.array_equal(sel, src["hit"].astype(bool)) and mixed_waves(sel) >= 10
    assert_compacted(rt.compact_rays({k: src[k] for k in RECORD_NAMES}, "hit", origins=O, dirs=D, max_t=max_t, rot=src["rot"]), want, "the host form")
    stats = rt.last_stats()
    assert_compacted(device_compact(torch, rt, n, "hit", src, NAMES, torch.cuda.Stream()), want, "the device form on a stream of its own")
    assert rt.last_stats() == stats, "the device form changed the statistics"


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_edges_of_the_flag_mode(rrt, teapot, n):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    stream = torch.cuda.Stream()
    assert n != BIG or ceil_div(ceil_div(n, TILE), SCAN) == 5, "BIG is meant to take five passes of the scan block"
    rng = np.random.default_rng(n)
    point = rng.standard_normal((n, 3))
    tri = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for what, flag in flag_patterns(n).items():
        want = compacted(flag != 0, {})
        assert want["count"] == {"all 0": 0, "all 1": n, "alternating": n // 2, "only the first": 1, "only the last": 1}.get(what, want["count"])
        assert_compacted(device_compact(torch, rt, n, "flag", {}, (), stream, flag=flag), want, f"n = {n}, {what}: index and count alone, the device form")
        if n <= 4097:
            got = rt.compact_rays(dict(point=point, tri=tri), "flag", flag=flag)
            assert_compacted(got, compacted(flag != 0, dict(point=point, tri=tri)), f"n = {n}, {what}: point and tri gathered, the host form")
    if n <= 4097:                                                # one output alone: index without count, count without index
        flag = flag_patterns(n)["a random half"]
        want = compacted(flag != 0, dict(tri=tri))
        got = device_compact(torch, rt, n, "flag", dict(tri=tri), ("tri",), stream, flag=flag, index=False, count=False)
        assert_same_bits(got["tri"], want["tri"], f"n = {n}: tri alone")
        got = device_compact(torch, rt, n, "flag", {}, (), stream, flag=flag, index=False)
        assert got == dict(count=want["count"]), f"n = {n}: count alone"
        got = device_compact(torch, rt, n, "flag", {}, (), stream, flag=flag, count=False)
        assert_same_bits(got["index"], want["index"], f"n = {n}: index alone")


# ------------------------------------------------------------------ 3
def test_the_synthesised_bound(rrt, teapot):
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    n = 3000
    rng = np.random.default_rng(3)
    flag = (rng.random(n) < 0.4).astype(np.uint8)
    O = rng.standard_normal((n, 3))
    got = rt.compact_rays({}, "flag", flag=flag, origins=O, max_t=True)
    want = compacted(flag != 0, dict(origins=O), synth_max_t=True)
    assert 0 < want["count"] < n
    assert_compacted(got, want, "max_t synthesised")
    k = want["count"]
    assert (bits(got["max_t"][:k]) == 0x7FF0000000000000).all() and (bits(got["max_t"][k:]) == 0x7FF8000000000000).all()
    # a bound that is given is copied, bits and all: a NaN with a payload, a negative bound, -0.0 and +inf among the survivors
    max_t = rng.random(n) + 1.0
    keep = np.flatnonzero(flag)
    special = np.array([0x7FF8000000000123, 0xFFF0000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xBFF0000000000000], np.uint64).view(np.float64)
    max_t[keep[:5]] = special
    O[keep[5]] = (-0.0, np.nan, -np.inf)
    got = rt.compact_rays({}, "flag", flag=flag, origins=O, max_t=max_t)
    assert_compacted(got, compacted(flag != 0, dict(origins=O, max_t=max_t)), "max_t given")
    assert_same_bits(got["max_t"][:5], special, "the special bounds, first among the survivors")
    assert_same_bits(got["origins"][5], np.array([-0.0, np.nan, -np.inf]), "the special origin")
    assert int(bits(got["max_t"])[-1]) == 0x7FF8000000000000


@pytest.mark.parametrize("n", (1, 1025))
def test_a_host_array_named_twice_in_src(rrt, teapot, n):
    """The intended use of the host form (rrt.h): next_origin as origins, next_dir as dirs -- the same two ndarrays twice, so src holds equal pointers."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rng = np.random.default_rng(2 * n + 1)
    A, B = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    assert not np.array_equal(A, B)
    flag = flag_patterns(n)["a random half"]
    got = rt.compact_rays(dict(next_origin=A, next_dir=B), "flag", flag=flag, origins=A, dirs=B)
    assert_compacted(got, compacted(flag != 0, dict(origins=A, dirs=B, next_origin=A, next_dir=B)), f"n = {n}: two host arrays, each named twice")


# ------------------------------------------------------------------ 4
def test_mirror_on_the_mirror_room(rrt):
    A = mirror_room()
    lights = [rrt.Light(k, i, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS]
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    rt = rrt.RayTracer(sd, lights)
    O, D = rays_of(CREATION, RW, RH)
    rec = rt.surface_rays(O, D, planes=("material", "point"))
    table = rt.materials()
    hit = selection("hit", n_mats=len(table), material=rec["material"])
    sel = hit & (kr_of(A, rec["material"]) > 0.0)
    assert np.array_equal(sel, selection("mirror", n_mats=len(table), material=rec["material"], kr=[m["kr"] for m in table]))
    want = compacted(sel, rec)
    print(f"mirror room level 0: {len(sel)} records, {int(hit.sum())} hits, {want['count']} of them on a mirror")
    assert 0 < want["count"] < int(hit.sum())
    assert_compacted(rt.compact_rays(rec, "mirror"), want, "MIRROR")
    assert_compacted(rt.compact_rays(rec, "hit"), compacted(hit, rec), "HIT on the same records")
    rt.set_materials([dict(m, kr=0.0) for m in table])
    assert_compacted(rt.compact_rays(rec, "mirror"), compacted(np.zeros(len(sel), bool), rec), "MIRROR with every kr = 0")
    assert rt.compact_rays(rec, "mirror")["count"] == 0
    rt.set_materials([dict(m, kr=0.25 if i == 1 else 0.0) for i, m in enumerate(table)])           # the other material is the mirror now
    swapped = hit & (rec["material"] == 1)
    assert 0 < swapped.sum() < hit.sum()
    assert_compacted(rt.compact_rays(rec, "mirror"), compacted(swapped, rec), "MIRROR with the matte block as the only mirror")
    rt.set_materials(table)
    assert_compacted(rt.compact_rays(rec, "mirror"), want, "MIRROR with the table restored")


# ------------------------------------------------------------------ 5, 8
def assert_padded_batch_feeds_the_ambient_stage(torch, rt, rec, rot, n_mats, want, what):
    """Compact HIT (the three records, and rot if given) -> ambient_rays_into on all n padded records -> two scatters into prefilled arrays, on one stream:
    equal to `want` (the masks of the original records) and to open_of it; the tail of the padded outputs is 0 / n."""
    n = len(rec["material"])
    hit = selection("hit", n_mats=n_mats, material=rec["material"])
    count = int(hit.sum())
    assert 0 < count < n and mixed_waves(hit) >= 1, f"{what}: {count} hits of {n} records, {mixed_waves(hit)} waves with hits and misses"
    stream = torch.cuda.Stream()
    names = INPUTS + (("rot",) if rot is not None else ())
    src = {k: to_device(torch, rec[k]) for k in INPUTS}
    if rot is not None:
        src["rot"] = to_device(torch, rot)
    packed = {k: torch.empty_like(t) for k, t in src.items()}
    index, count_t = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(rt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    padded = {k: torch.full((n,), -1515870811, dtype=torch.int32, device="cuda") for k in OUTPUTS}
    final = dict(occluded=torch.zeros(n, dtype=torch.int32, device="cuda"), open=torch.full((n,), len(T8), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    s = stream.cuda_stream
    rt.compact_rays_into(packed, src, "hit", index, count_t, scratch, stream=s)
    rt.ambient_rays_into(padded, {k: packed[k] for k in INPUTS}, T8, T8_MAX_T, rot_t=packed.get("rot"), stream=s)
    for k in OUTPUTS:
        rt.scatter_rays_into(index, padded[k], final[k], stream=s)
    stream.synchronize()
    assert int(count_t.cpu().numpy().view(np.uint32)[0]) == count, what
    model = compacted(hit, {k: rec[k] for k in names} if rot is None else dict({k: rec[k] for k in INPUTS}, rot=np.asarray(rot)))
    for k in names:
        assert_same_bits(packed[k].cpu().numpy().view(ARRAYS[k][0]).reshape(model[k].shape), model[k], f"{what}: the packed {k}")
    got_padded = {k: padded[k].cpu().numpy().view(np.uint32) for k in OUTPUTS}
    assert (got_padded["occluded"][count:] == 0).all() and (got_padded["open"][count:] == len(T8)).all(), f"{what}: the tail of the padded outputs is not 0 / n"
    assert_same_bits(got_padded["occluded"][:count], want[hit], f"{what}: the padded masks vs the original records' masks, in order")
    assert_same_bits(final["occluded"].cpu().numpy().view(np.uint32), want, f"{what}: occluded, scattered back")
    assert_same_bits(final["open"].cpu().numpy().view(np.uint32), open_of(want, hit, len(T8)), f"{what}: open, scattered back")


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_the_padded_batch_feeds_the_ambient_stage(rrt, teapot, kept, mode):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    rec = kept["rec"]
    for r in (False, True):
        want = kept["want"][r]
        assert (want != 0).any()
        direct = rt.ambient_rays(rec, T8, T8_MAX_T, rot=kept["rot"] if r else None)
        assert_same_bits(direct["occluded"], want, f"walk {mode}, rot {r}: rt.ambient_rays on the original records vs the shadow query")
        assert_padded_batch_feeds_the_ambient_stage(torch, rt, rec, kept["rot"] if r else None, kept["n_mats"], want, f"teapot level 1, walk {mode}, rot {r}")


def two_levels_of_records(rt, cam):
    """The level-0 records of the 32x24 frame in the pose `cam`, and behind them the level-1 records of its hits: rays that leave the scene among them."""
    O, D = rays_of(cam, RW, RH)
    l0 = rt.surface_rays(O, D, planes=INPUTS)
    _, l1 = level1(rt, cam, RW, RH)
    return {k: np.concatenate([l0[k], l1[k]]) for k in INPUTS}


def test_a_soup_with_group_records(rrt, teapot_arrays):
    torch = pytest.importorskip("torch")
    A = soup_scene(teapot_arrays)
    rt = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), rrt.default_lights())
    supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
    assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records"
    rec = two_levels_of_records(rt, CREATION)
    rot = standard_rot(len(rec["material"]))
    want = rt.ambient_rays(rec, T8, T8_MAX_T, rot=rot)["occluded"]
    assert_same_bits(want, by_shadow_query(rt, Fan(rec, len(A["materials"]), T8, rot), T8_MAX_T), "soup: rt.ambient_rays vs the shadow query")
    assert (want != 0).sum() >= 50
    assert_padded_batch_feeds_the_ambient_stage(torch, rt, rec, rot, len(A["materials"]), want, "soup, levels 0 and 1")


def test_the_chain_shortcut_scene(rrt):
    torch = pytest.importorskip("torch")
    A, names = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    rt = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), chain_rrt_lights(rrt), rrt.Vector3d(*eye))
    rt.set_camera(**cam)
    assert rt.chain_info["n_chains"] >= 1, rt.chain_info
    rec = two_levels_of_records(rt, cam)
    rot = standard_rot(len(rec["material"]))
    want = rt.ambient_rays(rec, T8, T8_MAX_T, rot=rot)["occluded"]
    assert_same_bits(want, by_shadow_query(rt, Fan(rec, len(A["materials"]), T8, rot), T8_MAX_T), "chain scene: rt.ambient_rays vs the shadow query")
    assert (want != 0).sum() >= 50
    assert_padded_batch_feeds_the_ambient_stage(torch, rt, rec, rot, len(A["materials"]), want, "chain scene, levels 0 and 1")


# ------------------------------------------------------------------ 6
def test_a_chain_on_the_device_alone(rrt, teapot, kept):
    """surface_rays_into -> compact (next_origin / next_dir as the rays, a synthesised bound) -> surface_rays_into on the n padded rays -> compact -> ambient_rays_into,
    on one stream of the test's own; the host sees nothing until the stream is synchronised at the end."""
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    O, D = rays_of(CREATION, W, H)
    n = len(D)
    h0 = kept["l0"]["hit"].astype(bool)
    c1 = int(h0.sum())
    hit1, rot1 = kept["fans"][True].hit, np.zeros((n, 2))
    rot1[:c1] = kept["rot"]
    c2 = int(hit1.sum())
    assert 0 < c2 < c1 < n
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o_t, d_t, rot1_t = to_device(torch, O), to_device(torch, D), to_device(torch, rot1)
    l0 = dict(material=torch.empty(n, **i32), next_origin=torch.empty(3 * n, **f64), next_dir=torch.empty(3 * n, **f64))
    rays1 = dict(origins=torch.empty(3 * n, **f64), dirs=torch.empty(3 * n, **f64), max_t=torch.empty(n, **f64))
    rec1 = dict(point=torch.empty(3 * n, **f64), normal=torch.empty(3 * n, **f64), material=torch.empty(n, **i32))
    rec2 = dict(rot=torch.empty(2 * n, **f64), **{k: torch.empty_like(t) for k, t in rec1.items()})
    index1, index2, counts = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(2, **i32)
    scratch = torch.empty(rt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    out = {k: torch.full((n,), -1515870811, **i32) for k in OUTPUTS}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rt.surface_rays_into(o_t, d_t, l0, stream=s)
    rt.compact_rays_into(rays1, dict(material=l0["material"], origins=l0["next_origin"], dirs=l0["next_dir"]), "hit", index1, counts[0:1], scratch, stream=s)
    rt.surface_rays_into(rays1["origins"], rays1["dirs"], rec1, max_t_t=rays1["max_t"], stream=s)
    rt.compact_rays_into(rec2, dict(rot=rot1_t, **rec1), "hit", index2, counts[1:2], scratch, stream=s)
    rt.ambient_rays_into(out, {k: rec2[k] for k in INPUTS}, T8, T8_MAX_T, rot_t=rec2["rot"], stream=s)
    stream.synchronize()
    assert counts.cpu().numpy().view(np.uint32).tolist() == [c1, c2]
    want_index1 = compacted(h0, {})["index"]
    assert_same_bits(index1.cpu().numpy().view(np.uint32), want_index1, "level 0 -> 1: index")
    got1 = {k: t.cpu().numpy().view(ARRAYS[k][0]).reshape((n, 3) if ARRAYS[k][1] == 3 else (n,)) for k, t in rec1.items()}
    for k in INPUTS:
        assert_same_bits(got1[k][:c1], np.asarray(kept["rec"][k]), f"the first count level-1 records vs the host path's: {k}")
        assert_same_bits(got1[k][c1:], dead(k, n - c1), f"the tail of the level-1 records holds the miss values: {k}")
    full_hit1 = np.zeros(n, bool)
    full_hit1[:c1] = hit1
    assert_same_bits(index2.cpu().numpy().view(np.uint32), compacted(full_hit1, {})["index"], "level 1 -> 2: index")
    want = kept["want"][True]
    got = {k: t.cpu().numpy().view(np.uint32) for k, t in out.items()}
    assert (want[hit1] != 0).any()
    assert_same_bits(got["occluded"][:c2], want[hit1], "the final masks of the survivors vs the shadow query's, in order")
    assert_same_bits(got["open"][:c2], open_of(want, hit1, len(T8))[hit1], "the final open counts of the survivors")
    assert (got["occluded"][c2:] == 0).all() and (got["open"][c2:] == len(T8)).all(), "the dead tail: mask 0, open n"


# ------------------------------------------------------------------ 7
@pytest.mark.parametrize("elem", (1, 4, 8, 16, 24))
def test_scatter(rrt, teapot, elem):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    n = 5000
    rng = np.random.default_rng(elem)
    dtype, width = {1: (np.uint8, 1), 4: (np.uint32, 1), 8: (np.float64, 1), 16: (np.float64, 2), 24: (np.float64, 3)}[elem]
    shape = (n, width) if width > 1 else (n,)
    src = rng.integers(0, 256, n * elem, dtype=np.uint8).view(dtype).reshape(shape)           # (random bytes: NaN patterns among the doubles)
    dst = np.full(n * elem, 0xA5, np.uint8).view(dtype).reshape(shape)
    index = rng.permutation(n).astype(np.uint32)
    index[::7] = DEAD_INDEX
    index[3::11] = n + np.arange(len(index[3::11]), dtype=np.uint32) * 1000                     # n itself first: the smallest index that is skipped
    index[5] = 0xFFFFFFFE
    want = scattered(index, src, dst)
    named = np.zeros(n, bool)
    named[index[index < n]] = True
    assert 1000 < named.sum() < n - 1000 and (bits(want[~named]) == bits(dst[~named])).all()
    got = rt.scatter_rays(index, src, dst.copy())
    assert_same_bits(got, want, f"elem_bytes {elem}: the host form")
    stream = torch.cuda.Stream()
    g = Guarded(torch, dtype, n * width)
    g.t.copy_(to_device(torch, dst))
    index_t, src_t = to_device(torch, index), to_device(torch, src)
    torch.cuda.synchronize()
    rt.scatter_rays_into(index_t, src_t, g.t, stream=stream.cuda_stream)
    stream.synchronize()
    assert_same_bits(g.read(f"elem_bytes {elem}").reshape(shape), want, f"elem_bytes {elem}: the device form")
    # scatter after compact puts the selected elements back where they were
    flag = flag_patterns(n)["a random half"]
    index = rt.compact_rays({}, "flag", flag=flag)["index"]
    packed = np.concatenate([src[flag != 0], np.zeros_like(src[flag == 0])])
    back = rt.scatter_rays(index, packed, dst.copy())
    assert_same_bits(back[flag != 0], src[flag != 0], f"elem_bytes {elem}: scatter after compact, the selected elements")
    assert_same_bits(back[flag == 0], dst[flag == 0], f"elem_bytes {elem}: scatter after compact, the others keep their pattern")
    # an index that occurs twice: one of the two values, and no fault
    twice = np.array([2, 2, DEAD_INDEX, 0], np.uint32)
    got = rt.scatter_rays(twice, src[:4], dst[:4].copy())
    assert bits(got[2]).tolist() in (bits(src[0]).tolist(), bits(src[1]).tolist()) and (bits(got[0]) == bits(src[3])).all() and (bits(got[[1, 3]]) == bits(dst[[1, 3]])).all()


# ------------------------------------------------------------------ 9
def test_state_is_untouched(rrt, teapot, kept):
    torch = pytest.importorskip("torch")
    rec, n_mats = kept["rec"], kept["n_mats"]
    n = len(rec["material"])
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = [rt.render(W, H) for _ in range(2)][-1]
    before = dict(stats=rt.last_stats(), camera=rt.camera(), lights=[(l.kind, l.intensity, (l.v.x, l.v.y, l.v.z)) for l in rt.lights()], materials=rt.materials())
    hit = selection("hit", n_mats=n_mats, material=rec["material"])
    want = compacted(hit, {k: rec[k] for k in INPUTS})
    stream = torch.cuda.Stream()
    first = device_compact(torch, rt, n, "hit", {k: rec[k] for k in INPUTS}, INPUTS, stream)
    again = device_compact(torch, rt, n, "hit", {k: rec[k] for k in INPUTS}, INPUTS, stream)
    assert_compacted(first, want, "the first run")
    assert_compacted(again, first, "the same compaction twice")
    assert_compacted(rt.compact_rays({k: rec[k] for k in INPUTS}, "mirror"), compacted(hit & (kr_of(dict(materials=before["materials"]), rec["material"]) > 0.0),
                                                                                         {k: rec[k] for k in INPUTS}), "MIRROR, the host form")
    back = rt.scatter_rays(first["index"], first["material"], np.full(n, 0xFFFFFFFF, np.uint32))
    assert_same_bits(back, np.where(hit, rec["material"], 0xFFFFFFFF).astype(np.uint32), "material, scattered back")
    # refusals of the device form with a real raytracer leave the guarded outputs as they were
    src_t = {k: to_device(torch, rec[k]) for k in INPUTS}
    out = {k: Guarded(torch, ARRAYS[k][0], ARRAYS[k][1] * n) for k in INPUTS}
    index, count, scratch = Guarded(torch, np.uint32, n), Guarded(torch, np.uint32, 1), Guarded(torch, np.uint8, rt.compact_scratch_bytes(n))
    small = scratch.t[:rt.compact_scratch_bytes(n) - 1]
    outs = {k: g.t for k, g in out.items()}
    refused = [("a scratch one byte short", lambda: rt.compact_rays_into(outs, src_t, "hit", index.t, count.t, small)),
               ("no scratch", lambda: rt.compact_rays_into(outs, src_t, "hit", index.t, count.t, None)),
               ("FLAG without a flag array", lambda: rrt._call("rrt_compact_rays_device", rt._h, n, 2, None, rrt._ray_set(src_t), rrt._ray_set(outs), rrt._ptr(index.t),
                                                               rrt._ptr(count.t), rrt._ptr(scratch.t), scratch.t.numel(), None)),
               ("an unknown select", lambda: rrt._call("rrt_compact_rays_device", rt._h, n, 7, None, rrt._ray_set(src_t), rrt._ray_set(outs), rrt._ptr(index.t),
                                                       rrt._ptr(count.t), rrt._ptr(scratch.t), scratch.t.numel(), None)),
               ("an array of out without its array of src", lambda: rt.compact_rays_into(dict(outs, tri=index.t), src_t, "hit", None, count.t, scratch.t)),
               ("no output", lambda: rt.compact_rays_into({}, src_t, "hit", None, None, scratch.t)),
               ("a scatter of 3-byte elements", lambda: rrt._call("rrt_scatter_rays_device", rt._h, n, rrt._ptr(src_t["material"]), 3, rrt._ptr(src_t["material"]),
                                                                 rrt._ptr(index.t), None))]
    for what, call in refused:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        torch.cuda.synchronize()
        assert all(g.untouched() for g in (*out.values(), index, count, scratch)), f"{what}: an output of a refused call was written"
    after = dict(stats=rt.last_stats(), camera=rt.camera(), lights=[(l.kind, l.intensity, (l.v.x, l.v.y, l.v.z)) for l in rt.lights()], materials=rt.materials())
    assert after == before, "the calls changed the statistics, the camera, the lights or the materials"
    assert np.array_equal(rt.render(W, H), frame) and rt.last_stats()["filter_variant"] == before["stats"]["filter_variant"], "the next frame, or its variant, differs"
