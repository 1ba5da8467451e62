"""Stable sort of ray batches and records by a coherence key on the device (include/rrt.h: rrt_sort_rays[_device]) on the GPU.

The statement under test: the result is the contract's stable ascending sort -- index, the sorted keys, count, every requested array gathered byte for byte, the
dead entries in the tail in source order -- as sort_checks.py restates it in numpy, the keys of the RAY and RECORD modes are the model's with the root box in
force, and a batch sorted this way feeds rrt_surface_rays_device and rrt_ambient_rays_device unchanged: what they give for the sorted batch, scattered back with
`index`, is what they give for the original one.  Every comparison is byte for byte (doubles through their integer bits); every device output sits between guard
elements, the scratch included.

Constants of csrc/sort.hip that decide the sizes below: a hist / place block covers a tile of 4096 entries (kSortTile) in four rounds of 1024 (16 waves of 64);
a row of tile counts is scanned in chunks of 256 tiles with a carry.  BIG has 258 tiles: two chunks, the second one partly filled.
"""
import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T
from ambient_rays_checks import INPUTS, OUTPUTS, kept_records as kept, open_of, standard_rot  # noqa: F401  (fixtures: kept)
from bitwise import assert_same_bits
from compact_checks import ARRAYS, NAMES, RECORD_NAMES, Guarded, ceil_div, selection, to_device
from gpu_checks import FORCED_MODES, chain_rrt_lights, chain_scene
from scenes import CREATION, rays_of, teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import soup_scene
from sort_checks import DEAD_KEY, assert_sorted, dead_rays, has_ties, key_patterns, ray_key, root_box_of, sorted_batch

pytestmark = pytest.mark.gpu

W, H = 64, 48
RW, RH = 32, 24
TILE, ROUND, SCAN = 4096, 1024, 256                              # csrc/device_scene.hpp: kSortTile; csrc/sort.hip: kThreads, kFlatBlock
BIG = 2 ** 20 + 4097                                             # 258 tiles: two chunks of a row's scan
EDGE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 4095, 4096, 4097, 8191, 8193, 70001, BIG)
HOST_TOO = 4097                                                  # up to this size the host form is checked as well
SENTINEL = -1515870811                                           # 0xA5A5A5A5 as int32


def shaped(name, a, n):
    return np.asarray(a).reshape((n, ARRAYS[name][1]) if ARRAYS[name][1] > 1 else (n,))


def device_sort(torch, rt, n, key, src, out_names, stream, keys=None, index=True, keys_out=True, count=True):
    """rt.sort_rays_into of the host arrays `src` ({name: array}; keys: uint32 [n]) into guarded outputs on `stream`: {"index", "keys", "count", name: array}."""
    src_t = {name: to_device(torch, a) for name, a in src.items()}
    keys_t = None if keys is None else to_device(torch, keys)
    out = {name: Guarded(torch, ARRAYS[name][0], ARRAYS[name][1] * n) for name in out_names}
    index_g, keys_g = (Guarded(torch, np.uint32, n) if index else None), (Guarded(torch, np.uint32, n) if keys_out else None)
    count_g = Guarded(torch, np.uint32, 1) if count else None
    scratch = Guarded(torch, np.uint8, rt.sort_scratch_bytes(n))
    torch.cuda.synchronize()
    rt.sort_rays_into({name: g.t for name, g in out.items()}, src_t, key, index_g and index_g.t, keys_g and keys_g.t, count_g and count_g.t, scratch.t,
                      keys_t=keys_t, stream=stream.cuda_stream)
    stream.synchronize()
    scratch.read("scratch")
    got = {name: shaped(name, g.read(name), n) for name, g in out.items()}
    if index:
        got["index"] = index_g.read("index")
    if keys_out:
        got["keys"] = keys_g.read("keys_out")
    if count:
        got["count"] = int(count_g.read("count")[0])
    return got


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_given_keys(rrt, teapot, n):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    stream = torch.cuda.Stream()
    assert n != BIG or ceil_div(ceil_div(n, TILE), SCAN) == 2, "BIG is meant to take two chunks of a row's scan"
    rng = np.random.default_rng(n)
    point = rng.integers(0, 256, 24 * n, dtype=np.uint8).view(np.float64).reshape(n, 3)        # (random bytes: NaN patterns among the doubles)
    tri = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    src = dict(point=point, tri=tri)
    for what, keys in key_patterns(n).items():
        want = sorted_batch(keys, src)
        if (n >= 3 and what in ("all equal", "two values alternating")) or (n >= 63 and what in ("random in [0, 8)", "only the top byte differs")):
            assert has_ties(keys), (n, what)
        if n >= 2 and what == "strictly descending":
            assert want["index"].tolist()[:2] == [n - 1, n - 2] and not has_ties(keys)
        if what == "every 11th dead":
            assert want["count"] == n - len(keys[::11]) and (n < 64 or 0 < want["count"] < n)
        else:
            assert want["count"] == n
        assert_sorted(device_sort(torch, rt, n, "given", src, ("point", "tri"), stream, keys=keys), want, f"n = {n}, {what}: the device form")
        if n <= HOST_TOO:
            assert_sorted(rt.sort_rays(dict(tri=tri, point=point), key="given", keys=keys), want, f"n = {n}, {what}: the host form")
    if n <= HOST_TOO:                                            # one output alone
        keys = key_patterns(n)["every 11th dead"]
        want = sorted_batch(keys, src)
        got = device_sort(torch, rt, n, "given", dict(tri=tri), ("tri",), stream, keys=keys, index=False, keys_out=False, count=False)
        assert_same_bits(got["tri"], want["tri"], f"n = {n}: tri alone")
        assert device_sort(torch, rt, n, "given", {}, (), stream, keys=keys, index=False, keys_out=False) == dict(count=want["count"]), f"n = {n}: count alone"
        got = device_sort(torch, rt, n, "given", {}, (), stream, keys=keys, keys_out=False, count=False)
        assert_same_bits(got["index"], want["index"], f"n = {n}: index alone")
        got = device_sort(torch, rt, n, "given", {}, (), stream, keys=keys, index=False, count=False)
        assert_same_bits(got["keys"], want["keys"], f"n = {n}: keys_out alone")


# ------------------------------------------------------------------ 2
# per n: dead entries (every 11th bound NaN, one 0.0, one negative); groups of equal alive keys and, at 129, the key of the entry with the special direction -- both
# by the model for the seed of ray_batch (the copies of a neighbour, and at the larger sizes chance: half the origins are clamped into the outer cells)
RAY_CASES = {129: (14, 1, 0x3e4fe02), 4097: (375, 41, None), 70001: (6366, 1046, None)}


def ray_batch(n):
    """The batch of part 2: (origins, dirs, max_t, the index of the special direction, the index of the special origin)."""
    rng = np.random.default_rng(3000 + n)
    O = rng.uniform(-25.0, 25.0, (n, 3))
    D = rng.standard_normal((n, 3))
    max_t = rng.uniform(1.0, 100.0, n)
    for i in range(97, n, 97):                                   # equal alive keys: a copy of the neighbour
        O[i], D[i] = O[i - 1], D[i - 1]
    max_t[::11] = np.nan
    free = [i for i in range(1, n) if i % 11 and i % 97 and (i + 1) % 97 and (i + 1) % 11]
    i_zero, i_neg, i_dir = free[3], free[7], free[12]
    i_org = next(i for i in free[20:] if D[i, 0] < 0.0 and D[i, 1] > 0.0 and D[i, 2] > 0.0)
    max_t[i_zero], max_t[i_neg] = 0.0, -3.5
    D[i_dir] = (-0.0, 0.0, np.nan)
    O[i_org] = (np.nan, np.inf, -np.inf)
    return O, D, max_t, i_dir, i_org


def equal_alive_groups(keys):
    values, counts = np.unique(keys[keys != DEAD_KEY], return_counts=True)
    return int((counts > 1).sum())


@pytest.mark.parametrize("n", tuple(RAY_CASES))
def test_ray_keys(rrt, teapot, n):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    box = root_box_of(rt.octree())
    assert box[0].tolist() == [-20.0] * 3 and box[1].tolist() == [20.0] * 3
    O, D, max_t, i_dir, i_org = ray_batch(n)
    dead = dead_rays(max_t, n)
    keys = ray_key(O, D, dead, box)
    # the batch is what it is meant to be, by the model alone
    groups = equal_alive_groups(keys)
    clamped = ((O < -20.0) | (O >= 20.0)).any(1).mean()
    print(f"n = {n}: {int(dead.sum())} dead, {groups} groups of equal alive keys, {clamped:.3f} of the origins clamped, special keys {int(keys[i_dir]):#x} {int(keys[i_org]):#x}")
    assert int(dead.sum()) == RAY_CASES[n][0]
    copies = [i for i in range(97, n, 97) if not dead[i] and not dead[i - 1]]
    assert len(copies) >= 1 and all(keys[i] == keys[i - 1] for i in copies) and groups == RAY_CASES[n][1]
    assert 0.4 < clamped < 0.6, "about half the origins are meant to be clamped"
    assert ((O < -20.0).any() and (O > 20.0).any())
    alive = keys[~dead]
    assert all(len(np.unique((alive >> s) & 0xFF)) > 1 for s in (0, 8, 16, 24)), "a key byte is constant across the batch"
    assert not dead[i_dir] and not dead[i_org]
    assert keys[i_dir] < 2 ** 27 and keys[i_dir] == (RAY_CASES[n][2] or keys[i_dir]), "the direction (-0.0, 0.0, NaN) sets no sign bit"
    assert keys[i_org] == 0x0a492492, "the origin (NaN, +inf, -inf) lies in cell (0, 511, 0); its direction is (-, +, +)"
    rec = rt.surface_rays(O, D, max_t)
    src = dict(origins=O, dirs=D, max_t=max_t, rot=standard_rot(n), **rec)
    assert tuple(src) == NAMES
    want = sorted_batch(keys, src)
    assert want["count"] == n - RAY_CASES[n][0]
    got = device_sort(torch, rt, n, "ray", src, NAMES, torch.cuda.Stream())
    assert_sorted(got, want, f"n = {n}: the device form, all sixteen arrays")
    if n <= HOST_TOO:
        host = rt.sort_rays({k: rec[k] for k in RECORD_NAMES}, key="ray", origins=O, dirs=D, max_t=max_t, rot=src["rot"])
        assert_sorted(host, want, f"n = {n}: the host form, all sixteen arrays")
        # without a bound every ray is alive
        free = rt.sort_rays({}, key="ray", origins=O, dirs=D)
        assert_sorted(free, sorted_batch(ray_key(O, D, np.zeros(n, bool), box), dict(origins=O, dirs=D)), f"n = {n}: no max_t")
        assert free["count"] == n


# ------------------------------------------------------------------ 3
def test_record_keys_on_the_level_0_records_of_the_teapot(rrt, teapot, teapot_arrays):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    O, D = rays_of(CREATION, W, H)
    n = len(D)
    rec = rt.surface_rays(O, D)
    hit = selection("hit", n_mats=len(teapot_arrays["materials"]), material=rec["material"])
    keys = ray_key(rec["point"], rec["normal"], ~hit, root_box_of(rt.octree()))
    want = sorted_batch(keys, rec)
    print(f"teapot level 0: {n} records, {want['count']} hits, {len(np.unique(keys))} distinct keys")
    assert want["count"] == int(hit.sum()) and 0 < want["count"] < n and np.array_equal(hit, rec["hit"].astype(bool))
    assert np.array_equal(want["index"][want["count"]:], np.flatnonzero(~hit)), "the model's tail is not the misses in source order"
    assert len(np.unique(keys)) > 100
    got = device_sort(torch, rt, n, "record", rec, RECORD_NAMES, torch.cuda.Stream())
    assert_sorted(got, want, "the device form")
    assert np.array_equal(got["index"][got["count"]:], np.flatnonzero(~hit)) and (got["keys"][got["count"]:] == DEAD_KEY).all()
    assert_sorted(rt.sort_rays(rec, key="record"), want, "the host form")


# ------------------------------------------------------------------ 4
def test_the_root_box_in_force(rrt, teapot_arrays):
    A = teapot_arrays
    second, third = (-10.0, 30.0, -8.0, 24.0, -16.0, 16.0), (-7.0, 9.0, -3.0, 13.0, -6.5, 9.5)
    rt = rrt.RayTracer.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"], rrt.default_lights(), root=second)
    n = 4097
    O, D, max_t, _, _ = ray_batch(n)
    seen = []
    for what, root in (("the raytracer's own root box", second), ("the root box of set_triangles", third), ("root=None keeps the box in force", third)):
        if what != "the raytracer's own root box":
            rt.set_triangles(A["pos"], A["uv"], A["nrm"], A["mat"], root if "None" not in what else None)
        box = root_box_of(rt.octree())
        assert (box[0].tolist(), box[1].tolist()) == (list(root[0::2]), list(root[1::2])), what
        keys = ray_key(O, D, dead_rays(max_t, n), box)
        assert_sorted(rt.sort_rays({}, key="ray", origins=O, dirs=D, max_t=max_t), sorted_batch(keys, dict(origins=O, dirs=D, max_t=max_t)), what)
        seen.append(keys)
    assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[1], seen[2])
    assert not np.array_equal(seen[0], ray_key(O, D, dead_rays(max_t, n), (np.full(3, -20.0), np.full(3, 20.0))))


# ------------------------------------------------------------------ 5
def two_levels(rt, cam, w, h, l0=None):
    """The primary rays of the w x h frame in the pose `cam` and behind them the reflection rays of its hits, with a bound that kills every 13th."""
    O0, D0 = rays_of(cam, w, h)
    if l0 is None:
        l0 = rt.surface_rays(O0, D0, planes=("hit", "next_origin", "next_dir"))
    h0 = l0["hit"].astype(bool)
    O, D = np.concatenate([O0, l0["next_origin"][h0]]), np.concatenate([D0, l0["next_dir"][h0]])
    max_t = np.full(len(O), 80.0)
    max_t[::13] = np.nan
    return np.ascontiguousarray(O), np.ascontiguousarray(D), max_t


def assert_sorted_rays_feed_the_surface_stage(torch, rt, O, D, max_t, what):
    """Sort RAY -> surface_rays_into with all twelve outputs on the sorted rays -> a scatter of each, on one stream: equal to rt.surface_rays on the original rays."""
    n = len(O)
    want = rt.surface_rays(O, D, max_t)
    assert 0 < int(want["hit"].sum()) < n and (want["lights"] != 0).any(), what
    src = dict(origins=to_device(torch, O), dirs=to_device(torch, D), max_t=to_device(torch, max_t))
    rays = {k: torch.empty_like(t) for k, t in src.items()}
    index = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = torch.empty(rt.sort_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    mid = {k: to_device(torch, np.zeros(ARRAYS[k][1] * n, ARRAYS[k][0])) for k in RECORD_NAMES}
    final = {k: to_device(torch, np.full(ARRAYS[k][1] * n * np.dtype(ARRAYS[k][0]).itemsize, 0xA5, np.uint8).view(ARRAYS[k][0])) for k in RECORD_NAMES}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rt.sort_rays_into(rays, src, "ray", index, None, None, scratch, stream=s)
    rt.surface_rays_into(rays["origins"], rays["dirs"], mid, max_t_t=rays["max_t"], stream=s)
    for k in RECORD_NAMES:
        rt.scatter_rays_into(index, mid[k], final[k], stream=s)
    stream.synchronize()
    idx = index.cpu().numpy().view(np.uint32)
    assert np.array_equal(np.sort(idx), np.arange(n)), f"{what}: index is no permutation"
    assert not np.array_equal(idx, np.arange(n)), f"{what}: the sort left the batch in its order"
    for k in RECORD_NAMES:
        assert_same_bits(shaped(k, final[k].cpu().numpy().view(ARRAYS[k][0]), n), want[k], f"{what}: {k} of the sorted rays, scattered back")


def assert_sorted_records_feed_the_ambient_stage(torch, rt, rec, rot, n_mats, want, what):
    """Sort RECORD (the three records and rot) -> ambient_rays_into on the sorted records -> two scatters, on one stream: equal to `want`, the masks of the original
    records, and to open_of it."""
    n = len(rec["material"])
    hit = selection("hit", n_mats=n_mats, material=rec["material"])
    assert 0 < int(hit.sum()) < n and (want != 0).any(), what
    src = dict(rot=to_device(torch, rot), **{k: to_device(torch, rec[k]) for k in INPUTS})
    packed = {k: torch.empty_like(t) for k, t in src.items()}
    index, count_t = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(rt.sort_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    mid = {k: torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for k in OUTPUTS}
    final = {k: torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for k in OUTPUTS}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rt.sort_rays_into(packed, src, "record", index, None, count_t, scratch, stream=s)
    rt.ambient_rays_into(mid, {k: packed[k] for k in INPUTS}, T8, T8_MAX_T, rot_t=packed["rot"], stream=s)
    for k in OUTPUTS:
        rt.scatter_rays_into(index, mid[k], final[k], stream=s)
    stream.synchronize()
    assert int(count_t.cpu().numpy().view(np.uint32)[0]) == int(hit.sum()), what
    assert_same_bits(final["occluded"].cpu().numpy().view(np.uint32), want, f"{what}: occluded of the sorted records, scattered back")
    assert_same_bits(final["open"].cpu().numpy().view(np.uint32), open_of(want, hit, len(T8)), f"{what}: open of the sorted records, scattered back")


def records_of(rt, O, D, max_t):
    return rt.surface_rays(O, D, max_t, planes=INPUTS)


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_the_sorted_batch_feeds_the_stages_on_the_teapot(rrt, teapot, kept, mode):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    O, D, max_t = two_levels(rt, CREATION, W, H, kept["l0"])
    assert_sorted_rays_feed_the_surface_stage(torch, rt, O, D, max_t, f"teapot, walk {mode}")
    want = rt.ambient_rays(kept["rec"], T8, T8_MAX_T, rot=kept["rot"])["occluded"]
    assert_same_bits(want, kept["want"][True], f"walk {mode}: rt.ambient_rays on the original records vs the shadow query")
    assert_sorted_records_feed_the_ambient_stage(torch, rt, kept["rec"], kept["rot"], kept["n_mats"], want, f"teapot level 1, walk {mode}")


def assert_both_stages(torch, rt, cam, n_mats, what):
    O, D, max_t = two_levels(rt, cam, RW, RH)
    assert_sorted_rays_feed_the_surface_stage(torch, rt, O, D, max_t, what)
    rec = records_of(rt, O, D, max_t)
    rot = standard_rot(len(rec["material"]))
    want = rt.ambient_rays(rec, T8, T8_MAX_T, rot=rot)["occluded"]
    assert_sorted_records_feed_the_ambient_stage(torch, rt, rec, rot, n_mats, want, what)


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_the_sorted_batch_feeds_the_stages_on_a_soup_with_group_records(rrt, teapot_arrays, mode):
    torch = pytest.importorskip("torch")
    A = soup_scene(teapot_arrays)
    rt = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), rrt.default_lights(), box_filter=mode)
    supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
    assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records"
    assert_both_stages(torch, rt, CREATION, len(A["materials"]), f"soup, walk {mode}")


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_the_sorted_batch_feeds_the_stages_on_the_chain_scene(rrt, mode):
    torch = pytest.importorskip("torch")
    A, names = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    rt = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), chain_rrt_lights(rrt), rrt.Vector3d(*eye),
                       box_filter=mode)
    rt.set_camera(**cam)
    assert rt.chain_info["n_chains"] >= 1, rt.chain_info
    assert_both_stages(torch, rt, cam, len(A["materials"]), f"chain scene, walk {mode}")


# ------------------------------------------------------------------ 6
def test_a_chain_on_the_device_alone(rrt, teapot, kept):
    """surface_rays_into -> sort RAY (next_origin / next_dir as the rays, rot along) -> surface_rays_into on the sorted rays -> compact HIT -> ambient_rays_into, on
    one stream of the test's own; the host sees nothing until the stream is synchronised at the end.  Two scatters bring the masks back to source order, where they
    equal the same chain through the host forms."""
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    O, D = rays_of(CREATION, W, H)
    n = len(D)
    rot = standard_rot(n)
    # the host forms, in source order
    l0 = rt.surface_rays(O, D, planes=("next_origin", "next_dir"))
    rec1 = rt.surface_rays(l0["next_origin"], l0["next_dir"], planes=INPUTS)
    hit1 = selection("hit", n_mats=kept["n_mats"], material=rec1["material"])
    want = rt.ambient_rays(rec1, T8, T8_MAX_T, rot=rot)
    assert 0 < int(hit1.sum()) < n and (want["occluded"] != 0).any()
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o_t, d_t, rot_t = to_device(torch, O), to_device(torch, D), to_device(torch, rot)
    l0_t = dict(next_origin=torch.empty(3 * n, **f64), next_dir=torch.empty(3 * n, **f64))
    rays1 = dict(origins=torch.empty(3 * n, **f64), dirs=torch.empty(3 * n, **f64), rot=torch.empty(2 * n, **f64))
    rec1_t = dict(point=torch.empty(3 * n, **f64), normal=torch.empty(3 * n, **f64), material=torch.empty(n, **i32))
    rec2 = dict(rot=torch.empty(2 * n, **f64), **{k: torch.empty_like(t) for k, t in rec1_t.items()})
    index1, index2, count = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(1, **i32)
    sort_scratch = torch.empty(rt.sort_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    compact_scratch = torch.empty(rt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    out = {k: torch.full((n,), SENTINEL, **i32) for k in OUTPUTS}
    sorted_out = dict(occluded=torch.zeros(n, **i32), open=torch.full((n,), len(T8), **i32))
    final = {k: torch.full((n,), SENTINEL, **i32) for k in OUTPUTS}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rt.surface_rays_into(o_t, d_t, l0_t, stream=s)
    rt.sort_rays_into(rays1, dict(origins=l0_t["next_origin"], dirs=l0_t["next_dir"], rot=rot_t), "ray", index1, None, None, sort_scratch, stream=s)
    rt.surface_rays_into(rays1["origins"], rays1["dirs"], rec1_t, stream=s)
    rt.compact_rays_into(rec2, dict(rot=rays1["rot"], **rec1_t), "hit", index2, count, compact_scratch, stream=s)
    rt.ambient_rays_into(out, {k: rec2[k] for k in INPUTS}, T8, T8_MAX_T, rot_t=rec2["rot"], stream=s)
    for k in OUTPUTS:
        rt.scatter_rays_into(index2, out[k], sorted_out[k], stream=s)
        rt.scatter_rays_into(index1, sorted_out[k], final[k], stream=s)
    stream.synchronize()
    assert int(count.cpu().numpy().view(np.uint32)[0]) == int(hit1.sum())
    keys = ray_key(l0["next_origin"], l0["next_dir"], np.zeros(n, bool), root_box_of(rt.octree()))
    assert_same_bits(index1.cpu().numpy().view(np.uint32), sorted_batch(keys, {})["index"], "level 0 -> 1: index of the sort")
    for k in OUTPUTS:
        assert_same_bits(final[k].cpu().numpy().view(np.uint32), want[k], f"{k}: the device chain, scattered back twice, vs the host forms in source order")


# ------------------------------------------------------------------ 7
def test_state_is_untouched(rrt, teapot, kept):
    torch = pytest.importorskip("torch")
    rec = {k: kept["rec"][k] for k in INPUTS}
    n = len(rec["material"])
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    frame = [rt.render(W, H) for _ in range(2)][-1]
    before = dict(stats=rt.last_stats(), camera=rt.camera(), lights=[(l.kind, l.intensity, (l.v.x, l.v.y, l.v.z)) for l in rt.lights()], materials=rt.materials())
    hit = selection("hit", n_mats=kept["n_mats"], material=rec["material"])
    want = sorted_batch(ray_key(rec["point"], rec["normal"], ~hit, root_box_of(rt.octree())), rec)
    stream = torch.cuda.Stream()
    first = device_sort(torch, rt, n, "record", rec, INPUTS, stream)       # (device_sort reads the scratch's guards)
    again = device_sort(torch, rt, n, "record", rec, INPUTS, stream)
    assert_sorted(first, want, "the first run")
    assert_sorted(again, first, "the same sort twice")
    assert rt.last_stats() == before["stats"], "the device form changed the statistics"
    assert_sorted(rt.sort_rays(rec, key="record"), want, "the host form")
    assert rt.last_stats() == before["stats"], "the host form changed the statistics"
    back = rt.scatter_rays(first["index"], first["material"], np.full(n, 0x5A5A5A5A, np.uint32))
    assert_same_bits(back, np.asarray(rec["material"]), "material, scattered back: the inverse of the sort")
    # refusals of the device form with a real raytracer leave the guarded outputs as they were
    src_t = {k: to_device(torch, rec[k]) for k in INPUTS}
    out = {k: Guarded(torch, ARRAYS[k][0], ARRAYS[k][1] * n) for k in INPUTS}
    index, keys_out, count = Guarded(torch, np.uint32, n), Guarded(torch, np.uint32, n), Guarded(torch, np.uint32, 1)
    scratch = Guarded(torch, np.uint8, rt.sort_scratch_bytes(n))
    small = scratch.t[:rt.sort_scratch_bytes(n) - 1]
    outs = {k: g.t for k, g in out.items()}
    raw = lambda mode, keys: rrt._call("rrt_sort_rays_device", rt._h, n, mode, keys, rrt._ray_set(src_t), rrt._ray_set(outs), rrt._ptr(index.t), rrt._ptr(keys_out.t),
                                       rrt._ptr(count.t), rrt._ptr(scratch.t), scratch.t.numel(), None)
    refused = [("a scratch one byte short", lambda: rt.sort_rays_into(outs, src_t, "record", index.t, keys_out.t, count.t, small)),
               ("no scratch", lambda: rt.sort_rays_into(outs, src_t, "record", index.t, keys_out.t, count.t, None)),
               ("GIVEN without keys", lambda: raw(0, None)),
               ("RAY without origins", lambda: raw(1, None)),
               ("an unknown mode", lambda: raw(7, None)),
               ("an array of out without its array of src", lambda: rt.sort_rays_into(dict(outs, tri=index.t), src_t, "record", None, keys_out.t, count.t, scratch.t)),
               ("no output", lambda: rt.sort_rays_into({}, src_t, "record", None, None, None, scratch.t))]
    for what, call in refused:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        torch.cuda.synchronize()
        assert all(g.untouched() for g in (*out.values(), index, keys_out, count, scratch)), f"{what}: an output of a refused call was written"
    after = dict(stats=rt.last_stats(), camera=rt.camera(), lights=[(l.kind, l.intensity, (l.v.x, l.v.y, l.v.z)) for l in rt.lights()], materials=rt.materials())
    assert after == before, "the calls changed the statistics, the camera, the lights or the materials"
    assert np.array_equal(rt.render(W, H), frame) and rt.last_stats()["filter_variant"] == before["stats"]["filter_variant"], "the next frame, or its variant, differs"
