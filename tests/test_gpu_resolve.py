"""Surface records from kept hits (include/rrt.h: rrt_resolve_hits, rrt_resolve_hits_device, rrt_resolve_hits_counted_device) on the GPU: from the t, u, v and
tri an earlier walk left for a ray -- rrt_intersect_rays', rrt_surface_rays' or a frame's visibility planes -- the seven arrays rrt_surface_rays writes for that
ray, with no primary walk, and the triangle -> slot table the call reads (RRT_BUF_TRI_SLOT).

Every comparison of arrays is bit for bit (f64 through its integer bits).  The reference is rrt_surface_rays on the same rays -- the contract of rrt.h -- and,
so that the call is not only compared with the library itself, the host restatement of tests/ray_surface_checks.py around the oracle's intersector.  Every
comparison asserts that its batch holds hits, misses and lights that are and are not reached, so an empty batch cannot pass.
"""
import numpy as np
import pytest

from bitwise import assert_same_arrays, same
from compact_checks import to_device
from gpu_checks import CHAIN_CAMERA, CHAIN_LIGHTS, FORCED_MODES, ORIGIN, chain_main_rays, chain_rrt_lights, chain_scene, oracle_for, traced_rows
from ray_surface_checks import DTYPES, NAMES, SENTINEL, VECTORS, assert_miss_values, device_arrays, expected_ray_planes, rows, to_host
from scenes import CREATION, MOVED_EYE, TARGET, teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import MIRROR_ROOM_LIGHTS, mirror_room, soup_scene
from surface_checks import frame_dirs, traced_cols

pytestmark = pytest.mark.gpu

KEPT = ("t", "u", "v", "tri")                                    # what the call reads
OUTPUTS = NAMES[5:]                                              # what it writes: albedo, point, normal, material, lights, next_origin, next_dir
WALK_FREE = tuple(n for n in OUTPUTS if n != "lights")

W, H = 64, 48
RW, RH = 32, 24

T8 = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [-0.6, 0.0, 0.8], [0.0, 0.6, 0.8], [0.0, -0.6, 0.8], [0.8, 0.0, 0.6], [0.0, 0.8, 0.6], [-0.48, -0.64, 0.6]])


def kept_of(rt, O, D, M=None):
    """rrt_intersect_rays' five arrays as the planes dict rrt_resolve_hits reads"""
    hit, t, u, v, tri = rt.intersect_rays(O, D, M)
    return dict(hit=hit.astype(np.uint8), t=t, u=u, v=v, tri=tri)


def assert_resolves_to_the_fused_call(rt, O, D, M, what, min_hits, min_misses=1):
    """intersect -> resolve equals rrt_surface_rays' seven arrays; returns (kept, want)"""
    want = rt.surface_rays(O, D, M)
    kept = kept_of(rt, O, D, M)
    hit = want["hit"].astype(bool)
    assert_same_arrays(kept, want, ("hit",) + KEPT, f"{what}: intersect_rays vs surface_rays")
    assert hit.sum() >= min_hits and (~hit).sum() >= min_misses, f"{what}: {int(hit.sum())} hits, {int((~hit).sum())} misses"
    got = rt.resolve_hits(O, D, kept)
    assert tuple(got) == OUTPUTS
    assert_same_arrays(got, want, OUTPUTS, what)
    stats = rt.last_stats()
    assert (stats["width"], stats["height"], stats["rays_primary"]) == (len(D), 1, len(D)) and stats["kernel_ms"] > 0, stats
    return kept, want


@pytest.fixture(scope="module")
def rays4096(rrt, teapot):
    """4096 reflection rays off the teapot frame's hits -- none starts at the eye -- a quarter of them bounded at half their hit's t (a miss), a quarter beyond it;
    read-only."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    d = frame_dirs(CREATION, W, H).reshape(-1, 3)
    l0 = rt.surface_rays(np.broadcast_to(np.asarray(ORIGIN), d.shape), d, planes=("hit", "next_origin", "next_dir"))
    on = np.flatnonzero(l0["hit"])
    assert len(on) >= 4096, len(on)
    pick = on[np.linspace(0, len(on) - 1, 4096).astype(np.int64)]
    O, D = np.ascontiguousarray(l0["next_origin"][pick]), np.ascontiguousarray(l0["next_dir"][pick])
    t = rt.surface_rays(O, D, planes=("t",))["t"]
    k = np.arange(4096) % 4
    M = np.where(k == 1, 0.5 * t, np.where(k == 2, 2.0 * t + 1.0, np.inf))
    M[(t == 0.0) & (k == 1)] = 3.0                                # (a miss keeps a positive bound: 0.0 would be a dead ray)
    for a in (O, D, M):
        a.setflags(write=False)
    return O, D, M


@pytest.fixture(scope="module")
def teapot_expected(ob, rrt, teapot_arrays, rays4096):
    O, D, M = rays4096
    lights = rrt.default_lights()
    return expected_ray_planes(oracle_for(ob, teapot_arrays, lights), teapot_arrays, lights, O, D, M)


# ------------------------------------------------------------------ 1: equal to the fused call, and to the oracle
@pytest.mark.parametrize("mode", (None,) + FORCED_MODES)
def test_teapot_rays_resolve_to_the_fused_call_and_to_the_oracle(rrt, teapot, rays4096, teapot_expected, mode):
    O, D, M = rays4096
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    kept, want = assert_resolves_to_the_fused_call(rt, O, D, M, f"teapot, walk {mode}", 500, 500)
    hit, m = want["hit"].astype(bool), want["lights"]
    bounded_away = int((~hit & (np.arange(4096) % 4 == 1)).sum())
    dark = int((hit & ((m >> 1) & 1 == 0)).sum()), int((hit & ((m >> 2) & 1 == 0)).sum())
    assert bounded_away >= 100 and min(dark) >= 5, (bounded_away, dark)
    got = rt.resolve_hits(O, D, kept)
    assert_same_arrays(dict(kept, **got), teapot_expected, NAMES, f"teapot, walk {mode}: against the oracle")
    assert teapot_expected["bumped"].sum() >= 50, "no hit of the batch goes through a bump map"


def test_the_mirror_room_the_soup_and_the_chain_scene(rrt, ob, teapot_arrays):
    # the mirror room: no bump map, flat normals -- and level 1, the rays off its mirrors
    A = mirror_room()
    lights = [rrt.Light(k, i, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS]
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    d = frame_dirs(CREATION, RW, RH).reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(ORIGIN), d.shape))
    for mode in (None,) + FORCED_MODES:
        rt = rrt.RayTracer(sd, lights, box_filter=mode)
        _, l0 = assert_resolves_to_the_fused_call(rt, o, d, None, f"mirror room, walk {mode}", 2500, 0)
        assert_resolves_to_the_fused_call(rt, l0["next_origin"], l0["next_dir"], None, f"mirror room, level 1, walk {mode}", 2500, 0)
    # the soup: long own lists with group records; level 1 of the 32 x 24 frame
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode in (None,) + FORCED_MODES:
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode)
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records (clusters.cpp)"
        _, l0 = assert_resolves_to_the_fused_call(rt, o, d, None, f"soup, walk {mode}", 300, 0)          # (the soup fills the frame: the misses come at level 1)
        on = l0["hit"].astype(bool)
        assert_resolves_to_the_fused_call(rt, l0["next_origin"][on], l0["next_dir"][on], None, f"soup, level 1, walk {mode}", 300)
    # the chain scene, with and without the shortcut, against the oracle too
    A, _names = chain_scene("main")
    R = chain_main_rays()
    O = np.concatenate([r[0] for r in R.values()]); D = np.concatenate([r[1] for r in R.values()]); M = np.concatenate([r[2] for r in R.values()])
    ref = expected_ray_planes(oracle_for(ob, A, CHAIN_LIGHTS, CHAIN_CAMERA), A, CHAIN_LIGHTS, O, D, M)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode, shortcut in [(m, True) for m in FORCED_MODES] + [("bundle", False)]:
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*CHAIN_CAMERA), box_filter=mode, chain_shortcut=shortcut)
        kept, _ = assert_resolves_to_the_fused_call(rt, O, D, M, f"chain scene, walk {mode}, shortcut {shortcut}", 300)
        assert_same_arrays(rt.resolve_hits(O, D, kept), ref, OUTPUTS, f"chain scene, walk {mode}, shortcut {shortcut}: against the oracle")


# ------------------------------------------------------------------ 2: a frame's visibility buffer
@pytest.mark.parametrize("k", (0, 1), ids=["creation pose", f"eye {MOVED_EYE}"])
@pytest.mark.parametrize("w,h", [(64, 48), (97, 61)])
def test_a_frames_visibility_buffer_resolves_to_its_surface_buffer(rrt, teapot, w, h, k):
    cam = CREATION if k == 0 else rrt.look_at(MOVED_EYE, TARGET)
    names = ("albedo", "point", "normal", "material", "lights")
    for mode in (None,) + FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        rt.set_camera(**cam)
        vis = rt.visibility(w, h)
        want = dict(rt.surface(w, h), albedo=vis["albedo"])
        rays = rt.frame_rays(w, h, order=rrt.ORDER_ROWS)
        assert len(rays["dirs"]) == 4 * w * h
        got = rt.resolve_hits(rays["origins"], rays["dirs"], vis, outputs=names)
        got = {n: a.reshape((h, w, 4, 3) if n in VECTORS else (h, w, 4)) for n, a in got.items()}
        ix = np.ix_(traced_rows(h), traced_cols(w))
        hit = vis["hit"][ix].astype(bool)
        assert hit.mean() >= 0.4 and not hit.all(), f"{hit.mean():.3f} of the traced sub-samples hit"
        assert_same_arrays({n: a[ix] for n, a in got.items()}, {n: a[ix] for n, a in want.items()}, names, f"{w}x{h}, pose {k}, walk {mode}")
        untraced = np.ones((h, w), bool)
        untraced[ix] = False
        assert untraced.sum() == w * h - len(traced_rows(h)) * len(traced_cols(w)) and untraced[0].all() and (w % 2 == 0 or untraced[:, -1].all())
        assert_miss_values(got, untraced, f"{w}x{h}, pose {k}, walk {mode}: the pixels the reference never traces")


# ------------------------------------------------------------------ 3: the device forms


def sentinel_of(name, shape):
    return np.full(shape, SENTINEL[name], {np.uint8: np.uint8, np.float64: np.float64, np.uint32: np.int32}[DTYPES[name]]).view(DTYPES[name])


def test_what_is_not_asked_for_is_neither_written_nor_computed(rrt, teapot, rays4096):
    torch = pytest.importorskip("torch")
    O, D, M = (a[::3][:1000] for a in rays4096)                # (every third ray: the batch reaches from the sky above the teapot down to the floor)
    n = len(D)
    stream = torch.cuda.Stream()
    o_t, d_t = to_device(torch, O), to_device(torch, D)
    walk_free = {}
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        want = rt.surface_rays(O, D, M)
        assert 100 <= want["hit"].sum() <= 900
        kept_t = {name: to_device(torch, want[name]) for name in KEPT}
        torch.cuda.synchronize()
        subsets = [(name,) for name in OUTPUTS] + [("point", "material"), WALK_FREE, OUTPUTS]
        for subset in subsets:
            out = device_arrays(torch, n, OUTPUTS)
            planes = {k: t for k, t in kept_t.items() if k in ("t", "tri")} if subset == ("point", "material") else kept_t      # (u and v NULL)
            rt.resolve_hits_into({name: out[name] for name in subset}, o_t, d_t, planes, stream=stream.cuda_stream)
            stream.synchronize()
            got = to_host(out, n)
            assert_same_arrays(got, want, subset, f"walk {mode}, outputs {subset}")
            for name in set(OUTPUTS) - set(subset):
                assert same(got[name], sentinel_of(name, got[name].shape)), f"walk {mode}, outputs {subset}: array {name} was not passed and was written"
            if subset == WALK_FREE:
                walk_free[mode] = got
    for mode in FORCED_MODES[1:]:
        assert_same_arrays(walk_free[mode], walk_free[FORCED_MODES[0]], WALK_FREE, f"without lights, walk {mode} vs walk {FORCED_MODES[0]}")


SMALL_BOUNDS = (0, 1, 63, 64, 65, 128, 129, 130, 2 ** 32 - 1)    # on a batch of 129: n - 1, n, n + 1 among them


def test_the_counted_form_on_a_stream_of_its_own(rrt, teapot, rays4096):
    torch = pytest.importorskip("torch")
    n = 129
    O, D, M = (a[1000:1000 + n] for a in rays4096)
    stream = torch.cuda.Stream()
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        want = rt.surface_rays(O, D, M)
        hit = want["hit"].astype(bool)
        assert 10 <= hit.sum() <= 119 and 0 < hit[:64].sum() < 64, int(hit.sum())
        for m in SMALL_BOUNDS:
            mm = min(m, n)
            # beyond the bound: rays and t, u, v of 0xFF bytes (NaN), and a tri that IS a triangle -- an entry that was processed would not keep its sentinel
            o, d = O.copy(), D.copy()
            kept = {name: want[name].copy() for name in KEPT}
            for a in (o, d, kept["t"], kept["u"], kept["v"]):
                a[mm:] = np.frombuffer(b"\xff" * 8, np.float64)[0]
            kept["tri"][mm:] = 0
            out = device_arrays(torch, n, OUTPUTS)
            bound = torch.tensor([m - 2 ** 32 if m >= 2 ** 31 else m], dtype=torch.int32, device="cuda")
            tensors = to_device(torch, o), to_device(torch, d), {name: to_device(torch, a) for name, a in kept.items()}
            torch.cuda.synchronize()
            rt.resolve_hits_into(out, tensors[0], tensors[1], tensors[2], stream=stream.cuda_stream, bound_t=bound)
            stats = rt.last_stats()
            stream.synchronize()
            got = to_host(out, n)
            assert_same_arrays(rows(got, slice(0, mm)), rows(want, slice(0, mm)), OUTPUTS, f"walk {mode}, bound {m}: the first {mm} entries")
            for name in OUTPUTS:
                assert same(got[name][mm:], sentinel_of(name, got[name][mm:].shape)), f"walk {mode}, bound {m}: {name} was written at or beyond the bound"
            assert (stats["width"], stats["height"], stats["rays_primary"]) == (n, 1, n), stats


MISS_FILL = dict(albedo=0x00FFFFFF, point=0.0, normal=0.0, material=-1, lights=0, next_origin=0.0, next_dir=0.0)


def test_intersect_compact_resolve_scatter_is_the_fused_call(rrt, teapot, rays4096):
    """The split pipeline of rrt.h on one stream, with no host read of the count: rrt_intersect_rays_device, rrt_compact_rays_device with the hit bytes as the
    flag, rrt_resolve_hits_counted_device bounded by the count, seven scatters bounded by it -- from arrays that hold the miss values, the result is
    rrt_surface_rays_device on the raw batch."""
    torch = pytest.importorskip("torch")
    O, D, M = rays4096
    n = len(D)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o_t, d_t, m_t = to_device(torch, O), to_device(torch, D), to_device(torch, M)
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        want = rt.surface_rays(O, D, M)
        c = int(want["hit"].sum())
        assert 500 <= c <= n - 500, c
        raw = dict(hit=torch.empty(n, dtype=torch.uint8, device="cuda"), t=torch.empty(n, **f64), u=torch.empty(n, **f64), v=torch.empty(n, **f64), tri=torch.empty(n, **i32))
        packed = dict(origins=torch.full((3 * n,), np.nan, **f64), dirs=torch.full((3 * n,), np.nan, **f64), t=torch.full((n,), np.nan, **f64),
                      u=torch.full((n,), np.nan, **f64), v=torch.full((n,), np.nan, **f64), tri=torch.full((n,), 0, **i32))
        index, count = torch.full((n,), 7, **i32), torch.full((1,), -1, **i32)
        scratch = torch.empty(rt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        padded = device_arrays(torch, n, OUTPUTS)
        final = {name: torch.full((n * (3 if name in VECTORS else 1),), MISS_FILL[name], **(f64 if name in VECTORS else i32)) for name in OUTPUTS}
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        rt.intersect_rays_into(o_t, d_t, raw, m_t, stream=s)
        rt.compact_rays_into(packed, dict(origins=o_t, dirs=d_t, **{k: raw[k] for k in KEPT}), "flag", index, count, scratch, flag_t=raw["hit"], stream=s)
        rt.resolve_hits_into(padded, packed["origins"], packed["dirs"], {k: packed[k] for k in KEPT}, stream=s, bound_t=count)
        for name in OUTPUTS:
            rt.scatter_rays_into(index, padded[name], final[name], stream=s, bound_t=count)
        stream.synchronize()
        assert int(count.cpu().numpy().view(np.uint32)[0]) == c, f"walk {mode}"
        assert_same_arrays(to_host(final, n), want, OUTPUTS, f"walk {mode}: the split pipeline, scattered back, vs the fused call")
        got = to_host(padded, n)
        for name in OUTPUTS:
            assert same(got[name][c:], sentinel_of(name, got[name][c:].shape)), f"walk {mode}: the packed {name} was written beyond the count"


# ------------------------------------------------------------------ 4: edits are followed without a walk
def test_edits_are_followed_from_the_old_hits(rrt, teapot, teapot_arrays, rays4096):
    O, D, M = rays4096
    L, V = rrt.Light, rrt.Vector3d
    A = teapot_arrays
    lights = rrt.default_lights()
    for mode in (None, "bundle"):
        rt = rrt.RayTracer(teapot, lights, box_filter=mode)
        base = rt.surface_rays(O, D, M)
        old = {name: base[name] for name in KEPT}                                         # kept once, before every edit
        # a moved point light: only `lights` was stale
        moved = [lights[0], L.Point(0.4, V(6.0, 8.0, -12.0)), lights[2], lights[3]]
        rt.set_lights(moved)
        got = rt.resolve_hits(O, D, old)
        assert_same_arrays(got, rt.surface_rays(O, D, M), OUTPUTS, f"walk {mode}: a moved point light")
        assert (got["lights"] != base["lights"]).sum() >= 100
        assert_same_arrays(rt.resolve_hits(O, D, old, outputs=("lights",)), got, ("lights",), f"walk {mode}: lights alone")
        rt.set_lights(lights)
        # a bump map removed, a colour texture changed: albedo and normal were stale
        mats = [dict(m) for m in A["materials"]]
        assert mats[0]["bump"] >= 0 and mats[2]["tex"] != mats[0]["tex"], mats
        mats[0]["bump"] = -1
        mats[2]["tex"] = mats[0]["tex"]
        rt.set_materials(mats)
        got = rt.resolve_hits(O, D, old)
        assert_same_arrays(got, rt.surface_rays(O, D, M), OUTPUTS, f"walk {mode}: new materials")
        assert (got["albedo"] != base["albedo"]).sum() >= 50 and (got["normal"] != base["normal"]).any(1).sum() >= 50
        rt.set_materials(A["materials"])
        # a new pose: the rays are the caller's
        rt.set_camera(**rrt.look_at(MOVED_EYE, TARGET))
        assert_same_arrays(rt.resolve_hits(O, D, old), rt.surface_rays(O, D, M), OUTPUTS, f"walk {mode}: a new pose")
        assert_same_arrays(rt.resolve_hits(O, D, old), base, OUTPUTS, f"walk {mode}: everything as it was")


# ------------------------------------------------------------------ 5: edges
def test_edges_of_the_batch_and_of_the_values(rrt, teapot, teapot_arrays, rays4096):
    O, D, M = (a[::13][:300] for a in rays4096)
    n_tris = len(teapot_arrays["mat"])
    for mode in FORCED_MODES:
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        whole = rt.surface_rays(O, D, M)
        hit = whole["hit"].astype(bool)
        assert 30 <= hit.sum() <= 270 and 0 < hit[:129].sum() < 129 and 0 < hit[-129:].sum() < 129, int(hit.sum())
        for n in (1, 63, 64, 65, 129):
            for start in (0, 300 - n):
                sl = slice(start, start + n)
                assert_same_arrays(rt.resolve_hits(O[sl], D[sl], rows(whole, sl)), rows(whole, sl), OUTPUTS, f"walk {mode}: {n} entries from {start}")
        # misses only: nothing is walked, every array holds the miss values
        miss = np.flatnonzero(~hit)[:130]
        got = rt.resolve_hits(O[miss], D[miss], rows(whole, miss))
        assert_miss_values(got, slice(None), f"walk {mode}: misses only")
        # tri at the end of the table and beyond it, on entries that hit
        on = np.flatnonzero(hit)[:8]
        kept = {name: whole[name][on].copy() for name in KEPT}
        kept["tri"][:4] = (n_tris - 1, n_tris, n_tris + 1, 0xFFFFFFFF)
        got = rt.resolve_hits(O[on], D[on], kept)
        assert got["material"][0] == teapot_arrays["mat"][n_tris - 1] and same(got["point"][0], O[on][0] + D[on][0] * kept["t"][0]), f"walk {mode}: tri = n_tris - 1 is a hit"
        assert_miss_values(got, slice(1, 4), f"walk {mode}: tri = n_tris, n_tris + 1, 0xFFFFFFFF")
        assert_same_arrays(rows(got, slice(4, 8)), rows(whole, on[4:]), OUTPUTS, f"walk {mode}: the entries behind them")
        # NaN and infinities in t, u, v of some entries: the call returns, the other entries are exact
        kept = {name: whole[name].copy() for name in KEPT}
        bad = np.flatnonzero(hit)[::3]
        values = (np.nan, np.inf, -np.inf)
        for j, i in enumerate(bad):
            kept[("t", "u", "v")[j % 3]][i] = values[(j // 3) % 3]
        good = np.ones(300, bool)
        good[bad] = False
        got = rt.resolve_hits(O, D, kept)
        assert len(bad) >= 20 and (hit & good).sum() >= 40
        assert_same_arrays(rows(got, good), rows(whole, good), OUTPUTS, f"walk {mode}: the entries beside non-finite ones")
        assert same(got["material"][bad], whole["material"][bad]), f"walk {mode}: the material of an entry does not depend on t, u, v"


# ------------------------------------------------------------------ 6: downstream
def test_the_resolved_records_feed_shading_and_ambient_occlusion(rrt, teapot, rays4096):
    O, D, _ = rays4096
    for mode in (None, "ray"):
        rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
        rec = rt.resolve_hits(O, D, kept_of(rt, O, D))
        hit = rec["material"] != 0xFFFFFFFF
        assert 500 <= hit.sum() <= 3596, int(hit.sum())
        want = rt.get_ray_colours(O, D)
        assert same(rt.shade_rays(D, rec)["colour"], want), f"walk {mode}: shade_rays on the resolved records, with the mask, vs get_ray_colours"
        assert same(rt.shade_rays(D, {k: a for k, a in rec.items() if k != "lights"})["colour"], want), f"walk {mode}: ... without the mask"
        assert len(np.unique(want[hit])) >= 100
        fused = rt.surface_rays(O, D)
        a, b = rt.ambient_rays(rec, T8, 2.5), rt.ambient_rays(fused, T8, 2.5)
        assert same(a["occluded"], b["occluded"]) and same(a["open"], b["open"]) and (a["occluded"][hit] != 0).sum() >= 10, f"walk {mode}: ambient_rays"


# ------------------------------------------------------------------ 7: the table
def assert_table(rt, n_tris, what):
    """RRT_BUF_TRI_SLOT against RRT_BUF_ATTR (orig: the last word of a 128-byte record) and, where the set-up keeps it, RRT_BUF_SLOT_TRI; returns the table"""
    table = rt.buffer("tri_slot").view(np.uint32)
    attr = rt.buffer("attr").reshape(-1, 128)
    orig = attr[:, 124:128].copy().view(np.uint32).reshape(-1)
    slot_tri = rt.buffer("slot_tri").view(np.uint32)
    assert len(table) == n_tris and len(orig) > 0, f"{what}: {len(table)} entries for {n_tris} triangles"
    assert len(slot_tri) == 0 or same(slot_tri, orig), f"{what}: slot_tri is not the attribute records' orig"
    live = np.flatnonzero(orig != 0xFFFFFFFF)
    assert (orig[live] < n_tris).all()
    lowest = np.full(n_tris, 0xFFFFFFFF, np.uint32)
    np.minimum.at(lowest, orig[live], live.astype(np.uint32))
    assert same(table, lowest), f"{what}: the table is not the lowest slot of every triangle on {int((table != lowest).sum())} triangles"
    in_tree = table != 0xFFFFFFFF
    assert (orig[table[in_tree]] == np.flatnonzero(in_tree)).all(), f"{what}: a triangle's slot holds another triangle"
    assert (attr[live] == attr[table[orig[live]]]).all(), f"{what}: two slots of one triangle hold different attribute bytes"
    return table, int(in_tree.sum()), int(len(live) - in_tree.sum())


def test_the_triangle_to_slot_table(rrt, teapot, teapot_arrays):
    lights = rrt.default_lights()
    rt = rrt.RayTracer(teapot, lights)
    n = len(teapot_arrays["mat"])
    table, in_tree, second_slots = assert_table(rt, n, "teapot")
    assert in_tree == n and second_slots >= 1, f"teapot: {in_tree} of {n} triangles in the tree, {second_slots} second slots (inline leaves)"
    assert same(assert_table(rrt.RayTracer(teapot, lights), n, "teapot, created again")[0], table), "two creations give different tables"
    assert same(assert_table(rrt.RayTracer(teapot, lights, host_setup=True), n, "teapot, host set-up")[0], table), "the host set-up gives another table"
    A = soup_scene(teapot_arrays)
    soup = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    soup_table, in_tree, _ = assert_table(rrt.RayTracer(soup, lights), len(A["mat"]), "soup")
    assert in_tree == len(A["mat"])
    assert same(assert_table(rrt.RayTracer(soup, lights, host_setup=True), len(A["mat"]), "soup, host set-up")[0], soup_table)
    C, _names = chain_scene("main")
    chain = rrt.SceneData.from_arrays(C["pos"], C["uv"], C["nrm"], C["mat"], C["materials"], C["textures"])
    assert_table(rrt.RayTracer(chain, chain_rrt_lights(rrt), rrt.Vector3d(*CHAIN_CAMERA)), len(C["mat"]), "chain scene")
    # after set_triangles the table is the new scene's: the soup's triangles with the teapot's materials in force, and the old hits' triangle indices beyond it miss
    rt.set_triangles(A["pos"], A["uv"], A["nrm"], A["mat"])
    assert same(assert_table(rt, len(A["mat"]), "teapot -> soup by set_triangles")[0], soup_table)
    got = rt.resolve_hits(np.zeros((2, 3)), np.tile([0.0, 0.0, 1.0], (2, 1)), dict(t=np.ones(2), u=np.zeros(2), v=np.zeros(2), tri=np.array([len(A["mat"]) - 1, len(A["mat"])], np.uint32)))
    assert got["material"][0] == A["mat"][-1] and got["material"][1] == 0xFFFFFFFF
