"""The counted device forms (include/rrt.h: COUNTED DEVICE FORMS) on the GPU: the nine `_device` calls of the per-ray pipeline bound by a count that lives in
device memory, and the frame by ray generations as their first user.

The statement under test, with m = min(n, *d_count): entries [0, m) of every output are what the uncounted call with n = m writes, byte for byte; entries [m, n) of
every output keep the 0xA5 bytes they were prefilled with, and nothing in [m, n) of an input reaches the result -- each call runs twice, once with NaN / 0xFF bytes
there and once with entries that hit, and the two runs are byte-equal.  The bound is read on the device, in stream order.  The reference is the library's own
uncounted call and the numpy restatements of compact_checks.py and wavefront_checks.py.
"""
import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T
from ambient_rays_checks import INPUTS, OUTPUTS, standard_rot
from bitwise import assert_same_bits
from compact_checks import ARRAYS, DEAD_INDEX, NAMES, RECORD_NAMES, Guarded, compacted, flag_patterns, mixed_waves, scattered, selection, to_device
from gpu_checks import FORCED_MODES, chain_rrt_lights, chain_scene
from scenes import CREATION, rays_of, teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import MIRROR_ROOM_LIGHTS, mirror_room, soup_scene
from wavefront_checks import ORDERS, host, mix_case, mix_level

pytestmark = pytest.mark.gpu

W, H = 64, 48
RW, RH = 32, 24
T4 = np.ascontiguousarray(T8[:4])                                # the four samples of part 1's ambient fans
F8, U4, U1 = np.float64, np.uint32, np.uint8
# name -> (dtype, doubles or words per entry) of every array a per-ray call reads or writes
SHAPES = dict(origins=(F8, 3), dirs=(F8, 3), max_t=(F8, 1), rot=(F8, 2), colours=(U4, 1), shadow=(U1, 1), occluded=(U4, 1), colour=(U4, 1), local=(F8, 3), kr=(F8, 1), open=(U4, 1),
              **{name: ARRAYS[name][:2] for name in RECORD_NAMES})


def as_i32(v):
    return int(np.array([v], np.uint32).view(np.int32)[0])


def bound_tensor(torch, value):
    return torch.tensor([as_i32(value)], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------ the batch of parts 1, 2 and 3: the teapot's 64x48 frame rays in the creation pose
@pytest.fixture(scope="module")
def batch(rrt, teapot, teapot_arrays):
    """The rays tests/test_gpu_compact.py uses (the 12 032 the reference traces of the 64x48 frame), their level-0 records by the host form (made once, read-only), w = the first wave with hits and misses."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    O, D = rays_of(CREATION, W, H)
    n = len(D)
    max_t = np.linspace(50.0, 60.0, n)
    rec = rt.surface_rays(O, D, max_t)
    hit = rec["hit"].astype(bool)
    assert 0 < hit.sum() < n and mixed_waves(hit) >= 10, f"{int(hit.sum())} hits of {n}, {mixed_waves(hit)} waves with hits and misses"
    assert np.array_equal(hit, selection("hit", n_mats=len(teapot_arrays["materials"]), material=rec["material"]))
    waves = hit[:n // 64 * 64].reshape(-1, 64)
    w = int(np.flatnonzero(waves.any(1) & ~waves.all(1))[0])
    data = dict(origins=O, dirs=D, max_t=max_t, rot=standard_rot(n), **rec)
    for a in data.values():
        a.setflags(write=False)
    return dict(n=n, w=w, hit=hit, first_hit=int(np.flatnonzero(hit)[0]), data=data, n_mats=len(teapot_arrays["materials"]))


def bounds_of(n, w):
    return (0, 1, 64 * w, 64 * w + 1, 64 * w + 31, 64 * w + 63, 64 * w + 64, n - 1, n, n + 1, 0xFFFFFFFF)


# what each of the six ray calls reads, what it writes, and the call itself: call(rt, inputs, outputs, stream, bound_t) with {name: device tensor}
def _records(I, names):
    return {k: I[k] for k in names}


RAY_CALLS = {
    "intersect": (("origins", "dirs", "max_t"), ("hit", "t", "u", "v", "tri"),
                  lambda rt, I, O, s, b: rt.intersect_rays_into(I["origins"], I["dirs"], O, max_t_t=I["max_t"], stream=s, bound_t=b)),
    "get_ray_colours": (("origins", "dirs"), ("colours",),
                        lambda rt, I, O, s, b: rt.get_ray_colours_into(I["origins"], I["dirs"], O["colours"], stream=s, bound_t=b)),
    "occluded": (("origins", "dirs", "max_t"), ("shadow",),
                 lambda rt, I, O, s, b: rt.occluded_into(I["origins"], I["dirs"], O["shadow"], max_t_t=I["max_t"], stream=s, bound_t=b)),
    "surface": (("origins", "dirs", "max_t"), RECORD_NAMES,
                lambda rt, I, O, s, b: rt.surface_rays_into(I["origins"], I["dirs"], O, max_t_t=I["max_t"], stream=s, bound_t=b)),
    "shade": (("dirs", "albedo", "point", "normal", "material"), ("colour", "local", "kr"),          # (no mask: the shadow rays of the records' hits are walked)
              lambda rt, I, O, s, b: rt.shade_rays_into(O, I["dirs"], _records(I, ("albedo", "point", "normal", "material")), depth=0, stream=s, bound_t=b)),
    "ambient": (INPUTS, OUTPUTS,
                lambda rt, I, O, s, b: rt.ambient_rays_into(O, _records(I, INPUTS), T4, T8_MAX_T, stream=s, bound_t=b)),
    "ambient, rot": (INPUTS + ("rot",), OUTPUTS,
                     lambda rt, I, O, s, b: rt.ambient_rays_into(O, _records(I, INPUTS), T4, T8_MAX_T, rot_t=I["rot"], stream=s, bound_t=b)),
}


def run_ray_call(torch, rt, call, inputs, n, out_names, stream, bound=None):
    """One launch of `call` on the first n entries of the device inputs into guarded outputs of n entries prefilled with 0xA5: {name: flat host array}."""
    I = {k: t[:SHAPES[k][1] * n] for k, t in inputs.items()}
    out = {k: Guarded(torch, SHAPES[k][0], SHAPES[k][1] * n) for k in out_names}
    b = None if bound is None else bound_tensor(torch, bound)
    torch.cuda.synchronize()
    call(rt, I, {k: g.t for k, g in out.items()}, stream.cuda_stream, b)
    stream.synchronize()
    assert b is None or int(b.cpu().numpy().view(np.uint32)[0]) == bound, "the bound was written"
    return {k: g.read(k) for k, g in out.items()}


def assert_bounded(got, want, m, n, what):
    """got: outputs of n entries; [0, m) equals `want` (outputs of m entries), [m, n) is still 0xA5"""
    for k, a in got.items():
        width = SHAPES[k][1]
        assert len(a) == width * n
        if m:
            assert_same_bits(a[:width * m], want[k], f"{what}: {k} of the first {m} entries vs the uncounted call with n = {m}")
        tail = a[width * m:].view(np.uint8)
        assert (tail == 0xA5).all(), f"{what}: {k} was written at or beyond entry {m} ({int((tail != 0xA5).sum())} bytes)"


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("mode", FORCED_MODES)
@pytest.mark.parametrize("name", tuple(RAY_CALLS))
def test_a_counted_ray_call(rrt, teapot, batch, name, mode):
    torch = pytest.importorskip("torch")
    in_names, out_names, call = RAY_CALLS[name]
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    stream = torch.cuda.Stream()
    n, w, data = batch["n"], batch["w"], batch["data"]
    clean = {k: to_device(torch, data[k]) for k in in_names}
    for m in bounds_of(n, w):
        mm = min(m, n)
        what = f"{name}, walk {mode}, bound {m}"
        want = run_ray_call(torch, rt, call, clean, mm, out_names, stream) if mm else None
        runs = []
        for tail in ("0xFF", "hits"):
            host_in = {}
            for k in in_names:
                a = np.array(data[k]).reshape(n, -1)
                if tail == "0xFF":
                    a[mm:].view(np.uint8)[...] = 0xFF                # (doubles: a NaN; material: no material)
                else:
                    a[mm:] = a[batch["first_hit"]]                   # a ray that hits / the record of a hit
                host_in[k] = a
            dirty = {k: to_device(torch, a) for k, a in host_in.items()}
            got = run_ray_call(torch, rt, call, dirty, n, out_names, stream, bound=m)
            assert_bounded(got, want, mm, n, f"{what}, tail of the inputs = {tail}")
            runs.append(got)
        for k in out_names:
            assert_same_bits(runs[0][k], runs[1][k], f"{what}: {k}, the two runs")
        stats = rt.last_stats()
        assert (stats["width"], stats["height"], stats["rays_primary"]) == (n, 1, n), (what, stats)      # the host does not know m


# ------------------------------------------------------------------ 2
def test_the_bound_is_read_in_stream_order(rrt, teapot, batch):
    """torch writes 10 into the count, a counted call follows, torch writes 64w + 31, a second counted call into other outputs follows: one stream, no
    synchronisation in between, and each output obeys its own bound."""
    torch = pytest.importorskip("torch")
    in_names, out_names, call = RAY_CALLS["surface"]
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    n, w, data = batch["n"], batch["w"], batch["data"]
    inputs = {k: to_device(torch, data[k]) for k in in_names}
    setup = torch.cuda.Stream()
    full = run_ray_call(torch, rt, call, inputs, n, out_names, setup)
    outs = [{k: Guarded(torch, SHAPES[k][0], SHAPES[k][1] * n) for k in out_names} for _ in range(2)]
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    bounds = (10, 64 * w + 31)
    with torch.cuda.stream(stream):
        for m, out in zip(bounds, outs):
            count.fill_(m)
            call(rt, inputs, {k: g.t for k, g in out.items()}, stream.cuda_stream, count)
    stream.synchronize()
    for m, out in zip(bounds, outs):
        got = {k: g.read(k) for k, g in out.items()}
        assert_bounded(got, {k: full[k][:SHAPES[k][1] * m] for k in out_names}, m, n, f"the call enqueued behind the write of {m}")
    assert int(count.cpu()[0]) == bounds[1]


# ------------------------------------------------------------------ 3
def counted_compact(torch, rt, n, m, select, src, out_names, stream, flag=None):
    """rt.compact_rays_into with the bound m into guarded outputs; the bound and the output count are neighbouring words of one tensor."""
    src_t = {k: to_device(torch, a) for k, a in src.items()}
    flag_t = None if flag is None else to_device(torch, flag)
    out = {k: Guarded(torch, ARRAYS[k][0], ARRAYS[k][1] * n) for k in out_names}
    index, pair, scratch = Guarded(torch, U4, n), Guarded(torch, U4, 2), Guarded(torch, U1, rt.compact_scratch_bytes(n))
    pair.t[0] = as_i32(m)
    torch.cuda.synchronize()
    rt.compact_rays_into({k: g.t for k, g in out.items()}, src_t, select, index.t, pair.t[1:2], scratch.t, flag_t=flag_t, stream=stream.cuda_stream, bound_t=pair.t[0:1])
    stream.synchronize()
    scratch.read("scratch")
    words = pair.read("bound and count")
    assert int(words[0]) == m, "the bound was written"
    return dict({k: g.read(k) for k, g in out.items()}, index=index.read("index"), count=words[1:2])


def assert_counted_compaction(got, sel, src, n, m, what, synth_max_t=False):
    mm = min(m, n)
    if mm == 0:
        assert int(got["count"][0]) == 0, f"{what}: count {int(got['count'][0])} with nothing below the bound"
        want = {}
    else:
        want = compacted(np.asarray(sel)[:mm], {k: np.asarray(a)[:mm] for k, a in src.items()}, synth_max_t=synth_max_t)
        assert int(got["count"][0]) == want["count"], f"{what}: count {int(got['count'][0])} vs {want['count']}"
    for k, a in got.items():
        if k == "count":
            continue
        width = 1 if k == "index" else ARRAYS[k][1]
        if mm:
            assert_same_bits(a[:width * mm].reshape(np.asarray(want[k]).shape), want[k], f"{what}: {k} below the bound")
        tail = a[width * mm:].view(np.uint8)
        assert (tail == 0xA5).all(), f"{what}: {k} was written at or beyond entry {mm}"
    return want.get("count", 0)


SMALL = 3 * 1024 + 17
COMPACT_BOUNDS = {SMALL: (0, 1, 1023, 1024, 1025, 2048, SMALL - 1, SMALL, 5000), 300001: (7, 262145)}     # 262145: one entry behind the 256th tile, the scan's second pass


@pytest.mark.parametrize("n", tuple(COMPACT_BOUNDS))
def test_a_counted_compaction_by_flag(rrt, teapot, n):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.render(16, 12)
    stats = rt.last_stats()
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(n)
    tri = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U4)
    point = rng.standard_normal((n, 3))
    for what, flag in flag_patterns(n).items():
        for m in COMPACT_BOUNDS[n]:
            got = counted_compact(torch, rt, n, m, "flag", dict(tri=tri, point=point), ("tri", "point"), stream, flag=flag)
            assert_counted_compaction(got, flag != 0, dict(tri=tri, point=point), n, m, f"n = {n}, bound {m}, {what}")
    assert rt.last_stats() == stats, "a counted compaction touched rrt_last_stats"


@pytest.mark.parametrize("n", tuple(COMPACT_BOUNDS))
def test_a_counted_compaction_by_hit_with_all_sixteen_arrays(rrt, teapot, batch, n):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    stream = torch.cuda.Stream()
    at = (64 * batch["w"] + np.arange(n)) % batch["n"]              # (the frame's records from wave w on, repeated for the large batch)
    src = {k: np.ascontiguousarray(batch["data"][k][at]) for k in NAMES}
    sel = selection("hit", n_mats=batch["n_mats"], material=src["material"])
    assert 0 < sel[:64].sum() < 64, "the first wave needs survivors and dead entries"
    for m in COMPACT_BOUNDS[n]:
        got = counted_compact(torch, rt, n, m, "hit", src, NAMES, stream)
        count = assert_counted_compaction(got, sel, src, n, m, f"HIT, n = {n}, bound {m}")
        assert m < 64 or 0 < count < min(m, n)
    # a synthesised bound: +inf for the survivors, NaN for the dead slots below the bound, nothing beyond it
    less = {k: src[k] for k in ("origins", "material")}
    m = COMPACT_BOUNDS[n][-1] - 3
    src_t = {k: to_device(torch, a) for k, a in less.items()}
    out = dict(origins=Guarded(torch, F8, 3 * n), max_t=Guarded(torch, F8, n))
    count, scratch = Guarded(torch, U4, 1), Guarded(torch, U1, rt.compact_scratch_bytes(n))
    torch.cuda.synchronize()
    rt.compact_rays_into({k: g.t for k, g in out.items()}, src_t, "hit", None, count.t, scratch.t, stream=stream.cuda_stream, bound_t=bound_tensor(torch, m))
    stream.synchronize()
    got = dict({k: g.read(k) for k, g in out.items()}, count=count.read("count"))
    assert_counted_compaction(got, sel, dict(origins=less["origins"]), n, m, f"HIT, n = {n}, bound {m}, max_t synthesised", synth_max_t=True)


# ------------------------------------------------------------------ 4
SMALL_BOUNDS = (0, 1, 63, 64, 65, 199, 200, 300)


@pytest.mark.parametrize("elem", (1, 4, 8, 16, 24))
def test_a_counted_scatter(rrt, teapot, elem):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    stream = torch.cuda.Stream()
    n = 200
    rng = np.random.default_rng(elem)
    dtype, width = {1: (U1, 1), 4: (U4, 1), 8: (F8, 1), 16: (F8, 2), 24: (F8, 3)}[elem]
    shape = (n, width) if width > 1 else (n,)
    src = rng.integers(0, 256, n * elem, dtype=U1).view(dtype).reshape(shape)
    dst = np.full(n * elem, 0xA5, U1).view(dtype).reshape(shape)
    index = rng.permutation(n).astype(U4)                           # every j names a position of its own, in range: one that is read is seen in dst
    index[2::9] = DEAD_INDEX
    index[5::13] = n + np.arange(len(index[5::13]), dtype=U4) * 7   # n itself first: the smallest index that is skipped
    assert index[n - 1] < n
    index_t, src_t = to_device(torch, index), to_device(torch, src)
    for m in SMALL_BOUNDS:
        mm = min(m, n)
        below = np.arange(n) < mm
        assert mm == n or (index[~below] < n).sum() >= 1, "no index beyond the bound would be seen"
        assert not 63 <= mm <= 65 or ((index[below] >= mm) & (index[below] < n)).any(), "no index below the bound names a position at or beyond it"
        want = scattered(np.where(below, index, DEAD_INDEX), src, dst)           # the contract's scatter on the first m: an index beyond them is not read
        g = Guarded(torch, dtype, n * width)
        g.t.copy_(to_device(torch, dst))
        torch.cuda.synchronize()
        rt.scatter_rays_into(index_t, src_t, g.t, stream=stream.cuda_stream, bound_t=bound_tensor(torch, m))
        stream.synchronize()
        assert_same_bits(g.read(f"elem_bytes {elem}").reshape(shape), want, f"elem_bytes {elem}, bound {m}")


# ------------------------------------------------------------------ 5
def test_a_counted_mix(rrt, teapot, batch):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    stream = torch.cuda.Stream()
    n, n_mats = 200, batch["n_mats"]
    local, kr, reflected, material = mix_case(n, n_mats)
    full = mix_level(local, kr, reflected, material, n_mats)
    assert (full[190:] != mix_level(local, None, None, material, n_mats)[190:]).any(), "nothing near the end of the batch mixes"
    tensors = [to_device(torch, a) for a in (local, kr, reflected, material)]
    for what, (k, r, mt) in {"all arrays": (1, 2, 3), "no material": (1, 2, None), "local alone": (None, None, None)}.items():
        pick = lambda i, arrays: None if i is None else arrays[i]
        for m in SMALL_BOUNDS:
            mm = min(m, n)
            host_arrays = (local, kr, reflected, material)
            want = mix_level(local[:mm], *(None if i is None else host_arrays[i][:mm] for i in (k, r, mt)), n_mats) if mm else np.zeros(0, U4)
            g = Guarded(torch, U4, n)
            torch.cuda.synchronize()
            rt.mix_rays_into(g.t, tensors[0], kr_t=pick(k, tensors), reflected_t=pick(r, tensors), material_t=pick(mt, tensors), stream=stream.cuda_stream,
                             bound_t=bound_tensor(torch, m))
            stream.synchronize()
            got = g.read("colour")
            assert_same_bits(got[:mm], want, f"mix, {what}, bound {m}: the first {mm} entries vs the restatement")
            assert (got[mm:] == 0xA5A5A5A5).all(), f"mix, {what}, bound {m}: an entry at or beyond the bound was written"


# ------------------------------------------------------------------ 6
def assert_counted_pipeline(torch, rrt, make_rt, O, D, n_mats, what):
    """surface -> compact (HIT, count c) -> ambient counted by c -> two scatters counted by c, on one stream with no synchronisation; from occluded = 0 and
    open = n_samples the result is rrt_ambient_rays on the raw records, bit for bit, in every forced walk."""
    n = len(D)
    rot = standard_rot(n)
    for mode in FORCED_MODES:
        rt = make_rt(mode)
        rec = rt.surface_rays(O, D, planes=INPUTS)
        hit = selection("hit", n_mats=n_mats, material=rec["material"])
        c = int(hit.sum())
        assert 0 < c < n and mixed_waves(hit) >= 1, f"{what}: {c} hits of {n} records"
        want = rt.ambient_rays(rec, T8, T8_MAX_T, rot=rot)
        assert (want["occluded"] != 0).any() and (want["open"][hit] < len(T8)).any(), f"{what}: the reference masks are all empty"
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        o_t, d_t, rot_t = to_device(torch, O), to_device(torch, D), to_device(torch, rot)
        raw = dict(point=torch.empty(3 * n, **f64), normal=torch.empty(3 * n, **f64), material=torch.empty(n, **i32))
        packed = dict(rot=torch.full((2 * n,), np.nan, **f64), **{k: torch.full_like(t, -1) for k, t in raw.items()})      # (beyond c: NaN and 0xFF bytes)
        index, count = torch.full((n,), 7, **i32), torch.full((1,), -1, **i32)
        scratch = torch.empty(rt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        padded = {k: Guarded(torch, U4, n) for k in OUTPUTS}
        final = dict(occluded=torch.zeros(n, **i32), open=torch.full((n,), len(T8), **i32))
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        rt.surface_rays_into(o_t, d_t, raw, stream=s)
        rt.compact_rays_into(packed, dict(rot=rot_t, **raw), "hit", index, count, scratch, stream=s)
        rt.ambient_rays_into({k: g.t for k, g in padded.items()}, {k: packed[k] for k in INPUTS}, T8, T8_MAX_T, rot_t=packed["rot"], stream=s, bound_t=count)
        for k in OUTPUTS:
            rt.scatter_rays_into(index, padded[k].t, final[k], stream=s, bound_t=count)
        stream.synchronize()
        assert int(count.cpu().numpy().view(U4)[0]) == c, f"{what}, walk {mode}"
        for k in OUTPUTS:
            assert_same_bits(host(final[k], U4, (n,)), want[k], f"{what}, walk {mode}: {k}, scattered back, vs rrt_ambient_rays on the raw records")
            got = padded[k].read(k)
            assert_same_bits(got[:c], want[k][hit], f"{what}, walk {mode}: the padded {k} below the count")
            assert (got[c:] == 0xA5A5A5A5).all(), f"{what}, walk {mode}: the padded {k} was written beyond the count"


def with_level_1(rt, O, D):
    """The rays and behind them the reflection rays of their hits: rays that leave the scene among them"""
    l0 = rt.surface_rays(O, D, planes=("hit", "next_origin", "next_dir"))
    h0 = l0["hit"].astype(bool)
    return np.ascontiguousarray(np.concatenate([O, l0["next_origin"][h0]])), np.ascontiguousarray(np.concatenate([D, l0["next_dir"][h0]]))


def test_a_counted_pipeline_on_the_teapot(rrt, teapot, batch):
    torch = pytest.importorskip("torch")
    assert_counted_pipeline(torch, rrt, lambda mode: rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), np.array(batch["data"]["origins"]),
                            np.array(batch["data"]["dirs"]), batch["n_mats"], "teapot")


def test_a_counted_pipeline_on_a_soup_with_group_records(rrt, teapot_arrays):
    torch = pytest.importorskip("torch")
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    rt = rrt.RayTracer(sd, rrt.default_lights())
    supers = rt.buffer("supers").view(U4).reshape(-1, 8)
    assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records"
    O, D = with_level_1(rt, *rays_of(CREATION, RW, RH))
    assert_counted_pipeline(torch, rrt, lambda mode: rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode), O, D, len(A["materials"]), "soup")


def test_a_counted_pipeline_on_the_chain_scene(rrt):
    torch = pytest.importorskip("torch")
    A, names = chain_scene("main")
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])

    def make(mode):
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*eye), box_filter=mode)
        rt.set_camera(**cam)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        return rt
    O, D = with_level_1(make(None), *rays_of(cam, RW, RH))
    assert_counted_pipeline(torch, rrt, make, O, D, len(A["materials"]), "chain scene")


# ------------------------------------------------------------------ 7
def alive_per_level(rt, w, h, levels):
    """The compaction counts of the frame's generations by host calls: [mirror hits of level 0, of level 1, ...]"""
    rays = rt.frame_rays(w, h)
    O, D, M = rays["origins"], rays["dirs"], rays["max_t"]
    alive = []
    for _ in range(levels):
        rec = rt.surface_rays(O, D, M, planes=("material", "next_origin", "next_dir"))
        nxt = rt.compact_rays(dict(material=rec["material"]), "mirror", origins=rec["next_origin"], dirs=rec["next_dir"], max_t=True)
        alive.append(nxt["count"])
        O, D, M = nxt["origins"], nxt["dirs"], nxt["max_t"]
    return alive


def assert_the_driver_reads_only_what_it_wrote(torch, rrt, rt, what):
    """render_wavefront_into at 64x48 and 5x3 in both orders with the work memory prefilled with 0x00 (reads as a valid material, index 0 and kr 0.0), 0xA5 and 0xFF
    (reads as dead everywhere): three equal frames, equal to render's."""
    stream = torch.cuda.Stream()
    for w, h in ((W, H), (5, 3)):
        want = rt.render(w, h)
        for order in ORDERS:
            need = rt.wavefront_work_bytes(w, h, None, order)
            frames = []
            for fill in (0x00, 0xA5, 0xFF):
                with torch.cuda.stream(stream):
                    work = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
                    fb = torch.full((w * h,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                    rt.render_wavefront_into(fb, work, w, h, order=order, stream=stream.cuda_stream)
                stream.synchronize()
                frames.append(host(fb, U4, (h, w)))
                assert_same_bits(frames[-1], want, f"{what}, {w}x{h}, order {order}, work memory of {fill:#04x} bytes: render_wavefront_into vs render")
            assert (frames[0] == frames[1]).all() and (frames[1] == frames[2]).all()


@pytest.mark.parametrize("depth", (0, 1, 5))
def test_the_driver_on_the_mirror_room(rrt, depth):
    torch = pytest.importorskip("torch")
    A = mirror_room()
    lights = [rrt.Light(k, i, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS]
    rt = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), lights, max_reflection_depth=depth)
    if depth == 5:
        alive = alive_per_level(rt, W, H, 5)
        assert alive[4] >= 1000 and all(a >= b for a, b in zip(alive, alive[1:])), f"the mirror room's rays alive per level: {alive}"
    assert_the_driver_reads_only_what_it_wrote(torch, rrt, rt, f"mirror room, depth {depth}")


def test_the_driver_on_the_teapot(rrt, teapot):
    torch = pytest.importorskip("torch")
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    alive = alive_per_level(rt, W, H, 5)
    print(f"the teapot's rays alive at levels 1 to 5: {alive}")
    assert alive[0] > 0 and alive[-1] == 0, f"the teapot's rays alive at levels 1 to 5: {alive} (its chains are meant to end before the depth limit)"
    assert_the_driver_reads_only_what_it_wrote(torch, rrt, rt, "teapot")


def test_the_driver_on_a_soup(rrt, teapot_arrays):
    """The soup as the other tests trace it, and with every kr = 0: nothing is alive at level 1, and the path of an empty batch runs for five levels."""
    torch = pytest.importorskip("torch")
    A = soup_scene(teapot_arrays)
    rt = rrt.RayTracer(rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"]), rrt.default_lights())
    assert_the_driver_reads_only_what_it_wrote(torch, rrt, rt, "soup")
    rt.set_materials([dict(m, kr=0.0) for m in rt.materials()])
    assert alive_per_level(rt, W, H, 1) == [0], "a soup without mirrors has rays alive at level 1"
    assert_the_driver_reads_only_what_it_wrote(torch, rrt, rt, "soup, every kr = 0")
