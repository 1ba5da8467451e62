"""Ambient occlusion from kept surface buffers (include/rrt.h: rrt_ambient_surface, rrt_ambient_surface_device) on the GPU.

The statement under test: bit k of the `occluded` plane of a hit IS what rrt_occluded_rays returns for the ray the contract defines -- origin = point + normal *
surface_offset, direction = (tg*sx + bt*sy) + n*sz in the reference's tangent frame, the call's max_t -- bit for bit, in every traversal variant; `grey` is the
contract's integer formula of that plane.  The rays are restated in numpy from the planes of rt.surface() (ambient_checks.py).  Every comparison asserts its
conditions BY THE REFERENCE ANSWERS, so an empty result cannot pass.

Two sets of planes carry part 1.  The teapot as loaded: three of its four materials have a bump map, so no normal of its frame is exactly (0, 1, 0) and no hit
takes the length(tg) == 0 branch of the tangent frame (0 such hits by the oracle's exact planes).  The same teapot with its bump maps switched off: the table top
then has the normal (0, 1, 0) and 2405 hits take that branch.  The oracle, run on the CPU for the 64x48 frame with T8 and max_t 2.0, gave
  as loaded:       hit fraction 0.594, occluded fraction 0.435, per sample 0.380-0.563 occluded, 0 fallback hits;
  bump maps off:   hit fraction 0.594, occluded fraction 0.143, per sample 0.064-0.387 occluded, 2405 fallback hits.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from ambient_checks import H, T8, T8_MAX_T, W, Rays, by_oracle, by_shadow_query, crop, freeze, grey_of, popcount, traced_mask
from bitwise import assert_same_arrays, assert_same_bits
from gpu_checks import ALL_MODES, CHAIN_LIGHTS, FORCED_MODES, chain_rrt_lights, chain_scene, oracle_for
from scenes import teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import soup_scene
from surface_checks import NO_MATERIAL, traced_pixels_in

pytestmark = pytest.mark.gpu

INF = float("inf")
INPUTS = ("point", "normal", "material")
SCENES = ("teapot", "teapot, bump maps off")
W2, H2 = 97, 61
REGION = (5, 3, 41, 30)


@pytest.fixture(scope="module")
def scenes(rrt, teapot, teapot_arrays):
    """name -> (SceneData, arrays): the teapot as loaded, and with bump = -1 in every material."""
    A = teapot_arrays
    flat = copy.deepcopy(A["materials"])
    assert sum(m["bump"] >= 0 for m in flat) >= 1
    for m in flat:
        m["bump"] = -1
    return {SCENES[0]: (teapot, A), SCENES[1]: (rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], flat, A["textures"]), dict(A, materials=flat))}


@pytest.fixture(scope="module")
def kept(rrt, scenes):
    """name -> (raytracer in the default mode, its planes of the 64x48 frame, the rays of T8 from them, the `occluded` plane of T8 at max_t 2.0 by rt.occluded); read-only."""
    out = {}
    for name, (sd, A) in scenes.items():
        rt = rrt.RayTracer(sd, rrt.default_lights())
        planes = rt.surface(W, H, planes=INPUTS)
        rays = Rays(planes, len(A["materials"]), T8)
        want = by_shadow_query(rt, rays, T8_MAX_T)
        freeze(want, *planes.values())
        out[name] = (rt, planes, rays, want)
    return out


def mask_figures(plane, rays):
    """(occluded fraction of all rays, per-sample occluded fraction [n]) over the hits, from an `occluded` plane."""
    m = plane[rays.hit]
    per = np.array([float(((m >> np.uint32(k)) & np.uint32(1)).mean()) for k in range(rays.n)])
    return float(popcount(m).sum()) / (m.size * rays.n), per


def assert_caps(plane, rays, what):
    frac, per = mask_figures(plane, rays)
    print(f"{what}: hit fraction {rays.hit.mean():.3f}, occluded fraction {frac:.3f}, per sample {per.min():.3f}-{per.max():.3f}, {int(rays.fallback.sum())} fallback hits")
    assert rays.hit.mean() >= 0.5, f"{what}: hit fraction {rays.hit.mean():.3f} (< 0.5)"
    assert frac >= 0.05, f"{what}: occluded fraction {frac:.3f} (< 0.05)"
    assert per.min() >= 0.02 and (1.0 - per).min() >= 0.40, f"{what}: per sample {per.tolist()}: want each occluded on >= 2 % and open on >= 40 % of the hits"


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("max_t", (T8_MAX_T, INF))
@pytest.mark.parametrize("name", SCENES)
def test_the_mask_is_the_shadow_query(rrt, ob, scenes, kept, name, max_t):
    sd, A = scenes[name]
    _, planes, rays, _ = kept[name]
    if name == SCENES[1]:
        print(f"{name}: {int(rays.fallback.sum())} hits take the length(tg) == 0 branch")
        assert rays.fallback.sum() >= 1000, f"{name}: {int(rays.fallback.sum())} hits take the length(tg) == 0 branch (< 1000)"
    for mode in ALL_MODES:
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode)
        assert_same_arrays(rt.surface(W, H, planes=INPUTS), planes, INPUTS, f"{name}, walk {mode}: the planes the rays were formed from")
        want = by_shadow_query(rt, rays, max_t)
        if max_t == T8_MAX_T:
            assert_caps(want, rays, f"{name}, walk {mode}, by rrt_occluded_rays")
        assert (want != 0).any() and (popcount(want[rays.hit]) < rays.n).any(), f"{name}, walk {mode}, max_t {max_t}: the reference masks are all empty or all full"
        got = rt.ambient(W, H, planes, T8, max_t, outputs=("occluded",))
        assert_same_bits(got["occluded"], want, f"{name}, walk {mode}, max_t {max_t}: occluded vs rrt_occluded_rays")
        if mode == "lane" and max_t == T8_MAX_T and name == SCENES[0]:
            ref = by_oracle(oracle_for(ob, A, rrt.default_lights()), rays, max_t)
            assert_caps(ref, rays, f"{name}, by the oracle")
            assert_same_bits(got["occluded"], ref, f"{name}, walk {mode}, max_t {max_t}: occluded vs the oracle's intersector")


# ------------------------------------------------------------------ 2
def test_sample_counts(kept):
    rt, planes, rays, want = kept[SCENES[0]]
    one = rt.ambient(W, H, planes, T8[:1], T8_MAX_T, outputs=("occluded",))["occluded"]
    assert (want & np.uint32(1)).any() and not (want[rays.hit] & np.uint32(1)).all()
    assert_same_bits(one, want & np.uint32(1), "n = 1: bit 0 of the mask of T8")
    full = rt.ambient(W, H, planes, np.tile(T8, (4, 1)), T8_MAX_T, outputs=("occluded",))["occluded"]
    assert (want >> np.uint32(7)).any(), "sample 7 is never occluded: bit 31 would show nothing"
    assert_same_bits(full, want * np.uint32(0x01010101), "n = 32, T8 four times: the mask of T8 in every byte")


# ------------------------------------------------------------------ 3
@pytest.fixture(scope="module")
def odd_frame(rrt, teapot, teapot_arrays):
    """A raytracer, its planes of the 97x61 frame and both outputs of T8 at max_t 2.0 over the whole frame (read-only)."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    planes = rt.surface(W2, H2, planes=INPUTS)
    out = rt.ambient(W2, H2, planes, T8, T8_MAX_T)
    freeze(*planes.values(), *out.values())
    return rt, planes, out


def test_an_odd_frame(odd_frame, teapot_arrays):
    rt, planes, out = odd_frame
    rays = Rays(planes, len(teapot_arrays["materials"]), T8)
    want = by_shadow_query(rt, rays, T8_MAX_T)
    assert rays.hit.mean() >= 0.4 and (want != 0).sum() >= 1000, (rays.hit.mean(), int((want != 0).sum()))
    assert_same_bits(out["occluded"], want, f"{W2}x{H2}: occluded vs rrt_occluded_rays")
    traced = traced_mask(W2, H2)
    assert not traced[0].any() and not traced[1].any() and not traced[:, -1].any() and traced[2:, :-1].all()
    assert (out["occluded"][~traced] == 0).all() and (out["grey"][~traced] == 0).all(), "row 0, row 1 and the last column of an odd-sized frame are 0 in both outputs"
    assert (out["grey"][traced] != 0).any()
    assert_same_bits(out["grey"], grey_of(want, planes["material"], len(teapot_arrays["materials"]), 8, traced), f"{W2}x{H2}: grey vs the integer formula")


def test_a_region_is_a_crop_of_the_frame(odd_frame):
    rt, full_planes, full = odd_frame
    busy = np.argwhere((full["occluded"] != 0).all(-1) & (popcount(full["occluded"]) < 8).all(-1))
    assert len(busy) >= 1, "no pixel whose four sub-samples all have some rays occluded and some open"
    py, px = (int(v) for v in busy[len(busy) // 2])
    for region in (REGION, (px, py, 1, 1), (W2 - 3, 0, 3, 3)):
        x0, y0, w, h = region
        part = rt.surface(W2, H2, region=region, planes=INPUTS)
        assert_same_arrays(part, crop(full_planes, region), INPUTS, f"region {region}: planes")
        got = rt.ambient(W2, H2, part, T8, T8_MAX_T, region=region)
        stats = rt.last_stats()
        for n in ("occluded", "grey"):
            assert_same_bits(got[n], full[n][y0:y0 + h, x0:x0 + w], f"region {region}: {n} vs the crop of the whole frame")
        assert (stats["width"], stats["height"], stats["rays_primary"]) == (W2, H2, 4 * traced_pixels_in(region, W2, H2)) and stats["kernel_ms"] > 0, (region, stats)
    assert (full["occluded"][3:33, 5:46] != 0).sum() >= 500, "the region of the test shows few occluded rays"


# ------------------------------------------------------------------ 4
def test_grey(kept, teapot_arrays):
    rt, planes, rays, want = kept[SCENES[0]]
    n_mats = len(teapot_arrays["materials"])
    traced = traced_mask(W, H)
    got = rt.ambient(W, H, planes, T8, T8_MAX_T)
    assert_same_bits(got["occluded"], want, "both outputs asked for: occluded")
    assert_same_bits(got["grey"], grey_of(got["occluded"], planes["material"], n_mats, 8, traced), "grey vs the integer formula of the occluded and material planes")
    only = rt.ambient(W, H, planes, T8, T8_MAX_T, outputs=("grey",))
    assert set(only) == {"grey"}
    assert_same_bits(only["grey"], got["grey"], "grey alone vs grey beside occluded")
    levels = np.unique(got["grey"][traced])
    print(f"grey: {len(levels)} levels among the traced pixels, {levels.min():#08x} to {levels.max():#08x}")
    assert len(levels) >= 16 and levels.max() == 0x00FFFFFF
    # a wave of misses only -- an aligned block of 4 x 4 traced pixels -- leaves without walking: its pixels are white, its masks 0
    blocks = ((planes["material"] >= n_mats).all(-1) & traced).reshape(H // 4, 4, W // 4, 4).all((1, 3))
    assert blocks.any(), "no aligned 4x4 block of traced pixels is all misses"
    by, bx = (int(v) for v in np.argwhere(blocks)[0])
    assert (got["grey"][4 * by:4 * by + 4, 4 * bx:4 * bx + 4] == 0x00FFFFFF).all() and (got["occluded"][4 * by:4 * by + 4, 4 * bx:4 * bx + 4] == 0).all(), (by, bx)
    # hit samples with material = n_mats (and 0xFFFFFFFF) count as open and have mask 0; nothing else moves
    edited = dict(planes, material=planes["material"].copy())
    a, b = (slice(16, 24), slice(24, 40)), (slice(28, 36), slice(8, 20))
    shadowed = lambda s: int((want[s] != 0).sum())
    assert shadowed(a) >= 32 and shadowed(b) >= 32, f"the edited blocks hold {shadowed(a)} and {shadowed(b)} sub-samples with an occluded ray: the edit shows little"
    edited["material"][a] = n_mats
    edited["material"][b] = NO_MATERIAL
    want_edit = want.copy()
    want_edit[a] = 0
    want_edit[b] = 0
    again = rt.ambient(W, H, edited, T8, T8_MAX_T)
    assert_same_bits(again["occluded"], want_edit, "material = n_mats and 0xFFFFFFFF in two blocks: occluded")
    assert_same_bits(again["grey"], grey_of(want_edit, edited["material"], n_mats, 8, traced), "material = n_mats and 0xFFFFFFFF in two blocks: grey")
    assert (again["grey"][a] == 0x00FFFFFF).all() and (again["grey"][b] == 0x00FFFFFF).all()


# ------------------------------------------------------------------ 5
def assert_walks(rrt, make_rt, n_mats, what, modes):
    ref_rt = make_rt(modes[0][0], modes[0][1])
    planes = ref_rt.surface(W, H, planes=INPUTS)
    rays = Rays(planes, n_mats, T8)
    for mode, kw in modes:
        rt = make_rt(mode, kw)
        assert_same_arrays(rt.surface(W, H, planes=INPUTS), planes, INPUTS, f"{what}, walk {mode} {kw}: the planes the rays were formed from")
        want = by_shadow_query(rt, rays, T8_MAX_T)
        n_bits = int(popcount(want).sum())
        print(f"{what}, walk {mode} {kw}: {int(rays.hit.sum())} hits, {n_bits} of {int(rays.hit.sum()) * 8} rays occluded by rrt_occluded_rays")
        assert n_bits >= 100 and n_bits < int(rays.hit.sum()) * 8, f"{what}, walk {mode}: {n_bits} occluded rays by the reference"
        got = rt.ambient(W, H, planes, T8, T8_MAX_T)
        assert_same_bits(got["occluded"], want, f"{what}, walk {mode} {kw}: occluded vs rrt_occluded_rays")
        assert_same_bits(got["grey"], grey_of(want, planes["material"], n_mats, 8, traced_mask(W, H)), f"{what}, walk {mode} {kw}: grey")
        yield rt


def test_a_soup_with_long_own_lists(rrt, teapot_arrays):
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    make = lambda mode, kw: rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, **kw)
    modes = [(m, {}) for m in FORCED_MODES] + [(None, dict(no_cull=True))]
    for rt, (mode, kw) in zip(assert_walks(rrt, make, len(A["materials"]), "soup", modes), modes):
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert len(supers) > 0
        if not kw:
            assert (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records (clusters.cpp): the kernels' group instantiation did not run"


def test_the_chain_shortcut_scene(rrt):
    """The hand-built chain scene that holds the triangle `big` (gpu_checks.chain_scene("main")), seen as tests/test_gpu_shade.py sees it."""
    A, names = chain_scene("main")
    assert "big" in names
    eye = (2.5, 2.5, -3.0)
    cam = rrt.look_at(eye, (3.0, 3.0, 3.0))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])

    def make(mode, kw):
        rt = rrt.RayTracer(sd, chain_rrt_lights(rrt), rrt.Vector3d(*eye), box_filter=mode, **kw)
        rt.set_camera(**cam)
        assert rt.chain_info["n_chains"] >= 1, rt.chain_info
        return rt
    modes = [(m, {}) for m in FORCED_MODES] + [("bundle", dict(chain_shortcut=False))]
    assert len(CHAIN_LIGHTS) == 3
    for _ in assert_walks(rrt, make, len(A["materials"]), "chain scene", modes):
        pass


# ------------------------------------------------------------------ 6
def device_planes(torch, planes):
    return {n: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda().reshape(-1) for n, a in planes.items()}


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_the_device_form(rrt, teapot, kept, mode):
    torch = pytest.importorskip("torch")
    _, planes, _, _ = kept[SCENES[0]]
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    x0, y0, w, h = REGION
    part = crop(planes, REGION)
    host = rt.ambient(W, H, part, T8, T8_MAX_T, region=REGION)
    assert (host["occluded"] != 0).sum() >= 500
    G, SENTINEL = 64, -1515870811
    stream = torch.cuda.Stream()
    tensors = device_planes(torch, part)
    occluded = torch.full((G + 4 * w * h + G,), SENTINEL, dtype=torch.int32, device="cuda")
    grey = torch.full((G + w * h + G,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rt.ambient_into(dict(occluded=occluded[G:-G], grey=grey[G:-G]), tensors, T8, T8_MAX_T, W, H, region=REGION, stream=stream.cuda_stream)
    stream.synchronize()
    stats = rt.last_stats()
    for name, t, shape in (("occluded", occluded, (h, w, 4)), ("grey", grey, (h, w))):
        a = t.cpu().numpy()
        assert (a[:G] == SENTINEL).all() and (a[-G:] == SENTINEL).all(), f"{name}: an element outside the output was written"
        assert_same_bits(a[G:-G].view(np.uint32).reshape(shape), host[name], f"walk {mode}: {name} of the device form vs the host form")
    assert (stats["width"], stats["height"], stats["rays_primary"]) == (W, H, 4 * traced_pixels_in(REGION, W, H)), stats
    assert stats["filter_variant"] == rrt.VARIANT_NAMES.index(mode) and stats["kernel_ms"] > 0, stats
    # one output only: the other tensor is not touched
    grey.fill_(SENTINEL); occluded.fill_(SENTINEL)
    torch.cuda.synchronize()
    rt.ambient_into(dict(grey=grey[G:-G]), tensors, T8, T8_MAX_T, W, H, region=REGION, stream=stream.cuda_stream)
    stream.synchronize()
    assert (occluded.cpu().numpy() == SENTINEL).all()
    assert_same_bits(grey.cpu().numpy()[G:-G].view(np.uint32).reshape(h, w), host["grey"], f"walk {mode}: grey alone, device form")


@pytest.mark.parametrize("frames_before", (0, 1, 2))
def test_the_tuning_state_is_untouched(rrt, teapot, kept, odd_frame, frames_before):
    """An ambient call is no frame of its size: between two frames of a size it runs the variant kept for that size and leaves it, and the count of frames, alone."""
    _, planes, _, want = kept[SCENES[0]]
    _, odd_planes, odd = odd_frame
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    before, variant = None, None
    for _ in range(frames_before):
        before = rt.render(W, H)
        variant = rt.last_stats()["filter_variant"]
    got = rt.ambient(W, H, planes, T8, T8_MAX_T, outputs=("occluded",))
    stats = rt.last_stats()
    assert_same_bits(got["occluded"], want, f"after {frames_before} frames")
    assert (stats["width"], stats["height"], stats["rays_primary"]) == (W, H, 4 * traced_pixels_in((0, 0, W, H), W, H)) and stats["kernel_ms"] > 0, stats
    assert_same_bits(rt.ambient(W2, H2, odd_planes, T8, T8_MAX_T, outputs=("occluded",))["occluded"], odd["occluded"], "another size")   # must not become "the" size either
    again = rt.ambient(W, H, planes, T8, T8_MAX_T, outputs=("occluded",))
    assert rt.last_stats()["filter_variant"] == stats["filter_variant"]
    assert_same_bits(again["occluded"], want, "after a call of another size")
    after = rt.render(W, H)
    if frames_before:
        assert stats["filter_variant"] == variant, (stats["filter_variant"], variant)
        assert np.array_equal(after, before)
    if frames_before == 2:                                                        # measured already: the kept variant stays
        assert rt.last_stats()["filter_variant"] == variant, (rt.last_stats()["filter_variant"], variant)
    if frames_before == 0:
        assert rt.last_stats()["filter_variant"] == stats["filter_variant"], "an ambient call before any frame runs the first frame's variant"


# ------------------------------------------------------------------ 7
def test_refusals_leave_the_outputs_as_they_were(rrt, teapot, kept):
    _, planes, _, want = kept[SCENES[0]]
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    x0, y0, w, h = REGION
    part = crop(planes, REGION)
    tiny = crop(planes, (0, 0, 1, 1))
    L = rrt.lib()
    PATTERN = 0xA5A5A5A5
    occluded, grey = np.full((h, w, 4), PATTERN, np.uint32), np.full((h, w), PATTERN, np.uint32)
    dirs = np.ascontiguousarray(T8)
    cs = rrt.CSurface(**{n: part[n].ctypes.data for n in INPUTS})
    creg = rrt.CRegion(*REGION)

    def samples(d=dirs, n=8, max_t=T8_MAX_T):
        return rrt.CAmbientSamples(dirs=None if d is None else d.ctypes.data_as(C.POINTER(C.c_double)), n=n, max_t=max_t)

    def out(o=occluded, g=grey):
        return rrt.CAmbient(occluded=None if o is None else o.ctypes.data, grey=None if g is None else g.ctypes.data)

    def raw(planes_p, samples_p, out_p, width=W, height=H, region=creg):
        status = L.rrt_ambient_surface(rt._h, width, height, C.byref(region), planes_p, samples_p, out_p)
        if status != rrt.OK:
            raise rrt.RrtError(status, "rrt_ambient_surface", (L.rrt_last_error_detail() or b"").decode())

    def bad_dir(value):
        d = dirs.copy()
        d[5, 1] = value
        return d
    nan_dirs, inf_dirs, many = bad_dir(np.nan), bad_dir(-np.inf), np.ascontiguousarray(np.tile(dirs, (5, 1)))   # (kept alive here: the structs only point at them)

    def without_plane(name):
        return rrt.CSurface(**{n: part[n].ctypes.data for n in INPUTS if n != name})

    calls = [("a NULL surface struct", lambda: raw(None, C.byref(samples()), C.byref(out()))),
             ("a NULL samples struct", lambda: raw(C.byref(cs), None, C.byref(out()))),
             ("a NULL output struct", lambda: raw(C.byref(cs), C.byref(samples()), None))]
    calls += [(f"plane {name} missing", (lambda name=name: raw(C.byref(without_plane(name)), C.byref(samples()), C.byref(out())))) for name in INPUTS]
    calls += [("both outputs NULL", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out(None, None)))),
              ("n == 0", lambda: raw(C.byref(cs), C.byref(samples(n=0)), C.byref(out()))),
              ("n == 33", lambda: raw(C.byref(cs), C.byref(samples(d=many, n=33)), C.byref(out()))),
              ("NULL dirs", lambda: raw(C.byref(cs), C.byref(samples(d=None)), C.byref(out()))),
              ("a NaN direction component", lambda: raw(C.byref(cs), C.byref(samples(d=nan_dirs)), C.byref(out()))),
              ("an infinite direction component", lambda: raw(C.byref(cs), C.byref(samples(d=inf_dirs)), C.byref(out()))),
              ("max_t NaN", lambda: raw(C.byref(cs), C.byref(samples(max_t=np.nan)), C.byref(out()))),
              ("max_t 0", lambda: raw(C.byref(cs), C.byref(samples(max_t=0.0)), C.byref(out()))),
              ("max_t -1", lambda: raw(C.byref(cs), C.byref(samples(max_t=-1.0)), C.byref(out()))),
              ("max_t -inf", lambda: raw(C.byref(cs), C.byref(samples(max_t=-np.inf)), C.byref(out()))),
              ("a frame of no width", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), width=0)),
              ("a frame of 2^31 pixels", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), width=65536, height=32768)),
              ("region beyond the last column", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), region=rrt.CRegion(W - 40, 3, 41, 30))),
              ("region beyond the last row", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), region=rrt.CRegion(5, H - 29, 41, 30))),
              ("w == 0", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), region=rrt.CRegion(5, 3, 0, 30))),
              ("h == 0", lambda: raw(C.byref(cs), C.byref(samples()), C.byref(out()), region=rrt.CRegion(5, 3, 41, 0))),
              ("the Python form, 33 directions", lambda: rt.ambient(W, H, tiny, many[:33], T8_MAX_T, region=(0, 0, 1, 1))),
              ("the Python form, a plane missing", lambda: rt.ambient(W, H, {n: tiny[n] for n in ("point", "material")}, dirs, T8_MAX_T, region=(0, 0, 1, 1)))]
    for what, call in calls:
        with pytest.raises(rrt.RrtError) as e:
            call()
        assert e.value.status == rrt.ERR_INVALID_ARG, what
        assert (occluded == PATTERN).all() and (grey == PATTERN).all(), f"{what}: an output of a refused call was written"
    raw(C.byref(cs), C.byref(samples(max_t=INF)), C.byref(out()))                  # +inf is a valid max_t
    assert not (occluded == PATTERN).any() and not (grey == PATTERN).any(), "an accepted call leaves elements of its outputs unwritten"
    raw(C.byref(cs), C.byref(samples()), C.byref(out()))
    assert_same_bits(occluded, want[y0:y0 + h, x0:x0 + w], "after the refusals: occluded of the region")
