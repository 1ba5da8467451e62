"""The two forms of a query agree bit for bit (include/rrt.h): the region form of surface, shade and ambient, which takes its rays or hits from the planes of a
frame, and the per-ray form, which takes them from a batch -- rrt_render_surface_device against rrt_surface_rays_device, rrt_shade_surface_device against
rrt_shade_rays_device, rrt_ambient_surface_device against rrt_ambient_rays_device.  render.hip states the surface and shade state machines once for both forms
(surface_body, shade_body) and the ambient sample loop once per form; whichever way they are stated, a frame's sub-samples handed to the per-ray form in the
planes' order must come back as the frame's planes, pixels and masks.

All device forms, in the three forced walks.  Comparisons are bit for bit (f64 through its integer bits) on the sub-samples the reference traces.  No test passes
vacuously: each asserts floors on what it compared, at most half of what the CPU oracle alone yields for the scene and size (counted with
surface_checks.expected_planes and ambient_checks.by_oracle; the counts stand beside the floors).
"""
import numpy as np
import pytest

from ambient_checks import table8
from bitwise import assert_same_bits
from gpu_checks import FORCED_MODES, ORIGIN, mix4
from ray_surface_checks import kr_of
from scenes import CREATION, room_without_oracle as room  # noqa: F401  (fixtures: room)
from surface_checks import frame_dirs, traced_part

pytestmark = pytest.mark.gpu

torch = None                                                                 # (set by the fixture below: collecting this module imports no torch)

VECTORS = ("point", "normal")
SHARED = ("hit", "t", "u", "v", "tri", "albedo", "point", "normal", "material", "lights")   # what the per-ray surface record shares with the frame planes
DTYPES = dict(hit=np.uint8, t=np.float64, u=np.float64, v=np.float64, tri=np.uint32, albedo=np.uint32, point=np.float64, normal=np.float64, material=np.uint32,
              lights=np.uint32)
SHADE_INPUTS = ("point", "normal", "material", "albedo", "lights")
AMBIENT_INPUTS = ("point", "normal", "material")
# floors, beside the CPU oracle's counts for the scene, the size and the creation pose
TEAPOT_HITS = {(97, 61): 6700, (64, 48): 3500}       # oracle: 13487 of 22656 sub-samples hit; 7142 of 12032
ROOM_HITS, ROOM_MIRRORS = 6000, 5500                 # oracle: 12032 of 12032 sub-samples hit, 11062 of them a material with kr > 0
AMBIENT_MASKS = {2.0: 3400, np.inf: 3500}            # oracle: 6917 and 7123 of the 7142 hits have an occluded ray among the 8 of T8


def empty(name, n):
    dtype = DTYPES[name]
    return torch.empty(n * (3 if name in VECTORS else 1), dtype={np.uint8: torch.uint8, np.uint32: torch.int32, np.float64: torch.float64}[dtype], device="cuda")


def upload(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).reshape(-1).cuda()


def host(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


def frame_planes(rt, w, h):
    """(device tensors, host arrays [h][w][4] / [h][w][4][3]) of all ten planes of the whole frame, from ONE rrt_render_surface_device launch"""
    dev = {name: empty(name, 4 * w * h) for name in SHARED}
    rt.surface_into(dev, w, h)
    torch.cuda.synchronize()
    return dev, {name: host(t, DTYPES[name]).reshape((h, w, 4, 3) if name in VECTORS else (h, w, 4)) for name, t in dev.items()}


def flat_traced(planes, w, h, names):
    """the traced sub-samples of frame planes as [n] / [n][3] arrays, in the order of frame_dirs(...).reshape(-1, 3)"""
    part = traced_part({name: planes[name] for name in names}, w, h)
    return {name: np.ascontiguousarray(a.reshape((-1, 3) if name in VECTORS else (-1,))) for name, a in part.items()}


@pytest.fixture(scope="module", autouse=True)
def _torch():
    global torch
    torch = pytest.importorskip("torch")


# ------------------------------------------------------------------ surface
@pytest.mark.parametrize("mode", FORCED_MODES)
def test_surface_planes_of_a_frame_are_the_records_of_its_primary_rays(rrt, teapot, mode):
    w, h = 97, 61                                                            # odd both ways: rows 0 and 1 and the last column are never traced
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    _, planes = frame_planes(rt, w, h)
    want = flat_traced(planes, w, h, SHARED)
    d = frame_dirs(CREATION, w, h).reshape(-1, 3)
    n = len(d)
    assert n == 22656 == want["hit"].size
    out = {name: empty(name, n) for name in SHARED}
    rt.surface_rays_into(upload(np.broadcast_to(np.asarray(ORIGIN, np.float64), d.shape)), upload(d), out)
    torch.cuda.synchronize()
    hits = int(want["hit"].sum())
    print(f"walk {mode}: {hits} of {n} sub-samples hit")
    assert hits >= TEAPOT_HITS[(w, h)], f"only {hits} sub-samples hit (< {TEAPOT_HITS[(w, h)]})"
    for name in SHARED:
        assert_same_bits(host(out[name], DTYPES[name]).reshape(want[name].shape), want[name], f"teapot {w}x{h}, walk {mode}, {name}")


# ------------------------------------------------------------------ shade
def check_shade(rt, w, h, mode, what, min_hits, kr=None, min_mirrors=0):
    dev, planes = frame_planes(rt, w, h)
    rec = flat_traced(planes, w, h, SHADE_INPUTS)
    d = frame_dirs(CREATION, w, h)
    rows, cols = d.shape[:2]
    n = rows * cols * 4
    hit = rec["material"] != 0xFFFFFFFF
    mirrors = int((hit & (kr(rec["material"]) > 0.0)).sum()) if kr else 0
    print(f"{what}, walk {mode}: {int(hit.sum())} of {n} sub-samples hit, {mirrors} on a mirror")
    assert int(hit.sum()) >= min_hits, f"{what}: only {int(hit.sum())} sub-samples hit (< {min_hits})"
    assert mirrors >= min_mirrors, f"{what}: only {mirrors} sub-samples on a material with kr > 0 (< {min_mirrors})"
    d_t = upload(d.reshape(-1, 3))
    rec_t = {name: upload(a) for name, a in rec.items()}
    for masked in (True, False):
        names = [name for name in SHADE_INPUTS if masked or name != "lights"]
        fb = torch.empty(w * h, dtype=torch.int32, device="cuda")
        rt.shade_into(fb, {name: dev[name] for name in names}, w, h)
        colour = torch.empty(n, dtype=torch.int32, device="cuda")
        rt.shade_rays_into(dict(colour=colour), d_t, {name: rec_t[name] for name in names}, depth=0)
        torch.cuda.synchronize()
        want = traced_part(dict(fb=host(fb).reshape(h, w)), w, h)["fb"]
        got = mix4(host(colour).reshape(-1, 4)).reshape(rows, cols)
        assert_same_bits(got, np.ascontiguousarray(want), f"{what}, walk {mode}, {'with' if masked else 'without'} the lights mask: mixed shade_rays colours vs the shaded pixels")


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_shaded_pixels_of_the_mirror_room_are_the_mixed_colours_of_its_records(rrt, room, mode):
    A, lights, sd = room
    check_shade(rrt.RayTracer(sd, lights, box_filter=mode), 64, 48, mode, "mirror room 64x48", ROOM_HITS, lambda m: kr_of(A, m), ROOM_MIRRORS)


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_shaded_pixels_of_the_teapot_are_the_mixed_colours_of_its_records(rrt, teapot, mode):
    check_shade(rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode), 97, 61, mode, "teapot 97x61", TEAPOT_HITS[(97, 61)])


# ------------------------------------------------------------------ ambient
@pytest.mark.parametrize("mode", FORCED_MODES)
def test_ambient_masks_of_a_frame_are_the_masks_of_its_records(rrt, teapot, mode):
    w, h = 64, 48
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    dev, planes = frame_planes(rt, w, h)
    rec = flat_traced(planes, w, h, AMBIENT_INPUTS)
    n = rec["material"].size
    hits = int((rec["material"] != 0xFFFFFFFF).sum())
    assert n == 12032 and hits >= TEAPOT_HITS[(w, h)], f"only {hits} of {n} sub-samples hit (< {TEAPOT_HITS[(w, h)]})"
    rec_t = {name: upload(a) for name, a in rec.items()}
    for max_t in (2.0, np.inf):
        frame = torch.empty(4 * w * h, dtype=torch.int32, device="cuda")
        rt.ambient_into(dict(occluded=frame), {name: dev[name] for name in AMBIENT_INPUTS}, table8(), max_t, w, h)
        rays = torch.empty(n, dtype=torch.int32, device="cuda")
        rt.ambient_rays_into(dict(occluded=rays), rec_t, table8(), max_t)                # (no rotation)
        torch.cuda.synchronize()
        want = np.ascontiguousarray(traced_part(dict(occluded=host(frame).reshape(h, w, 4)), w, h)["occluded"].reshape(-1))
        nonzero = int((want != 0).sum())
        print(f"walk {mode}, max_t {max_t}: {nonzero} of {hits} hits have an occluded ray")
        assert nonzero >= AMBIENT_MASKS[max_t], f"max_t {max_t}: only {nonzero} non-zero masks (< {AMBIENT_MASKS[max_t]})"
        assert_same_bits(host(rays), want, f"teapot {w}x{h}, walk {mode}, max_t {max_t}: occluded of the records vs the frame's plane")
