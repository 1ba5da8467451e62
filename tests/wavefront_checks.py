"""Helpers of the tests of the two ends of the per-ray pipeline and of the frame by ray generations (include/rrt.h: rrt_frame_rays, rrt_mix_rays, rrt_mix_pixels,
rrt_render_wavefront): the numpy restatement of both entry orders and of a frame's ray batch -- built on gpu_checks.pose_dirs / traced_rows and
surface_checks.traced_cols, the restatements the other tests use -- one level of the unwind by shade_rays_checks.mixed with its inputs (mix_case), and the pixels by gpu_checks.mix4.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np
import pytest

from bitwise import assert_same_bits
from gpu_checks import mix4, pose_dirs, traced_rows
from ray_surface_checks import WHITE, clamp_u8, pack
from shade_rays_checks import mixed
from surface_checks import traced_cols, traced_pixels_in

ROWS, TILES = 0, 1                                               # RRT_ORDER_ROWS, RRT_ORDER_TILES
ORDERS = (ROWS, TILES)
ARRAYS = ("origins", "dirs", "max_t")                             # what rrt_frame_rays writes, in its order
WIDTHS = dict(origins=3, dirs=3, max_t=1)
DEAD_BOUND = 0x7FF8000000000000                                   # max_t of a dead entry: compaction's dead value
SENTINEL = -12345.5
VARIANT = dict(lane=0, bundle=1, ray=2)                           # filter_variant of rrt_last_stats per forced walk

# the frames of the GPU tests and, per frame, the whole frame and two regions cut off the 4x4 tile boundaries; the second has a tile straddling each of its edges
FRAMES = ((64, 48), (97, 61), (2, 2), (5, 3))
REGIONS = {(64, 48): (None, (3, 5, 13, 7), (6, 9, 21, 18)), (97, 61): (None, (3, 5, 13, 7), (90, 1, 7, 58)), (2, 2): (None, (1, 0, 1, 2), (0, 1, 2, 1)),
           (5, 3): (None, (3, 1, 2, 2), (1, 0, 3, 3))}


def region_of(w, h, region):
    return (0, 0, w, h) if region is None else tuple(int(v) for v in region)


def tile_rectangle(region):
    """(first tile column, first tile row, tiles per row, tile rows) of the 4x4-pixel tiles of the frame that the region touches"""
    x0, y0, rw, rh = region
    return x0 // 4, y0 // 4, (x0 + rw + 3) // 4 - x0 // 4, (y0 + rh + 3) // 4 - y0 // 4


def ray_count(w, h, region, order):
    """rrt_frame_ray_count restated; 0 for what the library refuses"""
    if w <= 0 or h <= 0 or w * h > 0x7FFFFFFF or order not in ORDERS:
        return 0
    x0, y0, rw, rh = region_of(w, h, region)
    if rw <= 0 or rh <= 0 or x0 < 0 or y0 < 0 or x0 + rw > w or y0 + rh > h:
        return 0
    _, _, tw, th = tile_rectangle((x0, y0, rw, rh))
    n = 4 * rw * rh if order == ROWS else 64 * tw * th
    return n if n <= 0xFFFFFFFF else 0


def entries(w, h, region, order):
    """(px, py, sub, inside) per entry of the batch: the canvas pixel, the sub-sample, and whether the pixel lies in the region (always, in rows order)"""
    x0, y0, rw, rh = region_of(w, h, region)
    e = np.arange(ray_count(w, h, (x0, y0, rw, rh), order), dtype=np.int64)
    sub, q = e & 3, e >> 2
    if order == ROWS:
        px, py = x0 + q % rw, y0 + q // rw
    else:
        tx0, ty0, tw, _ = tile_rectangle((x0, y0, rw, rh))
        pix, tile = q & 15, q >> 4
        px, py = (tx0 + tile % tw) * 4 + (pix & 3), (ty0 + tile // tw) * 4 + (pix >> 2)
    inside = (px >= x0) & (px < x0 + rw) & (py >= y0) & (py < y0 + rh)
    return px, py, sub, inside


def traced_mask(w, h):
    """[h][w]: the pixels the reference traces (engine.rs:146-158)"""
    m = np.zeros((h, w), bool)
    m[np.ix_(traced_rows(h), traced_cols(w))] = True
    return m


def alive_entries(w, h, region, order):
    px, py, _, inside = entries(w, h, region, order)
    return inside & traced_mask(w, h)[np.minimum(py, h - 1), np.minimum(px, w - 1)]


def expected_rays(cam, w, h, region, order, viewport=(1.0, 1.0, 1.0)):
    """The batch rrt_frame_rays writes: origins [n][3], dirs [n][3], max_t [n]; a dead entry is zeros and the NaN 0x7FF8000000000000"""
    px, py, sub, _ = entries(w, h, region, order)
    alive = alive_entries(w, h, region, order)
    full = np.zeros((h, w, 4, 3))
    rows, cols = traced_rows(h), traced_cols(w)
    if len(rows) and len(cols):
        full[np.ix_(rows, cols)] = pose_dirs(cam, w, h, rows, cols, viewport).transpose(0, 2, 1, 3)
    n = len(px)
    dirs, origins = np.zeros((n, 3)), np.zeros((n, 3))
    dirs[alive] = full[py[alive], px[alive], sub[alive]]
    origins[alive] = np.asarray(cam["eye"], np.float64)
    max_t = np.full(n, DEAD_BOUND, np.uint64).view(np.float64)
    max_t[alive] = np.inf
    return dict(origins=origins, dirs=dirs, max_t=max_t)


def mix_level(local, kr, reflected, material, n_mats):
    """rrt_mix_rays restated: WHITE where material is no material, the clamped local where nothing mixes, shade_rays_checks.mixed where kr > 0; kr, reflected and
    material may be None as in the call"""
    n = len(local)
    hit = np.ones(n, bool) if material is None else np.asarray(material, np.uint32) < n_mats
    with np.errstate(invalid="ignore"):
        c = np.where(hit, pack(clamp_u8(local)), np.uint32(WHITE)).astype(np.uint32)
        if kr is not None and reflected is not None:
            go = hit & (kr > 0.0)
            if go.any():
                c[go] = mixed(local[go], kr[go], np.asarray(reflected, np.uint32)[go] & np.uint32(0xFFFFFF))
    return c


def expected_pixels(colours, w, h, region, order):
    """rrt_mix_pixels restated: [region.h][region.w], gpu_checks.mix4 of a traced pixel's four sub-sample colours, 0 for a pixel the reference never traces"""
    x0, y0, rw, rh = region_of(w, h, region)
    px, py, sub, inside = entries(w, h, region, order)
    planes = np.zeros((rh, rw, 4), np.uint32)
    planes[py[inside] - y0, px[inside] - x0, sub[inside]] = np.asarray(colours, np.uint32)[inside] & np.uint32(0xFFFFFF)
    fb = mix4(planes.reshape(-1, 4)).reshape(rh, rw)
    fb[~traced_mask(w, h)[y0:y0 + rh, x0:x0 + rw]] = 0
    return fb


def host(t, dtype, shape):
    """A device tensor as a host array of `dtype` and `shape` with the same bits"""
    return t.cpu().numpy().view(dtype).reshape(shape)


def assert_wavefront_is_render(rrt, torch, rt, w, h, region, what, forced=None):
    """render_wavefront of the whole frame (host form) and of `region` (device form: a stream of the test's own, exactly wavefront_work_bytes of work memory
    prefilled with 0xA5) in both orders is rt's own frame; rrt_last_stats as rrt.h says; afterwards render gives the same frame from the same kept variant.
    rt.max_reflection_depth: the depth rt was created with (the caller sets the attribute)."""
    rt.render(w, h)
    want = rt.render(w, h)                                         # (the second frame of a size: an unforced raytracer has measured now)
    kept = rt.last_stats()["filter_variant"]
    assert forced is None or kept == VARIANT[forced], f"{what}: variant {kept} runs, {forced} = {VARIANT[forced]} was forced"
    stream = torch.cuda.Stream()
    x0, y0, rw, rh = region
    for order in ORDERS:
        got = rt.render_wavefront(w, h, order=order)
        assert_same_bits(got, want, f"{what}, order {order}: render_wavefront vs render")
        s = rt.last_stats()
        assert (s["width"], s["height"], s["rays_primary"], s["filter_variant"]) == (w, h, 4 * traced_pixels_in((0, 0, w, h), w, h), kept) and s["kernel_ms"] > 0, s
        need = rt.wavefront_work_bytes(w, h, region, order)
        n = rrt.frame_ray_count(w, h, region, order)
        depth = rt.max_reflection_depth
        assert 0 < need <= n * (229 + 40 * (depth + 1)) + 16384, f"{what}: {need} bytes of work memory for {n} entries at depth {depth}"
        with torch.cuda.stream(stream):
            work = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
            fb = torch.full((rw * rh,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            assert work.data_ptr() % 256 == 0, f"{what}: the work memory lies at {work.data_ptr():#x}"
            rt.render_wavefront_into(fb, work, w, h, region=region, order=order, stream=stream.cuda_stream)
        stream.synchronize()
        assert_same_bits(host(fb, np.uint32, (rh, rw)), want[y0:y0 + rh, x0:x0 + rw], f"{what}, order {order}, region {region}: render_wavefront_into vs render")
        s = rt.last_stats()
        assert (s["width"], s["height"], s["rays_primary"], s["filter_variant"]) == (w, h, 4 * traced_pixels_in(region, w, h), kept) and s["kernel_ms"] > 0, s
        with pytest.raises(rrt.RrtError):                          # one byte less is refused, and the framebuffer stays
            rt.render_wavefront_into(fb, work[:need - 1], w, h, region=region, order=order, stream=stream.cuda_stream)
    assert_same_bits(rt.render(w, h), want, f"{what}: render after render_wavefront")
    assert rt.last_stats()["filter_variant"] == kept, f"{what}: render runs another variant after render_wavefront"
    return want


# ------------------------------------------------------------------ the inputs of one level of the unwind
def mix_case(n, n_mats):
    """A third misses, a third with kr = 0, a third with kr in (0, 1]; local with negatives, values above 255, exact integers, NaN and +-inf; junk in reflected's top byte"""
    rng = np.random.default_rng(n)
    local = rng.uniform(-40.0, 320.0, (n, 3))
    whole = rng.random((n, 3)) < 0.25
    local[whole] = np.round(local[whole])
    for j, v in enumerate((np.nan, np.inf, -np.inf, 255.0, 256.0, 0.0, -0.0, 254.99999999999997)):
        local[(3 * j + 1) % n, j % 3] = v
    kind = np.arange(n) % 3
    material = np.where(kind == 0, 0xFFFFFFFF, rng.integers(0, n_mats, n)).astype(np.uint32)
    material[np.flatnonzero(kind == 0)[::2]] = n_mats               # (misses by the first index that is no material, and by 0xFFFFFFFF)
    kr = np.where(kind == 2, 1.0 - rng.random(n), 0.0)
    kr[(kind == 2) & (np.arange(n) % 5 == 0)] = 1.0
    kr[(kind == 1) & (np.arange(n) % 7 == 0)] = -0.5
    kr[(kind == 1) & (np.arange(n) % 11 == 0)] = np.nan
    reflected = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return local, kr, reflected, material
