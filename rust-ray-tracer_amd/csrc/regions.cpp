// regions.cpp -- regions of a frame behind include/rrt.h: visibility and surface buffers, frames shaded and ambient occlusion from kept buffers, the pick of one
// pixel, the fused frame of a region and of a list of tiles in device memory, the four deferred stages over such a list, and the tile tests that produce one.  The calls share one check of the region (host_planes.hpp: region_in_force), one check of a list (check_tile_list), one routine per stage that fills its planes, one launch (launch_stage_frame) and, for their host forms, the routine that
// carves the kept device allocation and copies the planes up and down (launches.hpp: with_kept_planes) over the mirrored structs (host_planes.hpp: mirror_planes).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "launches.hpp"

namespace rrt {

// ---- regions of a frame: visibility buffers, surface buffers, shading and ambient occlusion from kept buffers, pick.  Each is one launch of its kernel over the tiles
// the region touches (rrt.h: rrt_render_visibility_device, rrt_render_surface_device, rrt_shade_surface_device, rrt_ambient_surface_device).
// The variant: the forced one, else the one kept for this frame size, else the first-frame rule's.  Reads the tuning state, never writes it: a
// region call is not a frame of that size.
int visibility_variant(const rrt_raytracer* rt, uint32_t width, uint32_t height) {
    if (rt->variant_forced) return rt->walk;
    if (rt->tuned_w == width && rt->tuned_h == height && rt->tuned_world == 1u) return rt->walk;
    return first_frame_variant(rt, width, height);
}

// ---- ambient occlusion from kept planes and from ray records.  The checks of a sample table (not null), for both
void check_ambient_samples(const rrt_ambient_samples& samples) {
    if (samples.n == 0 || samples.n > RRT_MAX_AMBIENT_SAMPLES) throw Error{RRT_ERR_INVALID_ARG, "bad sample count: 1 to RRT_MAX_AMBIENT_SAMPLES directions"};
    if (!samples.dirs) throw Error{RRT_ERR_INVALID_ARG, "null sample directions"};
    for (uint32_t k = 0; k < 3 * samples.n; k++)
        if (!std::isfinite(samples.dirs[k])) throw Error{RRT_ERR_INVALID_ARG, "a sample direction has a non-finite component"};
    if (!(samples.max_t > 0.0)) throw Error{RRT_ERR_INVALID_ARG, "max_t is NaN or not positive"};
}

}  // namespace rrt

namespace {

using namespace rrt;

// ---- where a stage runs: the front end of its kernel argument (device_scene.hpp: Region, TileList) and the primary rays its launch records.
template <class Front> struct Place { Front front; uint64_t rays_primary; };
// region r (checked) of a frame: 4 rays per traced pixel of it
Place<Region> in_region(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r) {
    Region p{};
    p.F = frame_params(rt, width, height, 0, 1, false);
    p.F.row_begin = r.y0; p.F.row_end = r.y0 + r.h;
    p.col_begin = r.x0; p.col_end = r.x0 + r.w;
    p.tile_x0 = r.x0 / 8; p.tile_y0 = r.y0 / 8;
    p.tiles_w = (p.col_end + 7) / 8 - p.tile_x0;
    p.F.tile_begin = 0; p.F.tile_end = p.tiles_w * ((p.F.row_end + 7) / 8 - p.tile_y0);
    return {p, 4 * traced_pixels_in(r, width, height)};
}
static_assert(kMaxTileList == RRT_MAX_TILE_LIST, "rrt.h names the launch bound of a tile list");
// A list (checked) of tiles of a frame in device memory.  Nothing of the list is read here: the kernel reads it, and the bound, when it runs; the library does not
// know which tiles the list names, and records no ray.
Place<TileList> in_list(const rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles) {
    TileList l{};
    l.F = frame_params(rt, width, height, 0, 1, false);
    l.F.xcd_chunk = 0;                                                   // the caller's order is the schedule
    l.tiles = d_tiles; l.count = d_count; l.n = n;
    return {l, 0};
}
// The checks of a list, behind those of the stage: false for the empty list, which launches nothing.
bool check_tile_list(uint32_t n, const uint32_t* d_tiles) {
    if (n > kMaxTileList) throw Error{RRT_ERR_INVALID_ARG, "the list is longer than RRT_MAX_TILE_LIST entries: its grid would not fit a launch"};
    if (n == 0) return false;                                            // nothing is launched, rrt_last_stats stays as it was
    if (!d_tiles) throw Error{RRT_ERR_INVALID_ARG, "null tile list"};
    return true;
}
// (the front end of a stage that writes no visibility plane: a region carries six null plane pointers, device_scene.hpp: BareFront)
VisStage<Region> bare(const Region& r) { return {r, VisPlanes{}}; }
TileList bare(const TileList& l) { return l; }

// The one stage launch: the finished kernel argument q on the caller's stream, timed by the raytracer's events and recorded.
template <class Params> void launch_stage_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const Params& q, uint64_t rays_primary, void* stream) {
    const int variant = visibility_variant(rt, width, height);
    timed_launch(rt, stream, [&] { return launch_stage(rt->scene, q, stream, variant); });
    record(rt, width, height, rays_primary, variant);
}

// ---- the planes of each stage, from the structs of rrt.h with planes in device memory: one routine each, for both front ends.
VisPlanes vis_planes(const rrt_visibility& d) { return {d.hit, d.t, d.u, d.v, d.tri, d.albedo}; }
SurfacePlanes surface_planes(const rrt_surface& d) { return {d.point, d.normal, d.material, d.lights}; }
ShadePlanes shade_planes(const rrt_visibility& d_vis, const rrt_surface& d, void* d_fb) {
    return {d.point, d.normal, d.material, d_vis.albedo, d.lights, static_cast<uint32_t*>(d_fb)};
}
// (the sample table is copied into the kernel's argument here: no device memory holds it)
AmbientPlanes ambient_planes(const rrt_surface& d, const rrt_ambient_samples& samples, const rrt_ambient& d_out) {
    AmbientPlanes p{};
    p.point = d.point; p.normal = d.normal; p.material = d.material;
    p.occluded = d_out.occluded; p.grey = d_out.grey;
    p.n_samples = samples.n; p.max_t = samples.max_t;
    std::memcpy(p.dirs, samples.dirs, sizeof(double) * 3 * samples.n);
    return p;
}

// ---- the host forms of the region calls.  Their planes live in the raytracer's kept device allocation for one call (with_kept_planes), the structs' planes in
// the order of their fields (host_planes.hpp: mirror_planes).  (rrt_pick relies on that order: see pick_pixel.)
constexpr size_t kVis = kFields<rrt_visibility>, kSurf = kFields<rrt_surface>, kAmb = kFields<rrt_ambient>;
using VisDirs = FieldDirs<rrt_visibility>;
using SurfDirs = FieldDirs<rrt_surface>;

// ---- visibility buffers.  every check of a visibility call, before any GPU work; returns the region in force
rrt_region check_visibility(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* planes) {
    check_frame(rt, width, height);
    if (!planes) throw Error{RRT_ERR_INVALID_ARG, "null planes struct"};
    if (!planes->hit && !planes->t && !planes->u && !planes->v && !planes->tri && !planes->albedo) throw Error{RRT_ERR_INVALID_ARG, "no plane requested: all six pointers are null"};
    return region_in_force(width, height, region);
}

// the planes of a region or a list (checked) into device memory
template <class Front> void launch_visibility_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const Place<Front>& at, const rrt_visibility& d_planes, void* stream) {
    launch_stage_frame(rt, width, height, VisStage<Front>{at.front, vis_planes(d_planes)}, at.rays_primary, stream);
}

void visibility_to_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& planes) {
    DeviceGuard guard(rt->device);
    HostPlane pl[kVis];
    mirror_planes(pl, planes, 4 * (size_t)r.w * r.h, VisDirs::every(kDown));
    with_kept_planes(rt, pl, [&](void* stream) { launch_visibility_frame(rt, width, height, in_region(rt, width, height, r), mirrored<rrt_visibility>(pl), stream); });
}

// One pixel: a one-tile launch into the kept allocation and ONE copy of its six plane slots back.  All six planes of the pixel's four sub-samples are wanted, carved
// only, and the first of the list: they fill the first table_bytes(kVisibilityElem, 4) bytes of the allocation, each where the carving put it; sub-sample 0 is the answer.
rrt_pick_result pick_pixel(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t px, uint32_t py) {
    DeviceGuard guard(rt->device);
    alignas(8) char back[table_bytes(kVisibilityElem, 4)];
    HostPlane pl[kVis];
    mirror_planes(pl, rrt_visibility{(uint8_t*)back, (double*)back, (double*)back, (double*)back, (uint32_t*)back, (uint32_t*)back}, 4, VisDirs::every(kCarve));   // (every plane wanted)
    rrt_visibility d{};
    with_kept_planes(rt, pl, [&](void* stream) {
        d = mirrored<rrt_visibility>(pl);
        launch_visibility_frame(rt, width, height, in_region(rt, width, height, rrt_region{px, py, 1, 1}), d, stream);
        HIP_TRY(hipMemcpyAsync(back, d.hit, sizeof back, hipMemcpyDeviceToHost, (hipStream_t)stream));
    });
    auto at = [&](const void* dev) { return back + (static_cast<const char*>(dev) - reinterpret_cast<const char*>(d.hit)); };   // where the copy of a device plane begins
    rrt_pick_result out{};
    uint8_t hit; std::memcpy(&hit, at(d.hit), 1); out.hit = hit;
    std::memcpy(&out.t, at(d.t), 8); std::memcpy(&out.u, at(d.u), 8); std::memcpy(&out.v, at(d.v), 8);
    std::memcpy(&out.tri, at(d.tri), 4); std::memcpy(&out.albedo, at(d.albedo), 4);
    return out;
}

// ---- surface buffers.  every check, before any GPU work; returns the region in force
rrt_region check_surface(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_surface* planes) {
    check_frame(rt, width, height);
    if (!planes) throw Error{RRT_ERR_INVALID_ARG, "null surface planes struct"};
    if (!planes->point && !planes->normal && !planes->material && !planes->lights) throw Error{RRT_ERR_INVALID_ARG, "no surface plane requested: all four pointers are null"};
    return region_in_force(width, height, region);
}

template <class Front>
void launch_surface_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const Place<Front>& at, const rrt_visibility& d_vis, const rrt_surface& d_planes, void* stream) {
    launch_stage_frame(rt, width, height, SurfaceStage<Front>{at.front, vis_planes(d_vis), surface_planes(d_planes)}, at.rays_primary, stream);
}

void surface_to_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& vis, const rrt_surface& planes) {
    DeviceGuard guard(rt->device);
    const size_t n = 4 * (size_t)r.w * r.h;
    HostPlane pl[kVis + kSurf];
    mirror_planes(pl, vis, n, VisDirs::every(kDown));
    mirror_planes(pl + kVis, planes, n, SurfDirs::every(kDown));
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_surface_frame(rt, width, height, in_region(rt, width, height, r), mirrored<rrt_visibility>(pl), mirrored<rrt_surface>(pl + kVis), stream);
    });
}

// ---- shading from kept planes.  every check, before any GPU work; returns the region in force
rrt_region check_shade(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* vis, const rrt_surface* planes, const void* out) {
    check_frame(rt, width, height);
    if (!vis || !planes) throw Error{RRT_ERR_INVALID_ARG, "null planes struct: shading reads the albedo plane of the visibility struct and the planes of the surface struct"};
    if (!vis->albedo || !planes->point || !planes->normal || !planes->material) throw Error{RRT_ERR_INVALID_ARG, "null plane: albedo, point, normal and material are all required"};
    if (!out) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
    return region_in_force(width, height, region);
}

// the pixels of a region or a list (checked) from planes in device memory into d_fb
template <class Front>
void launch_shade_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const Place<Front>& at, const rrt_visibility& d_vis, const rrt_surface& d_planes, void* d_fb, void* stream) {
    launch_stage_frame(rt, width, height, ShadeStage<Front>{bare(at.front), shade_planes(d_vis, d_planes, d_fb)}, at.rays_primary, stream);
}

// Host form: the given planes up, the region's pixels down.  The list keeps the order point, normal, material, albedo, lights: the surface struct lies in two runs
// of it, around the visibility struct's.
void shade_from_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& vis, const rrt_surface& planes, uint32_t* out_fb) {
    DeviceGuard guard(rt->device);
    const size_t px = (size_t)r.w * r.h, n = 4 * px;
    enum : size_t { kSurfA, kAlbedo = kSurfA + kSurf, kSurfB = kAlbedo + kVis, kOut = kSurfB + kSurf, kEnd };
    HostPlane pl[kEnd];
    mirror_planes(pl + kSurfA, planes, n, SurfDirs().set(kUp, &rrt_surface::point, &rrt_surface::normal, &rrt_surface::material));
    mirror_planes(pl + kAlbedo, vis, n, VisDirs().set(kUp, &rrt_visibility::albedo));
    mirror_planes(pl + kSurfB, planes, n, SurfDirs().set(kUp, &rrt_surface::lights));
    pl[kOut] = plane_down(out_fb, sizeof(uint32_t), px);
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_shade_frame(rt, width, height, in_region(rt, width, height, r), mirrored<rrt_visibility>(pl + kAlbedo), mirrored<rrt_surface>(pl + kSurfA, pl + kSurfB), pl[kOut].dev, stream);
    });
}

// ---- the fused frame of a region.  every check, before any GPU work; returns the region in force and, through `pitch`, the pitch in force (0: the region's width)
rrt_region check_render_region(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const void* out, uint32_t& pitch) {
    check_frame(rt, width, height);
    if (!out) throw Error{RRT_ERR_INVALID_ARG, "null output"};
    const rrt_region r = region_in_force(width, height, region);
    if (pitch == 0) pitch = r.w;
    if (pitch < r.w) throw Error{RRT_ERR_INVALID_ARG, "pitch is smaller than the region's width (0 = the region's width)"};
    return r;
}

// the pixels of region r (checked) into rows of `pitch` elements from d_out
void launch_render_region_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, uint32_t* d_out, uint32_t pitch, void* stream) {
    const Place<Region> at = in_region(rt, width, height, r);
    launch_stage_frame(rt, width, height, RenderRegionParams{bare(at.front), d_out, pitch, 0}, at.rays_primary, stream);
}

// Host form: the region's pixels, tight in the kept allocation, down into the caller's rows.  A tight `out` is a plane like any other; rows with a gap are only
// carved, and come down row by row in one strided copy behind the launch, so the gap is never written.
void render_region_to_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, uint32_t* out, uint32_t pitch) {
    DeviceGuard guard(rt->device);
    const bool tight = pitch == r.w;
    HostPlane pl[1] = {HostPlane{out, sizeof(uint32_t), (size_t)r.w * r.h, tight ? kDown : kCarve}};
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_render_region_frame(rt, width, height, r, static_cast<uint32_t*>(pl[0].dev), r.w, stream);
        if (!tight) HIP_TRY(hipMemcpy2DAsync(out, sizeof(uint32_t) * (size_t)pitch, pl[0].dev, sizeof(uint32_t) * (size_t)r.w, sizeof(uint32_t) * (size_t)r.w, r.h,
                                             hipMemcpyDeviceToHost, (hipStream_t)stream));
    });
}

// ---- tile selection: tests over planes that produce the list of a tile-list frame (rrt.h: rrt_mark_tiles, rrt_select_tiles; tiles.hip).  Not ray calls: no
// timed_launch, no record, and nothing of the tuning or coverage state is looked at.
static_assert(sizeof(rrt_tile_test) == 72, "rrt_tile_test is 72 bytes");
struct TileFrame { rrt_region r; uint32_t tiles_x, tiles_y, n_tiles; };
// the checks of the frame and the region, and the tiles of the frame
TileFrame check_tile_frame(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region) {
    check_frame(rt, width, height);
    TileFrame f{};
    f.r = region_in_force(width, height, region);
    f.tiles_x = (width + 7) / 8; f.tiles_y = (height + 7) / 8;
    const uint64_t n = (uint64_t)f.tiles_x * f.tiles_y;
    if (n > RRT_MAX_TILE_LIST) throw Error{RRT_ERR_INVALID_ARG, "the frame has more tiles than RRT_MAX_TILE_LIST: its list would not fit a tile-list launch"};
    f.n_tiles = (uint32_t)n;
    return f;
}
// every check of one test (not null)
void check_tile_test(const rrt_tile_test& t) {
    const uint32_t kind = t.test & ~RRT_TILE_KEEP;
    if (kind > RRT_TILE_DIFFERS) throw Error{RRT_ERR_INVALID_ARG, "unknown tile test: want RRT_TILE_NONZERO, RANGE, SET or DIFFERS, optionally | RRT_TILE_KEEP"};
    if (t.elem_bytes != 1 && t.elem_bytes != 4 && t.elem_bytes != 8) throw Error{RRT_ERR_INVALID_ARG, "bad elem_bytes of a tile test: want 1, 4 or 8"};
    if (t.per_pixel != 1 && t.per_pixel != 4) throw Error{RRT_ERR_INVALID_ARG, "bad per_pixel of a tile test: want 1 or 4"};
    if ((kind == RRT_TILE_RANGE || kind == RRT_TILE_SET) && t.elem_bytes != 4) throw Error{RRT_ERR_INVALID_ARG, "RRT_TILE_RANGE and RRT_TILE_SET read 4-byte elements"};
    if (!t.a) throw Error{RRT_ERR_INVALID_ARG, "null plane a of a tile test"};
    if (kind == RRT_TILE_DIFFERS && !t.b) throw Error{RRT_ERR_INVALID_ARG, "null plane b: RRT_TILE_DIFFERS compares a with b"};
    if ((uintptr_t)t.a % t.elem_bytes || (kind == RRT_TILE_DIFFERS && (uintptr_t)t.b % t.elem_bytes))
        throw Error{RRT_ERR_INVALID_ARG, "a plane of a tile test is not aligned to elem_bytes"};
}
// every check of a select call but those of its outputs: returns the frame
TileFrame check_tile_tests(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_tile_test* tests, uint32_t n_tests) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!tests) throw Error{RRT_ERR_INVALID_ARG, "null tile tests"};
    const TileFrame f = check_tile_frame(rt, width, height, region);
    if (n_tests == 0 || n_tests > RRT_MAX_TILE_TESTS) throw Error{RRT_ERR_INVALID_ARG, "bad n_tests: 1 to RRT_MAX_TILE_TESTS tests"};
    for (uint32_t k = 0; k < n_tests; k++) check_tile_test(tests[k]);
    return f;
}
bool reads_b(const rrt_tile_test& t) { return (t.test & ~RRT_TILE_KEEP) == RRT_TILE_DIFFERS; }
size_t tile_plane_bytes(const rrt_tile_test& t, const rrt_region& r) { return (size_t)r.w * r.h * t.per_pixel * t.elem_bytes; }
// The kernel's argument of test t (checked) over planes d_a, d_b in device memory.  The 16-byte path: every 16-byte chunk of a stretch (tiles.hip) is aligned and
// wholly inside or outside the region when the planes, the row pitch and the byte at which the region's rows begin in a row of the frame are multiples of 16.
TileTestParams tile_test_params(const TileFrame& f, const rrt_tile_test& t, const void* d_a, const void* d_b, uint8_t* d_marks, bool keep) {
    TileTestParams q{};
    q.a = d_a; q.b = reads_b(t) ? d_b : nullptr; q.marks = d_marks;
    q.tiles_x = f.tiles_x; q.tiles_y = f.tiles_y;
    q.x0 = f.r.x0; q.y0 = f.r.y0; q.w = f.r.w; q.h = f.r.h;
    q.test = t.test & ~RRT_TILE_KEEP; q.keep = keep || (t.test & RRT_TILE_KEEP) ? 1u : 0u;
    q.elem_bytes = t.elem_bytes; q.per_pixel = t.per_pixel;
    q.lo = t.lo; q.hi = t.hi;
    std::memcpy(q.set, t.set, sizeof q.set);
    const uint64_t pixel_bytes = (uint64_t)t.per_pixel * t.elem_bytes;
    q.vec = (uintptr_t)q.a % 16 == 0 && (uintptr_t)q.b % 16 == 0 && (f.r.w * pixel_bytes) % 16 == 0 && (f.r.x0 * pixel_bytes) % 16 == 0 ? 1u : 0u;
    return q;
}
// tests[0, n) (checked) into d_marks on `stream`, one launch each: the first as given, the later ones joined
void launch_tile_tests(const TileFrame& f, const rrt_tile_test* tests, uint32_t n, const void* const* d_a, const void* const* d_b, uint8_t* d_marks, void* stream) {
    for (uint32_t k = 0; k < n; k++) HIP_TRY((hipError_t)launch_mark_tiles(tile_test_params(f, tests[k], d_a[k], d_b[k], d_marks, k > 0), stream));
}
// the marks into the list: compact.hip's launches with the marks as the flags and nothing to move
void launch_tile_list_of_marks(const TileFrame& f, const uint8_t* d_marks, uint32_t* d_tiles, uint32_t* d_count, void* d_scratch, void* stream) {
    CompactParams q{};
    q.flag = d_marks; q.index = d_tiles; q.tiles = static_cast<uint32_t*>(d_scratch);
    q.n = f.n_tiles; q.select = RRT_SELECT_FLAG;
    HIP_TRY((hipError_t)launch_compact(q, nullptr, d_count, stream));
}
// Host forms (checked): one allocation of the call's own (with_call_planes), the planes the tests read up -- a host plane that several tests name goes up once --
// the launches on the null stream, what was asked for down.  marks: the caller's (up as well when the first test joins them), or none: then only carved.
void tiles_from_host(rrt_raytracer* rt, const TileFrame& f, const rrt_tile_test* tests, uint32_t n, uint8_t* marks, bool want_list, uint32_t* tiles, uint32_t* count) {
    DeviceGuard guard(rt->device);
    enum : size_t { kScratch, kMarks, kTiles, kCount, kA, kB = kA + RRT_MAX_TILE_TESTS, kEnd = kB + RRT_MAX_TILE_TESTS };
    HostPlane pl[kEnd];
    pl[kScratch] = HostPlane{want_list ? rt : nullptr, 1, rrt_compact_scratch_bytes(f.n_tiles), kCarve};   // (only carved: a host pointer that is not null says it is wanted)
    pl[kMarks] = marks ? HostPlane{marks, 1, f.n_tiles, (tests[0].test & RRT_TILE_KEEP) ? kUp | kDown : kDown} : HostPlane{rt, 1, f.n_tiles, kCarve};
    pl[kTiles] = plane_down(tiles, 4, f.n_tiles); pl[kCount] = plane_down(count, 4, 1);
    size_t from_a[RRT_MAX_TILE_TESTS], from_b[RRT_MAX_TILE_TESTS];
    for (size_t e = kA; e < kEnd; e++) pl[e] = HostPlane{nullptr, 1, 0, kUp};
    for (size_t k = 0; k < n; k++) {
        const size_t bytes = tile_plane_bytes(tests[k], f.r);
        auto place = [&](size_t at, const void* host) {
            for (size_t e = kA; e < at; e++) if (pl[e].host == host && pl[e].bytes() >= bytes) return e;   // (the longer of two readings of one address went up)
            pl[at] = plane_up(host, 1, bytes);
            return at;
        };
        from_a[k] = place(kA + k, tests[k].a);
        from_b[k] = reads_b(tests[k]) ? place(kB + k, tests[k].b) : kB + k;
    }
    with_call_planes(pl, [&] {
        const void *d_a[RRT_MAX_TILE_TESTS], *d_b[RRT_MAX_TILE_TESTS];
        for (uint32_t k = 0; k < n; k++) { d_a[k] = pl[from_a[k]].dev; d_b[k] = pl[from_b[k]].dev; }
        rrt_tile_test own[RRT_MAX_TILE_TESTS];
        std::copy(tests, tests + n, own);
        if (!marks) own[0].test &= ~RRT_TILE_KEEP;                          // (no marks of the caller's: nothing to join)
        launch_tile_tests(f, own, n, d_a, d_b, (uint8_t*)pl[kMarks].dev, nullptr);
        if (want_list) launch_tile_list_of_marks(f, (const uint8_t*)pl[kMarks].dev, (uint32_t*)pl[kTiles].dev, (uint32_t*)pl[kCount].dev, pl[kScratch].dev, nullptr);
    });
}

// every check of a frame's call, before any GPU work; returns the region in force
rrt_region check_ambient(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_surface* planes, const rrt_ambient_samples* samples,
                         const rrt_ambient* out) {
    check_frame(rt, width, height);
    if (!planes || !samples || !out) throw Error{RRT_ERR_INVALID_ARG, "null struct: ambient occlusion takes the surface planes, the sample table and the output planes"};
    if (!planes->point || !planes->normal || !planes->material) throw Error{RRT_ERR_INVALID_ARG, "null plane: point, normal and material are all required"};
    if (!out->occluded && !out->grey) throw Error{RRT_ERR_INVALID_ARG, "no output requested: occluded and grey are both null"};
    check_ambient_samples(*samples);
    return region_in_force(width, height, region);
}

// the masks and grey pixels of a region or a list (checked) from planes in device memory
template <class Front>
void launch_ambient_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const Place<Front>& at, const rrt_surface& d_planes, const rrt_ambient_samples& samples,
                          const rrt_ambient& d_out, void* stream) {
    launch_stage_frame(rt, width, height, AmbientStage<Front>{bare(at.front), ambient_planes(d_planes, samples, d_out)}, at.rays_primary, stream);
}

// Host form: the three planes up, the requested outputs down.
void ambient_from_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_surface& planes, const rrt_ambient_samples& samples,
                       const rrt_ambient& out) {
    DeviceGuard guard(rt->device);
    const size_t px = (size_t)r.w * r.h, n = 4 * px;
    HostPlane pl[kSurf + kAmb];
    mirror_planes(pl, planes, n, SurfDirs().set(kUp, &rrt_surface::point, &rrt_surface::normal, &rrt_surface::material));
    const size_t count[kAmb] = {n, px};                                  // occluded per sub-sample, grey per pixel
    mirror_planes(pl + kSurf, out, count, FieldDirs<rrt_ambient>::every(kDown));
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_ambient_frame(rt, width, height, in_region(rt, width, height, r), mirrored<rrt_surface>(pl), samples, mirrored<rrt_ambient>(pl + kSurf), stream);
    });
}

}  // namespace

extern "C" {

int rrt_render_visibility_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* d_planes, void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_visibility(rt, width, height, region, d_planes);
        DeviceGuard guard(rt->device);
        launch_visibility_frame(rt, width, height, in_region(rt, width, height, r), *d_planes, stream);
        return RRT_OK;
    });
}

int rrt_render_visibility(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* planes) {
    return guarded([&]() -> int {
        const rrt_region r = check_visibility(rt, width, height, region, planes);
        visibility_to_host(rt, width, height, r, *planes);
        return RRT_OK;
    });
}

int rrt_render_surface_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* d_vis, const rrt_surface* d_planes,
                              void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_surface(rt, width, height, region, d_planes);
        DeviceGuard guard(rt->device);
        launch_surface_frame(rt, width, height, in_region(rt, width, height, r), d_vis ? *d_vis : rrt_visibility{}, *d_planes, stream);
        return RRT_OK;
    });
}

int rrt_render_surface(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* vis, const rrt_surface* planes) {
    return guarded([&]() -> int {
        const rrt_region r = check_surface(rt, width, height, region, planes);
        surface_to_host(rt, width, height, r, vis ? *vis : rrt_visibility{}, *planes);
        return RRT_OK;
    });
}

int rrt_shade_surface_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* d_vis, const rrt_surface* d_planes,
                             void* d_fb, void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_shade(rt, width, height, region, d_vis, d_planes, d_fb);
        DeviceGuard guard(rt->device);
        launch_shade_frame(rt, width, height, in_region(rt, width, height, r), *d_vis, *d_planes, d_fb, stream);
        return RRT_OK;
    });
}

int rrt_shade_surface(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* vis, const rrt_surface* planes,
                      uint32_t* out_fb) {
    return guarded([&]() -> int {
        const rrt_region r = check_shade(rt, width, height, region, vis, planes, out_fb);
        shade_from_host(rt, width, height, r, *vis, *planes, out_fb);
        return RRT_OK;
    });
}

int rrt_render_region_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t* d_out, uint32_t pitch, void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_render_region(rt, width, height, region, d_out, pitch);
        DeviceGuard guard(rt->device);
        launch_render_region_frame(rt, width, height, r, d_out, pitch, stream);
        return RRT_OK;
    });
}

int rrt_render_region(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t* out, uint32_t pitch) {
    return guarded([&]() -> int {
        const rrt_region r = check_render_region(rt, width, height, region, out, pitch);
        render_region_to_host(rt, width, height, r, out, pitch);
        return RRT_OK;
    });
}

int rrt_render_tile_list_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles, uint32_t* d_fb,
                                void* stream) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!d_fb) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
        if (!check_tile_list(n, d_tiles)) return RRT_OK;
        DeviceGuard guard(rt->device);
        const Place<TileList> at = in_list(rt, width, height, n, d_count, d_tiles);
        launch_stage_frame(rt, width, height, TileListParams{at.front, d_fb}, at.rays_primary, stream);
        return RRT_OK;
    });
}

int rrt_render_visibility_tile_list_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles,
                                           const rrt_visibility* d_planes, void* stream) {
    return guarded([&]() -> int {
        check_visibility(rt, width, height, nullptr, d_planes);
        if (!check_tile_list(n, d_tiles)) return RRT_OK;
        DeviceGuard guard(rt->device);
        launch_visibility_frame(rt, width, height, in_list(rt, width, height, n, d_count, d_tiles), *d_planes, stream);
        return RRT_OK;
    });
}

int rrt_render_surface_tile_list_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles,
                                        const rrt_visibility* d_vis, const rrt_surface* d_planes, void* stream) {
    return guarded([&]() -> int {
        check_surface(rt, width, height, nullptr, d_planes);
        if (!check_tile_list(n, d_tiles)) return RRT_OK;
        DeviceGuard guard(rt->device);
        launch_surface_frame(rt, width, height, in_list(rt, width, height, n, d_count, d_tiles), d_vis ? *d_vis : rrt_visibility{}, *d_planes, stream);
        return RRT_OK;
    });
}

int rrt_shade_surface_tile_list_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles,
                                       const rrt_visibility* d_vis, const rrt_surface* d_planes, void* d_fb, void* stream) {
    return guarded([&]() -> int {
        check_shade(rt, width, height, nullptr, d_vis, d_planes, d_fb);
        if (!check_tile_list(n, d_tiles)) return RRT_OK;
        DeviceGuard guard(rt->device);
        launch_shade_frame(rt, width, height, in_list(rt, width, height, n, d_count, d_tiles), *d_vis, *d_planes, d_fb, stream);
        return RRT_OK;
    });
}

int rrt_ambient_surface_tile_list_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles,
                                         const rrt_surface* d_planes, const rrt_ambient_samples* samples, const rrt_ambient* d_out, void* stream) {
    return guarded([&]() -> int {
        check_ambient(rt, width, height, nullptr, d_planes, samples, d_out);
        if (!check_tile_list(n, d_tiles)) return RRT_OK;
        DeviceGuard guard(rt->device);
        launch_ambient_frame(rt, width, height, in_list(rt, width, height, n, d_count, d_tiles), *d_planes, *samples, *d_out, stream);
        return RRT_OK;
    });
}

int rrt_mark_tiles_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_tile_test* test, uint8_t* d_marks, void* stream) {
    return guarded([&]() -> int {
        const TileFrame f = check_tile_tests(rt, width, height, region, test, 1);
        if (!d_marks) throw Error{RRT_ERR_INVALID_ARG, "null marks"};
        DeviceGuard guard(rt->device);
        launch_tile_tests(f, test, 1, &test->a, &test->b, d_marks, stream);
        return RRT_OK;
    });
}

int rrt_mark_tiles(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_tile_test* test, uint8_t* marks) {
    return guarded([&]() -> int {
        const TileFrame f = check_tile_tests(rt, width, height, region, test, 1);
        if (!marks) throw Error{RRT_ERR_INVALID_ARG, "null marks"};
        tiles_from_host(rt, f, test, 1, marks, false, nullptr, nullptr);
        return RRT_OK;
    });
}

int rrt_select_tiles_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_tile_test* tests, uint32_t n_tests, uint8_t* d_marks,
                            uint32_t* d_tiles, uint32_t* d_count, void* d_scratch, size_t scratch_bytes, void* stream) {
    return guarded([&]() -> int {
        const TileFrame f = check_tile_tests(rt, width, height, region, tests, n_tests);
        if (!d_marks) throw Error{RRT_ERR_INVALID_ARG, "null marks"};
        if (!d_tiles && !d_count) throw Error{RRT_ERR_INVALID_ARG, "no output requested: the list and the count are both null"};
        if (!d_scratch || scratch_bytes < rrt_compact_scratch_bytes(f.n_tiles)) throw Error{RRT_ERR_INVALID_ARG, "scratch too small or null: want rrt_compact_scratch_bytes(n_tiles) bytes of device memory"};
        DeviceGuard guard(rt->device);
        const void *d_a[RRT_MAX_TILE_TESTS], *d_b[RRT_MAX_TILE_TESTS];
        for (uint32_t k = 0; k < n_tests; k++) { d_a[k] = tests[k].a; d_b[k] = tests[k].b; }
        launch_tile_tests(f, tests, n_tests, d_a, d_b, d_marks, stream);
        launch_tile_list_of_marks(f, d_marks, d_tiles, d_count, d_scratch, stream);
        return RRT_OK;
    });
}

int rrt_select_tiles(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_tile_test* tests, uint32_t n_tests, uint32_t* tiles,
                     uint32_t* count) {
    return guarded([&]() -> int {
        const TileFrame f = check_tile_tests(rt, width, height, region, tests, n_tests);
        if (!tiles && !count) throw Error{RRT_ERR_INVALID_ARG, "no output requested: the list and the count are both null"};
        tiles_from_host(rt, f, tests, n_tests, nullptr, true, tiles, count);
        return RRT_OK;
    });
}

int rrt_ambient_surface_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_surface* d_planes,
                               const rrt_ambient_samples* samples, const rrt_ambient* d_out, void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_ambient(rt, width, height, region, d_planes, samples, d_out);
        DeviceGuard guard(rt->device);
        launch_ambient_frame(rt, width, height, in_region(rt, width, height, r), *d_planes, *samples, *d_out, stream);
        return RRT_OK;
    });
}

int rrt_ambient_surface(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_surface* planes,
                        const rrt_ambient_samples* samples, const rrt_ambient* out) {
    return guarded([&]() -> int {
        const rrt_region r = check_ambient(rt, width, height, region, planes, samples, out);
        ambient_from_host(rt, width, height, r, *planes, *samples, *out);
        return RRT_OK;
    });
}

int rrt_pick(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t px, uint32_t py, rrt_pick_result* out) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!out) throw Error{RRT_ERR_INVALID_ARG, "null result"};
        if (px >= width || py >= height) throw Error{RRT_ERR_INVALID_ARG, "pixel outside the frame"};
        *out = pick_pixel(rt, width, height, px, py);
        return RRT_OK;
    });
}

}  // extern "C"
