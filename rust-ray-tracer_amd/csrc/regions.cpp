// regions.cpp -- regions of a frame behind include/rrt.h: visibility and surface buffers, frames shaded and ambient occlusion from kept buffers, the pick of one
// pixel, the fused frame of a region and of a list of tiles in device memory.  The calls share one check of the region (host_planes.hpp: region_in_force), one launch (launch_region_frame) and, for their host forms, the routine that
// carves the kept device allocation and copies the planes up and down (launches.hpp: with_kept_planes) over the mirrored structs (host_planes.hpp: mirror_planes).
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

// the kernels' argument for region r (checked) of a frame and these planes
VisParams vis_params(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& d_planes) {
    VisParams p{};
    p.F = frame_params(rt, width, height, 0, 1, false);
    p.F.row_begin = r.y0; p.F.row_end = r.y0 + r.h;
    p.col_begin = r.x0; p.col_end = r.x0 + r.w;
    p.tile_x0 = r.x0 / 8; p.tile_y0 = r.y0 / 8;
    p.tiles_w = (p.col_end + 7) / 8 - p.tile_x0;
    p.F.tile_begin = 0; p.F.tile_end = p.tiles_w * ((p.F.row_end + 7) / 8 - p.tile_y0);
    p.hit = d_planes.hit; p.t = d_planes.t; p.u = d_planes.u; p.v = d_planes.v; p.tri = d_planes.tri; p.albedo = d_planes.albedo;
    return p;
}

// The one region launch: the finished kernel argument q of region r (checked) on the caller's stream, timed by the raytracer's events and recorded.
template <class Params> void launch_region_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const Params& q, void* stream) {
    const int variant = visibility_variant(rt, width, height);
    timed_launch(rt, stream, [&] { return launch_region(rt->scene, q, stream, variant); });
    record(rt, width, height, 4 * traced_pixels_in(r, width, height), variant);
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

// the planes of region r (checked) into device memory
void launch_visibility_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& d_planes, void* stream) {
    launch_region_frame(rt, width, height, r, vis_params(rt, width, height, r, d_planes), stream);
}

void visibility_to_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& planes) {
    DeviceGuard guard(rt->device);
    HostPlane pl[kVis];
    mirror_planes(pl, planes, 4 * (size_t)r.w * r.h, VisDirs::every(kDown));
    with_kept_planes(rt, pl, [&](void* stream) { launch_visibility_frame(rt, width, height, r, mirrored<rrt_visibility>(pl), stream); });
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
        launch_visibility_frame(rt, width, height, rrt_region{px, py, 1, 1}, d, stream);
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

void launch_surface_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& d_vis, const rrt_surface& d_planes, void* stream) {
    SurfaceParams q{};
    q.V = vis_params(rt, width, height, r, d_vis);
    q.point = d_planes.point; q.normal = d_planes.normal; q.material = d_planes.material; q.lights = d_planes.lights;
    launch_region_frame(rt, width, height, r, q, stream);
}

void surface_to_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& vis, const rrt_surface& planes) {
    DeviceGuard guard(rt->device);
    const size_t n = 4 * (size_t)r.w * r.h;
    HostPlane pl[kVis + kSurf];
    mirror_planes(pl, vis, n, VisDirs::every(kDown));
    mirror_planes(pl + kVis, planes, n, SurfDirs::every(kDown));
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_surface_frame(rt, width, height, r, mirrored<rrt_visibility>(pl), mirrored<rrt_surface>(pl + kVis), stream);
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

// the pixels of region r (checked) from planes in device memory into d_fb
void launch_shade_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& d_vis, const rrt_surface& d_planes, void* d_fb, void* stream) {
    ShadeParams q{};
    q.V = vis_params(rt, width, height, r, rrt_visibility{});            // (the kernel writes no plane)
    q.point = d_planes.point; q.normal = d_planes.normal; q.material = d_planes.material; q.albedo = d_vis.albedo; q.lights = d_planes.lights;
    q.out = static_cast<uint32_t*>(d_fb);
    launch_region_frame(rt, width, height, r, q, stream);
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
        launch_shade_frame(rt, width, height, r, mirrored<rrt_visibility>(pl + kAlbedo), mirrored<rrt_surface>(pl + kSurfA, pl + kSurfB), pl[kOut].dev, stream);
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
    RenderRegionParams q{};
    q.V = vis_params(rt, width, height, r, rrt_visibility{});            // (the kernel writes no plane)
    q.out = d_out; q.pitch = pitch;
    launch_region_frame(rt, width, height, r, q, stream);
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

// ---- the fused frame of a tile list in device memory.  Nothing of the list is read here: the kernel reads it, and the bound, when it runs.
static_assert(kMaxTileList == RRT_MAX_TILE_LIST, "rrt.h names the launch bound of a tile list");
void launch_tile_list_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_count, const uint32_t* d_tiles, uint32_t* d_fb, void* stream) {
    TileListParams q{};
    q.F = frame_params(rt, width, height, 0, 1, false);
    q.F.xcd_chunk = 0;                                                   // the caller's order is the schedule
    q.tiles = d_tiles; q.count = d_count; q.n = n; q.out = d_fb;
    const int variant = visibility_variant(rt, width, height);
    timed_launch(rt, stream, [&] { return launch_tile_list(rt->scene, q, stream, variant); });
    record(rt, width, height, 0, variant);                               // (the library does not know which tiles the list names)
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

// the masks and grey pixels of region r (checked) from planes in device memory.  The sample table is copied into the kernel's argument here: no device memory holds it.
void launch_ambient_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_surface& d_planes, const rrt_ambient_samples& samples,
                          const rrt_ambient& d_out, void* stream) {
    AmbientParams q{};
    q.V = vis_params(rt, width, height, r, rrt_visibility{});            // (the kernel writes no visibility plane)
    q.point = d_planes.point; q.normal = d_planes.normal; q.material = d_planes.material;
    q.occluded = d_out.occluded; q.grey = d_out.grey;
    q.n_samples = samples.n; q.max_t = samples.max_t;
    std::memcpy(q.dirs, samples.dirs, sizeof(double) * 3 * samples.n);
    launch_region_frame(rt, width, height, r, q, stream);
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
        launch_ambient_frame(rt, width, height, r, mirrored<rrt_surface>(pl), samples, mirrored<rrt_ambient>(pl + kSurf), stream);
    });
}

}  // namespace

extern "C" {

int rrt_render_visibility_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_visibility* d_planes, void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_visibility(rt, width, height, region, d_planes);
        DeviceGuard guard(rt->device);
        launch_visibility_frame(rt, width, height, r, *d_planes, stream);
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
        launch_surface_frame(rt, width, height, r, d_vis ? *d_vis : rrt_visibility{}, *d_planes, stream);
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
        launch_shade_frame(rt, width, height, r, *d_vis, *d_planes, d_fb, stream);
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
        if (n > kMaxTileList) throw Error{RRT_ERR_INVALID_ARG, "the list is longer than RRT_MAX_TILE_LIST entries: its grid would not fit a launch"};
        if (n == 0) return RRT_OK;                                         // nothing is launched, rrt_last_stats stays as it was
        if (!d_tiles) throw Error{RRT_ERR_INVALID_ARG, "null tile list"};
        DeviceGuard guard(rt->device);
        launch_tile_list_frame(rt, width, height, n, d_count, d_tiles, d_fb, stream);
        return RRT_OK;
    });
}

int rrt_ambient_surface_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, const rrt_surface* d_planes,
                               const rrt_ambient_samples* samples, const rrt_ambient* d_out, void* stream) {
    return guarded([&]() -> int {
        const rrt_region r = check_ambient(rt, width, height, region, d_planes, samples, d_out);
        DeviceGuard guard(rt->device);
        launch_ambient_frame(rt, width, height, r, *d_planes, *samples, *d_out, stream);
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
