// frames.cpp -- every launch behind include/rrt.h.
//   Frames: into a device framebuffer or a rank's tiles, into host memory, progressively.
//   Regions of a frame: visibility and surface buffers, frames shaded and ambient occlusion from kept buffers, the pick of one pixel.
//   Per-ray queries, the choice of the traversal variant, and the statistics of the last launch.
//   Compaction of ray batches and records between two per-ray stages, its inverse (compact.hip) and their sort by a coherence key (sort.hip): no ray is traced, so
//   these go past timed_launch and record.
//   The two ends of that pipeline -- a frame's primary rays as a batch, the unwind of one level, the pixels (wavefront.hip) -- and the frame by ray generations
//   that strings the stages together.
// Every launch goes through ONE seam: timed_launch (the raytracer's two events around it) and record (what it traced, into rrt_stats).  Every measurement of the
// variants goes through fastest_variant.  The region calls share one check of the region (region_in_force), one launch (launch_region_frame) and, for their host
// forms, one routine that carves the kept device allocation and copies the planes up and down (with_kept_planes).  The host forms of the per-ray calls, of compaction
// and of scatter share its sibling for a call that owns its memory (with_call_planes: one allocation per call, blocking copies, the null stream), and every per-ray
// launch that does not measure is timed and recorded in one place (recorded_ray_launch).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "api_internal.hpp"
#include "staging.hpp"

namespace {

using namespace rrt;

FrameParams frame_params(const rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t rank, uint32_t world, bool tiled) {
    FrameParams f{};
    f.width = width; f.height = height;
    f.x_scale = rt->opt.vp_w / (double)width;      // engine.rs:189
    f.y_scale = rt->opt.vp_h / (double)height;     // engine.rs:190
    f.z_value = rt->opt.vp_d;                      // engine.rs:191
    f.tiles_x = (width + 7) / 8; f.tiles_y = (height + 7) / 8;
    f.rank = rank; f.world = world; f.tiled_output = tiled ? 1u : 0u;
    f.tile_begin = 0; f.tile_end = f.tiles_x * f.tiles_y; f.row_begin = 0; f.row_end = height;
    const rrt_camera& c = rt->cam;                 // rrt_raytracer_set_camera; the eye itself is rt->scene.origin
    f.right[0] = c.right.x; f.right[1] = c.right.y; f.right[2] = c.right.z;
    f.up[0] = c.up.x; f.up[1] = c.up.y; f.up[2] = c.up.z;
    f.forward[0] = c.forward.x; f.forward[1] = c.forward.y; f.forward[2] = c.forward.z;
    // XCD-aware block order (render.hip): worth 2-4 % where the scene is far larger than an XCD's L2 (100 k / 1 M-triangle soups), costs 4 % on the teapot
    // (profiles/r03_xcd_chunk_sweep.txt; chunks as 64 x 64-pixel squares instead of 512 x 8 strips: 1 % slower again): on for scenes of 50 000 triangle slots and more.
    static const int forced = [] { const char* e = std::getenv("RRT_XCD_CHUNK"); return e ? std::atoi(e) : -1; }();
    f.xcd_chunk = forced >= 0 ? (uint32_t)forced : (rt->scene.n_slots >= 50000u ? 256u : 0u);
    return f;
}

// ---- the one timed launch and the one record of it.
// `launch` (returns hipError_t, as int) between the raytracer's two events on `stream`: rrt_last_stats reads the time between them.
template <class Launch> void timed_launch(rrt_raytracer* rt, void* stream, Launch&& launch) {
    HIP_TRY(hipEventRecord(rt->ev0, (hipStream_t)stream));
    HIP_TRY((hipError_t)launch());
    HIP_TRY(hipEventRecord(rt->ev1, (hipStream_t)stream));
}
// (blocking) the time between the two events of the last timed_launch
float elapsed_ms(rrt_raytracer* rt) {
    float ms = 0;
    HIP_TRY(hipEventSynchronize(rt->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, rt->ev0, rt->ev1));
    return ms;
}
// traced pixels (render_kernel): columns [0, 2*(W/2)), rows [H - 2*(H/2) + 1, H) -- of a region, and of the whole frame
uint64_t traced_pixels_in(const rrt_region& r, uint32_t width, uint32_t height) {
    const uint64_t col_end = std::min<uint64_t>((uint64_t)r.x0 + r.w, 2ull * (width / 2)), row_begin = std::max<uint64_t>(r.y0, (uint64_t)height - 2ull * (height / 2) + 1);
    const uint64_t cols = col_end > r.x0 ? col_end - r.x0 : 0, rows = (uint64_t)r.y0 + r.h > row_begin ? (uint64_t)r.y0 + r.h - row_begin : 0;
    return cols * rows;
}
uint64_t traced_pixels(uint32_t width, uint32_t height) { return traced_pixels_in(rrt_region{0, 0, width, height}, width, height); }
// what the last launch was, into rrt_stats: a frame's size, or (n, 1) for n rays; rays_primary is 0 for a rank's share (not tracked)
void record(rrt_raytracer* rt, uint32_t width, uint32_t height, uint64_t rays_primary, int variant) {
    rt->stats.width = width; rt->stats.height = height; rt->stats.rays_primary = rays_primary;
    rt->stats.scene_bytes = rt->scene_bytes; rt->stats.filter_variant = (uint32_t)variant; rt->stats.origin_plane_triangles = rt->scene.n_suspects;
    rt->stats_pending = true; rt->launched = true;
}
// Every variant twice (the first run warms caches), the second time counts; the fastest, the lowest index on a tie.  time_one(variant) -> ms, blocking.
template <class TimeOne> int fastest_variant(TimeOne&& time_one) {
    float best = 0; int best_v = 0;
    for (int variant = 0; variant < 3; variant++) {
        (void)time_one(variant);
        const float ms = time_one(variant);
        if (variant == 0 || ms < best) { best = ms; best_v = variant; }
    }
    return best_v;
}

// All traversal variants produce identical pixels; which is faster depends on how coherent the rays of a wave are (scene, camera, frame size).
// The reference renders ONE frame per run, so the first frame of a size costs nothing extra: it runs the variant a measured rule picks (node-coherent
// walk; bundle filter when the frame has more than ~1200 primary rays per triangle, lane filter below).  A caller that comes back for a SECOND
// frame of the same size is rendering repeatedly, and that frame is first rendered with every variant (each twice: the first run warms caches) on the
// caller's buffer and stream, timed with HIP events; the fastest is kept for that size.  This synchronises the stream once per size.
// First frame of a size (for a host that renders one frame per run, as the reference does, this IS the choice): the bundle filter pays once the
// frame holds enough rays per triangle for a 4x4-pixel wave to stay inside few nodes and long lists -- measured over 3 models x 5 frame sizes
// and the 100 k soup (profiles/r03_variant_sweep.json, re-measured with the final kernels: bundle wins at >= 1234 primary rays per triangle, by 4-12 %;
// lane filter wins at <= 719, by 12-180 %; nothing measured in between).
int first_frame_variant(const rrt_raytracer* rt, uint32_t width, uint32_t height) {
    const double rays_per_triangle = 4.0 * (double)width * (double)height / (double)(rt->scene.n_slots ? rt->scene.n_slots : 1u);
    return rays_per_triangle > 1200.0 ? 1 : 0;
}

void tune_variant(rrt_raytracer* rt, const FrameParams& f, uint32_t* d_out, void* stream) {
    if (rt->variant_forced) return;
    if (!(rt->tuned_w == f.width && rt->tuned_h == f.height && rt->tuned_world == f.world)) {
        rt->tuned_w = f.width; rt->tuned_h = f.height; rt->tuned_world = f.world;
        rt->size_frames = 0; rt->size_measured = false;
        rt->walk = first_frame_variant(rt, f.width, f.height);
    }
    if (rt->size_measured) return;
    if (++rt->size_frames < 2) return;
    rt->size_measured = true;
    if (f.world == 1) {
        rt->walk = fastest_variant([&](int variant) {
            timed_launch(rt, stream, [&] { return launch_render(rt->scene, f, d_out, stream, variant); });
            return elapsed_ms(rt);
        });
        return;
    }
    // One rank's share of a frame is a SHORT launch (a few waves per wave slot): alone it is bound by the latency of its last waves, not by
    // throughput, and a multi-GPU host keeps several frames in flight on separate streams precisely to hide that (bench.py).
    // So the variants are compared the way they will run: three launches at once on three streams, wall time per variant.
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    OwnedStream st[3];
    for (auto& q : st) HIP_TRY(hipStreamCreateWithFlags(&q.h, hipStreamNonBlocking));
    rt->walk = fastest_variant([&](int variant) {
        timed_launch(rt, st[0].h, [&] {
            for (int round = 0; round < 2; round++)
                for (auto& q : st) HIP_TRY((hipError_t)launch_render(rt->scene, f, d_out, q.h, variant));   // same pixels from every launch: the overlapping writes agree
            for (int i = 1; i < 3; i++) HIP_TRY(hipStreamSynchronize(st[i].h));
            return 0;
        });
        return elapsed_ms(rt);
    });
}

// The per-ray entry points take whatever rays the caller has: a coherent pixel grid or rays in all directions, and the three traversal variants are
// up to 5x apart on those (scattered rays: the ray walk; tools/random_rays_probe.py).  The first batch of at least kTuneMinRays rays is therefore
// used to measure them on its first kTuneSample rays (each twice, the first run warms caches; same outputs from every variant), and the fastest is
// kept for later calls.  A forced variant (RRT_FLAG_*_FILTER / RAY_WALK / NO_CULL) is used as is; smaller batches run the frame variant.
constexpr uint32_t kTuneMinRays = 16384, kTuneSample = 65536;
// the measurement: launch(variant) on the null stream; the result replaces an earlier one
template <class Launch> int measure_rays(rrt_raytracer* rt, Launch&& launch) {
    return rt->walk_rays = fastest_variant([&](int variant) {
        timed_launch(rt, nullptr, [&] { return launch(variant); });
        return elapsed_ms(rt);
    });
}
// the policy of the host forms; launch(m, variant) traces the first m rays of the batch
template <class Launch> int rays_variant(rrt_raytracer* rt, uint32_t n, Launch&& launch) {
    if (rt->variant_forced) return rt->walk;
    if (rt->walk_rays >= 0) return rt->walk_rays;
    if (n < kTuneMinRays) return rt->walk;
    return measure_rays(rt, [&](int variant) { return launch(std::min(n, kTuneSample), variant); });
}
// The device forms (rrt_intersect_rays_device, ...) never measure: the forced variant, else the one kept for per-ray calls, else the frame variant.
int device_rays_variant(const rrt_raytracer* rt) {
    if (rt->variant_forced) return rt->walk;
    return rt->walk_rays >= 0 ? rt->walk_rays : rt->walk;
}
// every check of a per-ray call, before any GPU work; n == 0 is a no-op
void check_rays(const rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, bool outputs_ok) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (n && (!origins || !dirs)) throw Error{RRT_ERR_INVALID_ARG, "null ray origins or directions"};
    if (n && !outputs_ok) throw Error{RRT_ERR_INVALID_ARG, "null output: a device form and rrt_surface_rays need one output pointer at least, the other host forms every one of their outputs"};
}

// one frame (or one rank's tiles of it) into a device buffer on the caller's stream, timed by the raytracer's events
void launch_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t rank, uint32_t world, bool tiled, void* d_out, void* stream) {
    DeviceGuard guard(rt->device);
    const FrameParams f = frame_params(rt, width, height, rank, world, tiled);
    tune_variant(rt, f, static_cast<uint32_t*>(d_out), stream);
    timed_launch(rt, stream, [&] { return launch_render(rt->scene, f, static_cast<uint32_t*>(d_out), stream, rt->walk); });
    record(rt, width, height, world == 1 ? 4 * traced_pixels(width, height) : 0, rt->walk);
}

// ---- regions of a frame: visibility buffers, surface buffers, shading and ambient occlusion from kept buffers, pick.  Each is one launch of its kernel over the tiles
// the region touches (rrt.h: rrt_render_visibility_device, rrt_render_surface_device, rrt_shade_surface_device, rrt_ambient_surface_device).
// The variant: the forced one, else the one kept for this frame size, else the first-frame rule's.  Reads the tuning state, never writes it: a
// region call is not a frame of that size.
int visibility_variant(const rrt_raytracer* rt, uint32_t width, uint32_t height) {
    if (rt->variant_forced) return rt->walk;
    if (rt->tuned_w == width && rt->tuned_h == height && rt->tuned_world == 1u) return rt->walk;
    return first_frame_variant(rt, width, height);
}

// The region in force: the caller's, or the whole frame; the last check of every region call, after those of its own arguments.
rrt_region region_in_force(uint32_t width, uint32_t height, const rrt_region* region) {
    const rrt_region r = region ? *region : rrt_region{0, 0, width, height};
    if (r.w == 0 || r.h == 0) throw Error{RRT_ERR_INVALID_ARG, "empty region"};
    if ((uint64_t)r.x0 + r.w > width || (uint64_t)r.y0 + r.h > height) throw Error{RRT_ERR_INVALID_ARG, "region sticks out of the frame"};
    return r;
}

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

// ---- the host forms of the region calls.  A plane of the caller's in host memory, and where it lives in the raytracer's kept device allocation for one call.
enum : int { kCarve = 0, kUp = 1, kDown = 2 };       // copied host -> device before the launch, device -> host after it (kUp | kDown: both), or only carved
struct HostPlane {
    void* host;              // the caller's pointer; null: the plane is not wanted, it gets no device memory and `dev` stays null
    size_t elem, count;      // bytes per element, elements
    int dir;
    void* dev = nullptr;
    size_t bytes() const { return elem * count; }
};
HostPlane plane_up(const void* host, size_t elem, size_t count) { return HostPlane{const_cast<void*>(host), elem, count, kUp}; }   // (an input is only read)
HostPlane plane_down(void* host, size_t elem, size_t count) { return HostPlane{host, elem, count, kDown}; }
// The six visibility planes of n sub-samples into pl[0, 6), in the order of rrt_visibility -- hit, t, u, v, tri, albedo -- and back as device pointers.  (rrt_pick
// relies on this order: see pick_pixel.)
constexpr int kPlanes = 6;
void visibility_planes(HostPlane* pl, const rrt_visibility& v, size_t n, int dir) {
    pl[0] = {v.hit, 1, n, dir}; pl[1] = {v.t, 8, n, dir}; pl[2] = {v.u, 8, n, dir}; pl[3] = {v.v, 8, n, dir}; pl[4] = {v.tri, 4, n, dir}; pl[5] = {v.albedo, 4, n, dir};
}
rrt_visibility device_visibility(const HostPlane* pl) {
    return rrt_visibility{(uint8_t*)pl[0].dev, (double*)pl[1].dev, (double*)pl[2].dev, (double*)pl[3].dev, (uint32_t*)pl[4].dev, (uint32_t*)pl[5].dev};
}

// the raytracer's own stream, for the calls that bring results into host memory: the device's shared set-up stream (staging.hpp: setup_stream; not owned)
hipStream_t own_stream(rrt_raytracer* rt) {
    if (!rt->own_stream) rt->own_stream = (hipStream_t)setup_stream();
    return rt->own_stream;
}

// The two pure pieces of a host-form call: the device bytes the wanted planes of a list need, a slot each (device_memory.hpp: slot_bytes), and their carving out of
// an arena IN THE ORDER OF THE LIST.
template <size_t K> size_t planes_bytes(const HostPlane (&planes)[K]) {
    size_t need = 0;
    for (const HostPlane& p : planes) if (p.host) need += slot_bytes(p.bytes());
    return need;
}
template <size_t K> void carve_planes(HostPlane (&planes)[K], DevArena arena) {
    for (HostPlane& p : planes) if (p.host) p.dev = arena.take<char>(p.bytes());
}

// One host-form call: the wanted planes carved out of the raytracer's kept device allocation (grown when a larger request comes) IN THE ORDER OF `planes` from offset
// 0, each in a slot of its own (device_memory.hpp: slot_bytes); the inputs up, launch(stream) on the raytracer's own stream, the outputs down, one wait.  Blocking:
// on return the outputs are in the caller's memory and its inputs are no longer read.
// (a page-locked plane's copy is only enqueued: all of those are in flight before the one wait)
template <size_t K, class Launch> void with_kept_planes(rrt_raytracer* rt, HostPlane (&planes)[K], Launch&& launch) {
    const size_t need = planes_bytes(planes);
    carve_planes(planes, DevArena{static_cast<char*>(rt->vis_buf.at_least(need)), rt->vis_buf.bytes, 0});
    const hipStream_t stream = own_stream(rt);
    for (const HostPlane& p : planes) if (p.host && (p.dir & kUp)) staged_upload(p.dev, p.host, p.bytes(), stream);
    launch(stream);
    for (const HostPlane& p : planes) if (p.host && (p.dir & kDown)) staged_download(p.host, p.dev, p.bytes(), stream);
    HIP_TRY(hipStreamSynchronize(stream));
}
// Its sibling for a call that owns its memory (the per-ray calls, compaction, scatter): the wanted planes carved from offset 0 of ONE device allocation made here and
// freed on return, or on a throw -- nothing is kept between calls; the inputs up, launch() on the null stream, the outputs down, every copy blocking: no wait of its own.
// (not one routine with with_kept_planes: kept or own allocation, own or null stream, staged or blocking copies, one wait or none -- it would branch on its caller)
template <size_t K, class Launch> void with_call_planes(HostPlane (&planes)[K], Launch&& launch) {
    const size_t need = planes_bytes(planes);
    const DevBuf mem = dev_alloc(need);
    carve_planes(planes, DevArena{static_cast<char*>(mem.h), need, 0});
    for (const HostPlane& p : planes) if (p.host && (p.dir & kUp)) HIP_TRY(hipMemcpy(p.dev, p.host, p.bytes(), hipMemcpyHostToDevice));
    launch();
    for (const HostPlane& p : planes) if (p.host && (p.dir & kDown)) HIP_TRY(hipMemcpy(p.host, p.dev, p.bytes(), hipMemcpyDeviceToHost));
}

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
    HostPlane pl[kPlanes];
    visibility_planes(pl, planes, 4 * (size_t)r.w * r.h, kDown);
    with_kept_planes(rt, pl, [&](void* stream) { launch_visibility_frame(rt, width, height, r, device_visibility(pl), stream); });
}

// One pixel: a one-tile launch into the kept allocation and ONE copy of its six plane slots back.  All six planes of the pixel's four sub-samples are wanted and fit
// a slot each, so plane k starts at byte 256 * k of the allocation, in the order of visibility_planes; sub-sample 0 is the answer.
rrt_pick_result pick_pixel(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t px, uint32_t py) {
    DeviceGuard guard(rt->device);
    alignas(8) char back[kPlanes * 256];
    HostPlane pl[kPlanes];
    visibility_planes(pl, rrt_visibility{(uint8_t*)back, (double*)back, (double*)back, (double*)back, (uint32_t*)back, (uint32_t*)back}, 4, kCarve);   // (every plane wanted)
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_visibility_frame(rt, width, height, rrt_region{px, py, 1, 1}, device_visibility(pl), stream);
        HIP_TRY(hipMemcpyAsync(back, pl[0].dev, sizeof back, hipMemcpyDeviceToHost, (hipStream_t)stream));
    });
    rrt_pick_result out{};
    uint8_t hit; std::memcpy(&hit, back, 1); out.hit = hit;
    std::memcpy(&out.t, back + 256, 8); std::memcpy(&out.u, back + 512, 8); std::memcpy(&out.v, back + 768, 8);
    std::memcpy(&out.tri, back + 1024, 4); std::memcpy(&out.albedo, back + 1280, 4);
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
    HostPlane pl[kPlanes + 4];
    visibility_planes(pl, vis, n, kDown);
    pl[6] = plane_down(planes.point, 24, n); pl[7] = plane_down(planes.normal, 24, n); pl[8] = plane_down(planes.material, 4, n); pl[9] = plane_down(planes.lights, 4, n);
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_surface_frame(rt, width, height, r, device_visibility(pl), rrt_surface{(double*)pl[6].dev, (double*)pl[7].dev, (uint32_t*)pl[8].dev, (uint32_t*)pl[9].dev}, stream);
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

// Host form: the given planes up, the region's pixels down.
void shade_from_host(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region& r, const rrt_visibility& vis, const rrt_surface& planes, uint32_t* out_fb) {
    DeviceGuard guard(rt->device);
    const size_t px = (size_t)r.w * r.h, n = 4 * px;
    HostPlane pl[] = {plane_up(planes.point, 24, n), plane_up(planes.normal, 24, n), plane_up(planes.material, 4, n), plane_up(vis.albedo, 4, n), plane_up(planes.lights, 4, n),
                      plane_down(out_fb, sizeof(uint32_t), px)};
    with_kept_planes(rt, pl, [&](void* stream) {
        rrt_visibility d_vis{}; d_vis.albedo = (uint32_t*)pl[3].dev;
        launch_shade_frame(rt, width, height, r, d_vis, rrt_surface{(double*)pl[0].dev, (double*)pl[1].dev, (uint32_t*)pl[2].dev, (uint32_t*)pl[4].dev}, pl[5].dev, stream);
    });
}

// ---- ambient occlusion from kept planes and from ray records.  The checks of a sample table (not null), for both
void check_ambient_samples(const rrt_ambient_samples& samples) {
    if (samples.n == 0 || samples.n > RRT_MAX_AMBIENT_SAMPLES) throw Error{RRT_ERR_INVALID_ARG, "bad sample count: 1 to RRT_MAX_AMBIENT_SAMPLES directions"};
    if (!samples.dirs) throw Error{RRT_ERR_INVALID_ARG, "null sample directions"};
    for (uint32_t k = 0; k < 3 * samples.n; k++)
        if (!std::isfinite(samples.dirs[k])) throw Error{RRT_ERR_INVALID_ARG, "a sample direction has a non-finite component"};
    if (!(samples.max_t > 0.0)) throw Error{RRT_ERR_INVALID_ARG, "max_t is NaN or not positive"};
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
    HostPlane pl[] = {plane_up(planes.point, 24, n), plane_up(planes.normal, 24, n), plane_up(planes.material, 4, n),
                      plane_down(out.occluded, sizeof(uint32_t), n), plane_down(out.grey, sizeof(uint32_t), px)};
    with_kept_planes(rt, pl, [&](void* stream) {
        launch_ambient_frame(rt, width, height, r, rrt_surface{(double*)pl[0].dev, (double*)pl[1].dev, (uint32_t*)pl[2].dev, nullptr}, samples,
                             rrt_ambient{(uint32_t*)pl[3].dev, (uint32_t*)pl[4].dev}, stream);
    });
}

// ---- per-ray queries.  The one recorded per-ray launch that does not measure: launch(variant) of n rays on `stream`, in the variant of the device forms.
template <class Launch> void recorded_ray_launch(rrt_raytracer* rt, uint32_t n, void* stream, Launch&& launch) {
    const int variant = device_rays_variant(rt);
    timed_launch(rt, stream, [&] { return launch(variant); });
    record(rt, n, 1, n, variant);
}
// The device forms (rrt.h: rrt_intersect_rays_device, ...): no allocation, no copy, no synchronisation; launch(variant) on the caller's stream.
// (device_ray_launch: the same for a call that has made its own checks -- rrt_shade_rays_device has no origins for check_rays)
template <class Launch> int device_ray_launch(rrt_raytracer* rt, uint32_t n, void* stream, Launch&& launch) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    recorded_ray_launch(rt, n, stream, launch);
    return RRT_OK;
}
template <class Launch> int device_ray_query(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, bool any_output, void* stream, Launch&& launch) {
    check_rays(rt, n, d_origins, d_dirs, any_output);
    return device_ray_launch(rt, n, stream, launch);
}
// The host forms: rays and the optional max_t up, launch(m, d_origins, d_dirs, d_max_t, d_out, variant) on the null stream (the variant by rays_variant, measured on a
// first large batch), every output down; blocking (with_call_planes).  out[k]: the caller's array of output k as a plane of n elements (plane_down).
// kEveryOutput: the call wants each of its outputs; kAnyOutput (rrt_surface_rays): one at least -- a null output gets no device memory, d_out[k] is null for the
// launch and nothing is downloaded for it.
enum OutputRule { kEveryOutput, kAnyOutput };
template <size_t K, class Launch>
int host_ray_query(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t, const HostPlane (&out)[K], Launch&& launch,
                   OutputRule rule = kEveryOutput) {
    bool every_output = true, any_output = false;
    for (const HostPlane& o : out) { every_output = every_output && o.host; any_output = any_output || o.host; }
    check_rays(rt, n, origins, dirs, rule == kAnyOutput ? any_output : every_output);
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    HostPlane pl[3 + K] = {plane_up(origins, 24, n), plane_up(dirs, 24, n), plane_up(max_t, 8, n)};
    std::copy(out, out + K, pl + 3);
    with_call_planes(pl, [&] {
        const double *d_o = (const double*)pl[0].dev, *d_d = (const double*)pl[1].dev, *d_m = (const double*)pl[2].dev;
        void* d_out[K];
        for (size_t k = 0; k < K; k++) d_out[k] = pl[3 + k].dev;
        const int variant = rays_variant(rt, n, [&](uint32_t m, int v) { return launch(m, d_o, d_d, d_m, d_out, v); });
        timed_launch(rt, nullptr, [&] { return launch(n, d_o, d_d, d_m, d_out, variant); });
        record(rt, n, 1, n, variant);
    });
    return RRT_OK;
}

// ---- the surface record of arbitrary rays (rrt.h: rrt_surface_rays).  The twelve arrays of an rrt_ray_surface in its order, as bytes per ray ...
constexpr size_t kRaySurfaceArrays = 12;
constexpr size_t kRaySurfaceElem[kRaySurfaceArrays] = {1, 8, 8, 8, 4, 4, 24, 24, 4, 4, 24, 24};
static_assert(sizeof(rrt_ray_surface) == kRaySurfaceArrays * sizeof(void*) && sizeof(RaySurfaceParams) == sizeof(rrt_ray_surface), "rrt_ray_surface is twelve pointers");
// ... and as the kernels' argument
RaySurfaceParams ray_surface_params(const rrt_ray_surface& o) {
    return RaySurfaceParams{o.hit, o.t, o.u, o.v, o.tri, o.albedo, o.point, o.normal, o.material, o.lights, o.next_origin, o.next_dir};
}
// every check of the struct, before any GPU work; true: an array is asked for
bool ray_surface_wanted(const rrt_raytracer* rt, const rrt_ray_surface* out) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!out) throw Error{RRT_ERR_INVALID_ARG, "null ray surface struct"};
    return out->hit || out->t || out->u || out->v || out->tri || out->albedo || out->point || out->normal || out->material || out->lights || out->next_origin || out->next_dir;
}

// ---- shading of arbitrary rays from kept records (rrt.h: rrt_shade_rays).  every check, before any GPU work; n == 0 is a no-op for valid handles and structs
void check_shade_rays(const rrt_raytracer* rt, uint32_t n, const double* dirs, const rrt_ray_surface* rec, const rrt_ray_shade* out) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!rec || !out) throw Error{RRT_ERR_INVALID_ARG, "null struct: shading rays reads the ray surface struct and writes the ray shade struct"};
    if (n && !out->colour && !out->local && !out->kr) throw Error{RRT_ERR_INVALID_ARG, "no output requested: colour, local and kr are all null"};
    if (n && !dirs) throw Error{RRT_ERR_INVALID_ARG, "null ray directions"};
    if (n && (!rec->albedo || !rec->point || !rec->normal || !rec->material)) throw Error{RRT_ERR_INVALID_ARG, "null array: albedo, point, normal and material are all required"};
}
// the kernels' argument from arrays in device memory
ShadeRaysParams shade_rays_params(const double* d_dirs, const rrt_ray_surface& d_rec, uint32_t depth, const rrt_ray_shade& d_out) {
    return ShadeRaysParams{d_dirs, d_rec.point, d_rec.normal, d_rec.material, d_rec.albedo, d_rec.lights, d_out.colour, d_out.local, d_out.kr, depth, 0u};
}
// Host form (checked), for a call without origins: the directions and the four or five arrays it reads up, one launch on the null stream in the variant of the
// device forms -- nothing is measured: there are no origins to measure a walk on -- the requested outputs down; blocking (with_call_planes).
int shade_rays_from_host(rrt_raytracer* rt, uint32_t n, const double* dirs, const rrt_ray_surface& rec, uint32_t depth, const rrt_ray_shade& out) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    const size_t N = n;
    HostPlane pl[] = {plane_up(dirs, 24, N), plane_up(rec.point, 24, N), plane_up(rec.normal, 24, N), plane_up(rec.material, 4, N), plane_up(rec.albedo, 4, N),
                      plane_up(rec.lights, 4, N), plane_down(out.colour, 4, N), plane_down(out.local, 24, N), plane_down(out.kr, 8, N)};
    with_call_planes(pl, [&] {
        rrt_ray_surface d_rec{};
        d_rec.point = (double*)pl[1].dev; d_rec.normal = (double*)pl[2].dev; d_rec.material = (uint32_t*)pl[3].dev; d_rec.albedo = (uint32_t*)pl[4].dev; d_rec.lights = (uint32_t*)pl[5].dev;
        const ShadeRaysParams q = shade_rays_params((const double*)pl[0].dev, d_rec, depth, rrt_ray_shade{(uint32_t*)pl[6].dev, (double*)pl[7].dev, (double*)pl[8].dev});
        recorded_ray_launch(rt, n, nullptr, [&](int variant) { return launch_shade_rays(rt->scene, n, q, nullptr, nullptr, variant); });
    });
    return RRT_OK;
}

// ---- ambient occlusion for ray records (rrt.h: rrt_ambient_rays).  every check, before any GPU work; the structs and the table are checked for n == 0 too
void check_ambient_rays(const rrt_raytracer* rt, uint32_t n, const rrt_ray_surface* rec, const rrt_ambient_samples* samples, const rrt_ray_ambient* out) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!rec || !samples || !out) throw Error{RRT_ERR_INVALID_ARG, "null struct: ambient occlusion of rays takes the ray surface struct, the sample table and the ray ambient struct"};
    if (n && (!rec->point || !rec->normal || !rec->material)) throw Error{RRT_ERR_INVALID_ARG, "null array: point, normal and material are all required"};
    if (n && !out->occluded && !out->open) throw Error{RRT_ERR_INVALID_ARG, "no output requested: occluded and open are both null"};
    check_ambient_samples(*samples);
}
// the kernels' argument from arrays in device memory.  The sample table is copied into it here: no device memory holds it.
AmbientRaysParams ambient_rays_params(const rrt_ray_surface& d_rec, const double* d_rot, const rrt_ambient_samples& samples, const rrt_ray_ambient& d_out) {
    AmbientRaysParams q{};
    q.point = d_rec.point; q.normal = d_rec.normal; q.material = d_rec.material;
    q.rot = d_rot;
    q.occluded = d_out.occluded; q.open = d_out.open;
    q.n_samples = samples.n; q.max_t = samples.max_t;
    std::memcpy(q.dirs, samples.dirs, sizeof(double) * 3 * samples.n);
    return q;
}
// Host form (checked): the three arrays and the optional rotations up, one launch on the null stream in the variant of the device forms -- nothing is measured --
// the requested outputs down; blocking (with_call_planes).
int ambient_rays_from_host(rrt_raytracer* rt, uint32_t n, const rrt_ray_surface& rec, const double* rot, const rrt_ambient_samples& samples, const rrt_ray_ambient& out) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    const size_t N = n;
    HostPlane pl[] = {plane_up(rec.point, 24, N), plane_up(rec.normal, 24, N), plane_up(rec.material, 4, N), plane_up(rot, 16, N),
                      plane_down(out.occluded, 4, N), plane_down(out.open, 4, N)};
    with_call_planes(pl, [&] {
        rrt_ray_surface d_rec{};
        d_rec.point = (double*)pl[0].dev; d_rec.normal = (double*)pl[1].dev; d_rec.material = (uint32_t*)pl[2].dev;
        const AmbientRaysParams q = ambient_rays_params(d_rec, (const double*)pl[3].dev, samples, rrt_ray_ambient{(uint32_t*)pl[4].dev, (uint32_t*)pl[5].dev});
        recorded_ray_launch(rt, n, nullptr, [&](int variant) { return launch_ambient_rays(rt->scene, n, q, nullptr, nullptr, variant); });
    });
    return RRT_OK;
}

// ---- surface records from kept hits (rrt.h: rrt_resolve_hits).  u and v are read for everything but point and material
bool resolve_reads_uv(const rrt_ray_surface& rec) { return rec.albedo || rec.normal || rec.lights || rec.next_origin || rec.next_dir; }
// every check, before any GPU work; n == 0 is a no-op for a valid handle and struct
void check_resolve_hits(const rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const rrt_ray_surface* rec) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!rec) throw Error{RRT_ERR_INVALID_ARG, "null struct: resolving hits reads t, u, v and tri of the ray surface struct and writes its other arrays"};
    if (n && !rec->albedo && !rec->point && !rec->normal && !rec->material && !rec->lights && !rec->next_origin && !rec->next_dir)
        throw Error{RRT_ERR_INVALID_ARG, "no output requested: albedo, point, normal, material, lights, next_origin and next_dir are all null"};
    if (n && (!origins || !dirs)) throw Error{RRT_ERR_INVALID_ARG, "null ray origins or directions"};
    if (n && (!rec->t || !rec->tri)) throw Error{RRT_ERR_INVALID_ARG, "null array: t and tri are required"};
    if (n && resolve_reads_uv(*rec) && (!rec->u || !rec->v)) throw Error{RRT_ERR_INVALID_ARG, "null array: u and v are required for every output but point and material"};
}
// the kernels' argument from arrays in device memory, with the triangle -> slot table of the scene in force
ResolveParams resolve_params(const rrt_raytracer* rt, const double* d_origins, const double* d_dirs, const rrt_ray_surface& d_rec) {
    const BuiltScene& G = rt->built;
    return ResolveParams{d_origins, d_dirs, d_rec.t, d_rec.u, d_rec.v, d_rec.tri, G.tri_slot, G.n_tris, G.n_slots_total,
                         d_rec.albedo, d_rec.point, d_rec.normal, d_rec.material, d_rec.lights, d_rec.next_origin, d_rec.next_dir};
}
// Host form (checked): the rays, t, tri and -- where something asked for reads them -- u and v up, one launch on the null stream in the variant of the device
// forms -- nothing is measured -- the requested outputs down; blocking (with_call_planes).
int resolve_hits_from_host(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const rrt_ray_surface& rec) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    const size_t N = n;
    const bool uv = resolve_reads_uv(rec);
    HostPlane pl[] = {plane_up(origins, 24, N), plane_up(dirs, 24, N), plane_up(rec.t, 8, N), plane_up(uv ? rec.u : nullptr, 8, N), plane_up(uv ? rec.v : nullptr, 8, N),
                      plane_up(rec.tri, 4, N), plane_down(rec.albedo, 4, N), plane_down(rec.point, 24, N), plane_down(rec.normal, 24, N), plane_down(rec.material, 4, N),
                      plane_down(rec.lights, 4, N), plane_down(rec.next_origin, 24, N), plane_down(rec.next_dir, 24, N)};
    with_call_planes(pl, [&] {
        rrt_ray_surface d_rec{};
        d_rec.t = (double*)pl[2].dev; d_rec.u = (double*)pl[3].dev; d_rec.v = (double*)pl[4].dev; d_rec.tri = (uint32_t*)pl[5].dev;
        d_rec.albedo = (uint32_t*)pl[6].dev; d_rec.point = (double*)pl[7].dev; d_rec.normal = (double*)pl[8].dev; d_rec.material = (uint32_t*)pl[9].dev;
        d_rec.lights = (uint32_t*)pl[10].dev; d_rec.next_origin = (double*)pl[11].dev; d_rec.next_dir = (double*)pl[12].dev;
        const ResolveParams q = resolve_params(rt, (const double*)pl[0].dev, (const double*)pl[1].dev, d_rec);
        recorded_ray_launch(rt, n, nullptr, [&](int variant) { return launch_resolve_hits(rt->scene, n, q, nullptr, nullptr, variant); });
    });
    return RRT_OK;
}

// ---- compaction of ray batches and records, and its inverse (rrt.h: rrt_compact_rays, rrt_scatter_rays).  These are not ray calls: no timed_launch, no record.
// The sixteen arrays of an rrt_ray_set in its order, as bytes per entry ...
constexpr size_t kRaySetArrays = 16, kRaySetMaxT = 2, kRaySetMaterial = 4 + 8;
constexpr size_t kRaySetElem[kRaySetArrays] = {24, 24, 8, 16, 1, 8, 8, 8, 4, 4, 24, 24, 4, 4, 24, 24};
static_assert(sizeof(rrt_ray_set) == kRaySetArrays * sizeof(void*) && sizeof(RaySetPtrs) == sizeof(rrt_ray_set), "rrt_ray_set is sixteen pointers");
// ... as an array of pointers (a NULL struct: sixteen NULLs) and as the kernels' argument
struct RaySetArrays { void* p[kRaySetArrays]; };
RaySetArrays ray_set_arrays(const rrt_ray_set* s) {
    RaySetArrays a{};
    if (s) std::memcpy(a.p, s, sizeof a.p);
    return a;
}
RaySetPtrs ray_set_ptrs(const RaySetArrays& a) {
    RaySetPtrs q;
    std::memcpy(&q, a.p, sizeof q);
    return q;
}
// The planes of two ray sets of N entries into pl[at_src, at_src + 16) and pl[at_dst, at_dst + 16): of src what the call reads (read[k], and the array is there) goes
// up, of dst what is set comes down.  A host array that src names twice goes up once: the later entry is no plane of the list and reads the device copy of the
// earlier one, from[k] (its own plane otherwise).
void ray_set_planes(HostPlane* pl, size_t at_src, size_t at_dst, const RaySetArrays& src, const RaySetArrays& dst, const bool (&read)[kRaySetArrays], size_t N,
                    size_t (&from)[kRaySetArrays]) {
    for (size_t k = 0; k < kRaySetArrays; k++) {
        const bool up = src.p[k] && read[k];
        from[k] = at_src + k;
        for (size_t e = 0; up && e < k; e++) if (pl[at_src + e].host == src.p[k] && kRaySetElem[e] == kRaySetElem[k]) from[k] = at_src + e;
        pl[at_src + k] = plane_up(up && from[k] == at_src + k ? src.p[k] : nullptr, kRaySetElem[k], N);
        pl[at_dst + k] = plane_down(dst.p[k], kRaySetElem[k], N);
    }
}
size_t compact_scratch_bytes(uint32_t n) { return n ? sizeof(uint32_t) * ((size_t)compact_tiles(n) + 1) : 0; }
// every check of a compaction but the scratch's, before any GPU work and before the handle is looked at
void check_compact(const rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* flag, const RaySetArrays& src, const RaySetArrays& dst,
                   const uint32_t* index, const uint32_t* count) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (select > RRT_SELECT_FLAG) throw Error{RRT_ERR_INVALID_ARG, "unknown select: want RRT_SELECT_HIT, RRT_SELECT_MIRROR or RRT_SELECT_FLAG"};
    if (n == 0) return;
    if (select == RRT_SELECT_FLAG ? !flag : !src.p[kRaySetMaterial])
        throw Error{RRT_ERR_INVALID_ARG, select == RRT_SELECT_FLAG ? "null flag array: RRT_SELECT_FLAG reads it" : "null src.rec.material: RRT_SELECT_HIT and RRT_SELECT_MIRROR read it"};
    bool any_output = index || count;
    for (size_t k = 0; k < kRaySetArrays; k++) {
        if (dst.p[k] && !src.p[k] && k != kRaySetMaxT) throw Error{RRT_ERR_INVALID_ARG, "an array of dst without its array of src (only max_t may be synthesised)"};
        any_output = any_output || dst.p[k];
    }
    if (!any_output) throw Error{RRT_ERR_INVALID_ARG, "no output requested: index, count and every array of dst are null"};
}
// the kernels' argument from arrays in device memory (checked)
CompactParams compact_params(const rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* d_flag, const RaySetArrays& d_src, const RaySetArrays& d_dst,
                             uint32_t* d_index, void* d_scratch) {
    CompactParams q{};
    q.src = ray_set_ptrs(d_src); q.dst = ray_set_ptrs(d_dst);
    q.flag = d_flag; q.mats = rt->scene.mats;
    q.index = d_index; q.tiles = static_cast<uint32_t*>(d_scratch);
    q.n = n; q.select = select; q.n_mats = rt->scene.n_mats;
    for (void* p : d_dst.p) if (p) q.any_dst = 1u;
    return q;
}
// Host form (checked): what the call reads up -- the src array of every dst array, the materials or the flags -- the three launches on the null stream, the
// requested outputs down; blocking (with_call_planes: the scratch is its first plane).  A host array that src names twice (the intended use: next_origin as
// origins, next_dir as dirs) goes up once: the later entry is no plane of the list and reads the device copy of the earlier one, from[k].
int compact_from_host(rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* flag, const RaySetArrays& src, const RaySetArrays& dst, uint32_t* index, uint32_t* count) {
    if (n == 0) { if (count) *count = 0; return RRT_OK; }
    DeviceGuard guard(rt->device);
    const size_t N = n;
    enum : size_t { kScratch, kSrc, kDst = kSrc + kRaySetArrays, kFlag = kDst + kRaySetArrays, kIndex, kCount, kEnd };
    HostPlane pl[kEnd];
    pl[kScratch] = HostPlane{rt, 1, compact_scratch_bytes(n), kCarve};     // (only carved: a host pointer that is not null says it is wanted)
    size_t from[kRaySetArrays];
    bool read[kRaySetArrays];
    for (size_t k = 0; k < kRaySetArrays; k++) read[k] = dst.p[k] || (k == kRaySetMaterial && select != RRT_SELECT_FLAG);
    ray_set_planes(pl, kSrc, kDst, src, dst, read, N, from);
    pl[kFlag] = plane_up(select == RRT_SELECT_FLAG ? flag : nullptr, 1, N); pl[kIndex] = plane_down(index, 4, N); pl[kCount] = plane_down(count, 4, 1);
    with_call_planes(pl, [&] {
        RaySetArrays d_src{}, d_dst{};
        for (size_t k = 0; k < kRaySetArrays; k++) { d_src.p[k] = pl[from[k]].dev; d_dst.p[k] = pl[kDst + k].dev; }
        const CompactParams q = compact_params(rt, n, select, (const uint8_t*)pl[kFlag].dev, d_src, d_dst, (uint32_t*)pl[kIndex].dev, pl[kScratch].dev);
        HIP_TRY((hipError_t)launch_compact(q, nullptr, (uint32_t*)pl[kCount].dev, nullptr));
    });
    return RRT_OK;
}
// every check of a scatter, before any GPU work and before the handle is looked at
void check_scatter(const rrt_raytracer* rt, uint32_t n, const uint32_t* index, uint32_t elem_bytes, const void* src, const void* dst) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16 && elem_bytes != 24) throw Error{RRT_ERR_INVALID_ARG, "bad elem_bytes: want 1, 4, 8, 16 or 24"};
    if (n && (!index || !src || !dst)) throw Error{RRT_ERR_INVALID_ARG, "null array: a scatter takes index, src and dst"};
}

// ---- stable sort of ray batches and records by a coherence key (rrt.h: rrt_sort_rays; sort.hip).  Not ray calls either.
constexpr size_t kRaySetOrigins = 0, kRaySetDirs = 1, kRaySetPoint = 4 + 6, kRaySetNormal = 4 + 7;
size_t sort_scratch_bytes(uint32_t n) { return sizeof(uint32_t) * sort_scratch_words(n); }
// the arrays of src the key mode reads
bool sort_key_reads(uint32_t key_mode, size_t k) {
    if (key_mode == RRT_SORT_KEY_RAY) return k == kRaySetOrigins || k == kRaySetDirs || k == kRaySetMaxT;
    if (key_mode == RRT_SORT_KEY_RECORD) return k == kRaySetPoint || k == kRaySetNormal || k == kRaySetMaterial;
    return false;
}
// every check of a sort but the scratch's, before any GPU work and before the handle is looked at
void check_sort(const rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* keys, const RaySetArrays& src, const RaySetArrays& dst, const uint32_t* index,
                const uint32_t* keys_out, const uint32_t* count) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (key_mode > RRT_SORT_KEY_RECORD) throw Error{RRT_ERR_INVALID_ARG, "unknown key mode: want RRT_SORT_KEY_GIVEN, RRT_SORT_KEY_RAY or RRT_SORT_KEY_RECORD"};
    if (n == 0) return;
    if (key_mode == RRT_SORT_KEY_GIVEN && !keys) throw Error{RRT_ERR_INVALID_ARG, "null keys: RRT_SORT_KEY_GIVEN reads them"};
    if (key_mode == RRT_SORT_KEY_RAY && (!src.p[kRaySetOrigins] || !src.p[kRaySetDirs])) throw Error{RRT_ERR_INVALID_ARG, "null src.origins or src.dirs: RRT_SORT_KEY_RAY reads them"};
    if (key_mode == RRT_SORT_KEY_RECORD && (!src.p[kRaySetPoint] || !src.p[kRaySetNormal] || !src.p[kRaySetMaterial]))
        throw Error{RRT_ERR_INVALID_ARG, "null src.rec.point, .normal or .material: RRT_SORT_KEY_RECORD reads them"};
    bool any_output = index || keys_out || count;
    for (size_t k = 0; k < kRaySetArrays; k++) {
        if (dst.p[k] && !src.p[k]) throw Error{RRT_ERR_INVALID_ARG, "an array of dst without its array of src"};
        any_output = any_output || dst.p[k];
    }
    if (!any_output) throw Error{RRT_ERR_INVALID_ARG, "no output requested: index, keys_out, count and every array of dst are null"};
}
// the kernels' argument from arrays in device memory (checked): the key is formed with the root box in force now
SortParams sort_params(const rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* d_keys, const RaySetArrays& d_src, const RaySetArrays& d_dst,
                       uint32_t* d_index, uint32_t* d_keys_out, uint32_t* d_count, void* d_scratch) {
    SortParams q{};
    q.src = ray_set_ptrs(d_src); q.dst = ray_set_ptrs(d_dst);
    q.keys = d_keys; q.index = d_index; q.keys_out = d_keys_out; q.count = d_count; q.scratch = static_cast<uint32_t*>(d_scratch);
    q.n = n; q.key_mode = key_mode; q.n_mats = rt->scene.n_mats;
    for (int a = 0; a < 3; a++) { q.lo[a] = rt->root.lo[a]; q.scale[a] = 512.0 / (rt->root.hi[a] - rt->root.lo[a]); }
    return q;
}
// Host form (checked): what the call reads up -- the src array of every dst array, the arrays the key mode reads, the given keys -- the launches on the null stream,
// the requested outputs down; blocking (with_call_planes: the scratch is its first plane).
int sort_from_host(rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* keys, const RaySetArrays& src, const RaySetArrays& dst, uint32_t* index,
                   uint32_t* keys_out, uint32_t* count) {
    if (n == 0) { if (count) *count = 0; return RRT_OK; }
    DeviceGuard guard(rt->device);
    const size_t N = n;
    enum : size_t { kScratch, kSrc, kDst = kSrc + kRaySetArrays, kKeys = kDst + kRaySetArrays, kIndex, kKeysOut, kCount, kEnd };
    HostPlane pl[kEnd];
    pl[kScratch] = HostPlane{rt, 1, sort_scratch_bytes(n), kCarve};        // (only carved: a host pointer that is not null says it is wanted)
    size_t from[kRaySetArrays];
    bool read[kRaySetArrays];
    for (size_t k = 0; k < kRaySetArrays; k++) read[k] = dst.p[k] || sort_key_reads(key_mode, k);
    ray_set_planes(pl, kSrc, kDst, src, dst, read, N, from);
    pl[kKeys] = plane_up(key_mode == RRT_SORT_KEY_GIVEN ? keys : nullptr, 4, N);
    pl[kIndex] = plane_down(index, 4, N); pl[kKeysOut] = plane_down(keys_out, 4, N); pl[kCount] = plane_down(count, 4, 1);
    with_call_planes(pl, [&] {
        RaySetArrays d_src{}, d_dst{};
        for (size_t k = 0; k < kRaySetArrays; k++) { d_src.p[k] = pl[from[k]].dev; d_dst.p[k] = pl[kDst + k].dev; }
        const SortParams q = sort_params(rt, n, key_mode, (const uint32_t*)pl[kKeys].dev, d_src, d_dst, (uint32_t*)pl[kIndex].dev, (uint32_t*)pl[kKeysOut].dev,
                                         (uint32_t*)pl[kCount].dev, pl[kScratch].dev);
        HIP_TRY((hipError_t)launch_sort(q, nullptr));
    });
    return RRT_OK;
}

// ---- the two ends of the per-ray pipeline (rrt.h: rrt_frame_rays, rrt_mix_rays, rrt_mix_pixels; wavefront.hip) and the frame by ray generations that closes it
// (rrt_render_wavefront).  The first three are not ray calls: no timed_launch, no record.
// A region of a frame as a batch of entries: the region in force, the rectangle of 4x4-pixel tiles of the FRAME it touches, and the number of entries in the order.
struct FrameBatch { rrt_region r; uint32_t order, tile_x0, tile_y0, tiles_w; uint64_t n; };
// no handle is looked at; throws what the region calls throw, and for an unknown order or a batch beyond the uint32 n of the per-ray calls
FrameBatch frame_batch(uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7FFFFFFFull) throw Error{RRT_ERR_INVALID_ARG, "bad frame size"};
    if (order > RRT_ORDER_TILES) throw Error{RRT_ERR_INVALID_ARG, "unknown order: want RRT_ORDER_ROWS or RRT_ORDER_TILES"};
    FrameBatch b{};
    b.r = region_in_force(width, height, region);
    b.order = order; b.tile_x0 = b.r.x0 / 4; b.tile_y0 = b.r.y0 / 4;
    b.tiles_w = (b.r.x0 + b.r.w + 3) / 4 - b.tile_x0;
    const uint32_t tiles_h = (b.r.y0 + b.r.h + 3) / 4 - b.tile_y0;
    b.n = order == RRT_ORDER_ROWS ? 4ull * b.r.w * b.r.h : 64ull * b.tiles_w * tiles_h;
    if (b.n > 0xFFFFFFFFull) throw Error{RRT_ERR_INVALID_ARG, "the region has more entries than a ray batch can hold (2^32 - 1)"};
    return b;
}
// every check of a call that takes a frame, a region and an order, before any GPU work
FrameBatch check_frame_batch(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    check_frame(rt, width, height);
    return frame_batch(width, height, region, order);
}
// the kernels' arguments (checked): the frame as launch_frame forms it, the eye in force
FrameRaysParams frame_rays_params(const rrt_raytracer* rt, uint32_t width, uint32_t height, const FrameBatch& b, double* d_origins, double* d_dirs, double* d_max_t) {
    const FrameParams f = frame_params(rt, width, height, 0, 1, false);
    FrameRaysParams q{};
    q.width = width; q.height = height; q.x_scale = f.x_scale; q.y_scale = f.y_scale; q.z_value = f.z_value;
    for (int k = 0; k < 3; k++) { q.right[k] = f.right[k]; q.up[k] = f.up[k]; q.forward[k] = f.forward[k]; q.eye[k] = rt->scene.origin[k]; }
    q.x0 = b.r.x0; q.y0 = b.r.y0; q.w = b.r.w; q.h = b.r.h;
    q.tile_x0 = b.tile_x0; q.tile_y0 = b.tile_y0; q.tiles_w = b.tiles_w; q.order = b.order;
    q.n = (uint32_t)b.n;
    q.origins = d_origins; q.dirs = d_dirs; q.max_t = d_max_t;
    return q;
}
MixPixelsParams mix_pixels_params(uint32_t width, uint32_t height, const FrameBatch& b, const uint32_t* d_colours, void* d_fb) {
    return MixPixelsParams{width, height, b.r.x0, b.r.y0, b.r.w, b.r.h, b.tile_x0, b.tile_y0, b.tiles_w, b.order, d_colours, static_cast<uint32_t*>(d_fb)};
}
void check_mix_rays(const rrt_raytracer* rt, uint32_t n, const double* local, const uint32_t* colour) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (n && (!local || !colour)) throw Error{RRT_ERR_INVALID_ARG, "null array: a mix takes local and writes colour"};
}

// The frame by ray generations.  Its work memory, as byte offsets into the caller's allocation, every array in a slot of its own (device_memory.hpp: slot_bytes):
// the rays of the level in hand and of the next one (origins, dirs, max_t, twice), the record arrays a level's surface launch writes and its shade launch reads, the
// colours of two levels and the scattered colours of the level below, the compaction's scratch -- 228 bytes per entry -- and, KEPT PER LEVEL for the way back up,
// local, kr, material and the compaction's index: 40 bytes per entry and level.  The compactions' counts, a uint32 per level, share the scratch's slot.
constexpr uint32_t kMaxLevels = RRT_MAX_REFLECT + 1;
struct WavefrontWork {
    size_t origins[2], dirs[2], max_t[2];
    size_t albedo, point, normal, lights, next_origin, next_dir;
    size_t colour[2], reflected, scratch;
    size_t local[kMaxLevels], kr[kMaxLevels], material[kMaxLevels], index[kMaxLevels];
    size_t counts;                          // one uint32 per level, behind the scratch in its slot: c[k], the count of level k's compaction -- the bound of level k + 1
    size_t bytes;
};
WavefrontWork wavefront_work(uint64_t n, uint32_t levels) {
    WavefrontWork w{};
    size_t used = 0;
    auto take = [&](size_t bytes) { const size_t at = used; used += slot_bytes(bytes ? bytes : 1); return at; };
    for (int i = 0; i < 2; i++) { w.origins[i] = take(24 * n); w.dirs[i] = take(24 * n); w.max_t[i] = take(8 * n); w.colour[i] = take(4 * n); }
    w.albedo = take(4 * n); w.point = take(24 * n); w.normal = take(24 * n); w.lights = take(4 * n); w.next_origin = take(24 * n); w.next_dir = take(24 * n);
    w.reflected = take(4 * n);
    const size_t scratch = compact_scratch_bytes((uint32_t)n);                 // (a multiple of 4: the counts behind it, in its slot, are aligned)
    w.scratch = take(scratch + sizeof(uint32_t) * kMaxLevels); w.counts = w.scratch + scratch;
    for (uint32_t k = 0; k < levels; k++) { w.local[k] = take(24 * n); w.kr[k] = take(8 * n); w.material[k] = take(4 * n); w.index[k] = take(4 * n); }
    w.bytes = used;
    return w;
}
uint32_t wavefront_levels(const rrt_raytracer* rt) { return std::min(rt->scene.max_reflection_depth, (uint32_t)RRT_MAX_REFLECT) + 1; }

// every check but the work memory's, before any GPU work
FrameBatch check_wavefront(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, const void* fb) {
    const FrameBatch b = check_frame_batch(rt, width, height, region, order);
    if (!fb) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
    return b;
}
// The pipeline of batch b (checked) on `stream`, with d_work (checked) carved as wavefront_work says: generate; per level surface -> shade (local and kr only, with
// the mask: it walks nothing) -> compaction of the mirror hits' next rays into the next level's rays; back up, per level the colours of the level below scattered
// into source order and mixed in; the pixels.  Every launch has the grid of n, but from level 1 on each is COUNTED (rrt.h: COUNTED DEVICE FORMS) by a count the
// pipeline itself left in the work memory, c[k] = the count of level k's compaction: surface, shade and compaction of level k by c[k - 1] (the compaction writes
// c[k]), the scatter of level k by c[k], the mix of level k by c[k - 1].  Blocks beyond a bound leave at once, and what lies beyond it in the arrays is neither
// written nor read: a level whose predecessor left nothing alive costs its launches and nothing else.  Level 0, its mix and the pixels run uncounted.  Only
// launchers that the per-ray entry points use are called; one pair of events around all of it, one record.
void launch_wavefront(rrt_raytracer* rt, uint32_t width, uint32_t height, const FrameBatch& b, void* d_fb, void* d_work, void* stream) {
    const uint32_t n = (uint32_t)b.n, levels = wavefront_levels(rt), last = levels - 1;
    const WavefrontWork w = wavefront_work(n, levels);
    char* base = static_cast<char*>(d_work);
    auto f64 = [&](size_t at) { return reinterpret_cast<double*>(base + at); };
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t*>(base + at); };
    uint32_t* const counts = u32(w.counts);
    const int variant = device_rays_variant(rt);
    timed_launch(rt, stream, [&]() -> int {
        HIP_TRY((hipError_t)launch_frame_rays(frame_rays_params(rt, width, height, b, f64(w.origins[0]), f64(w.dirs[0]), f64(w.max_t[0])), stream));
        for (uint32_t k = 0; k <= last; k++) {
            const uint32_t cur = k & 1u, nxt = cur ^ 1u;
            RaySurfaceParams rec{};
            rec.albedo = u32(w.albedo); rec.point = f64(w.point); rec.normal = f64(w.normal); rec.material = u32(w.material[k]); rec.lights = u32(w.lights);
            if (k < last) { rec.next_origin = f64(w.next_origin); rec.next_dir = f64(w.next_dir); }
            const uint32_t* alive = k ? counts + (k - 1) : nullptr;          // the entries of this level: c[k - 1]; all n at level 0
            HIP_TRY((hipError_t)launch_surface_rays(rt->scene, n, f64(w.origins[cur]), f64(w.dirs[cur]), f64(w.max_t[cur]), rec, alive, stream, variant));
            const ShadeRaysParams shade{f64(w.dirs[cur]), rec.point, rec.normal, rec.material, rec.albedo, rec.lights, nullptr, f64(w.local[k]), f64(w.kr[k]), k, 0u};
            HIP_TRY((hipError_t)launch_shade_rays(rt->scene, n, shade, alive, stream, variant));
            if (k == last) break;
            RaySetArrays src{}, dst{};                                     // the next rays of the mirror hits become the rays of level k + 1; max_t is synthesised
            src.p[kRaySetOrigins] = rec.next_origin; src.p[kRaySetDirs] = rec.next_dir; src.p[kRaySetMaterial] = rec.material;
            dst.p[kRaySetOrigins] = f64(w.origins[nxt]); dst.p[kRaySetDirs] = f64(w.dirs[nxt]); dst.p[kRaySetMaxT] = f64(w.max_t[nxt]);
            HIP_TRY((hipError_t)launch_compact(compact_params(rt, n, RRT_SELECT_MIRROR, nullptr, src, dst, u32(w.index[k]), base + w.scratch), alive, counts + k, stream));
        }
        for (uint32_t k = levels; k-- > 0;) {                              // the unwind, innermost level first (raytracer.rs:85-101)
            const uint32_t* reflected = nullptr;
            if (k < last) {
                HIP_TRY((hipError_t)launch_scatter(n, counts + k, u32(w.index[k]), 4, u32(w.colour[(k + 1) & 1u]), u32(w.reflected), stream));
                reflected = u32(w.reflected);
            }
            HIP_TRY((hipError_t)launch_mix_rays(MixRaysParams{u32(w.material[k]), f64(w.local[k]), f64(w.kr[k]), reflected, u32(w.colour[k & 1u]), n, rt->scene.n_mats},
                                                k ? counts + (k - 1) : nullptr, stream));
        }
        return launch_mix_pixels(mix_pixels_params(width, height, b, u32(w.colour[0]), d_fb), stream);
    });
    record(rt, width, height, 4 * traced_pixels_in(b.r, width, height), variant);
}

}  // namespace

extern "C" {

uint32_t rrt_tiles_per_rank(uint32_t width, uint32_t height, uint32_t world) {
    if (world == 0) return 0;
    const uint32_t n = ((width + 7) / 8) * ((height + 7) / 8);
    return (n + world - 1) / world;
}

int rrt_render_tiles_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t rank, uint32_t world, void* d_tiles, void* stream) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!d_tiles || world == 0 || rank >= world) throw Error{RRT_ERR_INVALID_ARG, "bad rank/world/buffer"};
        launch_frame(rt, width, height, rank, world, true, d_tiles, stream);
        return RRT_OK;
    });
}

int rrt_render_device(rrt_raytracer* rt, uint32_t width, uint32_t height, void* d_fb, void* stream) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!d_fb) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
        launch_frame(rt, width, height, 0, 1, false, d_fb, stream);
        return RRT_OK;
    });
}

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

int rrt_detile_device(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t world, const void* d_gathered, void* d_fb, void* stream) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!d_gathered || !d_fb || world == 0) throw Error{RRT_ERR_INVALID_ARG, "bad argument"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_detile(width, height, world, static_cast<const uint32_t*>(d_gathered), static_cast<uint32_t*>(d_fb), stream));
        return RRT_OK;
    });
}

// Page-locks a caller-owned framebuffer (e.g. the Rust host's Canvas.buffer, engine.rs:127) so that rrt_render can DMA the frame straight
// into it.  Optional: rrt_render works on pageable memory too, through a pinned staging buffer and one extra host copy.
int rrt_host_buffer_register(void* ptr, size_t bytes) {
    return guarded([&]() -> int {
        if (!ptr || !bytes) throw Error{RRT_ERR_INVALID_ARG, "null buffer"};
        HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
        return RRT_OK;
    });
}
int rrt_host_buffer_unregister(void* ptr) {
    return guarded([&]() -> int {
        if (!ptr) throw Error{RRT_ERR_INVALID_ARG, "null buffer"};
        HIP_TRY(hipHostUnregister(ptr));
        return RRT_OK;
    });
}

int rrt_render(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t* out_fb) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!out_fb) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
        DeviceGuard guard(rt->device);
        const size_t bytes = sizeof(uint32_t) * (size_t)width * height;
        uint32_t* d_fb = static_cast<uint32_t*>(rt->host_fb.at_least(bytes));
        const hipStream_t stream = own_stream(rt);
        launch_frame(rt, width, height, 0, 1, false, d_fb, stream);
        staged_download(out_fb, d_fb, bytes, stream);                      // page-locked out_fb (rrt_host_buffer_register, ...): one DMA; pageable: through the staging ring
        HIP_TRY(hipStreamSynchronize(stream));                             // blocking: the frame is in out_fb on return
        return RRT_OK;
    });
}

// Scene::draw_scene as the reference paces it (engine.rs:196-253): the scene rows y in [-H/2, H/2) in chunks of `chunk_rows` (50 there), each chunk
// traced, put into the canvas (put_pixel, engine.rs:146-158: scene row y -> canvas row H - (y + H/2), i.e. bottom-up), then canvas.update().
int rrt_render_progressive(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t* out_fb, uint32_t chunk_rows, rrt_update_fn on_update, void* user) {
    return guarded([&]() -> int {
        check_frame(rt, width, height);
        if (!out_fb) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
        if (chunk_rows == 0) chunk_rows = 50;                              // engine.rs:195
        DeviceGuard guard(rt->device);
        const size_t bytes = sizeof(uint32_t) * (size_t)width * height;
        uint32_t* d_fb = static_cast<uint32_t*>(rt->host_fb.at_least(bytes));
        FrameParams f = frame_params(rt, width, height, 0, 1, false);
        tune_variant(rt, f, d_fb, nullptr);                               // (first frame of a new size: picks the filter variant on the full frame)
        HIP_TRY(hipMemsetAsync(d_fb, 0, bytes, nullptr));                  // Canvas::new, engine.rs:135
        std::memset(out_fb, 0, bytes);
        const int64_t H = height, half = H / 2;
        timed_launch(rt, nullptr, [&] {                                   // ONE pair of events around all the bands
            for (int64_t cs = -half; cs < half; cs += chunk_rows) {        // engine.rs:198-199
                const int64_t ce = std::min<int64_t>(cs + chunk_rows, half);
                // canvas rows of the scene rows [cs, ce): H - (y + H/2); the row that lands on H (y = -H/2) is rejected by put_pixel (engine.rs:152-155)
                const int64_t r_lo = H - (ce - 1 + half), r_hi = std::min<int64_t>(H - (cs + half), H - 1);   // inclusive
                if (r_lo <= r_hi) {
                    f.row_begin = (uint32_t)r_lo; f.row_end = (uint32_t)r_hi + 1;
                    f.tile_begin = (f.row_begin / 8) * f.tiles_x; f.tile_end = ((f.row_end + 7) / 8) * f.tiles_x;
                    HIP_TRY((hipError_t)launch_render(rt->scene, f, d_fb, nullptr, rt->walk));
                    HIP_TRY(hipMemcpy(out_fb + (size_t)f.row_begin * width, d_fb + (size_t)f.row_begin * width,
                                      sizeof(uint32_t) * (size_t)width * (f.row_end - f.row_begin), hipMemcpyDeviceToHost));
                }
                if (on_update) on_update(user, out_fb, width, height, r_lo <= r_hi ? (uint32_t)r_lo : 0u, r_lo <= r_hi ? (uint32_t)(r_hi - r_lo + 1) : 0u);   // canvas.update(), engine.rs:253
            }
            return 0;
        });
        record(rt, width, height, 4 * traced_pixels(width, height), rt->walk);
        return RRT_OK;
    });
}

int rrt_get_ray_colours(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, uint32_t* colours) {
    return guarded([&]() -> int {
        const HostPlane out[] = {plane_down(colours, 4, n)};
        return host_ray_query(rt, n, origins, dirs, nullptr, out, [&](uint32_t m, const double* o, const double* d, const double*, void* const* x, int variant) {
            return launch_ray_colours(rt->scene, m, o, d, (uint32_t*)x[0], nullptr, nullptr, variant);
        });
    });
}

// (the host form wants all five outputs; rrt_intersect_rays_device writes the ones it is given)
int rrt_intersect_rays(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t,
                       uint8_t* hit, double* t, double* u, double* v, uint32_t* tri) {
    return guarded([&]() -> int {
        const HostPlane out[] = {plane_down(hit, 1, n), plane_down(t, 8, n), plane_down(u, 8, n), plane_down(v, 8, n), plane_down(tri, 4, n)};
        return host_ray_query(rt, n, origins, dirs, max_t, out, [&](uint32_t m, const double* o, const double* d, const double* mt, void* const* x, int variant) {
            return launch_intersect(rt->scene, m, o, d, mt, (uint8_t*)x[0], (double*)x[1], (double*)x[2], (double*)x[3], (uint32_t*)x[4], nullptr, nullptr, variant);
        });
    });
}

int rrt_occluded_rays(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t, uint8_t* occluded) {
    return guarded([&]() -> int {
        const HostPlane out[] = {plane_down(occluded, 1, n)};
        return host_ray_query(rt, n, origins, dirs, max_t, out, [&](uint32_t m, const double* o, const double* d, const double* mt, void* const* x, int variant) {
            return launch_occlusion(rt->scene, m, o, d, mt, (uint8_t*)x[0], nullptr, nullptr, variant);
        });
    });
}

// The device forms of the per-ray calls, and behind them their counted forms (rrt.h: COUNTED DEVICE FORMS): ONE body per call, the uncounted entry point gives it a
// null bound.  The bound is never looked at on the host: the same checks, the same grid, the same record.
int rrt_intersect_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const double* d_max_t,
                                      uint8_t* d_hit, double* d_t, double* d_u, double* d_v, uint32_t* d_tri, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, d_hit || d_t || d_u || d_v || d_tri, stream, [&](int variant) {
            return launch_intersect(rt->scene, n, d_origins, d_dirs, d_max_t, d_hit, d_t, d_u, d_v, d_tri, d_count, stream, variant);
        });
    });
}
int rrt_intersect_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t,
                              uint8_t* d_hit, double* d_t, double* d_u, double* d_v, uint32_t* d_tri, void* stream) {
    return rrt_intersect_rays_counted_device(rt, n, nullptr, d_origins, d_dirs, d_max_t, d_hit, d_t, d_u, d_v, d_tri, stream);
}

int rrt_get_ray_colours_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, uint32_t* d_colours, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, d_colours != nullptr, stream, [&](int variant) {
            return launch_ray_colours(rt->scene, n, d_origins, d_dirs, d_colours, d_count, stream, variant);
        });
    });
}
int rrt_get_ray_colours_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, uint32_t* d_colours, void* stream) {
    return rrt_get_ray_colours_counted_device(rt, n, nullptr, d_origins, d_dirs, d_colours, stream);
}

int rrt_occluded_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const double* d_max_t,
                                     uint8_t* d_occluded, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, d_occluded != nullptr, stream, [&](int variant) {
            return launch_occlusion(rt->scene, n, d_origins, d_dirs, d_max_t, d_occluded, d_count, stream, variant);
        });
    });
}
int rrt_occluded_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, uint8_t* d_occluded, void* stream) {
    return rrt_occluded_rays_counted_device(rt, n, nullptr, d_origins, d_dirs, d_max_t, d_occluded, stream);
}

int rrt_surface_rays(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t, const rrt_ray_surface* out) {
    return guarded([&]() -> int {
        (void)ray_surface_wanted(rt, out);                                 // (whether one is asked for is host_ray_query's own check: kAnyOutput)
        void* host[kRaySurfaceArrays];
        std::memcpy(host, out, sizeof host);
        HostPlane arrays[kRaySurfaceArrays];
        for (size_t k = 0; k < kRaySurfaceArrays; k++) arrays[k] = plane_down(host[k], kRaySurfaceElem[k], n);
        return host_ray_query(rt, n, origins, dirs, max_t, arrays, [&](uint32_t m, const double* o, const double* d, const double* mt, void* const* x, int variant) {
            rrt_ray_surface dev;
            std::memcpy(&dev, x, sizeof dev);
            return launch_surface_rays(rt->scene, m, o, d, mt, ray_surface_params(dev), nullptr, nullptr, variant);
        }, kAnyOutput);
    });
}

int rrt_surface_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const double* d_max_t,
                                    const rrt_ray_surface* d_out, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, ray_surface_wanted(rt, d_out), stream, [&](int variant) {
            return launch_surface_rays(rt->scene, n, d_origins, d_dirs, d_max_t, ray_surface_params(*d_out), d_count, stream, variant);
        });
    });
}
int rrt_surface_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, const rrt_ray_surface* d_out, void* stream) {
    return rrt_surface_rays_counted_device(rt, n, nullptr, d_origins, d_dirs, d_max_t, d_out, stream);
}

int rrt_shade_rays(rrt_raytracer* rt, uint32_t n, const double* dirs, const rrt_ray_surface* rec, uint32_t depth, const rrt_ray_shade* out) {
    return guarded([&]() -> int {
        check_shade_rays(rt, n, dirs, rec, out);
        return shade_rays_from_host(rt, n, dirs, *rec, depth, *out);
    });
}

int rrt_shade_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_dirs, const rrt_ray_surface* d_rec, uint32_t depth,
                                  const rrt_ray_shade* d_out, void* stream) {
    return guarded([&]() -> int {
        check_shade_rays(rt, n, d_dirs, d_rec, d_out);
        return device_ray_launch(rt, n, stream, [&](int variant) {
            return launch_shade_rays(rt->scene, n, shade_rays_params(d_dirs, *d_rec, depth, *d_out), d_count, stream, variant);
        });
    });
}
int rrt_shade_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_dirs, const rrt_ray_surface* d_rec, uint32_t depth, const rrt_ray_shade* d_out, void* stream) {
    return rrt_shade_rays_counted_device(rt, n, nullptr, d_dirs, d_rec, depth, d_out, stream);
}

int rrt_ambient_rays(rrt_raytracer* rt, uint32_t n, const rrt_ray_surface* rec, const double* rot, const rrt_ambient_samples* samples, const rrt_ray_ambient* out) {
    return guarded([&]() -> int {
        check_ambient_rays(rt, n, rec, samples, out);
        return ambient_rays_from_host(rt, n, *rec, rot, *samples, *out);
    });
}

int rrt_ambient_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const rrt_ray_surface* d_rec, const double* d_rot,
                                    const rrt_ambient_samples* samples, const rrt_ray_ambient* d_out, void* stream) {
    return guarded([&]() -> int {
        check_ambient_rays(rt, n, d_rec, samples, d_out);
        return device_ray_launch(rt, n, stream, [&](int variant) {
            return launch_ambient_rays(rt->scene, n, ambient_rays_params(*d_rec, d_rot, *samples, *d_out), d_count, stream, variant);
        });
    });
}
int rrt_ambient_rays_device(rrt_raytracer* rt, uint32_t n, const rrt_ray_surface* d_rec, const double* d_rot, const rrt_ambient_samples* samples,
                            const rrt_ray_ambient* d_out, void* stream) {
    return rrt_ambient_rays_counted_device(rt, n, nullptr, d_rec, d_rot, samples, d_out, stream);
}

int rrt_resolve_hits(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const rrt_ray_surface* rec) {
    return guarded([&]() -> int {
        check_resolve_hits(rt, n, origins, dirs, rec);
        return resolve_hits_from_host(rt, n, origins, dirs, *rec);
    });
}

int rrt_resolve_hits_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const rrt_ray_surface* d_rec,
                                    void* stream) {
    return guarded([&]() -> int {
        check_resolve_hits(rt, n, d_origins, d_dirs, d_rec);
        return device_ray_launch(rt, n, stream, [&](int variant) {
            return launch_resolve_hits(rt->scene, n, resolve_params(rt, d_origins, d_dirs, *d_rec), d_count, stream, variant);
        });
    });
}
int rrt_resolve_hits_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const rrt_ray_surface* d_rec, void* stream) {
    return rrt_resolve_hits_counted_device(rt, n, nullptr, d_origins, d_dirs, d_rec, stream);
}

size_t rrt_compact_scratch_bytes(uint32_t n) { return compact_scratch_bytes(n); }

int rrt_compact_rays(rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* flag, const rrt_ray_set* src, const rrt_ray_set* dst, uint32_t* index, uint32_t* count) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(src), d = ray_set_arrays(dst);
        check_compact(rt, n, select, flag, s, d, index, count);
        return compact_from_host(rt, n, select, flag, s, d, index, count);
    });
}

// (d_bound: the bound of the counted form, d_count_out: the call's output; the uncounted entry point gives a null bound)
int rrt_compact_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_bound, uint32_t select, const uint8_t* d_flag, const rrt_ray_set* d_src,
                                    const rrt_ray_set* d_dst, uint32_t* d_index, uint32_t* d_count_out, void* d_scratch, size_t scratch_bytes, void* stream) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(d_src), d = ray_set_arrays(d_dst);
        check_compact(rt, n, select, d_flag, s, d, d_index, d_count_out);
        if (d_bound && d_bound == d_count_out) throw Error{RRT_ERR_INVALID_ARG, "the bound and the output count are the same word: the scan would overwrite what later blocks read"};
        if (n == 0) return (int)RRT_OK;
        if (scratch_bytes < compact_scratch_bytes(n) || !d_scratch) throw Error{RRT_ERR_INVALID_ARG, "scratch too small or null: want rrt_compact_scratch_bytes(n) bytes of device memory"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_compact(compact_params(rt, n, select, d_flag, s, d, d_index, d_scratch), d_bound, d_count_out, stream));
        return (int)RRT_OK;
    });
}
int rrt_compact_rays_device(rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* d_flag, const rrt_ray_set* d_src, const rrt_ray_set* d_dst,
                            uint32_t* d_index, uint32_t* d_count, void* d_scratch, size_t scratch_bytes, void* stream) {
    return rrt_compact_rays_counted_device(rt, n, nullptr, select, d_flag, d_src, d_dst, d_index, d_count, d_scratch, scratch_bytes, stream);
}

int rrt_scatter_rays(rrt_raytracer* rt, uint32_t n, const uint32_t* index, uint32_t elem_bytes, const void* src, void* dst) {
    return guarded([&]() -> int {
        check_scatter(rt, n, index, elem_bytes, src, dst);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_up(index, 4, n), plane_up(src, elem_bytes, n), HostPlane{dst, elem_bytes, n, kUp | kDown}};   // (dst up too: the entries no index names keep their values)
        with_call_planes(pl, [&] { HIP_TRY((hipError_t)launch_scatter(n, nullptr, (const uint32_t*)pl[0].dev, elem_bytes, pl[1].dev, pl[2].dev, nullptr)); });
        return (int)RRT_OK;
    });
}

int rrt_scatter_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const uint32_t* d_index, uint32_t elem_bytes, const void* d_src, void* d_dst,
                                    void* stream) {
    return guarded([&]() -> int {
        check_scatter(rt, n, d_index, elem_bytes, d_src, d_dst);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_scatter(n, d_count, d_index, elem_bytes, d_src, d_dst, stream));
        return (int)RRT_OK;
    });
}
int rrt_scatter_rays_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_index, uint32_t elem_bytes, const void* d_src, void* d_dst, void* stream) {
    return rrt_scatter_rays_counted_device(rt, n, nullptr, d_index, elem_bytes, d_src, d_dst, stream);
}

size_t rrt_sort_scratch_bytes(uint32_t n) { return sort_scratch_bytes(n); }

int rrt_sort_rays(rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* keys, const rrt_ray_set* src, const rrt_ray_set* dst, uint32_t* index,
                  uint32_t* keys_out, uint32_t* count) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(src), d = ray_set_arrays(dst);
        check_sort(rt, n, key_mode, keys, s, d, index, keys_out, count);
        return sort_from_host(rt, n, key_mode, keys, s, d, index, keys_out, count);
    });
}

int rrt_sort_rays_device(rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* d_keys, const rrt_ray_set* d_src, const rrt_ray_set* d_dst,
                         uint32_t* d_index, uint32_t* d_keys_out, uint32_t* d_count, void* d_scratch, size_t scratch_bytes, void* stream) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(d_src), d = ray_set_arrays(d_dst);
        check_sort(rt, n, key_mode, d_keys, s, d, d_index, d_keys_out, d_count);
        if (n == 0) return (int)RRT_OK;
        if (scratch_bytes < sort_scratch_bytes(n) || !d_scratch) throw Error{RRT_ERR_INVALID_ARG, "scratch too small or null: want rrt_sort_scratch_bytes(n) bytes of device memory"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_sort(sort_params(rt, n, key_mode, d_keys, s, d, d_index, d_keys_out, d_count, d_scratch), stream));
        return (int)RRT_OK;
    });
}

uint32_t rrt_frame_ray_count(uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    uint32_t n = 0;
    (void)guarded([&]() -> int { n = (uint32_t)frame_batch(width, height, region, order).n; return RRT_OK; });
    return n;
}

int rrt_frame_rays_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, double* d_origins, double* d_dirs, double* d_max_t,
                          void* stream) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!d_origins && !d_dirs && !d_max_t) throw Error{RRT_ERR_INVALID_ARG, "no array requested: origins, dirs and max_t are all null"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_frame_rays(frame_rays_params(rt, width, height, b, d_origins, d_dirs, d_max_t), stream));
        return RRT_OK;
    });
}

int rrt_frame_rays(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, double* origins, double* dirs, double* max_t) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!origins && !dirs && !max_t) throw Error{RRT_ERR_INVALID_ARG, "no array requested: origins, dirs and max_t are all null"};
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_down(origins, 24, b.n), plane_down(dirs, 24, b.n), plane_down(max_t, 8, b.n)};
        with_call_planes(pl, [&] {
            HIP_TRY((hipError_t)launch_frame_rays(frame_rays_params(rt, width, height, b, (double*)pl[0].dev, (double*)pl[1].dev, (double*)pl[2].dev), nullptr));
        });
        return RRT_OK;
    });
}

int rrt_mix_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const uint32_t* d_material, const double* d_local, const double* d_kr,
                                const uint32_t* d_reflected, uint32_t* d_colour, void* stream) {
    return guarded([&]() -> int {
        check_mix_rays(rt, n, d_local, d_colour);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_mix_rays(MixRaysParams{d_material, d_local, d_kr, d_reflected, d_colour, n, rt->scene.n_mats}, d_count, stream));
        return (int)RRT_OK;
    });
}
int rrt_mix_rays_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_material, const double* d_local, const double* d_kr, const uint32_t* d_reflected, uint32_t* d_colour,
                        void* stream) {
    return rrt_mix_rays_counted_device(rt, n, nullptr, d_material, d_local, d_kr, d_reflected, d_colour, stream);
}

int rrt_mix_rays(rrt_raytracer* rt, uint32_t n, const uint32_t* material, const double* local, const double* kr, const uint32_t* reflected, uint32_t* colour) {
    return guarded([&]() -> int {
        check_mix_rays(rt, n, local, colour);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_up(material, 4, n), plane_up(local, 24, n), plane_up(kr, 8, n), plane_up(reflected, 4, n), plane_down(colour, 4, n)};
        with_call_planes(pl, [&] {
            HIP_TRY((hipError_t)launch_mix_rays(MixRaysParams{(const uint32_t*)pl[0].dev, (const double*)pl[1].dev, (const double*)pl[2].dev, (const uint32_t*)pl[3].dev,
                                                              (uint32_t*)pl[4].dev, n, rt->scene.n_mats}, nullptr, nullptr));
        });
        return (int)RRT_OK;
    });
}

int rrt_mix_pixels_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, const uint32_t* d_colours, void* d_fb, void* stream) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!d_colours || !d_fb) throw Error{RRT_ERR_INVALID_ARG, "null array: the pixels take colours and write a framebuffer"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_mix_pixels(mix_pixels_params(width, height, b, d_colours, d_fb), stream));
        return RRT_OK;
    });
}

int rrt_mix_pixels(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, const uint32_t* colours, uint32_t* out_fb) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!colours || !out_fb) throw Error{RRT_ERR_INVALID_ARG, "null array: the pixels take colours and write a framebuffer"};
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_up(colours, 4, b.n), plane_down(out_fb, 4, (size_t)b.r.w * b.r.h)};
        with_call_planes(pl, [&] { HIP_TRY((hipError_t)launch_mix_pixels(mix_pixels_params(width, height, b, (const uint32_t*)pl[0].dev, pl[1].dev), nullptr)); });
        return RRT_OK;
    });
}

size_t rrt_wavefront_work_bytes(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    size_t bytes = 0;
    (void)guarded([&]() -> int { bytes = wavefront_work(check_frame_batch(rt, width, height, region, order).n, wavefront_levels(rt)).bytes; return RRT_OK; });
    return bytes;
}

int rrt_render_wavefront_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, void* d_fb, void* d_work, size_t work_bytes,
                                void* stream) {
    return guarded([&]() -> int {
        const FrameBatch b = check_wavefront(rt, width, height, region, order, d_fb);
        if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 255u) || work_bytes < wavefront_work(b.n, wavefront_levels(rt)).bytes)
            throw Error{RRT_ERR_INVALID_ARG, "work memory null, not 256-byte aligned or too small: want rrt_wavefront_work_bytes(...) bytes of device memory"};
        DeviceGuard guard(rt->device);
        launch_wavefront(rt, width, height, b, d_fb, d_work, stream);
        return RRT_OK;
    });
}

int rrt_render_wavefront(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, uint32_t* out_fb) {
    return guarded([&]() -> int {
        const FrameBatch b = check_wavefront(rt, width, height, region, order, out_fb);
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {HostPlane{rt, 1, wavefront_work(b.n, wavefront_levels(rt)).bytes, kCarve},   // (only carved: a host pointer that is not null says it is wanted)
                          plane_down(out_fb, 4, (size_t)b.r.w * b.r.h)};
        with_call_planes(pl, [&] { launch_wavefront(rt, width, height, b, pl[1].dev, pl[0].dev, nullptr); });
        return RRT_OK;
    });
}

// Blocking: measure_rays on the first kTuneSample rays of a batch that is already on the device, whatever its size; the result replaces an earlier one.  The
// outputs go to an allocation of the raytracer's own, kept between calls.  The launches run on the null stream: the rays must be complete in memory.
int rrt_tune_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, uint32_t* variant_out) {
    return guarded([&]() -> int {
        check_rays(rt, n, d_origins, d_dirs, true);
        if (n && !rt->variant_forced) {
            DeviceGuard guard(rt->device);
            const uint32_t m = std::min(n, kTuneSample);
            constexpr size_t kBytes = (size_t)kTuneSample * (1 + 8 + 8 + 8 + 4);   // hit, t, u, v, tri of the largest sample (each a multiple of 256 bytes)
            DevArena arena{static_cast<char*>(rt->tune_buf.at_least(kBytes)), kBytes, 0};
            uint8_t* hit = arena.take<uint8_t>(m); double *t = arena.take<double>(m), *u = arena.take<double>(m), *v = arena.take<double>(m); uint32_t* tri = arena.take<uint32_t>(m);
            measure_rays(rt, [&](int variant) { return launch_intersect(rt->scene, m, d_origins, d_dirs, d_max_t, hit, t, u, v, tri, nullptr, nullptr, variant); });
        }
        if (variant_out) *variant_out = (uint32_t)device_rays_variant(rt);
        return (int)RRT_OK;
    });
}

#ifdef RRT_PROFILE
// developer build only: read and clear the 16 work counters
int rrt_prof_counters(rrt_raytracer* rt, unsigned long long* out16) {
    return guarded([&]() -> int {
        DeviceGuard guard(rt->device);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out16, rt->scene.prof, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(rt->scene.prof, 0, 24 * sizeof(unsigned long long)));
        return RRT_OK;
    });
}
// developer build `make band`: read and clear the four (alpha, delta)-band pair counters (render.hip: band_count)
int rrt_prof_band_counters(rrt_raytracer* rt, unsigned long long* out4) {
    return guarded([&]() -> int {
        DeviceGuard guard(rt->device);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out4, rt->scene.prof + 24, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(rt->scene.prof + 24, 0, 4 * sizeof(unsigned long long)));
        return RRT_OK;
    });
}
#endif

int rrt_last_stats(const rrt_raytracer* rt_c, rrt_stats* out) {
    return guarded([&]() -> int {
        rrt_raytracer* rt = const_cast<rrt_raytracer*>(rt_c);
        if (!rt || !out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        if (rt->stats_pending) {
            DeviceGuard guard(rt->device);
            rt->stats.kernel_ms = elapsed_ms(rt);
            rt->stats_pending = false;
        }
        if (!rt->launched) rt->stats.filter_variant = (uint32_t)rt->walk;   // (before the first launch: the forced variant, or 0)
        rt->stats.origin_plane_triangles = rt->scene.n_suspects; rt->stats.scene_bytes = rt->scene_bytes;
        {   // the exactness band of the index (clusters.cpp: find_origin_suspects has the per-pair formulas)
            // (from the build's own f64 values: cull_limit is their fp32 rounding, and +inf for a scene beyond 2^126)
            const double mag = rt->built.scene_magnitude, pad = rt->built.pad, eps = 0x1p-53;
            rt->stats.filter_pad = rt->scene.cull_enabled ? pad : 0.0;
            rt->stats.filter_alpha_unit = (rt->scene.cull_enabled && pad > 0) ? 8.0 * 64.0 * eps * mag / pad : 0.0;
            rt->stats.filter_delta_unit = (rt->scene.cull_enabled && pad > 0) ? 2.0 * (rt->stats.filter_alpha_unit * mag + 64.0 * eps * mag) : 0.0;
        }
        *out = rt->stats;
        return RRT_OK;
    });
}

}  // extern "C"
