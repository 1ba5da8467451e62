// launches.hpp -- what the units that launch share.  frames.cpp: whole frames; regions.cpp: regions of a frame; ray_queries.cpp: per-ray queries;
// ray_batches.cpp: ray batches between two per-ray stages and the frame by ray generations.
// Every launch goes through ONE seam: timed_launch (the raytracer's two events around it) and record (what it traced, into rrt_stats).  Every measurement of the
// variants goes through fastest_variant.  The host forms of the region calls share one routine that carves the kept device allocation and copies the planes up and
// down (with_kept_planes); those of the per-ray calls, of compaction, of sorting and of the pipeline's two ends share its sibling for a call that owns its memory
// (with_call_planes: one allocation per call, blocking copies, the null stream).  The plane lists themselves are pure: host_planes.hpp.
#pragma once
#include <algorithm>

#include "api_internal.hpp"
#include "host_planes.hpp"
#include "staging.hpp"

namespace rrt {

// the kernels' frame argument: the viewport, the tiles, a rank's share, the camera in force (frames.cpp)
FrameParams frame_params(const rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t rank, uint32_t world, bool tiled);

// ---- the one timed launch and the one record of it.
// `launch` (returns hipError_t, as int) between the raytracer's two events on `stream`: rrt_last_stats reads the time between them.
template <class Launch> void timed_launch(rrt_raytracer* rt, void* stream, Launch&& launch) {
    HIP_TRY(hipEventRecord(rt->ev0, (hipStream_t)stream));
    HIP_TRY((hipError_t)launch());
    HIP_TRY(hipEventRecord(rt->ev1, (hipStream_t)stream));
}
// (blocking) the time between the two events of the last timed_launch (frames.cpp)
float elapsed_ms(rrt_raytracer* rt);
// what the last launch was, into rrt_stats: a frame's size, or (n, 1) for n rays; rays_primary is 0 for a rank's share (not tracked) (frames.cpp)
void record(rrt_raytracer* rt, uint32_t width, uint32_t height, uint64_t rays_primary, int variant);
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

// ---- the variant policy.  The rule of the first frame of a size (frames.cpp, beside tune_variant), and the variant of a region call (regions.cpp)
int first_frame_variant(const rrt_raytracer* rt, uint32_t width, uint32_t height);
int visibility_variant(const rrt_raytracer* rt, uint32_t width, uint32_t height);

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
// The device forms (rrt_intersect_rays_device, ...) never measure: the forced variant, else the one kept for per-ray calls, else the frame variant.  (ray_queries.cpp)
int device_rays_variant(const rrt_raytracer* rt);

// ---- what the frame by ray generations (ray_batches.cpp) shares with the per-ray calls (ray_queries.cpp): the kernels' arguments of a surface record and of a
// shading of rays, from arrays in device memory
RaySurfaceParams ray_surface_params(const rrt_ray_surface& o);
ShadeRaysParams shade_rays_params(const double* d_dirs, const rrt_ray_surface& d_rec, uint32_t depth, const rrt_ray_shade& d_out);

// the checks of an ambient-occlusion sample table (not null), for a frame's call and for ray records (regions.cpp)
void check_ambient_samples(const rrt_ambient_samples& samples);

// the raytracer's own stream, for the calls that bring results into host memory: the device's shared set-up stream (staging.hpp: setup_stream; not owned) (frames.cpp)
hipStream_t own_stream(rrt_raytracer* rt);

// ---- the host forms.
// One host-form call: the wanted planes carved out of the raytracer's kept device allocation (grown when a larger request comes) IN THE ORDER OF `planes` from offset
// 0, each in a slot of its own (slots.hpp: slot_bytes); the inputs up, launch(stream) on the raytracer's own stream, the outputs down, one wait.  Blocking:
// on return the outputs are in the caller's memory and its inputs are no longer read.
// (a page-locked plane's copy is only enqueued: all of those are in flight before the one wait)
template <size_t K, class Launch> void with_kept_planes(rrt_raytracer* rt, HostPlane (&planes)[K], Launch&& launch) {
    const size_t need = planes_bytes(planes);
    void* const kept = rt->vis_buf.at_least(need);                        // (first: it may grow vis_buf.bytes)
    carve_planes(planes, kept, rt->vis_buf.bytes);
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
    carve_planes(planes, mem.h, need);
    for (const HostPlane& p : planes) if (p.host && (p.dir & kUp)) HIP_TRY(hipMemcpy(p.dev, p.host, p.bytes(), hipMemcpyHostToDevice));
    launch();
    for (const HostPlane& p : planes) if (p.host && (p.dir & kDown)) HIP_TRY(hipMemcpy(p.host, p.dev, p.bytes(), hipMemcpyDeviceToHost));
}

}  // namespace rrt
