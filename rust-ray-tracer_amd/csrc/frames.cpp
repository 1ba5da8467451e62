// frames.cpp -- whole frames behind include/rrt.h: into a device framebuffer or a rank's tiles, into host memory, progressively; the detile of gathered tiles,
// the registration of a host framebuffer, the choice of a frame's traversal variant (tune_variant) and the statistics of the last launch.
// It also holds the part of the launch seam that is no template (launches.hpp): frame_params, elapsed_ms, record, first_frame_variant, own_stream.
// Regions of a frame are in regions.cpp, per-ray queries in ray_queries.cpp, ray batches and the frame by ray generations in ray_batches.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cover_pool.hpp"
#include "coverage_rule.hpp"
#include "launches.hpp"

namespace rrt {

// the kernels' frame argument: the viewport, the tiles, a rank's share, the camera in force
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

// (blocking) the time between the two events of the last timed_launch
float elapsed_ms(rrt_raytracer* rt) {
    float ms = 0;
    HIP_TRY(hipEventSynchronize(rt->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, rt->ev0, rt->ev1));
    return ms;
}
// what the last launch was, into rrt_stats: a frame's size, or (n, 1) for n rays; rays_primary is 0 for a rank's share (not tracked)
void record(rrt_raytracer* rt, uint32_t width, uint32_t height, uint64_t rays_primary, int variant) {
    rt->stats.width = width; rt->stats.height = height; rt->stats.rays_primary = rays_primary;
    rt->stats.scene_bytes = rt->scene_bytes; rt->stats.filter_variant = (uint32_t)variant; rt->stats.origin_plane_triangles = rt->scene.n_suspects;
    rt->stats_pending = true; rt->launched = true;
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

// the raytracer's own stream, for the calls that bring results into host memory: the device's shared set-up stream (staging.hpp: setup_stream; not owned)
hipStream_t own_stream(rrt_raytracer* rt) {
    if (!rt->own_stream) rt->own_stream = (hipStream_t)setup_stream();
    return rt->own_stream;
}

}  // namespace rrt

namespace {

using namespace rrt;

// ---- the coverage pass (coverage.hip, coverage_rule.hpp).
// Whether the frame f may run with a coverage mask: RRT_COVERAGE_ON and F filled, or the reason why not.  The mask rests on the guarantee the index rests on -- a
// pair the reference accepts lies inside the triangle's padded box -- so it is off wherever that guarantee is not in force for every primary ray.
// It is also off where it cannot pay (RRT_FLAG_COVERAGE_ALWAYS lifts these two bounds: tests and timing at small sizes).  The pass costs an isolated frame about 20 us
// whatever its size (a clear, a kernel of one lane per box, two more dispatches) and more with the number of boxes; what it saves grows with the waves it proves empty.
// In a sequence of frames the pass runs beside the frame before (launch_whole_frame), but the library cannot know that a frame is not isolated: the bounds stay.
//  * Waves.  Measured on the teapot (profiles/coverage_ab.txt): 640 x 480 = 19 200 waves lost 7.5 us, 1920 x 1080 = 129 600 waves gains 24 us; the line through the
//    two crosses zero at about 45 000 waves, and nothing in between was measured: on from 49 152 waves (1024 x 768).
//  * Boxes per wave.  The fullest case measured is the 1 M soup at 3840 x 2160, two list slots per wave: no difference beyond the runs' range.  Beyond four slots per
//    wave nothing was measured and a frame that full has little to prove empty: off.
constexpr uint64_t kCoverMinWaves = 49152, kCoverMaxSlotsPerWave = 4;
uint32_t coverage_state(const rrt_raytracer* rt, const FrameParams& f, CoverageFrame& F) {
    const DevScene& S = rt->scene;
    if (rt->opt.flags & RRT_FLAG_NO_COVERAGE) return RRT_COVERAGE_OFF_FLAG;
    const uint64_t waves = 4ull * f.tiles_x * f.tiles_y;
    if (!(rt->opt.flags & RRT_FLAG_COVERAGE_ALWAYS) && (waves < kCoverMinWaves || rt->built.n_list_slots > kCoverMaxSlotsPerWave * waves)) return RRT_COVERAGE_OFF_SMALL_FRAME;
    if (!S.cull_enabled || !(rt->built.pad > 0)) return RRT_COVERAGE_OFF_NO_CULL;
    if (S.n_suspects != 0) return RRT_COVERAGE_OFF_SUSPECTS;
    // The filters are also off for a ray with a component of its origin or direction at or beyond cull_limit (render.hip: make_ray32).  The mask's argument is
    // geometric and does not need them to run, but "off wherever the filters would be off" is the rule, so the largest component a primary direction of this frame
    // can have is bounded the same way: |right| a + |up| b + |forward| c over the frame's extent.
    const double a = ((double)(f.width / 2u) + 1.0) * std::fabs(f.x_scale), b = ((double)(f.height - f.height / 2u) + 1.0) * std::fabs(f.y_scale), c = std::fabs(f.z_value);
    for (int k = 0; k < 3; k++) {
        if (!(std::fabs(S.origin[k]) < (double)S.cull_limit)) return RRT_COVERAGE_OFF_EYE_RANGE;
        if (!(std::fabs(f.right[k]) * a + std::fabs(f.up[k]) * b + std::fabs(f.forward[k]) * c < (double)S.cull_limit)) return RRT_COVERAGE_OFF_EYE_RANGE;
    }
    if (!coverage_frame(F, f.width, f.height, f.x_scale, f.y_scale, f.z_value, f.right, f.up, f.forward, S.origin)) return RRT_COVERAGE_OFF_CAMERA;
    return RRT_COVERAGE_ON;
}
// A buffer for the mask of a frame on `stream`, by the rule of cover_pool.hpp: a free one of this stream, else (while the stream holds fewer than two) one never used or a
// free one of another stream, else the stream's own least recently used one with `wait` set -- the caller enqueues the pass behind that buffer's `done`; index -1 when
// the stream holds none and all kCoverBufs are busy on other streams.  The host waits for nothing.  Allocates only when a buffer is new or a larger frame comes.
CoverPick take_cover_buffer(rrt_raytracer* rt, size_t bytes, void* stream) {
    CoverSlot slots[rrt_raytracer::kCoverBufs];
    for (int i = 0; i < rrt_raytracer::kCoverBufs; i++) {
        const rrt_raytracer::CoverBuf& b = rt->cover[i];
        slots[i] = CoverSlot{b.stream, b.used, false, b.age};
        if (!b.used) continue;
        slots[i].completed = hipEventQuery(b.done.h) == hipSuccess;
        if (!slots[i].completed) (void)hipGetLastError();                     // (hipErrorNotReady: its frame is still in flight)
    }
    const CoverPick pick = pick_cover_buffer(slots, rrt_raytracer::kCoverBufs, stream);
    if (pick.index < 0) return pick;
    rrt_raytracer::CoverBuf& b = rt->cover[pick.index];
    if (!b.done.h) HIP_TRY(hipEventCreateWithFlags(&b.done.h, hipEventDisableTiming));
    if (!b.ready.h) HIP_TRY(hipEventCreateWithFlags(&b.ready.h, hipEventDisableTiming));
    b.mask.at_least(bytes);                                                   // (a buffer that grows is freed first, and hipFree waits for the device: nothing reads it then)
    b.stream = stream; b.used = true; b.age = ++rt->cover_clock;
    return pick;
}
// The side stream of the pass, created by the first frame that has something to run beside.  Non-blocking: callers use the null stream, and a blocking stream would
// synchronise with it.  Of the highest priority the device offers, so that the pass's 25 blocks are not queued behind the 32 400 of the frame before it.
hipStream_t cover_stream(rrt_raytracer* rt) {
    if (!rt->cover_stream.h) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));          // (numerically lower is higher; both 0 where the device has no priorities)
        HIP_TRY(hipStreamCreateWithPriority(&rt->cover_stream.h, hipStreamNonBlocking, greatest));
    }
    return rt->cover_stream.h;
}
// Whether `stream` still has work: launch_whole_frame's `beside`.  Asked BEFORE timed_launch puts its first event on the stream -- behind that record every stream
// looks busy for some microseconds.
bool stream_busy(void* stream) {
    if (hipStreamQuery((hipStream_t)stream) == hipSuccess) return false;
    (void)hipGetLastError();                                                // (hipErrorNotReady: the frame before is still in flight)
    return true;
}
// One WHOLE frame of one GPU (f.world == 1, every tile, every row) for `stream`: the pass (clear, coverage kernel) and render_kernel, or render_kernel alone where the
// mask is off.  Every frame pays the pass again: nothing is kept from the frame before.  But the pass reads nothing that the frame before produces, so where the
// caller's stream still has work at the call -- a sequence of frames enqueued without waiting -- it runs on the side stream, beside that work:
//   side stream:      [wait for `done` of the buffer's last frame]  clear, coverage_kernel, record `ready`
//   caller's stream:  wait for `ready`, render_kernel, record `done`
// With two buffers per stream the pass of frame k+1 waits for frame k-1 at most: it starts when render_kernel of frame k-1 ends, runs while the caller's stream works
// through the events between two frames, and ends about when render_kernel of frame k starts (profiles/coverage_overlap_ab.txt; a pass that starts INSIDE a
// render_kernel is starved of wave slots until that kernel's tail, whatever the side stream's priority -- measured, and one more reason for the wait on `done`).
// Where the caller's stream is idle (`beside` false: a first frame, the blocking rrt_render, tune_variant's counted launches) there is nothing to run beside, and the
// pass goes in front of render_kernel on the caller's stream as one stream order: an isolated frame pays no dependency across streams.  Called inside timed_launch:
// kernel_ms is the time the frame held the caller's stream -- the wait for the mask, which is the whole pass on an idle stream and next to nothing in a sequence,
// plus render_kernel.
// A call that fails halfway (the catch below) still leaves `done` behind whatever it enqueued that touches the buffer: the pool must not hand out as free a buffer
// that the side stream is still writing.
int launch_whole_frame(rrt_raytracer* rt, const FrameParams& f, uint32_t* d_out, void* stream, int variant, bool beside) {
    CoverageFrame F;
    rt->cover_last = -1;
    rt->cover_off = coverage_state(rt, f, F);
    if (rt->cover_off != RRT_COVERAGE_ON) return launch_render(rt->scene, f, d_out, stream, variant);
    const CoverPick pick = take_cover_buffer(rt, sizeof(uint32_t) * (size_t)coverage_buffer_words(coverage_mask_words(F.tiles_x, F.tiles_y)), stream);
    if (pick.index < 0) { rt->cover_off = RRT_COVERAGE_OFF_POOL; return launch_render(rt->scene, f, d_out, stream, variant); }
    rrt_raytracer::CoverBuf& b = rt->cover[pick.index];
    uint32_t* const mask = static_cast<uint32_t*>(b.mask.mem.h);
    const hipStream_t frame_stream = (hipStream_t)stream;
    const hipStream_t pass_stream = beside ? cover_stream(rt) : frame_stream;
    hipStream_t last_user = pass_stream;                                     // the stream behind whose work `done` has to lie if the call ends here
    try {
        if (pick.wait) HIP_TRY(hipStreamWaitEvent(pass_stream, b.done.h, 0));
        // (the root's own list is the slots [0, root_slot_end): its boxes may be listed as wide, coverage_rule.hpp; none with RRT_FLAG_NO_WIDE_COVER)
        const uint32_t root_end = (rt->opt.flags & RRT_FLAG_NO_WIDE_COVER) ? 0u : rt->built.root_slot_end;
        HIP_TRY((hipError_t)launch_coverage(F, rt->scene.tboxes, rt->built.n_list_slots, root_end, mask, pass_stream));
        if (beside) {
            HIP_TRY(hipEventRecord(b.ready.h, pass_stream));
            HIP_TRY(hipStreamWaitEvent(frame_stream, b.ready.h, 0));
        }
        last_user = frame_stream;                                            // (render_kernel lies behind the pass: stream order, or `ready`)
        HIP_TRY((hipError_t)launch_render(rt->scene, f, d_out, stream, variant, mask));
        HIP_TRY(hipEventRecord(b.done.h, frame_stream));
    } catch (...) {
        if (hipEventRecord(b.done.h, last_user) != hipSuccess) (void)hipGetLastError();   // (best effort; the error that is reported is the first one)
        throw;
    }
    rt->cover_last = pick.index; rt->cover_tiles_x = F.tiles_x; rt->cover_tiles_y = F.tiles_y;
    return 0;
}
// The mask of the last frame (rt->cover_last >= 0) in host memory, coverage_mask_words words: waits for that frame and copies.  The bits of the last word beyond
// the frame's waves are cleared: a box that reaches the whole frame sets whole words.  The launch path never does this; the two getters below do, on request.
void read_cover_mask(rrt_raytracer* rt, uint32_t* words) {
    DeviceGuard guard(rt->device);
    const rrt_raytracer::CoverBuf& b = rt->cover[rt->cover_last];
    const uint64_t waves = 4ull * rt->cover_tiles_x * rt->cover_tiles_y;
    const uint32_t n = coverage_mask_words(rt->cover_tiles_x, rt->cover_tiles_y);
    HIP_TRY(hipEventSynchronize(b.done.h));
    HIP_TRY(hipMemcpy(words, b.mask.mem.h, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    if (n && waves % 32u) words[n - 1] &= (1u << (waves % 32u)) - 1u;
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
            const bool beside = stream_busy(stream);                       // (false in every counted run: elapsed_ms has waited for the one before)
            timed_launch(rt, stream, [&] { return launch_whole_frame(rt, f, d_out, stream, variant, beside); });   // (as the frames will run: with the coverage pass)
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

// one frame (or one rank's tiles of it) into a device buffer on the caller's stream, timed by the raytracer's events
void launch_frame(rrt_raytracer* rt, uint32_t width, uint32_t height, uint32_t rank, uint32_t world, bool tiled, void* d_out, void* stream) {
    DeviceGuard guard(rt->device);
    const FrameParams f = frame_params(rt, width, height, rank, world, tiled);
    tune_variant(rt, f, static_cast<uint32_t*>(d_out), stream);
    const bool beside = world == 1 && stream_busy(stream);                 // whether a whole frame's coverage pass has something to run beside (launch_whole_frame)
    timed_launch(rt, stream, [&] {
        if (world == 1) return launch_whole_frame(rt, f, static_cast<uint32_t*>(d_out), stream, rt->walk, beside);
        rt->cover_last = -1; rt->cover_off = RRT_COVERAGE_OFF_NOT_WHOLE;   // a rank's tiles: no mask
        return launch_render(rt->scene, f, static_cast<uint32_t*>(d_out), stream, rt->walk);
    });
    record(rt, width, height, world == 1 ? 4 * traced_pixels(width, height) : 0, rt->walk);
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
        rt->cover_last = -1; rt->cover_off = RRT_COVERAGE_OFF_NOT_WHOLE;   // bands of a frame: no mask
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

int rrt_raytracer_get_coverage_info(const rrt_raytracer* rt_c, uint32_t* state, uint64_t* n_waves, uint64_t* n_proved_empty) {
    return guarded([&]() -> int {
        rrt_raytracer* rt = const_cast<rrt_raytracer*>(rt_c);
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        const bool on = rt->cover_last >= 0;
        const uint64_t waves = on ? 4ull * rt->cover_tiles_x * rt->cover_tiles_y : 0ull;
        if (state) *state = on ? RRT_COVERAGE_ON : rt->cover_off;
        if (n_waves) *n_waves = waves;
        if (!n_proved_empty) return RRT_OK;
        *n_proved_empty = 0;
        if (!on) return RRT_OK;
        // on request only: bring the mask down and count the clear bits
        std::vector<uint32_t> h(coverage_mask_words(rt->cover_tiles_x, rt->cover_tiles_y));
        read_cover_mask(rt, h.data());
        uint64_t set = 0;
        for (uint32_t w : h) set += (uint64_t)__builtin_popcount(w);
        *n_proved_empty = waves - set;
        return RRT_OK;
    });
}

int rrt_raytracer_get_wide_cover_info(const rrt_raytracer* rt_c, uint32_t* n_wide, uint64_t* n_simple_waves) {
    return guarded([&]() -> int {
        rrt_raytracer* rt = const_cast<rrt_raytracer*>(rt_c);
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        if (n_wide) *n_wide = 0;
        if (n_simple_waves) *n_simple_waves = 0;
        if (rt->cover_last < 0) return RRT_OK;
        // the mask, then behind it: `whole`, `fine`, the count (coverage_rule.hpp); a simple wave is set in the mask and clear in `fine`
        const uint32_t n = coverage_mask_words(rt->cover_tiles_x, rt->cover_tiles_y);
        std::vector<uint32_t> h(n), tail((size_t)n + 2);                   // tail: `whole`, `fine`, the count
        read_cover_mask(rt, h.data());                                     // (waits for the frame)
        DeviceGuard guard(rt->device);
        HIP_TRY(hipMemcpy(tail.data(), static_cast<const uint32_t*>(rt->cover[rt->cover_last].mask.mem.h) + n, sizeof(uint32_t) * ((size_t)n + 2), hipMemcpyDeviceToHost));
        const uint32_t* fine = tail.data() + 1;
        uint64_t simple = 0;
        for (uint32_t w = 0; w < n; w++) simple += (uint64_t)__builtin_popcount(h[w] & ~fine[w]);
        // a box that reaches the whole frame makes every wave ordinary, and blocks that see its flag leave before they list: the list is then of no use, and reported empty
        if (n_wide) *n_wide = tail[0] ? 0u : std::min<uint32_t>(fine[n], kMaxWide);
        if (n_simple_waves) *n_simple_waves = simple;
        return RRT_OK;
    });
}

int rrt_raytracer_get_coverage_mask(const rrt_raytracer* rt_c, uint32_t* words, uint64_t n_words) {
    return guarded([&]() -> int {
        rrt_raytracer* rt = const_cast<rrt_raytracer*>(rt_c);
        if (!rt || !words) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        if (rt->cover_last < 0) return RRT_OK;                             // the last frame ran without a mask: nothing is written
        if (n_words != coverage_mask_words(rt->cover_tiles_x, rt->cover_tiles_y)) throw Error{RRT_ERR_INVALID_ARG, "n_words is not the number of mask words of the last frame"};
        read_cover_mask(rt, words);
        return RRT_OK;
    });
}

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
