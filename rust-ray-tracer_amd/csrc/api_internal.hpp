// api_internal.hpp -- what the units behind include/rrt.h share: the two handle types, the one place that turns exceptions into status codes, and
// the few helpers more than one of them needs.  api.cpp: models and process-wide calls; raytracer.cpp: creation and scene set-up; scene_update.cpp: lights, materials and
// triangles of a living raytracer; frames.cpp, regions.cpp, ray_queries.cpp, ray_batches.cpp: every launch (launches.hpp is what those four share); multi.cpp: N GPUs of one node.
#pragma once
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "device_memory.hpp"
#include "device_scene.hpp"
#include "hip_check.hpp"
#include "model.hpp"
#include "scene_build.hpp"

struct rrt_model { rrt::Model m; };

struct rrt_raytracer {
    int device = 0;
    rrt::DevScene scene{};
    rrt_options opt{};
    rrt::BuiltScene built;           // the scene's buffers (one allocation) and counts, as the GPU or the host set-up built them
    rrt::DevBuf table_mem; rrt::DevArena tables;   // textures, material table, texture table (one allocation)
    // Host copies of the two small tables, kept for rrt_raytracer_set_materials / _get_materials: the material table in force, and the descriptors of the
    // resident textures (device pointer, width, height) that a new table's DevMaterial::tex_desc / bump_desc are filled from.
    std::vector<rrt_material> materials;
    std::vector<rrt::DevTexture> tex_descs;
#ifdef RRT_PROFILE
    rrt::DevBuf prof_mem;
#endif
    uint64_t scene_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    rrt_stats stats{};
    bool stats_pending = false;
    bool launched = false;           // some launch has been recorded in `stats`
    int walk = 0;                    // traversal variant used by this raytracer's frame launches: 0 lane filter, 1 bundle filter, 2 ray walk (see rrt.h)
    int walk_rays = -1;              // ... and by its per-ray entry points (rrt_get_ray_colours / rrt_intersect_rays / rrt_occluded_rays and their _device forms): -1 = not measured yet (launches.hpp: measure_rays)
    bool variant_forced = false;
    rrt::KeptBuf host_fb;            // device framebuffer kept between rrt_render / rrt_render_progressive calls (host-framebuffer entry points), grown when a larger frame comes
    rrt::KeptBuf vis_buf;            // device planes kept between the host forms of the region calls: rrt_render_visibility, rrt_pick, rrt_render_surface,
                                     // rrt_shade_surface, rrt_ambient_surface (launches.hpp: with_kept_planes carves it anew in every call; the per-ray host forms keep nothing: with_call_planes)
    rrt::KeptBuf tune_buf;           // outputs of the measurement launches of rrt_tune_rays_device
    uint32_t n_chains = 0, n_chain_nodes = 0;   // chain records in use (built.n_chains, or 0 where the shortcut's precondition fails: create_raytracer)
    double upload_ms = 0, hip_init_ms = 0, create_ms = 0;   // set-up stages of rrt_raytracer_create besides built.ms_octree / ms_index; wall time of the whole call
    bool gpu_setup = false;          // scene built on the device (default) or on the host (RRT_FLAG_HOST_SETUP)
    struct Buf { const void* p = nullptr; size_t bytes = 0; } bufs[17];   // rrt_raytracer_get_buffer (RRT_BUF_*)
    hipStream_t own_stream = nullptr;   // the stream of the calls that bring results into host memory (launches.hpp: own_stream), set at the first of them
    uint32_t tuned_w = 0, tuned_h = 0, tuned_world = 0;   // frame size the variant below belongs to
    uint32_t size_frames = 0;        // frames rendered at that size so far
    bool size_measured = false;      // ... and whether the variants have been timed on it (second frame of a size)
    // Camera (rrt_raytracer_set_camera, camera.cpp).  The eye is scene.origin; the basis goes into every FrameParams (launches.hpp: frame_params).
    rrt_camera cam{};                // pose in force
    rrt_vec3 origin0{};              // the eye this raytracer was created with (the creation pose)
    // The exactness guard of an eye other than the creation one: list, counter and search records in an allocation of the raytracer's own, made when the
    // eye first moves (the build's list is sized for its own finds only).  scene.suspects / scene.n_suspects always describe the eye in force.
    rrt::DevBuf guard_mem;
    // Scene updates (scene_update.cpp).  The root box in force (rrt_raytracer_set_triangles with root == NULL builds on it again), the share of scene_bytes
    // that belongs to `built` (adopt_built_scene), and the device memory kept between updates (rrt_raytracer_release_update_memory frees it).
    rrt::Box root{};
    uint64_t built_bytes = 0;
    rrt::BuildMemory update_mem;
    // Coverage pass of whole single-GPU frames (frames.cpp: launch_whole_frame; coverage.hip).  A buffer is a place for ONE frame's mask: cleared, filled and read by
    // that frame's own launches; nothing in it outlives the frame, and nothing here describes a scene or a camera.  Two events order its use:
    //   side stream (cover_stream):  [wait for `done` of the buffer's last frame, if that is still in flight]  clear, coverage_kernel, record `ready`
    //   caller's stream `stream`:    wait for `ready`, render_kernel, record `done`
    // so that the pass of a frame runs beside the render_kernel of the frame before it, which reads ANOTHER buffer: a stream alternates between two (cover_pool.hpp
    // has the choice; `age` is its launch counter).  A frame whose stream is idle at the call has nothing to run beside: its pass goes in front of render_kernel on the
    // caller's stream, with neither the side stream nor `ready`.  Several frames of one handle may be in flight on different streams, hence a small pool; a frame that
    // finds no buffer renders without a mask.  All of them share the ONE side stream, which runs in order: a pass that waits for its stream's `done` also holds back
    // the passes of other caller streams enqueued behind it (correct, but it couples streams that are otherwise independent; not measured).  The host never waits for an event here; rrt_raytracer_destroy waits for every `done` before the events and the stream go.
    struct CoverBuf { rrt::KeptBuf mask; rrt::HipOwned<hipEvent_t, hipEventDestroy> done, ready; void* stream = nullptr; bool used = false; uint64_t age = 0; };
    static constexpr int kCoverBufs = 8;
    CoverBuf cover[kCoverBufs];
    uint64_t cover_clock = 0;        // whole frames that took a buffer so far (CoverBuf::age)
    rrt::OwnedStream cover_stream;   // the side stream of the pass: non-blocking, of the highest priority the device offers; created by the first frame that overlaps
    int cover_last = -1;             // the buffer of the last whole frame, or -1: it ran without a mask ...
    uint32_t cover_off = RRT_COVERAGE_OFF_NO_FRAME;   // ... for this reason (RRT_COVERAGE_OFF_*; RRT_COVERAGE_ON with a buffer)
    uint32_t cover_tiles_x = 0, cover_tiles_y = 0;   // the tiles of that frame (rrt_raytracer_get_coverage_info counts its waves on request)
};

namespace rrt {

template <class F> int guarded(F&& f) {
    try { return f(); }
    catch (const Error& e) { set_error_detail(e.detail); return e.status; }
    catch (const HipFail& h) {
        set_error_detail(std::string(h.what) + ": " + hipGetErrorString(h.e));
        (void)hipGetLastError();
        return (h.e == hipErrorOutOfMemory) ? RRT_ERR_OOM : (h.e == hipErrorNoDevice || h.e == hipErrorInvalidDevice) ? RRT_ERR_NO_DEVICE : RRT_ERR_HIP;
    }
    catch (const std::bad_alloc&) { set_error_detail("host allocation failed"); return RRT_ERR_OOM; }
    catch (const std::exception& e) { set_error_detail(e.what()); return RRT_ERR_INVALID_ARG; }
    catch (...) { set_error_detail("unknown failure"); return RRT_ERR_INVALID_ARG; }
}

struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int dev) { HIP_TRY(hipGetDevice(&prev)); if (prev != dev) HIP_TRY(hipSetDevice(dev)); cur = dev; }
    ~DeviceGuard() { if (prev != cur) (void)hipSetDevice(prev); }
    int cur = 0;
};

inline void check_frame(const rrt_raytracer* rt, uint32_t width, uint32_t height) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7FFFFFFFull) throw Error{RRT_ERR_INVALID_ARG, "bad frame size"};
}

inline Box default_root(const double* root) {
    Box b;
    if (root) { b.lo[0] = root[0]; b.hi[0] = root[1]; b.lo[1] = root[2]; b.hi[1] = root[3]; b.lo[2] = root[4]; b.hi[2] = root[5]; }
    else for (int k = 0; k < 3; k++) { b.lo[k] = -20.0; b.hi[k] = 20.0; }   // utils.rs:145
    return b;
}

// what a set-up needs of a scene besides its triangles: materials and RGB8 textures (borrowed views).  api.cpp
struct SceneTables { const rrt_material* mats; uint32_t n_mats; std::vector<rrt_texture> tex; };
SceneTables tables_of(const Model& M);
void validate_tables(const SceneTables& T);

// raytracer.cpp, shared with scene_update.cpp: rt->built becomes the raytracer's scene; the checks of a light list (throws Error) and its store.
void adopt_built_scene(rrt_raytracer* rt);
void check_lights(const rrt_light* lights, uint32_t n_lights);
void store_lights(rrt_raytracer* rt, const rrt_light* lights, uint32_t n_lights);
// the device record of material `s` with its texture descriptors inline, from the descriptors of the resident textures (s.tex / s.bump checked by the caller)
DevMaterial dev_material(const rrt_material& s, const std::vector<DevTexture>& texs);

// The warm-up thread (api.cpp: DeviceWarmer): the loaders start it, rrt_raytracer_create waits for it.
void warm_up_start();
void warm_up_join();

}  // namespace rrt
