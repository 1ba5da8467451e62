// scene_update.cpp -- rrt_raytracer_set_lights / _get_lights, rrt_raytracer_set_materials / _get_materials, rrt_raytracer_set_triangles / _set_triangles_device and
// rrt_raytracer_release_update_memory: the scene of a living raytracer.  Lights live in DevScene and travel with the kernel arguments, so a new list is
// host work.  A new material table is one small copy over the resident one.  New triangles run the creation's build again (scene_build.hip: gpu_build_scene) into a second BuiltScene, from host arrays or from arrays
// already in device memory, and swap it in after the last call that can fail: textures, tables, options, lights and the camera pose stay resident, and
// the old scene stays in force, intact, on any failure.
#include <atomic>
#include <chrono>
#include <utility>

#include "api_internal.hpp"
#include "parallel.hpp"
#include "staging.hpp"

namespace {

using namespace rrt;

// Builds `src` on the raytracer's device (the current one) and makes the result the scene in force.  The exactness guard is searched for the eye in
// force (not the creation eye), into the new scene's own list: rt->guard_mem stays allocated for the next move of the eye.  Blocking.
void rebuild(rrt_raytracer* rt, const TriSource& src, uint32_t n_tris, const Box& root) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    BuildMemory& keep = rt->update_mem;
    BuiltScene next;
    try {
        gpu_build_scene(src, n_tris, root, !(rt->opt.flags & RRT_FLAG_NO_CULL), rt->scene.origin, setup_stream(), next, {}, &keep);
    } catch (...) {
        if (next.alloc.h && !keep.scene.buf.h) { keep.scene.buf = std::move(next.alloc); keep.scene.bytes = next.alloc_bytes; }   // (lent by `keep`, or new: kept either way)
        throw;
    }
    // ---- nothing from here on can fail
    std::swap(rt->built, next);
    keep.scene.buf = std::move(next.alloc); keep.scene.bytes = next.alloc_bytes;   // the retired scene's allocation serves the next update
    rt->root = root;
    adopt_built_scene(rt);
    rt->upload_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count() - rt->built.ms_octree - rt->built.ms_index;
    // What was measured on the old scene is forgotten: the variant kept for a frame size with that size's frame counter, and the variant kept for
    // per-ray calls.  A forced variant stays; the first-frame rule (frames.cpp: first_frame_variant) then sees the new triangle count.
    rt->tuned_w = rt->tuned_h = rt->tuned_world = 0; rt->size_frames = 0; rt->size_measured = false;
    rt->walk_rays = -1;
    if (!rt->variant_forced) rt->walk = 0;
}

rrt_raytracer* updatable(rrt_raytracer* rt, uint32_t n_tris, const void* pos, const void* uv, const void* nrm, const void* mat) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (n_tris && (!pos || !uv || !nrm || !mat)) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
    if (!rt->gpu_setup) throw Error{RRT_ERR_UNSUPPORTED, "this raytracer was set up on the host (RRT_FLAG_HOST_SETUP): its scene cannot be rebuilt on the device"};
    return rt;
}

}  // namespace

extern "C" {

int rrt_raytracer_set_lights(rrt_raytracer* rt, const rrt_light* lights, uint32_t n_lights) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        check_lights(lights, n_lights);                                   // (throws before anything is stored: the list in force stays)
        store_lights(rt, lights, n_lights);
        return RRT_OK;
    });
}

int rrt_raytracer_get_lights(const rrt_raytracer* rt, rrt_light* out, uint32_t capacity, uint32_t* n_lights) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        const DevScene& S = rt->scene;
        if (out && capacity < S.n_lights) throw Error{RRT_ERR_INVALID_ARG, "light array too small"};
        if (n_lights) *n_lights = S.n_lights;
        if (out) for (uint32_t i = 0; i < S.n_lights; i++) out[i] = rrt_light{S.lights[i].kind, 0u, S.lights[i].intensity, {S.lights[i].v[0], S.lights[i].v[1], S.lights[i].v[2]}};
        return RRT_OK;
    });
}

// One copy of the new table over the resident one, at its address (DevScene::mats stays); textures, scene and tuning state are not touched.  Every check runs
// before the copy: the table in force stays on a refusal.
int rrt_raytracer_set_materials(rrt_raytracer* rt, const rrt_material* mats, uint32_t n_mats) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        if (n_mats != rt->scene.n_mats) throw Error{RRT_ERR_INVALID_ARG, "the number of materials differs from the resident table's (the triangles index it)"};
        if (n_mats && !mats) throw Error{RRT_ERR_INVALID_ARG, "null material list"};
        if (n_mats == 0) return (int)RRT_OK;
        for (uint32_t i = 0; i < n_mats; i++) if (mats[i].bump < -1) throw Error{RRT_ERR_INVALID_ARG, "material bump index out of range (-1 = none)"};
        SceneTables T{mats, n_mats, {}};                                  // (the checks of creation: texture and bump indices, a bump map too small for the texels that address it)
        for (const DevTexture& t : rt->tex_descs) T.tex.push_back(rrt_texture{t.rgb, t.width, t.height});
        validate_tables(T);
        std::vector<DevMaterial> table(n_mats);
        for (uint32_t i = 0; i < n_mats; i++) table[i] = dev_material(mats[i], rt->tex_descs);
        DeviceGuard guard(rt->device);
        HIP_TRY(hipMemcpy(const_cast<DevMaterial*>(rt->scene.mats), table.data(), table.size() * sizeof(DevMaterial), hipMemcpyHostToDevice));   // blocking
        rt->materials.assign(mats, mats + n_mats);
        return (int)RRT_OK;
    });
}

int rrt_raytracer_get_materials(const rrt_raytracer* rt, rrt_material* out, uint32_t capacity, uint32_t* n_mats) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        const uint32_t n = (uint32_t)rt->materials.size();
        if (out && capacity < n) throw Error{RRT_ERR_INVALID_ARG, "material array too small"};
        if (n_mats) *n_mats = n;
        if (out) for (uint32_t i = 0; i < n; i++) out[i] = rt->materials[i];
        return RRT_OK;
    });
}

int rrt_raytracer_set_triangles(rrt_raytracer* rt, uint32_t n_tris, const double* pos, const double* uv, const double* nrm, const uint32_t* mat, const double* root) {
    return guarded([&]() -> int {
        updatable(rt, n_tris, pos, uv, nrm, mat);
        const uint32_t n_mats = rt->scene.n_mats;
        std::atomic<bool> bad{false};
        parallel_ranges(n_tris, 1 << 16, [&](size_t lo, size_t hi, size_t) { for (size_t i = lo; i < hi; i++) if (mat[i] >= n_mats) bad = true; });
        if (bad) throw Error{RRT_ERR_INVALID_ARG, "triangle material index out of range"};
        DeviceGuard guard(rt->device);
        TriSource src; src.pos = pos; src.uv = uv; src.nrm = nrm; src.mat = mat;
        rebuild(rt, src, n_tris, root ? default_root(root) : rt->root);
        return RRT_OK;
    });
}

int rrt_raytracer_set_triangles_device(rrt_raytracer* rt, uint32_t n_tris, const double* d_pos, const double* d_uv, const double* d_nrm, const uint32_t* d_mat,
                                       const double* root, void* stream) {
    return guarded([&]() -> int {
        updatable(rt, n_tris, d_pos, d_uv, d_nrm, d_mat);
        DeviceGuard guard(rt->device);
        hipStream_t st = (hipStream_t)setup_stream();
        if (n_tris) {
            // The build stream waits for what the caller's stream has been given so far: the arrays need not be complete when this is called.
            hipEvent_t ev = nullptr;
            HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            struct EvGuard { hipEvent_t e; ~EvGuard() { (void)hipEventDestroy(e); } } evg{ev};
            HIP_TRY(hipEventRecord(ev, (hipStream_t)stream));
            HIP_TRY(hipStreamWaitEvent(st, ev, 0));
            // A material index cannot be checked on the host here, and an unchecked one is an out-of-bounds table read in the frame kernels: they are
            // counted on the device, and the count is read back before anything is built.
            uint32_t* d_count = static_cast<uint32_t*>(rt->update_mem.t3.at_least(256));
            uint32_t n_bad = 0;
            HIP_TRY((hipError_t)launch_count_bad_materials(d_mat, n_tris, rt->scene.n_mats, d_count, st));
            HIP_TRY(hipMemcpyAsync(&n_bad, d_count, sizeof n_bad, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (n_bad) throw Error{RRT_ERR_INVALID_ARG, "triangle material index out of range"};
        }
        TriSource src; src.pos = d_pos; src.uv = d_uv; src.nrm = d_nrm; src.mat = d_mat; src.on_device = true;
        rebuild(rt, src, n_tris, root ? default_root(root) : rt->root);
        return RRT_OK;
    });
}

int rrt_raytracer_release_update_memory(rrt_raytracer* rt) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        BuildMemory& m = rt->update_mem;
        if (!m.t1.buf.h && !m.t2.buf.h && !m.t3.buf.h && !m.sort.buf.h && !m.scene.buf.h) return RRT_OK;   // nothing kept: no GPU call
        int prev = 0;                                                     // (as rrt_raytracer_destroy: the frees run on the raytracer's device, and nothing here fails)
        const bool have_device = hipGetDevice(&prev) == hipSuccess;
        if (have_device) (void)hipSetDevice(rt->device);
        m.release();
        if (have_device) (void)hipSetDevice(prev);
        return RRT_OK;
    });
}

}  // extern "C"
