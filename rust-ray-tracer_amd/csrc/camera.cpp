// camera.cpp -- rrt_raytracer_set_camera / _get_camera and rrt_camera_look_at: the pose a raytracer's frames are taken from.  The view basis is only
// stored (frame_params, frames.cpp, puts it into every FrameParams).  The eye is DevScene::origin, and the one thing besides it that depends on the eye is the index's
// exactness guard: the list of triangles whose plane passes through the eye.  The build computed it for the creation eye from the
// triangle array, which is gone; for a new eye it is searched again in the resident device records (scene_build.hip: k_suspects_resident).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "api_internal.hpp"

namespace {

using namespace rrt;

bool finite3(const rrt_vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// layout of rrt_raytracer::guard_mem: the list the kernels read, then -- in one piece, read back with one copy -- the counter and the search's records
constexpr size_t kListBytes = sizeof(DevSuspect) * (RRT_MAX_SUSPECTS + 1);
constexpr size_t kCountOff = slot_bytes(kListBytes);
struct SearchResult { uint32_t count, _pad; SuspectRecord rec[RRT_MAX_SUSPECTS + 1]; };
static_assert(offsetof(SearchResult, rec) == 8 && sizeof(SuspectRecord) == 40, "counter and records are read back as one block");

// The guard of `eye`, into the raytracer's own list: what a fresh rrt_raytracer_create at that origin computes (same formulas, same order: by push index).
// Blocking, on the null stream; the caller has no frame of this raytracer in flight (rrt.h).  Commits nothing before the last call that can fail.
void move_guard(rrt_raytracer* rt, const rrt_vec3& eye) {
    DeviceGuard guard(rt->device);
    if (!rt->guard_mem.h) rt->guard_mem = dev_alloc(kCountOff + sizeof(SearchResult));
    char* base = static_cast<char*>(rt->guard_mem.h);
    DevSuspect* d_list = reinterpret_cast<DevSuspect*>(base);
    SearchResult* d_res = reinterpret_cast<SearchResult*>(base + kCountOff);
    const double e[3] = {eye.x, eye.y, eye.z};
    HIP_TRY((hipError_t)launch_suspects_resident(rt->built.geom, rt->built.attr, rt->built.n_list_slots, e, rt->built.pad, &d_res->count, d_res->rec, nullptr));
    SearchResult h;
    HIP_TRY(hipMemcpy(&h, d_res, sizeof h, hipMemcpyDeviceToHost));
    if (h.count && h.count <= RRT_MAX_SUSPECTS) {                         // the appends land in any order
        std::sort(h.rec, h.rec + h.count, [](const SuspectRecord& a, const SuspectRecord& b) { return a.tri < b.tri; });
        DevSuspect list[RRT_MAX_SUSPECTS];
        for (uint32_t i = 0; i < h.count; i++) list[i] = h.rec[i].s;
        HIP_TRY(hipMemcpy(d_list, list, sizeof(DevSuspect) * h.count, hipMemcpyHostToDevice));
    }
    rt->scene.suspects = d_list; rt->scene.n_suspects = h.count;           // beyond the cap the list is not read: every ray from the eye runs unfiltered
    rt->bufs[RRT_BUF_SUSPECTS].p = d_list;
    rt->bufs[RRT_BUF_SUSPECTS].bytes = (size_t)(h.count > RRT_MAX_SUSPECTS ? 0 : h.count) * sizeof(DevSuspect);
}

}  // namespace

extern "C" {

int rrt_raytracer_set_camera(rrt_raytracer* rt, const rrt_camera* cam) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        const rrt_camera c = cam ? *cam : rrt_camera{rt->origin0, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        if (!finite3(c.eye) || !finite3(c.right) || !finite3(c.up) || !finite3(c.forward)) throw Error{RRT_ERR_INVALID_ARG, "non-finite camera component"};
        // A bit-equal eye keeps its guard: no GPU work, no synchronisation.  Without the index (RRT_FLAG_NO_CULL; a zero pad) there is no guard to move.
        const double eye[3] = {c.eye.x, c.eye.y, c.eye.z};
        if (std::memcmp(eye, rt->scene.origin, sizeof eye) != 0 && rt->scene.cull_enabled && rt->built.pad > 0) move_guard(rt, c.eye);
        rt->cam = c;
        for (int k = 0; k < 3; k++) rt->scene.origin[k] = eye[k];
        return RRT_OK;
    });
}

int rrt_raytracer_get_camera(const rrt_raytracer* rt, rrt_camera* out) {
    return guarded([&]() -> int {
        if (!rt || !out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        *out = rt->cam;
        return RRT_OK;
    });
}

int rrt_camera_look_at(rrt_vec3 eye, rrt_vec3 target, rrt_vec3 up_hint, rrt_camera* out) {
    return guarded([&]() -> int {
        if (!out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        if (!finite3(eye) || !finite3(target) || !finite3(up_hint)) throw Error{RRT_ERR_INVALID_ARG, "non-finite camera component"};
        auto length = [](const rrt_vec3& v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); };
        auto cross = [](const rrt_vec3& a, const rrt_vec3& b) { return rrt_vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
        const rrt_vec3 d{target.x - eye.x, target.y - eye.y, target.z - eye.z};
        const double ld = length(d);
        if (!(ld > 0.0) || !std::isfinite(ld)) throw Error{RRT_ERR_INVALID_ARG, "look_at: target equals eye (or lies out of range of it)"};
        const rrt_vec3 f{d.x / ld, d.y / ld, d.z / ld};
        const rrt_vec3 r = cross(up_hint, f);                             // left-handed like the reference: x right, y up, z forward
        const double lr = length(r), lu = length(up_hint);
        if (!(lr > 1e-12 * lu) || !std::isfinite(lr)) throw Error{RRT_ERR_INVALID_ARG, "look_at: up_hint is parallel to the view direction"};
        out->eye = eye;
        out->forward = f;
        out->right = rrt_vec3{r.x / lr, r.y / lr, r.z / lr};
        out->up = cross(out->forward, out->right);
        return RRT_OK;
    });
}

}  // extern "C"
