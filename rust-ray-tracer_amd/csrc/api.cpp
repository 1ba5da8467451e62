// api.cpp -- the process-wide part of the extern "C" surface declared in include/rrt.h (status strings, error detail, device count, the warm-up
// thread) and the model API.  No CPU rendering path exists in this library; every compute entry point launches the HIP kernels of render.hip
// (raytracer.cpp: scene set-up; frames.cpp, regions.cpp, ray_queries.cpp, ray_batches.cpp: launches; multi.cpp: N GPUs).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "api_internal.hpp"
#include "parallel.hpp"
#include "staging.hpp"

namespace rrt {
namespace {
thread_local std::string g_detail;
}
void set_error_detail(const std::string& s) { g_detail = s; }
}  // namespace rrt

namespace {

using namespace rrt;

// The HIP runtime, the process's first queue and this library's code object come up lazily, at the first HIP call that needs them (160-240 ms on a fresh
// process: runtime start 60-95, first queue 80-140, page-locked ring 13; RRT_SETUP_TRACE prints them).  A model is
// always loaded before a raytracer is created, so the loaders start that work on a helper thread and rrt_raytracer_create finds it done.
struct DeviceWarmer {
    std::thread th; std::once_flag once; std::mutex mu; bool joined = false;
    // HIP's current device is per thread, and the device a raytracer will use is only known at rrt_raytracer_create.  The helper warms the device
    // named by RRT_WARM_DEVICE, else LOCAL_RANK (one process per GPU under torchrun), else device 0 when it is the only one visible; with several
    // devices visible and no hint it brings up nothing device-specific (it would put a context and an allocation on GPU 0 for every rank).
    static int hinted_device(int n_dev) {
        for (const char* name : {"RRT_WARM_DEVICE", "LOCAL_RANK"})
            if (const char* e = std::getenv(name)) { char* end = nullptr; const long v = std::strtol(e, &end, 10); if (end != e && v >= 0 && v < n_dev) return (int)v; }
        return n_dev == 1 ? 0 : -1;
    }
    void start() {
        std::call_once(once, [this] {
            th = std::thread([] {
                const bool trace = std::getenv("RRT_SETUP_TRACE") != nullptr;
                auto lap = [trace, last = std::chrono::steady_clock::now()](const char* what) mutable {
                    if (!trace) return;
                    const auto now = std::chrono::steady_clock::now();
                    fprintf(stderr, "[warm-up]    %-34s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count()); last = now;
                };
                int n = 0;
                if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { (void)hipGetLastError(); return; }
                lap("hipGetDeviceCount (runtime start)");
                const int dev = hinted_device(n);
                if (dev >= 0 && hipSetDevice(dev) == hipSuccess && hipFree(nullptr) == hipSuccess) {
                    lap("hipSetDevice + hipFree(0) (context)");
                    void* p = nullptr; char probe[256] = {};
                    if (hipMalloc(&p, 1 << 20) == hipSuccess) {           // the first allocation and the first host-to-device copy of a process set up the
                        lap("first hipMalloc");
                        (void)hipMemcpy(p, probe, sizeof probe, hipMemcpyHostToDevice);   // the process's first queue (80-140 ms, whoever causes it: without this copy the first stream pays it)
                        lap("first hipMemcpy (pageable)");
                        (void)hipFree(p);
                    }
                    lap("first hipFree");
                    preload_kernels();
                    lap("code object (preload_kernels)");
                    staged_upload_warm();                                 // the pinned staging ring of the set-up uploads (staging.cpp)
                    lap("pinned ring + set-up streams");
                }
                (void)hipGetLastError();
            });
        });
    }
    void join() { std::lock_guard<std::mutex> lk(mu); if (!joined && th.joinable()) th.join(); joined = true; }
    ~DeviceWarmer() { join(); }
};
DeviceWarmer g_warmer;

}  // namespace

SceneTables rrt::tables_of(const Model& M) {
    SceneTables T{M.materials.data(), (uint32_t)M.materials.size(), {}};
    for (auto& t : M.textures) T.tex.push_back(rrt_texture{t.rgb.data(), t.width, t.height});
    return T;
}
void rrt::validate_tables(const SceneTables& T) {
    for (auto& t : T.tex) if (!t.rgb || t.width == 0 || t.height == 0) throw Error{RRT_ERR_INVALID_ARG, "texture with bad dimensions"};
    for (uint32_t i = 0; i < T.n_mats; i++) {
        const rrt_material& mat = T.mats[i];
        if (mat.tex < 0 || (size_t)mat.tex >= T.tex.size()) throw Error{RRT_ERR_INVALID_ARG, "material texture index out of range"};
        if (mat.bump >= (int32_t)T.tex.size()) throw Error{RRT_ERR_INVALID_ARG, "material bump index out of range"};
        if (mat.bump >= 0) {
            // The bump texel is addressed with the COLOUR texture's (x, y) and the bump map's width (raytracer.rs:127-128).  Where that index can
            // leave the bump map the reference panics on the first such hit; on the GPU it would be a wild read, so the scene is refused up front.
            const rrt_texture& t = T.tex[mat.tex]; const rrt_texture& b = T.tex[mat.bump];
            if ((uint64_t)b.width * (t.height - 1) + (t.width - 1) >= (uint64_t)b.width * b.height)
                throw Error{RRT_ERR_INVALID_ARG, "bump map too small for the texture whose texel indices address it (raytracer.rs:127-128 would index out of bounds)"};
        }
    }
}
void rrt::warm_up_start() { g_warmer.start(); }
void rrt::warm_up_join() { g_warmer.join(); }

namespace {
void validate_model(const Model& m) {
    for (auto& t : m.textures) if (t.rgb.size() != (size_t)3 * t.width * t.height) throw Error{RRT_ERR_INVALID_ARG, "texture with bad dimensions"};
    validate_tables(tables_of(m));
    for (auto& t : m.triangles) if (t.mat >= m.materials.size()) throw Error{RRT_ERR_INVALID_ARG, "triangle material index out of range"};
}
}  // namespace

extern "C" {

const char* rrt_strerror(int status) {
    switch (status) {
        case RRT_OK: return "ok";
        case RRT_ERR_INVALID_ARG: return "invalid argument";
        case RRT_ERR_HIP: return "HIP runtime error";
        case RRT_ERR_OOM: return "out of memory";
        case RRT_ERR_IO: return "could not read file";
        case RRT_ERR_PARSE: return "parse error";
        case RRT_ERR_DEPTH: return "octree too deep";
        case RRT_ERR_NO_DEVICE: return "no usable HIP device";
        case RRT_ERR_UNSUPPORTED: return "unsupported input";
        default: return "unknown status";
    }
}
const char* rrt_last_error_detail(void) { return rrt::g_detail.c_str(); }
const char* rrt_build_info(void) { return "librrt_hip: offload-arch=gfx950, f64, -ffp-contract=off, wave64 node-coherent octree walk"; }
void rrt_free(void* p) { std::free(p); }

int rrt_device_count(int* count) {
    return guarded([&]() -> int {
        if (!count) throw Error{RRT_ERR_INVALID_ARG, "null count"};
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
        *count = n;
        return RRT_OK;
    });
}

int rrt_model_load_obj(const char* obj_path, const double* root, rrt_model** out) {
    return guarded([&]() -> int {
        if (!obj_path || !out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        warm_up_start();
        auto m = std::make_unique<rrt_model>();
        load_obj(obj_path, default_root(root), m->m);
        validate_model(m->m);
        *out = m.release();
        return RRT_OK;
    });
}

int rrt_model_from_arrays(uint32_t n_tris, const double* pos, const double* uv, const double* nrm, const uint32_t* mat,
                          uint32_t n_mats, const rrt_material* mats, uint32_t n_tex, const rrt_texture* tex,
                          const double* root, rrt_model** out) {
    return guarded([&]() -> int {
        if (!out || (n_tris && (!pos || !uv || !nrm || !mat)) || (n_mats && !mats) || (n_tex && !tex)) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        warm_up_start();
        auto m = std::make_unique<rrt_model>();
        Model& M = m->m;
        M.root = default_root(root);
        M.materials.assign(mats, mats + n_mats);
        M.textures.resize(n_tex);
        for (uint32_t i = 0; i < n_tex; i++) if (!tex[i].rgb) throw Error{RRT_ERR_INVALID_ARG, "null texture data"};
        parallel_ranges(n_tex, 1, [&](size_t lo, size_t hi, size_t) {
            for (size_t i = lo; i < hi; i++) {
                M.textures[i].width = tex[i].width; M.textures[i].height = tex[i].height;
                M.textures[i].rgb.assign(tex[i].rgb, tex[i].rgb + (size_t)3 * tex[i].width * tex[i].height);
            }
        });
        M.triangles.resize_uninit(n_tris);
        parallel_ranges(n_tris, 1 << 14, [&](size_t lo, size_t hi, size_t) {
            auto rd = [](const double* p) { Vec3 v; v.x = p[0]; v.y = p[1]; v.z = p[2]; return v; };
            for (size_t i = lo; i < hi; i++) {
                Triangle& t = M.triangles[i];
                t.v1 = rd(pos + 9 * i); t.v2 = rd(pos + 9 * i + 3); t.v3 = rd(pos + 9 * i + 6);
                t.t1 = rd(uv + 9 * i);  t.t2 = rd(uv + 9 * i + 3);  t.t3 = rd(uv + 9 * i + 6);
                t.n1 = rd(nrm + 9 * i); t.n2 = rd(nrm + 9 * i + 3); t.n3 = rd(nrm + 9 * i + 6);
                t.mat = mat[i]; t._pad = 0;
            }
        });
        // (the octree is built where it is needed: on the GPU in rrt_raytracer_create, or by host_tree() for the getters below)
        validate_model(M);
        *out = m.release();
        return RRT_OK;
    });
}

void rrt_model_destroy(rrt_model* m) { delete m; }

int rrt_model_get_info(const rrt_model* m, rrt_model_info* out) {
    return guarded([&]() -> int {
        if (!m || !out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        const FlatOctree& T = host_tree(m->m);
        std::memset(out, 0, sizeof *out);
        out->n_tris = (uint32_t)m->m.triangles.size();
        out->n_tris_in_tree = (uint32_t)T.own_idx.size();
        out->n_nodes = (uint32_t)T.box.size(); out->max_depth = T.max_depth;
        out->n_mats = (uint32_t)m->m.materials.size(); out->n_tex = (uint32_t)m->m.textures.size();
        out->root_own_count = T.own_off[1] - T.own_off[0];
        for (size_t i = 0; i + 1 < T.own_off.size(); i++) out->max_own_count = std::max(out->max_own_count, T.own_off[i + 1] - T.own_off[i]);
        return RRT_OK;
    });
}

int rrt_model_get_triangles(const rrt_model* m, double* pos, double* uv, double* nrm, uint32_t* mat) {
    return guarded([&]() -> int {
        if (!m) throw Error{RRT_ERR_INVALID_ARG, "null model"};
        auto wr = [](double* p, const Vec3& v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; };
        for (size_t i = 0; i < m->m.triangles.size(); i++) {
            const Triangle& t = m->m.triangles[i];
            if (pos) { wr(pos + 9 * i, t.v1); wr(pos + 9 * i + 3, t.v2); wr(pos + 9 * i + 6, t.v3); }
            if (uv)  { wr(uv + 9 * i, t.t1);  wr(uv + 9 * i + 3, t.t2);  wr(uv + 9 * i + 6, t.t3); }
            if (nrm) { wr(nrm + 9 * i, t.n1); wr(nrm + 9 * i + 3, t.n2); wr(nrm + 9 * i + 6, t.n3); }
            if (mat) mat[i] = t.mat;
        }
        return RRT_OK;
    });
}

int rrt_model_get_materials(const rrt_model* m, rrt_material* out) {
    return guarded([&]() -> int {
        if (!m || !out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        std::copy(m->m.materials.begin(), m->m.materials.end(), out);
        return RRT_OK;
    });
}

int rrt_model_get_texture(const rrt_model* m, uint32_t index, rrt_texture* out) {
    return guarded([&]() -> int {
        if (!m || !out || index >= m->m.textures.size()) throw Error{RRT_ERR_INVALID_ARG, "bad texture index"};
        const Texture& t = m->m.textures[index];
        out->rgb = t.rgb.data(); out->width = t.width; out->height = t.height;
        return RRT_OK;
    });
}

int rrt_model_get_octree(const rrt_model* m, double* aabb, uint32_t* first_child, uint32_t* tri_count, uint32_t* own_off, uint32_t* own_idx) {
    return guarded([&]() -> int {
        if (!m) throw Error{RRT_ERR_INVALID_ARG, "null model"};
        const FlatOctree& T = host_tree(m->m);
        const size_t n = T.box.size();
        if (aabb) for (size_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) { aabb[6 * i + k] = T.box[i].lo[k]; aabb[6 * i + 3 + k] = T.box[i].hi[k]; }
        if (first_child) std::copy(T.first_child.begin(), T.first_child.end(), first_child);
        if (tri_count) std::copy(T.tri_count.begin(), T.tri_count.end(), tri_count);
        if (own_off) std::copy(T.own_off.begin(), T.own_off.end(), own_off);
        if (own_idx) std::copy(T.own_idx.begin(), T.own_idx.end(), own_idx);
        return RRT_OK;
    });
}

int rrt_decode_image_file(const char* path, uint8_t** rgb, uint32_t* width, uint32_t* height) {
    return guarded([&]() -> int {
        if (!path || !rgb || !width || !height) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        std::vector<uint8_t> bytes; uint32_t w = 0, h = 0, ch = 0;
        decode_image_file(path, bytes, w, h, ch);
        if (ch != 3) throw Error{RRT_ERR_UNSUPPORTED, "image is not 3 bytes per pixel"};
        uint8_t* p = static_cast<uint8_t*>(std::malloc(bytes.size() ? bytes.size() : 1));
        if (!p) throw std::bad_alloc();
        std::memcpy(p, bytes.data(), bytes.size());
        *rgb = p; *width = w; *height = h;
        return RRT_OK;
    });
}

}  // extern "C"
