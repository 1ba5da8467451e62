// raytracer.cpp -- rrt_raytracer_create / _create_from_arrays / _destroy and the getters of what the set-up built.  The scene is built by
// gpu_build_scene or host_build_scene (scene_build.hpp); this unit uploads textures and tables beside it and adopts the result (adopt_built_scene, which
// scene_update.cpp calls too).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>

#include "api_internal.hpp"
#include "parallel.hpp"
#include "staging.hpp"

namespace {

using namespace rrt;

// ids of rrt_raytracer_get_buffer (rrt.h: RRT_BUF_*)
enum { kBufNodes = 0, kBufGeom, kBufAttr, kBufSupers, kBufCboxes, kBufChildBoxes, kBufTboxes, kBufSuspects, kBufOctBox, kBufOctFirstChild, kBufOctTriCount, kBufOctOwnOff, kBufOctOwnIdx, kBufSlotTri, kBufSlotPos, kBufChains, kBufTriSlot, kBufCount };

// Textures, the material table and the texture table live in ONE allocation of their own, sized here.
void alloc_tables(rrt_raytracer* rt, const SceneTables& T) {
    size_t need = (size_t)1 << 16;
    for (auto& t : T.tex) need += (size_t)3 * t.width * t.height + 256;
    need += T.n_mats * sizeof(DevMaterial) + T.tex.size() * sizeof(DevTexture) + 1024;
    rt->table_mem = dev_alloc(need);
    rt->tables.base = static_cast<char*>(rt->table_mem.h); rt->tables.cap = need;
}

void upload_materials_and_textures(rrt_raytracer* rt, const SceneTables& T, hipStream_t st, std::vector<DevTexture>& texs, std::vector<DevMaterial>& mats) {
    texs.resize(T.tex.size());
    for (size_t i = 0; i < texs.size(); i++) {
        const size_t bytes = (size_t)3 * T.tex[i].width * T.tex[i].height;
        uint8_t* d = rt->tables.take<uint8_t>(bytes);
        staged_upload(d, T.tex[i].rgb, bytes, st);
        rt->scene_bytes += bytes;
        texs[i].rgb = d; texs[i].width = T.tex[i].width; texs[i].height = T.tex[i].height;
    }
    mats.resize(T.n_mats);
    for (size_t i = 0; i < mats.size(); i++) mats[i] = dev_material(T.mats[i], texs);
}

// the two small tables, on `st` (asynchronous: the vectors must outlive the caller's synchronise); the raytracer keeps host copies of the material table and
// of the texture descriptors (rrt_raytracer_set_materials)
void upload_tables(rrt_raytracer* rt, const SceneTables& T, const std::vector<DevTexture>& texs, const std::vector<DevMaterial>& mats, hipStream_t st) {
    rt->materials.assign(T.mats, T.mats + T.n_mats);
    rt->tex_descs = texs;
    DevMaterial* d_m = rt->tables.take<DevMaterial>(mats.size());
    DevTexture* d_t = rt->tables.take<DevTexture>(texs.size());
    if (!mats.empty()) HIP_TRY(hipMemcpyAsync(d_m, mats.data(), mats.size() * sizeof(DevMaterial), hipMemcpyHostToDevice, st));
    if (!texs.empty()) HIP_TRY(hipMemcpyAsync(d_t, texs.data(), texs.size() * sizeof(DevTexture), hipMemcpyHostToDevice, st));
    DevScene& S = rt->scene;
    S.mats = d_m; S.tex = d_t; S.n_mats = (uint32_t)mats.size(); S.n_tex = (uint32_t)texs.size();
}

}  // namespace

namespace rrt {

// What a set-up built (rt->built) becomes the raytracer's scene: the kernels' pointers and every scalar that follows from the build, the table of
// rrt_raytracer_get_buffer, the chain counts, scene_bytes.  A buffer the builder did not keep on the device (null) is reported with size 0.  Creation and
// rrt_raytracer_set_triangles both end here, so neither can forget one of them.  Needs rt->opt; the eye the build searched its exactness guard for is
// the one in force afterwards (scene.suspects / n_suspects describe it).  Host work only: nothing here can fail.
void adopt_built_scene(rrt_raytracer* rt) {
    const BuiltScene& G = rt->built;
    const rrt_options& o = rt->opt;
    DevScene& S = rt->scene;
    S.nodes = G.nodes; S.geom = G.geom; S.attr = G.attr; S.supers = G.supers; S.cboxes = G.cboxes; S.child_boxes = G.child_boxes; S.tboxes = G.tboxes; S.suspects = G.suspects;
    S.n_nodes = G.n_nodes; S.n_slots = G.n_in_tree;
    S.has_groups = G.has_groups; S.bounds_plain = G.bounds_plain;
    S.cull_limit = (float)(G.scene_magnitude * 4.0);
    S.fc_mask = G.inline_leaves ? 0x00FFFFFFu : 0xFFFFFFFFu;
    const size_t n_child_boxes = (size_t)(G.n_nodes > 1 ? G.n_nodes - 1 : 0) + 8, n_cboxes = (size_t)G.n_clusters + 8, n_tboxes = (size_t)G.n_list_slots + 8;
    const struct { int id; const void* p; size_t bytes; } kept[] = {
        {kBufNodes, G.nodes, (size_t)G.n_nodes * sizeof(DevNode)}, {kBufGeom, G.geom, (size_t)G.n_slots_total * sizeof(DevTriGeom)}, {kBufAttr, G.attr, (size_t)G.n_slots_total * sizeof(DevTriAttr)},
        {kBufSupers, G.supers, (size_t)G.n_sup_records * sizeof(DevSuper)}, {kBufCboxes, G.cboxes, n_cboxes * sizeof(DevClusterBox)},
        {kBufChildBoxes, G.child_boxes, n_child_boxes * sizeof(DevClusterBox)}, {kBufTboxes, G.tboxes, n_tboxes * sizeof(DevClusterBox)},
        {kBufSuspects, G.suspects, (size_t)(G.n_suspects > RRT_MAX_SUSPECTS ? 0 : G.n_suspects) * sizeof(DevSuspect)},
        {kBufOctBox, G.oct_box, (size_t)G.n_nodes * 48}, {kBufOctFirstChild, G.oct_first_child, (size_t)G.n_nodes * 4}, {kBufOctTriCount, G.oct_tri_count, (size_t)G.n_nodes * 4},
        {kBufOctOwnOff, G.oct_own_off, ((size_t)G.n_nodes + 1) * 4}, {kBufOctOwnIdx, G.oct_own_idx, (size_t)G.n_in_tree * 4},
        {kBufSlotTri, G.slot_tri, (size_t)G.n_slots_total * 4}, {kBufSlotPos, G.slot_pos, (size_t)G.n_slots_total * 4},
        {kBufChains, G.chains, (size_t)G.n_chains * sizeof(DevChain)}, {kBufTriSlot, G.tri_slot, (size_t)G.n_tris * 4}};
    for (const auto& k : kept) { rt->bufs[k.id].p = k.p; rt->bufs[k.id].bytes = k.p ? k.bytes : 0; }
    S.cull_enabled = (o.flags & RRT_FLAG_NO_CULL) ? 0u : 1u;
    S.cull_half_over_limit = S.cull_limit > 0.0f ? 0.5f / S.cull_limit : 0.0f;
    S.inner_shrink = (S.cull_enabled && G.all_inside_root) ? (float)(2.0 * G.pad) : 0.0f;   // 2 x the pad the boxes were built with; render.hip, single-candidate child test
    // The chain shortcut rests on the same "subtree box inside the octant box" argument as inner_shrink; without it the records stay unused.
    rt->n_chains = G.n_chains; rt->n_chain_nodes = G.n_chain_nodes;
    if (!(S.inner_shrink > 0.0f)) { rt->n_chains = 0; rt->n_chain_nodes = 0; }
    S.chains = (rt->n_chains && !(o.flags & RRT_FLAG_NO_CHAIN_SHORTCUT)) ? G.chains : nullptr;
    S.n_suspects = G.n_suspects;
    S.stack_levels = G.max_depth > 1 ? G.max_depth - 1 : 1;   // (only internal nodes push a frame; the deepest level holds leaves)
    const uint64_t bytes = (uint64_t)G.n_nodes * sizeof(DevNode) + (uint64_t)G.n_slots_total * (sizeof(DevTriGeom) + sizeof(DevTriAttr))
                         + ((uint64_t)G.n_sup_records + n_cboxes + n_child_boxes + n_tboxes) * 32;
    rt->scene_bytes += bytes - rt->built_bytes;                           // (an update replaces the share of the scene it retired)
    rt->built_bytes = bytes;
}

DevMaterial dev_material(const rrt_material& s, const std::vector<DevTexture>& texs) {
    DevMaterial d{};
    d.ka[0] = s.ka.x; d.ka[1] = s.ka.y; d.ka[2] = s.ka.z; d.kd[0] = s.kd.x; d.kd[1] = s.kd.y; d.kd[2] = s.kd.z;
    d.ks[0] = s.ks.x; d.ks[1] = s.ks.y; d.ks[2] = s.ks.z; d.ns = s.ns; d.kr = s.kr; d.tex = s.tex; d.bump = s.bump;
    d.tex_desc = texs[s.tex]; d.bump_desc = s.bump >= 0 ? texs[s.bump] : DevTexture{nullptr, 0, 0};
    return d;
}

void check_lights(const rrt_light* lights, uint32_t n_lights) {
    if (n_lights && !lights) throw Error{RRT_ERR_INVALID_ARG, "null light list"};
    if (n_lights > RRT_MAX_LIGHTS) throw Error{RRT_ERR_INVALID_ARG, "too many lights (max 16)"};
    for (uint32_t i = 0; i < n_lights; i++) if (lights[i].kind > 2) throw Error{RRT_ERR_INVALID_ARG, "bad light kind"};
}

void store_lights(rrt_raytracer* rt, const rrt_light* lights, uint32_t n_lights) {
    DevScene& S = rt->scene;
    S.n_lights = n_lights;
    for (uint32_t i = 0; i < n_lights; i++) {
        S.lights[i].kind = lights[i].kind; S.lights[i]._pad = 0; S.lights[i].intensity = lights[i].intensity;
        S.lights[i].v[0] = lights[i].v.x; S.lights[i].v[1] = lights[i].v.y; S.lights[i].v[2] = lights[i].v.z;
    }
}

}  // namespace rrt

namespace {

// ---- set-up on the HOST (RRT_FLAG_HOST_SETUP): host_build_scene (host_build.cpp), then textures and tables on the null stream.
void setup_on_host(rrt_raytracer* rt, const Model& M, rrt_vec3 origin, const rrt_options& o) {
    const double org[3] = {origin.x, origin.y, origin.z};
    host_build_scene(M, !(o.flags & RRT_FLAG_NO_CULL), org, rt->built);
    const auto t0 = std::chrono::steady_clock::now();
    const SceneTables T = tables_of(M);
    alloc_tables(rt, T);
    std::vector<DevTexture> texs; std::vector<DevMaterial> mats;
    upload_materials_and_textures(rt, T, nullptr, texs, mats);
    upload_tables(rt, T, texs, mats, nullptr);
    adopt_built_scene(rt);
    HIP_TRY(hipDeviceSynchronize());
    rt->upload_ms = rt->built.ms_upload + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- set-up on the GPU (default): the triangle array goes up through pinned staging, then octree, index and records are built there
// (scene_build.hip).  Nothing of the tree ever exists on the host unless a getter asks for it.
void setup_on_gpu(rrt_raytracer* rt, const TriSource& src, uint32_t n_tris, const Box& root, const SceneTables& T, rrt_vec3 origin, const rrt_options& o) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const bool trace = std::getenv("RRT_SETUP_TRACE") != nullptr;
    auto lap = [&, last = t0](const char* what) mutable { if (trace) { const auto n = clk::now(); fprintf(stderr, "[create]     %-34s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - last).count()); last = n; } };
    hipStream_t st = (hipStream_t)setup_stream();
    alloc_tables(rt, T);
    lap("stream, table arena");
    std::vector<DevTexture> texs; std::vector<DevMaterial> mats;
    const double org[3] = {origin.x, origin.y, origin.z};
    // The textures go up beside the build: their copies into page-locked memory are host work (19 MB: ~1.2 ms for the teapot's six), the build is GPU work
    // and waits -- started once the triangles have been through the ring, on a stream of their own, and joined before anything else of *rt is touched.
    hipStream_t st_tex = (hipStream_t)upload_stream();
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::unique_ptr<AsyncTask> tex_task;                                  // (declared after what it refers to: it is waited for first when the frame unwinds)
    auto start_textures = [&] {
        tex_task.reset(new AsyncTask([&, dev] {
            HIP_TRY(hipSetDevice(dev));                                   // (HIP's current device is per thread, and a pool worker keeps its last one)
            upload_materials_and_textures(rt, T, st_tex, texs, mats);
        }));
    };
    gpu_build_scene(src, n_tris, root, !(o.flags & RRT_FLAG_NO_CULL), org, st, rt->built, start_textures);
    lap("gpu_build_scene");
    if (!tex_task) start_textures();
    tex_task->wait();
    lap("texture upload joined");
    adopt_built_scene(rt);
    upload_tables(rt, T, texs, mats, st);   // small tables go through the same stream
    HIP_TRY(hipStreamSynchronize(st_tex));
    HIP_TRY(hipStreamSynchronize(st));
    lap("final synchronise");
    rt->upload_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count() - rt->built.ms_octree - rt->built.ms_index;   // uploads, allocations, synchronisation
}

// rrt_raytracer_create and rrt_raytracer_create_from_arrays: everything but where the triangles come from
int create_raytracer(const rrt_light* lights, uint32_t n_lights, rrt_vec3 origin, const rrt_options* opt, int device, rrt_raytracer** out,
                     const std::function<void(rrt_raytracer*, const rrt_options&)>& setup) {
    if (!out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
    check_lights(lights, n_lights);
    rrt_options o;
    if (opt) o = *opt; else { o.surface_offset = 0.0001; o.max_reflection_depth = 5; o.flags = 0; o.vp_w = o.vp_h = o.vp_d = 1.0; }
    if (o.max_reflection_depth > RRT_MAX_REFLECT) throw Error{RRT_ERR_INVALID_ARG, "max_reflection_depth > 8"};
    const auto t_create0 = std::chrono::steady_clock::now();
    warm_up_join();
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); throw Error{RRT_ERR_NO_DEVICE, "no HIP device visible"}; }
    if (device < 0 || device >= n_dev) throw Error{RRT_ERR_NO_DEVICE, "device index out of range"};
    const auto t_init0 = std::chrono::steady_clock::now();
    DeviceGuard guard(device);
    HIP_TRY(hipFree(nullptr));                                          // brings the HIP context of this device up (a one-off of the process: ~90 ms on a fresh one)
    const double hip_init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_init0).count();

    std::unique_ptr<rrt_raytracer, void (*)(rrt_raytracer*)> rt(new rrt_raytracer, rrt_raytracer_destroy);
    rt->hip_init_ms = hip_init_ms;
    rt->device = device; rt->opt = o;
    setup(rt.get(), o);

    DevScene& S = rt->scene;                                              // (what follows from the build: adopt_built_scene, in `setup`)
    S.max_reflection_depth = o.max_reflection_depth;
    S.origin[0] = origin.x; S.origin[1] = origin.y; S.origin[2] = origin.z;
    rt->origin0 = origin;
    rt->cam = rrt_camera{origin, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};   // the reference's view: down +z, y up (engine.rs:207-211)
    S.surface_offset = o.surface_offset;
    S.specular_all = (o.flags & RRT_FLAG_NO_SPECULAR_SKIP) ? 1u : 0u;
    store_lights(rt.get(), lights, n_lights);
#ifdef RRT_PROFILE
    rt->prof_mem = dev_alloc(32 * sizeof(unsigned long long)); HIP_TRY(hipMemset(rt->prof_mem.h, 0, 32 * sizeof(unsigned long long)));
    S.prof = static_cast<unsigned long long*>(rt->prof_mem.h);
#endif
    HIP_TRY(hipEventCreate(&rt->ev0)); HIP_TRY(hipEventCreate(&rt->ev1));
    // Own-list filter variant: forced by a flag, else a measured rule on the first frame of each frame size and measured on the second (tune_variant)
    rt->variant_forced = (o.flags & (RRT_FLAG_BUNDLE_FILTER | RRT_FLAG_LANE_FILTER | RRT_FLAG_RAY_WALK | RRT_FLAG_NO_CULL)) != 0;
    rt->walk = (o.flags & RRT_FLAG_NO_CULL) ? 0 : (o.flags & RRT_FLAG_BUNDLE_FILTER) ? 1 : (o.flags & RRT_FLAG_RAY_WALK) ? 2 : 0;
    rt->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create0).count();
    *out = rt.release();
    return RRT_OK;
}
}  // namespace

extern "C" {

int rrt_raytracer_create(const rrt_model* m, const rrt_light* lights, uint32_t n_lights, rrt_vec3 origin,
                         const rrt_options* opt, int device, rrt_raytracer** out) {
    return guarded([&]() -> int {
        if (!m) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        const Model& M = m->m;
        return create_raytracer(lights, n_lights, origin, opt, device, out, [&](rrt_raytracer* rt, const rrt_options& o) {
            rt->gpu_setup = !(o.flags & RRT_FLAG_HOST_SETUP); rt->root = M.root;
            if (rt->gpu_setup) { TriSource src; src.tris = M.triangles.data(); setup_on_gpu(rt, src, (uint32_t)M.triangles.size(), M.root, tables_of(M), origin, o); }
            else setup_on_host(rt, M, origin, o);
        });
    });
}

// RayTracer straight from the host's own arrays: rrt_model_from_arrays + rrt_raytracer_create without the model -- the arrays are uploaded from where
// they lie (through the pinned staging ring) and packed into triangle records on the device, so the library keeps no host copy of the scene and the
// loaders' copy (15 ms of the 1 M soup's 54 ms first frame) is not made.  Same scene in HBM, same frames.
int rrt_raytracer_create_from_arrays(uint32_t n_tris, const double* pos, const double* uv, const double* nrm, const uint32_t* mat,
                                     uint32_t n_mats, const rrt_material* mats, uint32_t n_tex, const rrt_texture* tex, const double* root,
                                     const rrt_light* lights, uint32_t n_lights, rrt_vec3 origin, const rrt_options* opt, int device, rrt_raytracer** out) {
    return guarded([&]() -> int {
        if ((n_tris && (!pos || !uv || !nrm || !mat)) || (n_mats && !mats) || (n_tex && !tex)) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        if (opt && (opt->flags & RRT_FLAG_HOST_SETUP)) throw Error{RRT_ERR_UNSUPPORTED, "RRT_FLAG_HOST_SETUP needs a model (rrt_model_from_arrays + rrt_raytracer_create)"};
        SceneTables T{mats, n_mats, std::vector<rrt_texture>(tex, tex + n_tex)};
        validate_tables(T);
        std::atomic<bool> bad{false};
        parallel_ranges(n_tris, 1 << 16, [&](size_t lo, size_t hi, size_t) { for (size_t i = lo; i < hi; i++) if (mat[i] >= n_mats) bad = true; });
        if (bad) throw Error{RRT_ERR_INVALID_ARG, "triangle material index out of range"};
        warm_up_start();
        const Box box = default_root(root);
        return create_raytracer(lights, n_lights, origin, opt, device, out, [&](rrt_raytracer* rt, const rrt_options& o) {
            rt->gpu_setup = true; rt->root = box;
            TriSource src; src.pos = pos; src.uv = uv; src.nrm = nrm; src.mat = mat;
            setup_on_gpu(rt, src, n_tris, box, T, origin, o);
        });
    });
}

// The octree as the GPU set-up built it (scene_build.hip), in the reference's node numbering: same layout as rrt_model_get_octree.
int rrt_raytracer_get_octree(const rrt_raytracer* rt, rrt_model_info* info, double* aabb, uint32_t* first_child, uint32_t* tri_count, uint32_t* own_off, uint32_t* own_idx) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        if (!rt->gpu_setup) throw Error{RRT_ERR_UNSUPPORTED, "this raytracer was set up on the host (RRT_FLAG_HOST_SETUP): ask the model (rrt_model_get_octree)"};
        DeviceGuard guard(rt->device);
        const BuiltScene& G = rt->built;
        if (aabb) HIP_TRY(hipMemcpy(aabb, G.oct_box, (size_t)G.n_nodes * 48, hipMemcpyDeviceToHost));
        if (first_child) HIP_TRY(hipMemcpy(first_child, G.oct_first_child, (size_t)G.n_nodes * 4, hipMemcpyDeviceToHost));
        if (tri_count) HIP_TRY(hipMemcpy(tri_count, G.oct_tri_count, (size_t)G.n_nodes * 4, hipMemcpyDeviceToHost));
        if (own_off) HIP_TRY(hipMemcpy(own_off, G.oct_own_off, ((size_t)G.n_nodes + 1) * 4, hipMemcpyDeviceToHost));
        if (own_idx && G.n_in_tree) HIP_TRY(hipMemcpy(own_idx, G.oct_own_idx, (size_t)G.n_in_tree * 4, hipMemcpyDeviceToHost));
        if (info) {
            std::memset(info, 0, sizeof *info);
            info->n_tris = G.n_tris; info->n_tris_in_tree = G.n_in_tree; info->n_nodes = G.n_nodes; info->max_depth = G.max_depth;
            info->n_mats = rt->scene.n_mats; info->n_tex = rt->scene.n_tex;
            std::vector<uint32_t> off((size_t)G.n_nodes + 1);
            HIP_TRY(hipMemcpy(off.data(), G.oct_own_off, off.size() * 4, hipMemcpyDeviceToHost));
            info->root_own_count = off[1] - off[0];
            for (size_t i = 0; i + 1 < off.size(); i++) info->max_own_count = std::max(info->max_own_count, off[i + 1] - off[i]);
        }
        return RRT_OK;
    });
}

int rrt_raytracer_get_chain_info(const rrt_raytracer* rt, uint32_t* n_chains, uint32_t* n_chain_nodes) {
    return guarded([&]() -> int {
        if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
        if (n_chains) *n_chains = rt->n_chains;
        if (n_chain_nodes) *n_chain_nodes = rt->n_chain_nodes;
        return RRT_OK;
    });
}

// Developer / test introspection: the bytes of one of the scene buffers in HBM (RRT_BUF_*).  out may be NULL to ask for the size only.
int rrt_raytracer_get_buffer(const rrt_raytracer* rt, uint32_t which, void* out, size_t capacity, size_t* bytes) {
    return guarded([&]() -> int {
        if (!rt || which >= (uint32_t)kBufCount) throw Error{RRT_ERR_INVALID_ARG, "bad buffer id"};
        const auto& b = rt->bufs[which];
        if (!b.p && b.bytes) throw Error{RRT_ERR_UNSUPPORTED, "buffer not kept by this set-up path"};
        if (bytes) *bytes = b.bytes;
        if (out) {
            if (capacity < b.bytes) throw Error{RRT_ERR_INVALID_ARG, "buffer too small"};
            DeviceGuard guard(rt->device);
            if (b.bytes) HIP_TRY(hipMemcpy(out, b.p, b.bytes, hipMemcpyDeviceToHost));
        }
        return RRT_OK;
    });
}

void rrt_raytracer_destroy(rrt_raytracer* rt) {
    if (!rt) return;
    int prev = 0;
    const bool have_device = hipGetDevice(&prev) == hipSuccess;
    if (have_device) {
        (void)hipSetDevice(rt->device);
        // Frames in flight: every mask buffer's last frame is waited for (its `done` lies behind its `ready`, so the side stream of the pass is idle then too)
        // before the events, the side stream and the buffers go with the raytracer below.
        for (const rrt_raytracer::CoverBuf& b : rt->cover) if (b.used && b.done.h) (void)hipEventSynchronize(b.done.h);
        if (rt->cover_stream.h) (void)hipStreamSynchronize(rt->cover_stream.h);
        if (rt->ev0) (void)hipEventDestroy(rt->ev0);
        if (rt->ev1) (void)hipEventDestroy(rt->ev1);
    }
    delete rt;                                                            // frees its device allocations (DevBuf members), on its device
    if (have_device) (void)hipSetDevice(prev);
}

int rrt_get_setup_times(const rrt_model* m, const rrt_raytracer* rt, rrt_setup_times* out) {
    return guarded([&]() -> int {
        if (!out) throw Error{RRT_ERR_INVALID_ARG, "null argument"};
        std::memset(out, 0, sizeof *out);
        if (m) { out->read_ms = m->m.read_ms; out->parse_ms = m->m.parse_ms; out->texture_ms = m->m.texture_ms; out->octree_ms = m->m.octree_ms; }
        if (rt) {
            out->index_ms = rt->built.ms_index; out->upload_ms = rt->upload_ms; out->hip_init_ms = rt->hip_init_ms; out->create_ms = rt->create_ms;
            out->gpu_setup = rt->gpu_setup ? 1.0 : 0.0;
            if (rt->gpu_setup || !m) out->octree_ms = rt->built.ms_octree;       // the tree this raytracer traces was built on its device
        }
        return RRT_OK;
    });
}

}  // extern "C"
