// scene_build.hpp -- the once-per-scene set-up and its result.  Two builders produce the same BuiltScene, byte for byte (tests/test_gpu_build.py):
//   gpu_build_scene   ON THE GPU (the default): octree build (src/collision/octree.rs:41-241, order-exact), own-list index
//                     (clusters.cpp restated level-parallel) and the device records, all from the uploaded triangle array (scene_build.hip);
//   host_build_scene  on the host (RRT_FLAG_HOST_SETUP): octree.cpp + clusters.cpp + the record fills of host_build.cpp, then one upload.
// raytracer.cpp drives either from rrt_raytracer_create and adopts the result.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>

#include "device_memory.hpp"
#include "device_scene.hpp"
#include "model.hpp"

namespace rrt {

// Everything the trace kernels read, in device memory, plus (GPU set-up only) the flattened octree in the reference's node numbering, kept on the
// device until the raytracer is destroyed so that rrt_raytracer_get_octree can hand it out.  A buffer the builder does not keep stays null.
struct BuiltScene {
    DevBuf alloc;   // ONE allocation, carved up into every buffer below
    size_t alloc_bytes = 0;   // its size (an update hands a retired one to the next build: BuildMemory)
    DevNode* nodes = nullptr; DevTriGeom* geom = nullptr; DevTriAttr* attr = nullptr;
    DevSuper* supers = nullptr; DevClusterBox* cboxes = nullptr; DevClusterBox* child_boxes = nullptr; DevClusterBox* tboxes = nullptr;
    DevSuspect* suspects = nullptr;
    DevChain* chains = nullptr; uint32_t n_chains = 0, n_chain_nodes = 0;   // chain records (device_scene.hpp: DevChain) and the chain nodes they cover
    // flattened octree, final ids (octree.rs numbering): same allocation
    double* oct_box = nullptr;          // [n_nodes][6] lo xyz, hi xyz
    uint32_t* oct_first_child = nullptr, *oct_tri_count = nullptr, *oct_own_off = nullptr /* n_nodes + 1 */, *oct_own_idx = nullptr /* n_in_tree */;
    uint32_t* slot_tri = nullptr, *slot_pos = nullptr;   // per device slot (tests)
    uint32_t* tri_slot = nullptr;       // [n_tris]: the LOWEST slot whose attr.orig is the triangle -- an inline leaf's triangle owns two (clusters.cpp) --, 0xFFFFFFFF for a
                                        // triangle outside the tree.  The inverse of attr.orig that rrt_resolve_hits reads; both builders keep it
    uint32_t n_tris = 0, n_nodes = 0, n_in_tree = 0, n_list_slots = 0, n_slots_total = 0, n_sup_records = 0, n_clusters = 0, max_depth = 0;
    uint32_t has_groups = 0, inline_leaves = 0, bounds_plain = 1, n_suspects = 0, all_inside_root = 0;   // all_inside_root: no triangle of the tree pokes out of the root box
    uint32_t root_slot_end = 0;         // the root node's own list is the slots [0, root_slot_end) (its padding slots included): the coverage pass may list boxes of it as wide
    double scene_magnitude = 0, pad = 0;
    // GPU set-up: GPU time of the three stages (HIP events on the build stream).  Host set-up: wall time of the host octree build (whenever it
    // ran for this model), of index + record fills, and of everything after them (scans, allocation, upload).
    double ms_upload = 0, ms_octree = 0, ms_index = 0;
};

// The triangles either as the model's array (Triangle records, SceneData.triangles) or as the caller's own arrays (rrt_raytracer_create_from_arrays:
// pos / uv / nrm [n][3][3] doubles, mat [n]) -- those are uploaded as they are and packed into Triangle records on the device.
// With on_device set, pos / uv / nrm / mat are DEVICE pointers of the current device (rrt_raytracer_set_triangles_device): the build reads them where they
// lie, nothing is staged or uploaded, and the caller has ordered the build stream behind whatever wrote them.
struct TriSource { const Triangle* tris = nullptr; const double* pos = nullptr; const double* uv = nullptr; const double* nrm = nullptr; const uint32_t* mat = nullptr;
                   bool on_device = false; };
// Device memory a raytracer keeps between the builds of its scene updates (rrt_raytracer_set_triangles), so that an update makes no hipMalloc and no
// hipFree (which synchronises the device): the build's three temporaries, the sort's extra storage where rocPRIM wanted any, and the scene allocation the
// last update retired.  A piece is reused when it is large enough and replaced by a larger one otherwise.
struct BuildMemory {
    struct Piece {
        DevBuf buf; size_t bytes = 0;
        void* at_least(size_t need) { if (bytes < need || !buf.h) { buf.reset(); bytes = 0; buf = dev_alloc(need); bytes = need; } return buf.h; }
        void release() { buf.reset(); bytes = 0; }
    };
    Piece t1, t2, t3, sort, scene;
    void release() { for (Piece* p : {&t1, &t2, &t3, &sort, &scene}) p->release(); }
};
// Builds the scene on the current HIP device from `src` (host arrays, uploaded here through pinned staging, or device arrays: TriSource).
// enable_cull = !RRT_FLAG_NO_CULL.  Throws rrt::Error (RRT_ERR_DEPTH when the octree is deeper than RRT_MAX_OCTREE_DEPTH) or HipFail; `out` is then
// to be discarded.
// `after_upload` (may be empty) is called once the triangles have been handed to the staging ring, before the octree build: the caller's other uploads
// (textures) can start there, beside the build, without competing with the triangles for the ring.
// `keep` (may be null: every temporary is allocated and freed here, as creation does) lends and keeps the device memory of the build; out.alloc may
// then be keep->scene's allocation.
void gpu_build_scene(const TriSource& src, uint32_t n_tris, const Box& root, bool enable_cull, const double origin[3], void* stream, BuiltScene& out,
                     const std::function<void()>& after_upload = {}, BuildMemory* keep = nullptr);
// Number of i < n with d_mat[i] >= n_mats (d_mat in device memory), through the counter d_count (device, 4 bytes): enqueued on `stream`, not synchronised.
// hipError_t cast to int.
int launch_count_bad_materials(const uint32_t* d_mat, uint32_t n, uint32_t n_mats, uint32_t* d_count, void* stream);

// The same scene from the model's host octree (host_tree(m)).  Keeps no octree, slot_tri or slot_pos on the device (tri_slot it keeps: a kernel reads it).  Returns after a
// hipDeviceSynchronize: the host arrays it uploaded from are gone.  Same exceptions.
void host_build_scene(const Model& m, bool enable_cull, const double origin[3], BuiltScene& out);

}  // namespace rrt
