// host_build.cpp -- the scene set-up on the HOST (round-2 path, RRT_FLAG_HOST_SETUP): octree.cpp + clusters.cpp + the record fills below (the host
// twins of scene_build.hip's k_idx_nodes / k_idx_slots), then one upload.  Kept as the second implementation the GPU set-up is checked against
// byte for byte (tests/test_gpu_build.py), and for A/B timing.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "clusters.hpp"
#include "parallel.hpp"
#include "scene_build.hpp"

namespace rrt {
namespace {

void fill_nodes(const FlatOctree& T, const ClusterSet& CS, DevNode* nodes) {
    parallel_ranges(T.box.size(), 1 << 14, [&](size_t nb, size_t ne, size_t) {
    for (size_t i = nb; i < ne; i++) {
        DevNode& d = nodes[i];
        for (int k = 0; k < 3; k++) {
            d.lo[k] = T.box[i].lo[k]; d.hi[k] = T.box[i].hi[k];
            // the split plane: child TFR (index 6, octree.rs:216-225) has lo == mid on every axis; for a leaf recompute it as subdivide would
            d.mid[k] = T.first_child[i] ? T.box[T.first_child[i] + 6].lo[k] : d.lo[k] + (d.hi[k] - d.lo[k]) / 2.0;
        }
        d.first_child = T.first_child[i]; d.sup_begin = CS.node_sup_begin[i]; d.sup_count = CS.node_sup_count[i];
        d.s0_begin = d.sup_count ? CS.supers[d.sup_begin].tri_begin : 0;
        d.flags = (T.tri_count[i] ? 0x100u : 0u) | ((d.sup_count ? CS.supers[d.sup_begin].tri_count : 0u) << 24);
        d.leaf_base = CS.node_leaf_slot[i] != kPadSlot ? CS.node_leaf_slot[i] : 0;   // a leaf has no children: the field holds its own dense slot instead
        if (d.first_child) for (uint32_t k = 8; k-- > 0;) {
            if (T.tri_count[d.first_child + k]) d.flags |= 1u << k;
            if (CS.node_leaf_slot[d.first_child + k] != kPadSlot) { d.flags |= 1u << (9 + k); d.leaf_base = CS.node_leaf_slot[d.first_child + k]; }   // ends at the first one
        }
    }
    });
}

void fill_slots(const Model& M, const ClusterSet& CS, DevTriGeom* geom, DevTriAttr* attr) {
    parallel_ranges(CS.slot_tri.size(), 1 << 14, [&](size_t sb, size_t se, size_t) {
    for (size_t s = sb; s < se; s++) {
        if (CS.slot_tri[s] == kPadSlot) { std::memset(&geom[s], 0, sizeof(DevTriGeom)); std::memset(&attr[s], 0, sizeof(DevTriAttr)); attr[s].orig = kPadSlot; continue; }
        const Triangle& t = M.triangles[CS.slot_tri[s]];
        DevTriGeom& g = geom[s];
        g.v1[0] = t.v1.x; g.v1[1] = t.v1.y; g.v1[2] = t.v1.z;
        g.e1[0] = edge_canon(t.v2.x - t.v1.x); g.e1[1] = edge_canon(t.v2.y - t.v1.y); g.e1[2] = edge_canon(t.v2.z - t.v1.z);   // ray.rs:60
        g.e2[0] = edge_canon(t.v3.x - t.v1.x); g.e2[1] = edge_canon(t.v3.y - t.v1.y); g.e2[2] = edge_canon(t.v3.z - t.v1.z);   // ray.rs:61
        g.pos = CS.slot_pos[s]; g._pad = 0;
        DevTriAttr& a = attr[s];
        a.uv[0] = t.t1.x; a.uv[1] = t.t1.y; a.uv[2] = t.t2.x; a.uv[3] = t.t2.y; a.uv[4] = t.t3.x; a.uv[5] = t.t3.y;
        a.nrm[0] = t.n1.x; a.nrm[1] = t.n1.y; a.nrm[2] = t.n1.z; a.nrm[3] = t.n2.x; a.nrm[4] = t.n2.y; a.nrm[5] = t.n2.z;
        a.nrm[6] = t.n3.x; a.nrm[7] = t.n3.y; a.nrm[8] = t.n3.z;
        a.mat = t.mat; a.orig = CS.slot_tri[s];
    }
    });
}

// every node plane (lo, mid, hi) is 0 or has magnitude in [2^-200, 2^200] (device_scene.hpp: DevScene::bounds_plain)
bool bounds_plain(const DevNode* nodes, size_t n_nodes) {
    for (size_t i = 0; i < n_nodes; i++) { const DevNode& d = nodes[i];
        for (int k = 0; k < 3; k++)
            for (double v : {d.lo[k], d.mid[k], d.hi[k]})
                if (!(v == 0.0 || (std::fabs(v) > 0x1p-200 && std::fabs(v) < 0x1p200))) return false;
    }
    return true;
}

// does any triangle of the tree poke out of the root box?  (NaN coordinates count as poking out)
bool any_triangle_out_of_root(const Model& M) {
    std::atomic<int> out_of_root{0};
    const Triangle* tr = M.triangles.data();
    parallel_ranges(M.triangles.size(), 1 << 14, [&](size_t b, size_t e, size_t) {
        for (size_t i = b; i < e && !out_of_root.load(std::memory_order_relaxed); i++) {
            const Vec3* v[3] = {&tr[i].v1, &tr[i].v2, &tr[i].v3};
            double lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                const double c[3] = {a == 0 ? v[0]->x : a == 1 ? v[0]->y : v[0]->z, a == 0 ? v[1]->x : a == 1 ? v[1]->y : v[1]->z, a == 0 ? v[2]->x : a == 1 ? v[2]->y : v[2]->z};
                lo[a] = std::fmin(c[0], std::fmin(c[1], c[2])); hi[a] = std::fmax(c[0], std::fmax(c[1], c[2]));
            }
            bool touch = true, inside = true;
            for (int a = 0; a < 3; a++) { if (hi[a] < M.root.lo[a] || lo[a] > M.root.hi[a]) touch = false; if (!(lo[a] >= M.root.lo[a] && hi[a] <= M.root.hi[a])) inside = false; }
            if (touch && !inside) out_of_root.store(1, std::memory_order_relaxed);
        }
    });
    return out_of_root.load() != 0;
}

// (asynchronous: the host array must outlive the hipDeviceSynchronize that ends the upload)
template <class T> void upload_records(DevArena& A, T*& dst, const T* host, size_t count) {
    dst = A.take<T>(count);
    if (count) HIP_TRY(hipMemcpyAsync(dst, host, sizeof(T) * count, hipMemcpyHostToDevice, nullptr));
}

}  // namespace

void host_build_scene(const Model& M, bool enable_cull, const double origin[3], BuiltScene& out) {
    using clk = std::chrono::steady_clock;
    const FlatOctree& T = host_tree(M);
    const size_t n_nodes = T.box.size();
    const auto t_index0 = clk::now();
    ClusterSet CS;
    build_clusters(M, enable_cull, CS);
    const size_t n_slots = CS.slot_tri.size();
    // (plain arrays: a std::vector would zero 250 MB on one thread before the workers fill it)
    std::unique_ptr<DevNode[]> nodes(new DevNode[n_nodes ? n_nodes : 1]);
    std::unique_ptr<DevTriGeom[]> geom(new DevTriGeom[n_slots ? n_slots : 1]); std::unique_ptr<DevTriAttr[]> attr(new DevTriAttr[n_slots ? n_slots : 1]);
    fill_nodes(T, CS, nodes.get());
    fill_slots(M, CS, geom.get(), attr.get());
    const auto t_index1 = clk::now();

    out.n_tris = (uint32_t)M.triangles.size(); out.n_nodes = (uint32_t)n_nodes; out.max_depth = T.max_depth;
    out.n_in_tree = (uint32_t)T.own_idx.size();   // every triangle in the tree appears in exactly one own list
    out.n_list_slots = CS.n_list_slots; out.n_slots_total = (uint32_t)n_slots; out.n_sup_records = (uint32_t)CS.supers.size(); out.n_clusters = CS.n_list_slots / 8;
    for (uint32_t k = 0; n_nodes && k < CS.node_sup_count[0]; k++) {      // the root's slots: its super-clusters' runs, each padded to a multiple of 8 (a group record holds none)
        const DevSuper& sp = CS.supers[CS.node_sup_begin[0] + k];
        if (sp.tri_count) out.root_slot_end = std::max(out.root_slot_end, (sp.tri_begin + sp.tri_count + 7u) & ~7u);
    }
    out.has_groups = CS.has_groups ? 1u : 0u; out.inline_leaves = CS.inline_leaves ? 1u : 0u;
    out.scene_magnitude = CS.scene_magnitude; out.pad = CS.pad;
    out.n_chains = (uint32_t)CS.chains.size(); out.n_chain_nodes = CS.n_chain_nodes;
    out.bounds_plain = bounds_plain(nodes.get(), n_nodes) ? 1u : 0u;
    out.all_inside_root = any_triangle_out_of_root(M) ? 0u : 1u;
    std::vector<DevSuspect> sus;   // exactness guard of the index for rays from `origin` (clusters.cpp, find_origin_suspects)
    if (enable_cull) find_origin_suspects(M, origin, CS.pad, sus);
    out.n_suspects = (uint32_t)sus.size();
    if (sus.size() > RRT_MAX_SUSPECTS) sus.clear();   // beyond the cap every ray from the origin runs unfiltered; the list is not read
    // the triangle -> slot table (scene_build.hpp: tri_slot): slots in ascending order, the first one of a triangle stays -- the lowest, as the GPU set-up's minimum
    std::vector<uint32_t> tri_slot(M.triangles.size(), kPadSlot);
    for (size_t s = 0; s < n_slots; s++) { const uint32_t tri = CS.slot_tri[s]; if (tri != kPadSlot && tri_slot[tri] == kPadSlot) tri_slot[tri] = (uint32_t)s; }

    const size_t bytes[] = {n_nodes * sizeof(DevNode), n_slots * sizeof(DevTriGeom), n_slots * sizeof(DevTriAttr), CS.supers.size() * sizeof(DevSuper),
                            CS.cboxes.size() * sizeof(DevClusterBox), CS.child_boxes.size() * sizeof(DevClusterBox), CS.tboxes.size() * sizeof(DevClusterBox),
                            CS.chains.size() * sizeof(DevChain), sus.size() * sizeof(DevSuspect), tri_slot.size() * sizeof(uint32_t)};
    size_t need = 0;
    for (size_t b : bytes) need += b + 512;   // (each buffer starts on a 256-byte boundary and is at least one record long)
    out.alloc = dev_alloc(need);
    DevArena A; A.base = static_cast<char*>(out.alloc.h); A.cap = need;
    upload_records(A, out.nodes, nodes.get(), n_nodes); upload_records(A, out.geom, geom.get(), n_slots); upload_records(A, out.attr, attr.get(), n_slots);
    upload_records(A, out.supers, CS.supers.data(), CS.supers.size()); upload_records(A, out.cboxes, CS.cboxes.data(), CS.cboxes.size());
    upload_records(A, out.child_boxes, CS.child_boxes.data(), CS.child_boxes.size()); upload_records(A, out.tboxes, CS.tboxes.data(), CS.tboxes.size());
    upload_records(A, out.chains, CS.chains.data(), CS.chains.size()); upload_records(A, out.suspects, sus.data(), sus.size());
    upload_records(A, out.tri_slot, tri_slot.data(), tri_slot.size());
    HIP_TRY(hipDeviceSynchronize());
    out.ms_octree = M.octree_ms;
    out.ms_index = std::chrono::duration<double, std::milli>(t_index1 - t_index0).count();
    out.ms_upload = std::chrono::duration<double, std::milli>(clk::now() - t_index1).count();
}

}  // namespace rrt
