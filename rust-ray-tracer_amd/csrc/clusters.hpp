// clusters.hpp -- host side of the own-list index: what clusters.cpp builds from the host octree (the host twin of scene_build.hip's index kernels).
#pragma once
#include <cstdint>
#include <vector>

#include "device_scene.hpp"

namespace rrt {

struct Model;
struct ClusterSet {
    std::vector<DevSuper> supers;
    std::vector<DevClusterBox> tboxes;                 // per slot, + 8 spare records
    std::vector<DevClusterBox> child_boxes;            // tight padded bounds of the subtree of node c at [c - 1]; the 8 children of a node are consecutive
    std::vector<DevClusterBox> cboxes;                 // one per 8 slots, + 8 spare records so a 4x64-byte burst never leaves the buffer
    std::vector<uint32_t> slot_tri, slot_pos;          // per device slot: triangle index in push order (kPadSlot for padding), position in its node's own list
    std::vector<uint32_t> node_sup_begin, node_sup_count;
    std::vector<uint32_t> node_leaf_slot;              // slot of the triangle of a single-triangle leaf that is tested at its parent (kPadSlot otherwise)
    std::vector<DevChain> chains;                      // one per qualifying chain, in the order of their heads' node ids (child_boxes carries the references)
    uint32_t n_chain_nodes = 0;                        // chain nodes covered by those records
    bool has_groups = false;                           // some list got group records
    bool inline_leaves = false;                        // single-triangle leaves are tested at their parents (node_leaf_slot, DevNode::leaf_base)
    uint32_t n_list_slots = 0;                         // slots [0, n_list_slots) belong to own lists (cboxes/tboxes cover these); leaf slots follow
    double scene_magnitude = 0;
    double pad = 0;                                    // absolute padding of every index box
};
constexpr uint32_t kPadSlot = 0xFFFFFFFFu;
void build_clusters(const Model& m, bool enable_cull, ClusterSet& out);
// exactness guard: the triangles (of the tree) whose plane contains `origin` to within the distance at which a ray from `origin` can be
// coplanar-to-rounding with them
void find_origin_suspects(const Model& m, const double origin[3], double pad, std::vector<DevSuspect>& out);

}  // namespace rrt
