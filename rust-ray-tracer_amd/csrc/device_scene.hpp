// device_scene.hpp -- layout of the scene in HBM and the host-side launch interface of the HIP kernels.
//
// Everything is uploaded once per raytracer (rrt_raytracer_create).  Layout choices:
//  * geometry is stored in OWN-LIST SLOT ORDER: slot s = position in the concatenation of every node's
//    `triangles` Vec (octree.rs:9) in node-id order, so a node's triangles are one contiguous run and the
//    traversal needs no tri_index indirection (ray.rs:119-120).  orig[s] maps back to push order.
//  * TriGeom keeps v1 and the two edges e1 = v2-v1, e2 = v3-v1.  The reference recomputes the edges on every
//    test (ray.rs:60-61); a f64 subtraction gives the same bits whenever it is done, so they are precomputed.
//  * one node is one 64-byte record: box + first_child + own run + occupancy flags of its 8 children, read with
//    wave-uniform (scalar) loads.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rrt {

struct DevNode {                 // 96 B
    double lo[3], hi[3];         // Aabb, aabb.rs:4-8
    double mid[3];               // the split planes lo + (hi-lo)/2 (octree.rs:136-138): with lo/hi they ARE the 8 children's boxes
    uint32_t first_child;        // 0 = leaf; children are first_child..first_child+7 (octree.rs:226-238)
    uint32_t sup_begin;          // first super-cluster of this node's own triangle list (clusters.cpp)
    uint32_t sup_count;
    uint32_t flags;              // bit k (0..7): child k has triangle_count > 0; bit 8: this node has triangle_count > 0 (ray.rs:112);
                                 // bit 9+k: child k is a single-triangle leaf whose triangle is tested here, at its parent (clusters.cpp);
                                 // bits 24..30: number of slots of the first super-cluster (<= 64; the only one when sup_count == 1)
    uint32_t s0_begin;           // first slot of the first super-cluster
    uint32_t leaf_base;          // dense slot of the triangle of the first such leaf child; the j-th such child (in child order) has slot leaf_base + j.
                                 // In the record of such a leaf itself: its own dense slot.
};
static_assert(sizeof(DevNode) == 96, "DevNode must be 96 bytes");

struct DevTriGeom { double v1[3], e1[3], e2[3]; uint32_t pos, _pad; };   // 80 B; pos = position in the node's own list (tie-break, ray.rs:124)
static_assert(sizeof(DevTriGeom) == 80, "DevTriGeom must be 80 bytes");
// An edge of a triangle with a NaN or infinite vertex can be NaN, and which NaN a subtraction returns (sign, payload) differs between the host CPU
// and the GPU.  Both set-ups store every NaN edge component as the one quiet NaN 0x7FF8000000000000, so that their records stay byte-identical.
// (Through integer bits: a compiler may treat a select between a NaN and x as x.)  The traversal only ever sees "some NaN" either way.
__host__ __device__ inline double edge_canon(double x) {
    uint64_t b; __builtin_memcpy(&b, &x, 8);
    if ((b & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (b & 0x000FFFFFFFFFFFFFull) != 0ull) b = 0x7FF8000000000000ull;
    __builtin_memcpy(&x, &b, 8);
    return x;
}

// own-list index (clusters.cpp): padded f32 boxes, rounded outward
// A super-cluster owns the slots [tri_begin, tri_begin + tri_count), tri_begin a multiple of 8, tri_count <= 64; its cluster c is the
// 8 slots from tri_begin + 8c, and the box of the cluster that starts at slot s is cboxes[s / 8].  Slots between the end of a
// super-cluster and the next multiple of 8 are padding (all-zero geometry, never hit).
// Box records.  While clusters.cpp builds the index they hold (lo, hi); build_clusters ends by rewriting every record IN PLACE to the device
// form (centre, half-extent) with [c - h, c + h] a superset of [lo, hi] (boxes_to_centre_half): the kernels' slab tests take the near and far
// plane of an axis as one packed FMA  c*inv + n -/+ h*|inv|  instead of two FMAs and a min/max pair.  An empty box is (0, -FLT_MAX): never
// hit; a box of the no-cull index is (0, FLT_MAX): always hit.
struct DevSuper { union { float lo[3]; float c[3]; }; union { float hi[3]; float h[3]; }; uint32_t tri_begin, tri_count; };     // 32 B
struct DevClusterBox { union { float lo[3]; float c[3]; }; union { float hi[3]; float h[3]; }; uint32_t _pad[2]; };             // 32 B
static_assert(sizeof(DevClusterBox) == 32 && sizeof(DevSuper) == 32, "cluster records must be 32 bytes");

// Chain shortcut (render.hip "chain shortcut").  A CHAIN NODE is an internal node with exactly one non-empty child; a chain is a
// maximal run of them below some parent: head d1, d2, ..., down to the first node D on that path that is not a chain node (the chain's END).  The
// reference's tree has such runs wherever the scene is small against the root box (octree.rs:77-80: the first triangle that reaches a node stays in it).
// A chain whose nodes' own lists hold at most kChainMaxTris triangles in all gets one record: D's padded subtree box (a copy of
// D's child_boxes record), D's node id, the number of those own triangles and their padded boxes (copies of their tboxes records) in chain order; unused
// triangle records are the empty box.  The child_boxes record of the head carries 1 + the record's index in _pad[1] (0: no chain record).
constexpr uint32_t kChainMaxTris = 4;   // K.  Every chain node owns at least one triangle, so K also bounds the length of a chain that gets a record.  Measured on the
                                        // teapot frame: K = 2 / 4 / 8 give the same time (profiles/r05_chain_shortcut.txt)
struct DevChain { float c[3], h[3]; uint32_t end_node, n_tris; DevClusterBox tri[kChainMaxTris]; };                             // 160 B
static_assert(sizeof(DevChain) == 32 + 32 * kChainMaxTris, "DevChain must be a box record plus kChainMaxTris box records");

struct DevTriAttr {                                                // 128 B: one cache line per shaded hit
    double uv[6];                // t1.x,t1.y, t2.x,t2.y, t3.x,t3.y (raytracer.rs:45-50 read x,y only)
    double nrm[9];               // n1, n2, n3
    uint32_t mat, orig;          // material index; triangle index in push order
};
static_assert(sizeof(DevTriAttr) == 128, "DevTriAttr must be 128 bytes");

struct DevTexture { const uint8_t* rgb; uint32_t width, height; };               // entities.rs:86-91
// material.rs:11-22, with the descriptors of its texture and bump map inline: a hit reads material -> texel, not material -> texture table -> texel
struct DevMaterial { double ka[3], kd[3], ks[3], ns, kr; int32_t tex, bump; DevTexture tex_desc, bump_desc; };
struct DevLight { uint32_t kind, _pad; double intensity; double v[3]; };         // entities.rs:5-9

// Exactness guard of the own-list index: a triangle whose plane contains the raytracer's origin to within rounding-noise
// distance.  A ray from that origin that is also parallel to the plane to within `alpha` lies IN the plane, the reference's Moller-Trumbore result
// for the pair is rounding noise, and the box filters -- which assume an accepted pair lies inside the padded box -- are switched off for that ray.
struct DevSuspect { double n[3]; double alpha2; };   // unit normal of the plane; squared sine threshold (>= 1: every direction)
#define RRT_MAX_SUSPECTS 64

#define RRT_MAX_LIGHTS 16
#define RRT_MAX_REFLECT 8

struct DevScene {                // passed to kernels by value (kernarg segment -> SGPRs)
    const DevNode* nodes;
    const DevTriGeom* geom;
    const DevSuper* supers;
    const DevClusterBox* cboxes;
    const DevClusterBox* child_boxes;
    const DevClusterBox* tboxes;          // one padded box per slot (per triangle)
    const DevTriAttr* attr;
    const DevMaterial* mats;
    const DevTexture* tex;
    uint32_t n_nodes, n_slots, n_mats, n_tex;
    uint32_t n_lights, max_reflection_depth, stack_levels;
    uint32_t fc_mask;            // 0x00FFFFFF when stack frames carry a leaf-hit mask above first_child (scenes below 2^24 nodes), else 0xFFFFFFFF
    double origin[3];
    double surface_offset;
    float cull_limit;            // rays with |origin| or |direction| components beyond this (or non-finite) skip the box culling
    float cull_half_over_limit;  // 0.5 / cull_limit (the fp32 filter's parameter scale, render.hip make_ray32)
    uint32_t cull_enabled;
    uint32_t has_groups;         // some own list carries group records (clusters.cpp): launches use the kernel instantiation that handles them
    uint32_t n_suspects;         // triangles whose plane passes through `origin` (see DevSuspect); more than RRT_MAX_SUSPECTS: every ray from `origin` runs unfiltered
    uint32_t specular_all;       // RRT_FLAG_NO_SPECULAR_SKIP: every specular term is evaluated, also those the f64 sum certainly absorbs (specular_skip.hpp).  (In what
                                 // was padding in front of the pointer below: no other field moves.)
    const DevSuspect* suspects;
    float inner_shrink;          // 2 x the filter's pad when every triangle of the tree lies inside the root box (a child's subtree box then lies inside its octant box), else 0: render.hip, RRT_CERTAIN_HIT
    uint32_t bounds_plain;       // every node plane (lo, mid, hi) is 0 or has magnitude in [2^-200, 2^200]: the walk may share the reciprocal of a ray's direction across its slab quotients (render.hip, RayRcp)
    const DevChain* chains;      // chain records (above), or nullptr when the shortcut is off: no record, inner_shrink == 0, RRT_FLAG_NO_CHAIN_SHORTCUT.  (Behind the
                                 // fields the other kernels read: where a pointer sits among the first sixteen words of the kernarg segment shapes their scalar loads.)
    DevLight lights[RRT_MAX_LIGHTS];
#ifdef RRT_PROFILE
    unsigned long long* prof;    // developer build only (make prof): 16 wave-level work counters + 6 s_memtime region timers + the specular pair, see tools/profile_counters.py
#endif
};

struct FrameParams {
    uint32_t width, height;      // canvas size
    double x_scale, y_scale, z_value;   // engine.rs:189-191
    uint32_t tiles_x, tiles_y;   // 8x8-pixel tiles covering the canvas
    uint32_t rank, world;        // tile k belongs to rank k % world
    uint32_t tiled_output;       // 0: out is the row-major framebuffer; 1: out is this rank's tile-major buffer
    uint32_t xcd_chunk;          // blocks per chunk of the XCD-aware block order (render.hip: render_kernel), 0 = plain order
    // A launch may cover a band of the frame only (progressive display, engine.rs:196-253): the tiles [tile_begin, tile_end) in row-major tile
    // order, and of those only the canvas rows [row_begin, row_end).  The whole frame: tile_begin = 0, tile_end = tiles_x*tiles_y, rows [0, height).
    uint32_t tile_begin, tile_end, row_begin, row_end;
    // View basis (rrt.h: rrt_camera), behind everything the kernels read before: the sub-sample ray through (a, b, c) = (xd*x_scale, yd*y_scale, z_value) has
    // direction right*a + up*b + forward*c.  Wave-uniform kernel arguments: they stay in scalar registers until the direction has been formed.
    double right[3], up[3], forward[3];
};

// ---- Arguments of the stage kernels (render.hip: visibility_kernel, surface_kernel, shade_kernel, ambient_kernel, colour_kernel; rrt.h: rrt_render_visibility_device
// and its neighbours, and their *_tile_list_device forms).  Every stage has ONE kernel body and two front ends; its argument is a front-end part -- where the waves
// of the launch lie in the frame -- plus the planes of the stage, which exist once.  Of kernels of their own, so that FrameParams and DevScene -- arguments of the
// frame kernels too -- stay as they are.
// Front end 1, a region of a frame.  The launch covers the 8x8-pixel tiles that intersect the region, in row-major order: tiles_w of them per row from tile
// (tile_x0, tile_y0); F.tile_begin / F.tile_end = [0, their number), F.rank / F.world = 0 / 1.  The region is the columns [col_begin, col_end) of the rows
// [F.row_begin, F.row_end); every plane is a plane of the REGION, [rows][columns][4 sub-samples] and its kin, the pixels [rows][columns].
struct Region {
    FrameParams F;
    uint32_t col_begin, col_end;
    uint32_t tile_x0, tile_y0, tiles_w, _pad;
};
// Front end 2, a list of tiles in device memory: the whole frame (F.rank / F.world = 0 / 1, F.xcd_chunk = 0: the list's order is the schedule), a list of n tile
// indices ty * F.tiles_x + tx and the bound -- null, or one uint32 in device memory: entries [min(n, *count), n) are not read.  tiles and count are only ever
// read; an entry is used as an index only after the compare with F.tile_end.  Every plane is a WHOLE-FRAME plane, [height][width][4 sub-samples] and its kin, the
// framebuffer and `grey` [height][width]: what the region form takes for the whole frame.
struct TileList {
    FrameParams F;
    const uint32_t *tiles, *count;
    uint32_t n, _pad;
};
// The planes.  Visibility: [..][4 sub-samples] each; a null plane is not written.
struct VisPlanes { uint8_t* hit; double *t, *u, *v; uint32_t* tri; uint32_t* albedo; };
// Surface: point and normal [..][4 sub-samples][3], material and lights [..][4 sub-samples]; a null plane is not written, and a null `lights` also means that no
// shadow ray is walked.
struct SurfacePlanes { double *point, *normal; uint32_t *material, *lights; };
// Shade: the five planes the kernel READS, laid out as the surface launch wrote them, and the framebuffer it writes.  `lights` may be null: the depth-0 shadow
// rays are then walked.
struct ShadePlanes { const double *point, *normal; const uint32_t *material, *albedo, *lights; uint32_t* out; };
// Ambient: the three planes the kernel READS, the two it writes (occluded: masks per sub-sample; grey: pixels; either may be null, not both) and the sample table:
// n_samples directions in the tangent frame of a hit, and the max_t of every ray.  The table travels in the kernel arguments, as the lights do: wave-uniform, read
// with scalar loads.
#ifndef RRT_MAX_AMBIENT_SAMPLES
#define RRT_MAX_AMBIENT_SAMPLES 32
#endif
struct AmbientPlanes {
    const double *point, *normal; const uint32_t* material;
    uint32_t *occluded, *grey;
    uint32_t n_samples, _pad;
    double max_t;
    double dirs[RRT_MAX_AMBIENT_SAMPLES][3];
};

// The stages.  Visibility: a front end and its six planes.  Surface: the same -- every visibility plane may be null here -- and the four surface planes.
template <class Front> struct VisStage { Front front; VisPlanes vis; };
template <class Front> struct SurfaceStage { Front front; VisPlanes vis; SurfacePlanes planes; };
// The stages that write no visibility plane.  Their region forms keep six unused plane pointers behind the region, as when their argument began with a whole
// visibility argument: where a pointer sits in the kernel-argument segment shapes a kernel's scalar loads, and no layout moves.
template <class Front> struct BareFrontOf { using type = Front; };
template <> struct BareFrontOf<Region> { using type = VisStage<Region>; };
template <class Front> using BareFront = typename BareFrontOf<Front>::type;
template <class Front> struct ShadeStage { BareFront<Front> front; ShadePlanes planes; };
template <class Front> struct AmbientStage { BareFront<Front> front; AmbientPlanes planes; };
// The fused colour.  Of a region: pixel (px, py) goes to out[(py - F.row_begin) * pitch + (px - col_begin)], pitch in elements and at least the region's width;
// nothing else of `out` is touched.  The pitch is the region front end's: a list stores into the row-major [height][width] framebuffer.
struct RenderRegionParams { VisStage<Region> front; uint32_t* out; uint32_t pitch, _pad; };
struct TileListParams { TileList front; uint32_t* out; };
// (the front end inside a `front` member)
__host__ __device__ inline const Region& front_end(const Region& r) { return r; }
__host__ __device__ inline const Region& front_end(const VisStage<Region>& v) { return v.front; }
__host__ __device__ inline const TileList& front_end(const TileList& l) { return l; }

using VisParams = VisStage<Region>;
using SurfaceParams = SurfaceStage<Region>;
using ShadeParams = ShadeStage<Region>;
using AmbientParams = AmbientStage<Region>;
using VisTileListParams = VisStage<TileList>;
using SurfaceTileListParams = SurfaceStage<TileList>;
using ShadeTileListParams = ShadeStage<TileList>;
using AmbientTileListParams = AmbientStage<TileList>;
static_assert(sizeof(DevScene) + sizeof(AmbientParams) < 4096 && sizeof(DevScene) + sizeof(AmbientTileListParams) < 4096,
              "the arguments of ambient_kernel, in either form, must fit the 4 KB kernel-argument segment");
// The byte layout of every argument is pinned: its size and where its first plane lies.
#define RRT_PIN_LAYOUT(T, first_plane, size, offset) static_assert(sizeof(T) == size && offsetof(T, first_plane) == offset, #T " must keep its layout")
RRT_PIN_LAYOUT(VisParams, vis.hit, 216, 168);               RRT_PIN_LAYOUT(VisTileListParams, vis.hit, 216, 168);
RRT_PIN_LAYOUT(SurfaceParams, planes.point, 248, 216);      RRT_PIN_LAYOUT(SurfaceTileListParams, planes.point, 248, 216);
RRT_PIN_LAYOUT(ShadeParams, planes.point, 264, 216);        RRT_PIN_LAYOUT(ShadeTileListParams, planes.point, 216, 168);
RRT_PIN_LAYOUT(AmbientParams, planes.point, 1040, 216);     RRT_PIN_LAYOUT(AmbientTileListParams, planes.point, 992, 168);
RRT_PIN_LAYOUT(RenderRegionParams, out, 232, 216);          RRT_PIN_LAYOUT(TileListParams, out, 176, 168);
#undef RRT_PIN_LAYOUT

// Argument of the per-ray surface kernels (render.hip: surface_rays_kernel; rrt.h: rrt_surface_rays_device): the twelve output arrays of a batch of n rays, in
// the order and layout of rrt_ray_surface -- [n] each, point / normal / next_origin / next_dir [n][3].  A null array is not written; which are null also decides
// what the kernel computes at all (no `lights`: no shadow walk).
struct RaySurfaceParams {
    uint8_t* hit; double *t, *u, *v; uint32_t *tri, *albedo;
    double *point, *normal; uint32_t *material, *lights;
    double *next_origin, *next_dir;
};
static_assert(sizeof(RaySurfaceParams) == 96, "RaySurfaceParams mirrors rrt_ray_surface: twelve pointers");

// Argument of the per-ray shade kernels (render.hip: shade_rays_kernel; rrt.h: rrt_shade_rays_device): the six arrays the kernel READS -- the rays' directions and
// the records the per-ray surface launch wrote for them, [n] each, dirs / point / normal [n][3]; `lights` may be null: the shadow rays of the records' hits are
// then walked -- the three it writes (colour [n], local [n][3], kr [n]; any may be null, not all: a null array is not written, and a null `colour` also means
// that no reflection ray is formed) and the recursion depth at which the batch stands.
struct ShadeRaysParams {
    const double *dirs, *point, *normal; const uint32_t *material, *albedo, *lights;
    uint32_t* colour; double *local, *kr;
    uint32_t depth, _pad;
};

// Argument of the per-ray ambient kernels (render.hip: ambient_rays_kernel; rrt.h: rrt_ambient_rays_device): the three arrays the kernel READS -- the records the
// per-ray surface launch wrote for a batch of n rays, point / normal [n][3], material [n] -- the optional rotation (rot: [n][2], (c, s) per record; null: the
// samples enter the tangent frame as they are), the two arrays it writes (occluded [n] masks, open [n] counts; either may be null, not both) and the sample table
// of AmbientPlanes, which travels in the kernel arguments in the same way.
struct AmbientRaysParams {
    const double *point, *normal; const uint32_t* material;
    const double* rot;
    uint32_t *occluded, *open;
    uint32_t n_samples, _pad;
    double max_t;
    double dirs[RRT_MAX_AMBIENT_SAMPLES][3];
};
static_assert(sizeof(DevScene) + 2 * sizeof(uint64_t) + sizeof(AmbientRaysParams) < 4096, "the arguments of ambient_rays_kernel, the bound of its counted form included, must fit the 4 KB kernel-argument segment");

// Argument of the resolve kernels (render.hip: resolve_hits_kernel; rrt.h: rrt_resolve_hits_device): the rays and the four arrays of kept hits the kernel READS
// -- [n] each, origins / dirs [n][3]; u and v may be null when only point and / or material are asked for -- the triangle -> slot table of the scene in force
// (BuiltScene::tri_slot: the lowest slot of every triangle, 0xFFFFFFFF for a triangle outside the tree; here and not in DevScene, whose layout every other kernel's
// arguments follow) and the seven arrays it writes, in the order and layout of rrt_ray_surface.  A null output is not written; a null `lights` also means that
// nothing is walked.  tri[i] is used as an index only after tri[i] < n_tris, tri_slot[tri[i]] only after the compare with n_slots.
struct ResolveParams {
    const double *origins, *dirs;
    const double *t, *u, *v; const uint32_t* tri;
    const uint32_t* tri_slot; uint32_t n_tris, n_slots;
    uint32_t* albedo; double *point, *normal; uint32_t *material, *lights;
    double *next_origin, *next_dir;
};

// Argument of the compaction kernels (compact.hip; rrt.h: rrt_compact_rays_device). RaySetPtrs mirrors rrt_ray_set: the rays, their bounds and rotations and the
// twelve record arrays of a batch, [n] each with the element widths of rrt.h; a null array of `dst` is not written, and only the arrays `dst` asks for are read of
// `src` -- besides `material`, which the HIT and MIRROR selections read.  dst.max_t with a null src.max_t: +inf for the survivors.
struct RaySetPtrs {
    double *origins, *dirs, *max_t, *rot;
    uint8_t* hit; double *t, *u, *v; uint32_t *tri, *albedo;
    double *point, *normal; uint32_t *material, *lights;
    double *next_origin, *next_dir;
};
static_assert(sizeof(RaySetPtrs) == 128, "RaySetPtrs mirrors rrt_ray_set: sixteen pointers");
// A count / place block covers a tile of kCompactTile consecutive entries; the scratch holds one uint32 per tile and the total behind them.
constexpr uint32_t kCompactTile = 1024;
constexpr uint32_t compact_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kCompactTile - 1) / kCompactTile); }
struct CompactParams {
    RaySetPtrs src, dst;
    const uint8_t* flag;         // RRT_SELECT_FLAG
    const DevMaterial* mats;     // RRT_SELECT_MIRROR: the resident table
    uint32_t* index;             // [n], or null
    uint32_t* tiles;             // the scratch: [compact_tiles(n) + 1]
    uint32_t n, select, n_mats;
    uint32_t any_dst;            // some array of `dst` is set (with a null `index` and none of them, only the count is wanted: nothing is placed)
};

// kernel launches (compact.hip).  Both return hipError_t cast to int; nothing is synchronised.
// d_bound: null, or the bound of a counted launch (rrt.h: COUNTED DEVICE FORMS) -- one uint32 in device memory, read by the kernels when they run; grids are those of n.
// count, scan and place of q on `stream`; the total goes to q.tiles[compact_tiles(q.n)] and, if it is not null, to *d_count
int launch_compact(const CompactParams& q, const uint32_t* d_bound, uint32_t* d_count, void* stream);
// d_dst[d_index[j]] = d_src[j], elem_bytes (1, 4, 8, 16 or 24) each, for every j in [0, n) -- with a bound [0, min(n, *d_bound)) -- with d_index[j] < n
int launch_scatter(uint32_t n, const uint32_t* d_bound, const uint32_t* d_index, uint32_t elem_bytes, const void* d_src, void* d_dst, void* stream);

// Argument of the tile-test kernel (tiles.hip: mark_tiles_kernel; rrt.h: rrt_mark_tiles_device): one test of rrt_tile_test over the planes a (and b: DIFFERS) of the
// region (x0, y0, w, h) of a frame of tiles_x x tiles_y 8x8-pixel tiles, into marks[tiles_x * tiles_y].  test: RRT_TILE_* without the KEEP bit, which is `keep`.
// vec: the host's choice of the 16-byte path, made once per launch (regions.cpp: tile_test_params has the rule).  Everything is checked by the caller.
struct TileTestParams {
    const void *a, *b;
    uint8_t* marks;
    uint32_t tiles_x, tiles_y;
    uint32_t x0, y0, w, h;
    uint32_t test, keep, elem_bytes, per_pixel;
    uint32_t lo, hi;
    uint32_t set[8];
    uint32_t vec, _pad;
};
// one launch of q on `stream`; returns hipError_t cast to int; nothing is synchronised
int launch_mark_tiles(const TileTestParams& q, void* stream);

// Argument of the sort kernels (sort.hip; rrt.h: rrt_sort_rays_device).  A hist / place block covers a tile of kSortTile consecutive entries.  The scratch, in
// 4-byte words: two (key, index) buffer pairs of n words per array, the digit counts of one pass, digit-major ([256][sort_tiles(n)]), and the 256 digit totals.
constexpr uint32_t kSortTile = 4096, kSortDigits = 256;
constexpr uint32_t sort_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kSortTile - 1) / kSortTile); }
constexpr size_t sort_scratch_words(uint32_t n) { return n ? 4 * (size_t)n + (size_t)kSortDigits * sort_tiles(n) + kSortDigits : 0; }
struct SortParams {
    RaySetPtrs src, dst;         // src: what the key mode and dst read; dst: the gathered arrays, null = not wanted
    const uint32_t* keys;        // RRT_SORT_KEY_GIVEN
    uint32_t *index, *keys_out;  // [n] each, or null
    uint32_t* count;             // [1], or null
    uint32_t* scratch;           // [sort_scratch_words(n)]
    uint32_t n, key_mode, n_mats, _pad;
    double lo[3], scale[3];      // the root box's lower corner and 512 / its extent, per axis (RAY and RECORD)
};
// key, four radix passes (hist, two scans, place) and the gather of q on `stream`
int launch_sort(const SortParams& q, void* stream);

// Arguments of the three kernels of wavefront.hip (rrt.h: rrt_frame_rays_device, rrt_mix_rays_device, rrt_mix_pixels_device).  A region of a frame as a batch of
// entries in one of two orders: order 0 (RRT_ORDER_ROWS), [h][w][4 sub-samples] over the region's pixels; order 1 (RRT_ORDER_TILES), the 4x4-pixel tiles of the FRAME
// that the region touches -- tiles_w per row from tile (tile_x0, tile_y0), row-major -- each [4][4][4 sub-samples].
// FrameRaysParams: what render_kernel forms a primary ray from (FrameParams: the size, the scales, the view basis) and the eye; a null output array is not written.
struct FrameRaysParams {
    uint32_t width, height;
    double x_scale, y_scale, z_value;       // engine.rs:189-191
    double right[3], up[3], forward[3], eye[3];
    uint32_t x0, y0, w, h;                  // the region, inside the frame
    uint32_t tile_x0, tile_y0, tiles_w, order;
    uint32_t n, _pad;                       // entries: 4 * w * h, or 64 * the tiles of the rectangle
    double *origins, *dirs, *max_t;         // [n][3], [n][3], [n]
};
// MixRaysParams: one level of the unwind over n entries; material, kr and reflected may be null.
struct MixRaysParams {
    const uint32_t* material; const double *local, *kr; const uint32_t* reflected;
    uint32_t* colour;
    uint32_t n, n_mats;
};
// MixPixelsParams: colours in the given order -> fb [h][w], the region's pixels.
struct MixPixelsParams {
    uint32_t width, height, x0, y0, w, h;
    uint32_t tile_x0, tile_y0, tiles_w, order;
    const uint32_t* colours; uint32_t* fb;
};
// kernel launches (wavefront.hip).  All return hipError_t cast to int; nothing is synchronised; n == 0 launches nothing.
int launch_frame_rays(const FrameRaysParams& q, void* stream);
int launch_mix_rays(const MixRaysParams& q, const uint32_t* d_bound, void* stream);   // (d_bound: as launch_compact's)
int launch_mix_pixels(const MixPixelsParams& q, void* stream);

// kernel launches (render.hip).  All return hipError_t cast to int; stream is a hipStream_t.
// walk: 0 = node-coherent walk with the lane filter, 1 = node-coherent walk with the bundle filter, 2 = ray walk (render.hip)
// d_cover: null, or the coverage mask of this WHOLE single-GPU frame (coverage.hip: launch_coverage on the same stream): a wave whose bit is clear stores WHITE
// and walks nothing.  Not an argument inside FrameParams or DevScene: those are arguments of the other kernels too.
int launch_render(const DevScene& s, const FrameParams& f, uint32_t* d_out, void* stream, int walk, const uint32_t* d_cover = nullptr);
// The coverage pass (coverage.hip; the rule: coverage_rule.hpp).  The mask of a frame of tiles_x x tiles_y tiles is coverage_mask_words words, one bit per wave
// in render_kernel's block order, and one more word behind them.  launch_coverage clears it and marks the waves that boxes[0, n_boxes) can reach, on `stream`.
struct CoverageFrame;
uint32_t coverage_mask_words(uint32_t tiles_x, uint32_t tiles_y);
int launch_coverage(const CoverageFrame& F, const DevClusterBox* boxes, uint32_t n_boxes, uint32_t root_end, uint32_t* mask, void* stream);
// One stage launch (render.hip: launch_stage), for Params = any of the ten arguments above: one block per quadrant of the tiles the region touches, or four
// blocks per entry of a list's n, the frame kernels' quadrants; no tile, or n == 0, launches nothing.  Defined and instantiated for the ten in render.hip.
// kMaxTileList: HIP refuses a launch of more than 2^32 - 1 threads in a grid dimension, and an entry takes 4 blocks of 64.
constexpr uint32_t kMaxTileList = 0xFFFFFFFFu / 256u;
template <class Params> int launch_stage(const DevScene& s, const Params& q, void* stream, int walk);
int launch_detile(uint32_t width, uint32_t height, uint32_t world, const uint32_t* d_gathered, uint32_t* d_fb, void* stream);
// The seven per-ray launchers (render.hip: each is launch_per_ray with its kernel): one lane per ray, 64 rays per block; n == 0 launches nothing.
// d_count: null, or the bound of a counted launch (rrt.h: COUNTED DEVICE FORMS) -- one uint32 in device memory, read by the kernel when it runs; the grid is that of n.
int launch_ray_colours(const DevScene& s, uint32_t n, const double* d_origins, const double* d_dirs, uint32_t* d_colours, const uint32_t* d_count, void* stream, int walk);
int launch_intersect(const DevScene& s, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t,
                     uint8_t* d_hit, double* d_t, double* d_u, double* d_v, uint32_t* d_tri, const uint32_t* d_count, void* stream, int walk);
// (any of the five outputs of launch_intersect may be null: that array is not written)
// Some/None of the same walk as a shadow query (render.hip: occlusion_kernel): d_occluded[n] = 1 / 0
int launch_occlusion(const DevScene& s, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, uint8_t* d_occluded, const uint32_t* d_count, void* stream, int walk);
// The full surface record of every ray's first hit and the reference's next ray (render.hip: surface_rays_kernel); any array of q may be null, not all
int launch_surface_rays(const DevScene& s, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, const RaySurfaceParams& q, const uint32_t* d_count, void* stream, int walk);
// The colour, the unquantised local colour and the kr of every ray from its kept record (render.hip: shade_rays_kernel); any output of q may be null, not all
int launch_shade_rays(const DevScene& s, uint32_t n, const ShadeRaysParams& q, const uint32_t* d_count, void* stream, int walk);
// The occlusion mask and the count of open rays of every record's hemisphere fan (render.hip: ambient_rays_kernel); either output of q may be null, not both
int launch_ambient_rays(const DevScene& s, uint32_t n, const AmbientRaysParams& q, const uint32_t* d_count, void* stream, int walk);
// The surface record of every kept hit, with no primary walk (render.hip: resolve_hits_kernel); any output of q may be null, not all.  With q.lights the shadow
// walks run in `walk`; without it the one walk-free instantiation runs, whatever `walk` is, with no dynamic LDS.
int launch_resolve_hits(const DevScene& s, uint32_t n, const ResolveParams& q, const uint32_t* d_count, void* stream, int walk);
// Exactness guard for a new eye (scene_build.hip: k_suspects_resident): searches the resident list slots geom[0, n_list_slots) and appends up to
// RRT_MAX_SUSPECTS + 1 records {push index, suspect} to d_out, counting every find in *d_count (zeroed here, on `stream`).  Not synchronised.
struct SuspectRecord { uint32_t tri; uint32_t _pad; DevSuspect s; };
int launch_suspects_resident(const DevTriGeom* geom, const DevTriAttr* attr, uint32_t n_list_slots, const double eye[3], double pad,
                             uint32_t* d_count, SuspectRecord* d_out, void* stream);
uint32_t stack_bytes_per_wave(uint32_t levels);
void preload_kernels();

}  // namespace rrt
