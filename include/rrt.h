/*
 * rrt.h -- C ABI of the MI355X-native per-pixel hot path of conor722/rust-ray-tracer.
 *
 * The reference has no FFI; its natural seam is `Scene::draw_scene(&mut self, rt: RayTracer)`
 * (src/scene/engine.rs:186) called from `main` (src/main.rs:68-74), one level above
 * `RayTracer::get_ray_colour` (src/scene/raytracer.rs:29).  This header is what a Rust
 * `extern "C"` block for that seam binds (see INTEGRATION.md for the binding a maintainer adds).
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returns RRT_OK (0) or a
 * negative rrt_status; nothing aborts or unwinds across the boundary (the reference panics instead:
 * main.rs:24,28; utils.rs:61,85,170,184,193,222,275,347-349).  All input pointers are borrowed for the
 * duration of the call only; the library copies what it keeps.  One caller thread per handle.
 * Host-side set-up work (parsing, texture decode, staging copies) runs on a process-wide pool of worker threads that the library creates on demand and keeps
 * (RRT_HOST_THREADS caps a stage's share of it; with LOCAL_WORLD_SIZE / WORLD_SIZE set, the hardware threads are divided among the ranks of the node); the
 * workers live until the process ends, so the library must not be unloaded (dlclose) while the process runs.  Tracing itself uses no host threads; rrt_render into a pageable buffer copies the frame out of the staging ring on the pool.
 *
 * There is NO CPU fallback in this library: every compute entry point runs hand-written HIP kernels on
 * gfx950 and fails with RRT_ERR_NO_DEVICE / RRT_ERR_HIP when no GPU is usable.
 */
#ifndef RRT_H
#define RRT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RRT_OK = 0,
    RRT_ERR_INVALID_ARG = -1,
    RRT_ERR_HIP = -2,          /* a HIP runtime call failed; rrt_last_error_detail() has the text */
    RRT_ERR_OOM = -3,
    RRT_ERR_IO = -4,           /* "Could not read file" (main.rs:28, utils.rs:171, 346-347) */
    RRT_ERR_PARSE = -5,        /* any `expect`/`unwrap` failure of utils.rs (bad number, missing vertex, ...) */
    RRT_ERR_DEPTH = -6,        /* octree deeper than RRT_MAX_OCTREE_DEPTH (e.g. duplicate triangles, octree.rs:79-92) */
    RRT_ERR_NO_DEVICE = -7,
    RRT_ERR_UNSUPPORTED = -8   /* e.g. a texture format the build-owned decoder does not read */
} rrt_status;

#define RRT_MAX_OCTREE_DEPTH 40

/* == Vector3d, src/scene/engine.rs:9-14 */
typedef struct { double x, y, z; } rrt_vec3;

/* == Light, src/scene/entities.rs:5-9.  kind: 0 Ambient{intensity}; 1 Point{intensity, position=v};
 * 2 Directional{intensity, direction=v} */
typedef struct { uint32_t kind; uint32_t _pad; double intensity; rrt_vec3 v; } rrt_light;

/* == Material, src/scene/material.rs:11-22 (name dropped).  tex/bump index rrt textures; bump = -1 => None */
typedef struct { rrt_vec3 ka, kd, ks; double ns, kr; int32_t tex, bump; } rrt_material;

/* == Texture, src/scene/entities.rs:86-91: RGB8, row-major, index = width*y + x (raytracer.rs:55) */
typedef struct { const uint8_t *rgb; uint32_t width, height; } rrt_texture;

/* RRT_FLAG_NO_CULL: walk every node's triangle list in full, in list order, exactly as ray.rs:119-129 does (no cluster boxes).
 * Default (0): the lists are indexed by padded cluster boxes that skip triangles a ray cannot reach.  Results are identical for every ray that does
 * not lie IN a triangle's plane to within rounding noise (where the reference's own Moller-Trumbore answer is noise): DESIGN.md section 4 gives the
 * bound.  Rays from the raytracer's origin -- every primary ray -- are guarded against that case too (rrt_stats.origin_plane_triangles); secondary
 * rays are not.  Tests compare the two modes bit for bit on every config and on 10^6 constructed near-coplanar rays. */
#define RRT_FLAG_NO_CULL 1u
/* The index boxes are tested either by every ray against one box at a time (LANE filter) or by 64 boxes at a time against the wave's ray
 * bundle (BUNDLE filter; faster on coherent rays, slower on scattered ones).  Both give the same pixels.  By default the FIRST frame of a frame
 * size runs the variant a measured rule picks -- bundle filter above ~1200 primary rays per triangle of the scene, lane filter below
 * (profiles/r03_variant_sweep.json: right on 17 of 18 scene x size points, 5 % off on the other) -- so a host that renders one frame per run, as the
 * reference does, pays nothing for the choice; a SECOND frame of the same size is first rendered with every variant (a one-off stream
 * synchronisation), the fastest being kept for that size; these flags force one. */
#define RRT_FLAG_LANE_FILTER 2u
#define RRT_FLAG_BUNDLE_FILTER 4u
/* Both of the above walk the octree node-coherently (one node per wave step, records in scalar registers): right for rays that share nodes.
 * RAY_WALK lets every ray of a wave visit its own node in every step (records through vector memory): right for scattered rays (large soups,
 * mirror bounces).  Same pixels again; the default measures all three on the second frame of a size. */
#define RRT_FLAG_RAY_WALK 8u
/* Set-up.  By default rrt_raytracer_create builds everything the kernels read ON THE GPU from the uploaded triangle array: the octree exactly as
 * Octree::push_triangle builds it one triangle at a time (octree.rs:41-241; level-parallel and order-exact, csrc/scene_build.hip), this build's index
 * over the own lists, and the device records.  HOST_SETUP does the same on the host's cores (csrc/octree.cpp, clusters.cpp) and uploads the result:
 * the two paths produce the same bytes in HBM (tests/test_gpu_build.py); the flag exists for that check and for A/B timing. */
#define RRT_FLAG_HOST_SETUP 16u
/* Chain shortcut: below a parent, a run of internal nodes with one non-empty child each and at most four own triangles
 * in all is skipped by the rays that certainly cross the box of the run's end and miss the boxes of those triangles; the bundle-filter walk
 * then enters the end directly.  Same results; this flag turns the shortcut off (tests, A/B timing). */
#define RRT_FLAG_NO_CHAIN_SHORTCUT (1u << 5)   /* 32; a developer switch, not one of the five flags above that tests/test_abi.py pins as the Python mirror's set */
/* Specular skip: a specular term that the f64 sum of a hit's lighting certainly absorbs -- I + term == I bit for bit, decided
 * from an fp32 upper bound (csrc/specular_skip.hpp) -- is not evaluated: no pow, no sqrt, no divide.  Same results; this flag evaluates every term
 * (tests, A/B timing). */
#define RRT_FLAG_NO_SPECULAR_SKIP (1u << 6)    /* 64; a developer switch like the one above */
/* Coverage pass: in front of every WHOLE frame of one GPU (rrt_render_device, rrt_render) a small kernel projects the padded box of
 * every triangle onto the frame and marks the 4x4-pixel waves it can reach; a wave no box reaches stores WHITE and walks nothing.  The pass runs again in
 * every frame, from the camera and scene in force at the call: nothing is kept between frames, so the setters need no care.  Where it runs is scheduling
 * alone.  If the frame's stream still has work when the frame is enqueued (a host that enqueues frames without waiting for each), the pass runs on a side
 * stream of the raytracer -- non-blocking, of the device's highest priority -- beside that work, and the frame's kernel waits for it behind an event: stream
 * order as the caller sees it is unchanged, the frame is complete when its stream says so.  If the stream is idle (a first frame, rrt_render), the pass goes
 * in front of the frame's kernel on that stream.  rrt_stats.kernel_ms covers what the frame's stream was held for: the wait for the mask -- the whole pass
 * on an idle stream, next to nothing in a sequence -- plus the kernel.  Same results; the pass is off by itself wherever the index's exactness guarantee is
 * not in force for every primary ray (rrt_raytracer_get_coverage_info says why), and for a rank's tiles and progressive frames.  This flag turns it off
 * (tests, A/B timing). */
#define RRT_FLAG_NO_COVERAGE (1u << 7)         /* 128; a developer switch like the two above */
#define RRT_FLAG_COVERAGE_ALWAYS (1u << 8)     /* 256; a developer switch: the pass also runs where it is judged not to pay (RRT_COVERAGE_OFF_SMALL_FRAME); tests and timing at small sizes */
/* Wide boxes: the pass also lists the up to 16 boxes of the octree root's own triangles that cover at least 1/128 of the frame (and 16
 * waves) -- a floor, a table, a mirror.  A wave that only listed boxes reach does not walk its primary rays: it tests them against those few triangles
 * directly, which is what the walk would return (in the bundle-filter kernel; the lane-filter and ray-walk kernels are built without the short way and walk).
 * Same results; read at creation.  With this flag the pass lists nothing and every covered wave walks
 * (tests, A/B timing).  rrt_raytracer_get_wide_cover_info counts. */
#define RRT_FLAG_NO_WIDE_COVER (1u << 9)       /* 512; a developer switch like RRT_FLAG_NO_COVERAGE */

/* Render constants that the reference hard-codes; NULL => these defaults. */
typedef struct {
    double surface_offset;            /* 1e-4, raytracer.rs:17 */
    uint32_t max_reflection_depth;    /* 5,    raytracer.rs:20 (<= 8 supported) */
    uint32_t flags;                   /* 0, or RRT_FLAG_* */
    double vp_w, vp_h, vp_d;          /* 1,1,1 Viewport::default, engine.rs:113-119 */
} rrt_options;

typedef struct {
    uint32_t n_tris, n_tris_in_tree;  /* triangles outside the root AABB are silently dropped, octree.rs:71-73 */
    uint32_t n_nodes, max_depth;      /* max_depth counts the root as 1 */
    uint32_t n_mats, n_tex;
    uint32_t root_own_count, max_own_count;
} rrt_model_info;

typedef struct {
    double   kernel_ms;               /* HIP-event time of the last render's trace kernel on its stream; for a whole frame with a coverage pass: the time the
                                         frame held that stream -- any wait for the mask, then the kernel (see RRT_FLAG_NO_COVERAGE) */
    uint32_t width, height;
    uint64_t rays_primary;            /* 4 * pixels actually traced */
    uint64_t scene_bytes;             /* bytes resident in HBM for this raytracer (geometry+octree+textures) */
    uint32_t filter_variant;          /* 0 = LANE filter, 1 = BUNDLE filter, 2 = RAY walk (forced, or measured on the first frame of this size) */
    uint32_t origin_plane_triangles;  /* triangles whose plane contains the raytracer's origin (the current eye, rrt_raytracer_set_camera) to rounding distance: rays from it that lie
                                       * in such a plane run with the index filters off (exactness guard); 0 for ordinary scenes */
    /* The index's exactness band.  filter_pad = absolute padding of every index box (2^-15 of the scene magnitude).  A (ray,
     * triangle) pair can only be treated differently from the reference-order walk if the ray's direction is within alpha of the triangle's plane AND
     * its origin within delta of it, alpha = filter_alpha_unit * R / sin(phi), delta = filter_delta_unit * R^2 / sin(phi)^2 (leading term), with
     * R = |origin - v1| + the longer edge in units of the scene magnitude and phi the angle between the edges: the `unit` values are those of a
     * right-angled triangle at the scene's magnitude (about 2e-9 and 1e-7 of it).  profiles/r03_band_counts.json: no pair of the five BASELINE frames
     * that the reference accepts lies inside the band. */
    double filter_pad, filter_alpha_unit, filter_delta_unit;
} rrt_stats;

/* ------------------------------------------------------------------ model = SceneData (scenedata.rs:5-13), host side */
typedef struct rrt_model rrt_model;

/* parse_obj_file_lines (utils.rs:139-213) on the file at obj_path (read as main.rs:28); "mtllib"/texture names
 * resolve relative to the .obj's directory (the reference resolves against the cwd; it is run from its root).
 * root = {min_x,max_x,min_y,max_y,min_z,max_z}, NULL => Octree::new(-20,20,-20,20,-20,20) (utils.rs:145).
 * The reference pushes every triangle into the octree as it parses (utils.rs:192-198).  Here the tree is built from the finished triangle list, in
 * the same order, WHERE IT IS NEEDED: on the GPU by rrt_raytracer_create, or on the host the first time rrt_model_get_info / rrt_model_get_octree
 * (or a RRT_FLAG_HOST_SETUP raytracer) asks for it.  RRT_ERR_DEPTH is therefore reported by those calls, not by the two loaders. */
int rrt_model_load_obj(const char *obj_path, const double *root, rrt_model **out);

/* For a host that already parsed the scene (the Rust host holds SceneData.triangles in push order):
 * pos/uv/nrm are [n][3][3] doubles (v1,v2,v3; uv z ignored), mat[n] indexes mats.  Textures are copied. */
int rrt_model_from_arrays(uint32_t n_tris, const double *pos, const double *uv, const double *nrm, const uint32_t *mat,
                          uint32_t n_mats, const rrt_material *mats, uint32_t n_tex, const rrt_texture *tex,
                          const double *root, rrt_model **out);
void rrt_model_destroy(rrt_model *m);

int rrt_model_get_info(const rrt_model *m, rrt_model_info *out);
int rrt_model_get_triangles(const rrt_model *m, double *pos, double *uv, double *nrm, uint32_t *mat);   /* any may be NULL */
int rrt_model_get_materials(const rrt_model *m, rrt_material *out);
int rrt_model_get_texture(const rrt_model *m, uint32_t index, rrt_texture *out);                        /* borrowed view */
/* The octree exactly as octree.rs:41-241 builds it, flattened: aabb[n_nodes][6] = min xyz,max xyz;
 * first_child (0 = leaf, else 8 consecutive ids, octree.rs:226-238); tri_count (octree.rs:75);
 * own_off[n_nodes+1], own_idx[] = each node's `triangles` Vec in insertion order. */
int rrt_model_get_octree(const rrt_model *m, double *aabb, uint32_t *first_child, uint32_t *tri_count,
                         uint32_t *own_off, uint32_t *own_idx);

/* Build-owned JPEG / PNG decode to RGB8 (stands where `image::ImageReader::open().decode()` does, utils.rs:345-368).  JPEG: 8-bit Huffman,
 * sequential or progressive, 4:4:4 / 4:2:2 / 4:2:0, any number of scans, restart markers -- bit-equal to libjpeg (islow IDCT, fancy upsampling);
 * PNG: 8-bit RGB or palette of 1-8 bits, Adam7-interlaced or not; BMP: uncompressed 24-bit or palette; TGA (by file name): 24-bit, plain or run-length coded.
 * Anything else, and anything that does not decode to 3 bytes per pixel (greyscale, alpha -- the reference walks
 * `as_bytes().chunks(3)` whatever the colour type), is RRT_ERR_UNSUPPORTED.  *rgb is malloc'd; free with rrt_free. */
int rrt_decode_image_file(const char *path, uint8_t **rgb, uint32_t *width, uint32_t *height);
void rrt_free(void *p);

/* ------------------------------------------------------------------ raytracer = RayTracer{scene_data,lights,origin} (raytracer.rs:22-26) on one GPU */
typedef struct rrt_raytracer rrt_raytracer;

/* Uploads the scene once to HBM of HIP device `device`.  opt may be NULL. */
int rrt_raytracer_create(const rrt_model *m, const rrt_light *lights, uint32_t n_lights, rrt_vec3 origin,
                         const rrt_options *opt, int device, rrt_raytracer **out);
/* The same raytracer straight from the host's own arrays (arguments as rrt_model_from_arrays, then as rrt_raytracer_create): what a host that has
 * parsed the scene itself -- the Rust host holds SceneData.triangles -- calls when it needs no rrt_model.  The arrays are uploaded from where they lie
 * and packed into triangle records on the device; the library keeps no host copy of the scene.  Same scene in HBM, same frames; the loaders' copy
 * (15 ms of a million triangles' 54 ms first frame) is not made.  RRT_FLAG_HOST_SETUP is refused here (RRT_ERR_UNSUPPORTED). */
int rrt_raytracer_create_from_arrays(uint32_t n_tris, const double *pos, const double *uv, const double *nrm, const uint32_t *mat,
                                     uint32_t n_mats, const rrt_material *mats, uint32_t n_tex, const rrt_texture *tex, const double *root,
                                     const rrt_light *lights, uint32_t n_lights, rrt_vec3 origin, const rrt_options *opt, int device,
                                     rrt_raytracer **out);
void rrt_raytracer_destroy(rrt_raytracer *rt);

/* Camera.  The reference looks from RayTracer.origin down +z with y up (main.rs:59-67, engine.rs:207-211); here eye and view basis can be set between frames.
 * eye = RayTracer.origin; the sub-sample ray through scene point (a, b, c) = (xd*x_scale, yd*y_scale, z_value) of engine.rs:207-236 has direction
 * right*a + up*b + forward*c, per component k:  d.k = (right.k*a + up.k*b) + forward.k*c  -- five f64 operations, each rounded on its own.  The library
 * neither normalises nor orthogonalises the basis (the reference's directions are not unit vectors either): a scaled, sheared or mirrored basis is the
 * caller's business.  Creation pose: eye = origin, right/up/forward = (1,0,0) (0,1,0) (0,0,1): exactly the reference's directions. */
typedef struct { rrt_vec3 eye, right, up, forward; } rrt_camera;          /* 96 bytes */
/* Applies to every frame-shaped launch made after it returns (rrt_render, rrt_render_device, rrt_render_tiles_device, rrt_render_progressive, the visibility calls and the
 * rrt_multi_* calls through the raytracers they hold: set the camera on each of them, or on each rank, between rrt_multi_sync and the next enqueue).  The
 * per-ray entry points keep taking the caller's own rays; their exactness guard is keyed to the current eye.  cam == NULL: back to the creation pose.
 * RRT_ERR_INVALID_ARG for a NULL rt or a non-finite component (the pose in force stays).
 * BLOCKING, and it must not overlap launches of this raytracer that are still in flight: frames enqueued with rrt_render_device, rrt_render_tiles_device,
 * rrt_render_visibility_device or rrt_multi_enqueue, and ray batches enqueued with rrt_intersect_rays_device, rrt_get_ray_colours_device or
 * rrt_occluded_rays_device (their exactness guard reads the suspect list of the current eye), must have been synchronised by the caller first (rrt_render,
 * rrt_render_progressive, rrt_render_visibility, rrt_pick and the host forms of the per-ray calls return with nothing in flight).
 * A new eye costs one pass over the resident triangles on the GPU and one read-back: the exactness guard (rrt_stats.origin_plane_triangles, RRT_BUF_SUSPECTS)
 * is recomputed for it, with the list a fresh rrt_raytracer_create at that origin would produce; a RRT_FLAG_NO_CULL raytracer has no guard and only stores
 * the pose.  An eye bit-equal to the current one costs no GPU work and no synchronisation: a pure rotation is free.
 * The traversal variant measured for a frame size (RRT_FLAG_LANE_FILTER above) is NOT measured again after a camera change. */
int rrt_raytracer_set_camera(rrt_raytracer *rt, const rrt_camera *cam);
int rrt_raytracer_get_camera(const rrt_raytracer *rt, rrt_camera *out);
/* Host only, no GPU.  Left-handed like the reference (x right, y up, z forward): forward = normalised(target - eye), right = normalised(cross(up_hint,
 * forward)), up = cross(forward, right).  RRT_ERR_INVALID_ARG when target == eye, when up_hint is parallel to the view direction (or zero), or when any
 * component is non-finite. */
int rrt_camera_look_at(rrt_vec3 eye, rrt_vec3 target, rrt_vec3 up_hint, rrt_camera *out);

/* Scene updates: the lights, the material table and the triangles of a living raytracer, between frames.  Textures, options, flags and the camera pose stay as
 * they are, resident; nothing is uploaded or allocated again that does not depend on what changed.  All the calls follow the contract of
 * rrt_raytracer_set_camera: every launch made after the call returns sees the change (frames, tiles, progressive frames, the visibility calls, the per-ray
 * calls in host and device form, and the rrt_multi_* calls through the raytracers they hold: set it on each of them, or on each rank, between
 * rrt_multi_sync and the next enqueue), and the call must not overlap launches of this raytracer that are still in flight.
 *
 * rrt_raytracer_set_lights: host work only, no GPU call and no synchronisation (the lights travel with the kernel arguments).  The checks of creation
 * apply -- n_lights > 16, a kind > 2 or a NULL list with n_lights > 0 is RRT_ERR_INVALID_ARG and the list in force stays; n_lights == 0 is valid.  Order
 * is kept: the reference's light loop (raytracer.rs) breaks out on its conditions, so order changes pixels.  Works on a RRT_FLAG_HOST_SETUP raytracer too.
 * rrt_raytracer_get_lights: the list in force; out may be NULL to ask for the count only, capacity < count with a non-NULL out is RRT_ERR_INVALID_ARG. */
int rrt_raytracer_set_lights(rrt_raytracer *rt, const rrt_light *lights, uint32_t n_lights);
int rrt_raytracer_get_lights(const rrt_raytracer *rt, rrt_light *out, uint32_t capacity, uint32_t *n_lights);
/* rrt_raytracer_set_materials: a new material table over the resident one, as rrt_raytracer_set_camera BLOCKING, applied to every launch made after it returns
 * and not to overlap launches in flight.  One small host-to-device copy into the table at its resident address: no texture is uploaded, nothing is rebuilt, the
 * traversal variants measured so far stay.  ALL OR NOTHING, RRT_ERR_INVALID_ARG with the table in force untouched for: n_mats different from the resident count
 * (the triangles index the table), a NULL list with n_mats > 0, `tex` outside [0, n_tex), `bump` outside [-1, n_tex), and -- the check of creation -- a bump map
 * too small for the texel indices of the colour texture that address it (raytracer.rs:127-128).  Works on a RRT_FLAG_HOST_SETUP raytracer too.  Afterwards the
 * raytracer is, frame for frame and plane for plane, the one rrt_raytracer_create_from_arrays makes from the same arrays with the new table; what kept surface
 * planes are worth after an edit is tabulated under rrt_shade_surface below.
 * rrt_raytracer_get_materials: the table in force; out may be NULL to ask for the count only, capacity < count with a non-NULL out is RRT_ERR_INVALID_ARG. */
int rrt_raytracer_set_materials(rrt_raytracer *rt, const rrt_material *mats, uint32_t n_mats);
int rrt_raytracer_get_materials(const rrt_raytracer *rt, rrt_material *out, uint32_t capacity, uint32_t *n_mats);
/* rrt_raytracer_set_triangles: new triangles, arrays as rrt_raytracer_create_from_arrays (mat[i] indexes the RESIDENT material table and is checked against
 * it).  BLOCKING.  Afterwards the raytracer is what rrt_raytracer_create_from_arrays would have made from these arrays with this raytracer's materials,
 * textures, options and flags, the lights and the camera pose in force: every RRT_BUF_* buffer, rrt_raytracer_get_octree, rrt_raytracer_get_chain_info,
 * rrt_stats.scene_bytes, every frame and every ray query; rrt_stats.origin_plane_triangles and RRT_BUF_SUSPECTS are those of the CURRENT eye, and
 * rrt_raytracer_set_camera(NULL) still returns to the creation pose.  n_tris may differ from before and may be 0.  root as there, except that NULL means the
 * root box in force.  Octree, index and records are built on the GPU by the kernels of creation (rrt_get_setup_times then reports octree_ms, index_ms and
 * upload_ms of the latest build; create_ms and hip_init_ms stay).  What the raytracer measured on the old scene is forgotten -- the traversal variant kept for
 * a frame size with that size's frame count, and the variant kept for per-ray calls -- so the next frame of a size is a first frame again (the rule then sees
 * the new triangle count); a forced variant stays.
 * ALL OR NOTHING: on any failure -- RRT_ERR_INVALID_ARG (NULL array with n_tris > 0, material index out of range), RRT_ERR_DEPTH, RRT_ERR_OOM, a HIP error that
 * leaves the device usable -- the old scene stays in force, intact and renderable.  RRT_ERR_UNSUPPORTED for a RRT_FLAG_HOST_SETUP raytracer.
 * rrt_raytracer_set_triangles_device: the same from arrays in device memory of rt's device (positions computed there by a simulation or skinning step: no
 * PCIe transfer), borrowed for the call only.  The build waits on an event recorded on `stream` (hipStream_t, NULL = default), so the caller need not
 * synchronise the stream that writes the arrays; the call itself is still BLOCKING (the build reads counters back).  The material indices are counted
 * against the resident table by a kernel before anything is built: any out of range is RRT_ERR_INVALID_ARG.
 * MEMORY KEPT: from the first update on, the raytracer keeps the build's temporary device allocations and the scene allocation the update retired, and
 * the next update reuses each that is large enough (no hipMalloc, no hipFree -- which synchronises the device -- per update).  That is of the order of
 * 1.1 kB per triangle of the largest update so far (about 1 GB for a million triangles) plus one more copy of the scene.
 * rrt_raytracer_release_update_memory frees it (RRT_OK for any valid handle; the next update allocates again); creation itself keeps nothing. */
int rrt_raytracer_set_triangles(rrt_raytracer *rt, uint32_t n_tris, const double *pos, const double *uv, const double *nrm,
                                const uint32_t *mat, const double *root);
int rrt_raytracer_set_triangles_device(rrt_raytracer *rt, uint32_t n_tris, const double *d_pos, const double *d_uv, const double *d_nrm,
                                       const uint32_t *d_mat, const double *root, void *stream);
int rrt_raytracer_release_update_memory(rrt_raytracer *rt);

/* Scene::draw_scene (engine.rs:186-255) + Canvas::put_pixel (engine.rs:146-158): fills out_fb[width*height]
 * (host memory), 0x00RRGGBB (entities.rs:32-36), row 0 = top; pixels the reference never writes (row 0, and for
 * odd sizes row 1 / the last column) are 0 as in Canvas::new (engine.rs:135).  Blocking. */
int rrt_render(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t *out_fb);

/* Optional: page-lock a caller-owned framebuffer (the Rust host's Canvas.buffer: Vec<u32>, engine.rs:127) so that rrt_render copies the
 * frame into it with one asynchronous DMA.  Without it rrt_render stages through pinned memory of its own plus one host copy
 * (pipelined in row chunks).  Unregister before the buffer is freed or reallocated. */
int rrt_host_buffer_register(void *ptr, size_t bytes);
int rrt_host_buffer_unregister(void *ptr);

/* Same, framebuffer in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default), not synchronised. */
int rrt_render_device(rrt_raytracer *rt, uint32_t width, uint32_t height, void *d_fb, void *stream);

/* Visibility buffers: the first-hit geometry of a frame's primary rays, which the frame kernels compute on the way to a colour and do not keep.  For
 * picking, selection and snapping (what is under this pixel), depth compositing, edge detection on triangle ids, a denoiser's albedo.
 * The ray of canvas pixel (px, py), sub-sample s is exactly the one a frame traces for it in the current pose (rrt_camera above; the vp_* options apply).
 * Per ray:  hit, t, u, v, tri = what rrt_intersect_rays returns for that origin and direction with max_t = NULL, its miss convention included (hit 0,
 * t = u = v = 0.0, tri = 0xFFFFFFFF);  albedo = the colour-texture texel the reference samples at the hit (raytracer.rs:43-55), 0x00RRGGBB, before lighting
 * and without the bump map; a miss gives 0x00FFFFFF, the reference's background.  Pixels the reference never traces (canvas row 0, row 1 for odd heights,
 * the last column for odd widths) are written as hit 0, t = u = v = 0.0, tri = 0xFFFFFFFF, albedo 0: every element of every requested plane inside the
 * region is written, the caller need not clear anything.
 * One launch of one walk per ray, in the traversal variant a flag forces, else the one kept for this frame size, else the first-frame rule's choice for it
 * (RRT_FLAG_LANE_FILTER above).  These calls do not count as frames of that size: they never trigger the measurement and leave the kept variant alone.
 * rrt_last_stats afterwards: kernel_ms and filter_variant of this launch, width / height = the frame size, rays_primary = 4 * the traced pixels inside the region.
 * RRT_ERR_INVALID_ARG, before any GPU work: NULL rt or planes struct, all six plane pointers NULL, a bad frame size, a region with w == 0 or h == 0 or one
 * that sticks out of the frame; rrt_pick: px >= width, py >= height or out == NULL.
 * Not covered: the rank/world tile partition, the rrt_multi_* path and the progressive path.  A multi-GPU host splits the frame with regions. */
/* A rectangle of canvas pixels: columns [x0, x0+w), rows [y0, y0+h), row 0 = top.  NULL where a region is taken = the whole frame. */
typedef struct { uint32_t x0, y0, w, h; } rrt_region;                       /* 16 bytes */
/* Output planes of a visibility frame, each [region.h][region.w][4], row-major.  The last index is the sub-sample in the order of
 * engine.rs:207-236: (x,y), (x+.5,y), (x,y+.5), (x+.5,y+.5).  Any pointer may be NULL (that plane is not written), but at least one is set. */
typedef struct { uint8_t *hit; double *t, *u, *v; uint32_t *tri; uint32_t *albedo; } rrt_visibility;   /* 48 bytes */
/* Planes in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default), not synchronised. */
int rrt_render_visibility_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                                 const rrt_visibility *d_planes, void *stream);
/* Planes in host memory; blocking.  Only the requested planes are downloaded (from one device allocation kept between calls). */
int rrt_render_visibility(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                          const rrt_visibility *planes);
typedef struct { uint32_t hit, tri; double t, u, v; uint32_t albedo, _pad; } rrt_pick_result;           /* 40 bytes */
/* Sub-sample 0 of canvas pixel (px, py) of a width x height frame in the current pose: one tile's launch.  Blocking. */
int rrt_pick(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t px, uint32_t py, rrt_pick_result *out);

/* Surface buffers: what the reference holds at the first hit of a frame's primary rays on its way to a colour, and does not keep -- the hit point, the shading
 * normal, the material and which lights reach the point.  With the albedo plane above this is what a host needs to shade deferred, to relight a still camera
 * without walking the primaries again, to feed a denoiser its normal and albedo, to bake a moved light's shadow mask, and to form its own shadow, reflection or
 * ambient-occlusion rays on the GPU for the device-resident batch calls below (hemisphere rays of a fixed table in one launch: rrt_ambient_surface below).
 * The ray of canvas pixel (px, py), sub-sample s is the one rrt_render_visibility* defines: the primary ray a frame traces for it in the current pose.
 * Per ray with a hit:
 *   point    = origin + direction * t (raytracer.rs:39), t as in the visibility plane;
 *   normal   = the value get_normal_at_intersection returns (raytracer.rs:114-162): the barycentric interpolation, the bump map where the material has one --
 *              read at the colour texture's texel indices with the bump texture's width, through the tangent frame built from the normal -- and the final
 *              normalisation: the n that the reference's shading uses for the primary segment;
 *   material = the index of the hit triangle's material in the material table (rrt_material order);
 *   lights   = a bit mask over the light list in force, bit k for light k (k < n_lights <= 16): 1 for an Ambient or Directional light; for a Point light 1
 *              when the reference's shadow query triangle_exists_between_points (raytracer.rs:164-188) from this hit reports "lit" and 0 when it reports
 *              occluded -- origin = point + normal * surface_offset, direction = light - point, max_t = |direction|: the negation of rrt_occluded_rays for
 *              that ray.  Bits >= n_lights are 0.  EVERY point light is tested, also those behind the `break` with which the reference's light loop ends at
 *              the first occluded point light (raytracer.rs:235-237): the lights that loop adds up are [0, ctz(~mask)).
 * A miss inside the traced area: point = normal = (0.0, 0.0, 0.0), material = 0xFFFFFFFF, lights = 0.  Pixels the reference never traces (canvas row 0, row 1
 * for odd heights, the last column for odd widths) are written the same way: every element of every requested plane inside the region is written.
 * vis / d_vis non-NULL: its non-NULL planes are written by the same launch, byte for byte as rrt_render_visibility* writes them for that region -- one launch
 * then yields everything a deferred shader needs.  All six of its pointers may be NULL.
 * `lights` NULL: no shadow ray is walked, the launch costs one walk per ray and the shading arithmetic of the hit.
 * Traversal variant, tuning state and rrt_last_stats as the visibility calls: the forced variant, else the one kept for this frame size, else the first-frame
 * rule's; the call never triggers or alters a measurement; kernel_ms and filter_variant of this launch, width / height = the frame size, rays_primary = 4 * the
 * traced pixels inside the region (shadow rays are not counted).
 * Exactness: the shadow walks are the frame kernels' shadow walks -- default mode, not guarded, the band documented under RRT_FLAG_NO_CULL -- so the mask is the
 * one a frame uses.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer as it was: NULL rt, NULL planes struct, all four surface pointers NULL, a bad frame size, a
 * region with w == 0 or h == 0 or one that sticks out of the frame.
 * rrt_raytracer_set_camera, rrt_raytracer_set_lights and rrt_raytracer_set_triangles[_device] apply to every surface launch made after they return, and must
 * not overlap one that is still in flight (rrt_render_surface returns with nothing in flight; rrt_render_surface_device must be synchronised by the caller).
 * Not covered, as for the visibility calls: the rank/world tile partition, the rrt_multi_* path and the progressive path. */
/* Output planes of a surface frame.  point, normal: [region.h][region.w][4][3] doubles (x, y, z);  material, lights: [region.h][region.w][4] uint32.
 * Sub-sample order and region as rrt_visibility / rrt_region.  Any pointer may be NULL, at least one is set. */
typedef struct { double *point, *normal; uint32_t *material, *lights; } rrt_surface;      /* 32 bytes */
/* Planes in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default), not synchronised. */
int rrt_render_surface_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                              const rrt_visibility *d_vis /* may be NULL */, const rrt_surface *d_planes, void *stream);
/* Planes in host memory; blocking.  Only the requested planes are downloaded (from the device allocation the visibility calls keep). */
int rrt_render_surface(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                       const rrt_visibility *vis /* may be NULL */, const rrt_surface *planes);

/* Shading from kept buffers: finishes a frame from the planes rrt_render_surface* wrote for it, with the lights and materials in force NOW, without walking
 * a primary ray.  For relighting and material edits under a still camera: move a dimmer, turn the sun, edit a material, shade again.
 * vis / d_vis and planes / d_planes are the structs the caller gave rrt_render_surface[_device] for the same frame size and region, in that layout
 * ([region.h][region.w][4], point and normal x 3 doubles).  READ: vis->albedo, planes->point, planes->normal, planes->material -- all four required -- and
 * planes->lights, which may be NULL.  The other five visibility pointers are ignored.  WRITTEN: out_fb / d_fb, [region.h][region.w] pixels, 0x00RRGGBB: each
 * the reference's Color::mix (entities.rs:49-69) of its four sub-samples; pixels the reference never traces (canvas row 0, row 1 of an odd height, the last
 * column of an odd width) are 0; every pixel of the region is written.  With region == NULL the output is exactly the framebuffer of rrt_render_device.
 * Input and output must not overlap.
 * CONTRACT.  If the planes are the ones rrt_render_surface* wrote for this frame size, region, pose and scene, the output is the same region of the frame
 * rrt_render produces with the lights and materials in force now, bit for bit.  Keeping the planes valid is the caller's business:
 *
 *   change since the planes were written                                              planes that are stale
 *   rrt_raytracer_set_camera, rrt_raytracer_set_triangles[_device]                    all
 *   set_lights: position of a Point light, kind or index of any light, list length    `lights` only (pass it as NULL)
 *   set_lights: intensities, or the vector of an Ambient or Directional light         none
 *   set_materials: `tex` of a material                                                `albedo`, `normal` (the bump texel is read at the colour texture's indices)
 *   set_materials: `bump`                                                             `normal`
 *   set_materials: ka, kd, ks, ns, kr                                                 none
 *
 * Per sub-sample of a traced pixel: material >= n_mats (0xFFFFFFFF, a miss, included) gives 0x00FFFFFF, the reference's background (raytracer.rs:109-111) -- no
 * table is read out of bounds whatever the planes hold.  Otherwise the sub-sample is the primary segment's hit as the reference holds it after
 * get_normal_at_intersection: point, normal, material, colour = the low 24 bits of albedo; the segment's direction is recomputed from the pixel, the sub-sample
 * and the current pose by the five operations of rrt_camera.  With `lights`, the lights the depth-0 sum adds up are [0, min(ctz(~mask), n_lights)) and no depth-0
 * shadow ray is walked; with `lights` NULL the depth-0 shadow rays are formed and walked as a frame walks them, the `break` at the first occluded point light
 * (raytracer.rs:235-237) included.  From there on it is the reference's get_ray_colour: compute_lighting_intensity, the reflection chain up to
 * max_reflection_depth with its shadow rays always walked, the u8 quantisation at every level of the unwind.
 * Exactness: no primary ray is walked, so the primary segment's guard (rrt_stats.origin_plane_triangles) has nothing to do; every walk of this call is a
 * secondary walk of a frame -- default mode, not guarded, the band documented under RRT_FLAG_NO_CULL.
 * Cost: pixels none of whose neighbours in a 4x4 block hits a mirror, shaded with a mask, walk nothing at all.
 * Traversal variant, tuning state and rrt_last_stats as the surface calls: the forced variant, else the one kept for this frame size, else the first-frame rule's;
 * the call never triggers or alters a measurement; kernel_ms and filter_variant of this launch, width / height = the frame size, rays_primary = 4 * the traced
 * pixels inside the region.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer and the output as they were: NULL rt, either struct NULL, a required plane NULL, a NULL
 * output, a bad frame size, a region with w == 0 or h == 0 or one that sticks out of the frame.
 * rrt_shade_surface_device: planes and framebuffer in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default), not synchronised.
 * rrt_shade_surface: planes and framebuffer in host memory; blocking: the planes are uploaded into the device allocation the visibility calls keep, the region's
 * pixels downloaded, and nothing is in flight on return.
 * Not covered, as for the visibility calls: the rank/world tile partition, the rrt_multi_* path and the progressive path. */
int rrt_shade_surface_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                             const rrt_visibility *d_vis, const rrt_surface *d_planes, void *d_fb, void *stream);
int rrt_shade_surface(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                      const rrt_visibility *vis, const rrt_surface *planes, uint32_t *out_fb);

/* Ambient occlusion from kept buffers: which of n hemisphere rays from every first hit of a frame are blocked, from the planes rrt_render_surface* wrote for
 * it, in ONE launch that forms the rays in registers.  (The same rays through rrt_occluded_rays_device cost 56 bytes of device memory each, written and read
 * again: over 6 GB for a 1920 x 1080 frame with 16 samples.)  For an ambient term under a still camera, for baking, for a contact-shadow mask.
 * planes / d_planes is the struct the caller gave rrt_render_surface[_device] for the same frame size and region, in that layout.  READ: point, normal and
 * material, all three required; `lights` is ignored.
 * samples: n directions (sx, sy, sz) in the tangent frame of a hit -- sz along the normal -- and one max_t for all rays, as rrt_occluded_rays takes it (+inf is
 * valid).  The table lies in HOST memory in both forms, is borrowed for the call and travels in the kernel arguments, as the lights do.
 * Per sub-sample of a traced pixel: material >= n_mats (0xFFFFFFFF, a miss, included) is a miss -- the rule of rrt_shade_surface; no table is indexed with a
 * caller's value.  Otherwise, with point p and normal n exactly as stored, the tangent frame is the reference's (raytracer.rs:137-152):
 *   tg = cross(n, (0,1,0));  if length(tg) == 0: tg = cross(n, (0,0,1));  tg = tg / length(tg);  bt = normalised(cross(n, tg))
 * and the ray of sample k = (sx, sy, sz) is
 *   origin = p + n * surface_offset;   direction.c = (tg.c*sx + bt.c*sy) + n.c*sz  per component -- five f64 operations, each rounded on its own, the shape of
 *   rrt_camera;   max_t = samples->max_t.
 * occluded: bit k = what rrt_occluded_rays returns for exactly that ray, byte for byte; bits at and above n are 0.  A miss gives 0, and so does a pixel the
 * reference never traces (canvas row 0, row 1 of an odd height, the last column of an odd width).
 * grey, one value per pixel, in exact integer arithmetic: open = the sum over the four sub-samples of n for a miss and n - popcount(occluded) for a hit;
 * g = (510*open + 4*n) / (8*n), truncating -- 255 * open / (4n) rounded half up; the pixel is g * 0x010101.  A pixel the reference never traces is 0.
 * The rays are not rotated per pixel and the grey value is not cosine-weighted: the mask lets the host weight.
 * Every element of every requested plane inside the region is written.  Inputs and outputs must not overlap.
 * A non-finite point or normal in the caller's planes gives unspecified bits for that sub-sample, and no fault.
 * Exactness: no primary ray is walked; every walk of this call is a shadow walk of a frame -- default mode, not guarded, the band documented under
 * RRT_FLAG_NO_CULL -- as the shadow walks of rrt_render_surface and rrt_shade_surface are.
 * Keeping the planes valid is the caller's business; the table under rrt_shade_surface says when: point, normal and material go stale with camera and triangle
 * changes (and normal with the `tex` / `bump` edits listed there), never with a change of lights.
 * Traversal variant, tuning state and rrt_last_stats as the surface calls: the forced variant, else the one kept for this frame size, else the first-frame rule's;
 * the call never triggers or alters a measurement; kernel_ms and filter_variant of this launch, width / height = the frame size, rays_primary = 4 * the traced
 * pixels inside the region (the hemisphere rays are not counted).
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer and the outputs as they were: NULL rt, planes, samples or out; a NULL required plane; both
 * outputs NULL; n == 0 or n > RRT_MAX_AMBIENT_SAMPLES; NULL dirs; a non-finite direction component; max_t NaN or <= 0; a bad frame size; a region with w == 0 or
 * h == 0 or one that sticks out of the frame.
 * rrt_ambient_surface_device: planes and outputs in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy and
 * no synchronisation.
 * rrt_ambient_surface: planes and outputs in host memory; blocking: the three planes are uploaded into the device allocation the visibility calls keep, only the
 * requested outputs are downloaded, and nothing is in flight on return.
 * Not covered, as for the surface calls: the rank/world tile partition, the rrt_multi_* path and the progressive path. */
#define RRT_MAX_AMBIENT_SAMPLES 32
/* dirs: n x 3 doubles (sx, sy, sz) in the tangent frame of the hit, HOST memory in both forms, borrowed for the call.  max_t as rrt_occluded_rays takes it. */
typedef struct { const double *dirs; uint32_t n, _pad; double max_t; } rrt_ambient_samples;   /* 24 bytes */
/* occluded: [region.h][region.w][4] uint32;  grey: [region.h][region.w] uint32.  Either may be NULL, not both. */
typedef struct { uint32_t *occluded; uint32_t *grey; } rrt_ambient;                            /* 16 bytes */
int rrt_ambient_surface_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                               const rrt_surface *d_planes, const rrt_ambient_samples *samples,
                               const rrt_ambient *d_out, void *stream);
int rrt_ambient_surface(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                        const rrt_surface *planes, const rrt_ambient_samples *samples, const rrt_ambient *out);

/* The fused frame of a region: the COLOURS of a rectangle of the frame from the kernel body that renders whole frames -- primary walk, lights, reflection chain
 * and unwind in one launch, nothing kept in memory on the way.  For the rectangle under an edited object, a render border, one GPU's share of a frame.
 * (The same pixels through rrt_render_surface + rrt_shade_surface cost more than a frame and about 120 bytes of planes per sub-sample.)
 * OUTPUT.  Pixel (px, py) of the region in force -- the whole frame for region == NULL -- is written to out[(py - y0) * pitch + (px - x0)], 0x00RRGGBB.  pitch is
 * in elements; 0 means region.w, a tight [h][w] array.  With out = fb + y0 * width + x0 and pitch = width the region lands in place in a whole framebuffer.
 * Nothing outside the region's w elements of each row is read or written: not the gap up to pitch, not a row before or after.
 * VALUE.  Exactly the one rrt_render writes at [py][px] for the pose, lights, materials and triangles in force, bit for bit, in every traversal variant -- 0
 * included for the pixels the reference never traces (canvas row 0, row 1 of an odd height, the last column of an odd width).
 * Traversal variant, tuning state and rrt_last_stats as the visibility calls: the forced variant, else the one kept for this frame size, else the first-frame
 * rule's; the call is not a frame of that size: it never triggers or alters a measurement and leaves the coverage state of the last frame
 * (rrt_raytracer_get_coverage_info) as it was; kernel_ms and filter_variant of this launch, width / height = the frame size, rays_primary = 4 * the traced pixels
 * inside the region.  No coverage pass runs in front of it (its mask is indexed by the whole frame's waves): a region that is the whole frame walks the waves
 * a frame with RRT_FLAG_NO_COVERAGE walks.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer and the output as they were: NULL rt, NULL out, a bad frame size, a region with w == 0 or
 * h == 0 or one that sticks out of the frame, a pitch other than 0 that is smaller than the region's width.
 * rrt_render_region_device: d_out in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no synchronisation.
 * Regions of one frame that do not overlap may be in flight on several streams, or on several raytracers of the same scene, into one buffer.
 * rrt_render_region: out in host memory; blocking: the pixels go through the device allocation the visibility calls keep and arrive in the caller's rows, the
 * gap between rows untouched; nothing is in flight on return.
 * Not covered: a coverage pass, lists of rectangles, the rank/world tile partition, the rrt_multi_* path and the progressive path. */
int rrt_render_region_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                             uint32_t *d_out, uint32_t pitch, void *stream);
int rrt_render_region(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                      uint32_t *out, uint32_t pitch);

/* The fused frame of a list of 8x8-pixel tiles that lies in DEVICE memory: re-render the tiles a kernel of the caller's flagged (stale after a reprojection, not
 * yet converged), in the order of the caller's choosing, with no read-back and no synchronisation -- in the style of the COUNTED DEVICE FORMS below.
 * d_fb is a whole row-major [height][width] framebuffer.  d_tiles[j] is a tile index in the frame kernels' numbering: ty * tiles_x + tx with
 * tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8.  With m = min(n, *d_count) -- m = n for d_count == NULL -- every pixel of the tiles d_tiles[0..m)
 * that lies inside the frame is written as rrt_render writes it, bit for bit; every other pixel of d_fb is neither read nor written.  The kernel reads *d_count
 * when it runs, in stream order: a kernel enqueued before the call on the same stream may write it, and the list.
 * ENTRIES.  d_tiles[j] is used as an index only after d_tiles[j] < tiles_x * tiles_y; any other value, 0xFFFFFFFF included, is skipped.  Entries [m, n) are never
 * read.  Duplicates are allowed: both waves store the same bits.  The list and the bound are only ever read.
 * LAUNCH.  The grid is sized by n, four blocks of 64 threads per entry (the frame kernels' quadrants); a block at or beyond m ends after one scalar load and a
 * compare.  n == 0: RRT_OK, nothing is launched and rrt_last_stats stays as it was.  n > RRT_MAX_TILE_LIST: RRT_ERR_INVALID_ARG -- HIP launches at most
 * 2^32 - 1 threads in a grid dimension, and an entry takes 256.
 * ORDER.  The caller's order is the schedule: block 4 j + q renders quadrant q of entry j; nothing is reordered (no XCD-aware block order).
 * Traversal variant and tuning state as for a region.  rrt_last_stats: kernel_ms and filter_variant of this launch, width / height = the frame size,
 * rays_primary = 0 -- the library does not read the list.  No coverage pass.
 * RRT_ERR_INVALID_ARG, before any GPU work: NULL rt, a bad frame size, NULL d_fb, n > RRT_MAX_TILE_LIST, NULL d_tiles with n > 0.
 * There is no host form: a host that knows its tiles has regions.
 * PRODUCER.  rrt_select_tiles_device below writes such a list and its count from planes in device memory, on the same stream: d_tiles and d_count of this call
 * are its outputs, n its n_tiles; rrt_mark_tiles_device is its first half, for a caller that compacts the marks itself. */
#define RRT_MAX_TILE_LIST 16777215u   /* (2^32 - 1) / 256 */
int rrt_render_tile_list_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t *d_count,
                                const uint32_t *d_tiles, uint32_t *d_fb, void *stream);

/* Tile selection on the device: tests over planes of a frame that produce the list rrt_render_tile_list_device reads -- the tiles in which a kept plane shows
 * what an edit touches, the tiles in which two frames differ, the tiles that are not empty -- with no read-back and no synchronisation.
 * TILES.  Numbered as rrt_render_tile_list_device numbers them: ty * tiles_x + tx, tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8; n_tiles = tiles_x * tiles_y.
 * PLANES.  a (and b) hold [region.h][region.w][per_pixel] elements of elem_bytes, tight, for the region in force (NULL = the whole frame): per_pixel 1 is a
 * framebuffer, 4 a sub-sample plane of rrt_visibility / rrt_surface / rrt_ambient.  They are aligned to elem_bytes; no more is demanded.  The marks overlap no plane.
 * ELEMENTS.  An element is read as an UNSIGNED INTEGER of elem_bytes (1, 4 or 8); no floating-point comparison happens anywhere: -0.0 is not zero and differs
 * from 0.0, a NaN equals itself (same payload) and differs from another.
 *   RRT_TILE_NONZERO   x != 0
 *   RRT_TILE_RANGE     lo <= x < hi                                 (elem_bytes 4)
 *   RRT_TILE_SET       x < 256 and bit (x & 31) of set[x >> 5]      (elem_bytes 4; the material plane against a set of materials)
 *   RRT_TILE_DIFFERS   a[i] != b[i]
 * A tile is SELECTED when any element of any of its pixels passes.  Only pixels inside both the frame and the region count -- the pixels the reference never
 * traces (canvas row 0, row 1 of an odd height, the last column of an odd width) included: the planes hold their miss values there, a framebuffer its 0.
 * MARKS.  marks[n_tiles], one byte per tile of the FRAME.  Without RRT_TILE_KEEP every byte is written: 1 for a selected tile, 0 for any other, a tile the region
 * does not touch included.  With RRT_TILE_KEEP (or'ed into .test) a selected tile's byte becomes 1 and NO other byte is written: the marks already there are
 * joined.  Bytes at or beyond n_tiles are never touched.
 * rrt_select_tiles*: tests[0, n_tests) in order into the marks -- tests[0] as given, every later one as if it had RRT_TILE_KEEP: the union -- and then the
 * compaction of rrt_compact_rays_device (RRT_SELECT_FLAG) over the marks: d_tiles[0, count) the ascending numbers of the marked tiles, 0xFFFFFFFF in
 * d_tiles[count, n_tiles), which the tile-list kernel skips; *d_count = count.  d_tiles or d_count may be NULL, not both.  Scratch: rrt_compact_scratch_bytes(n_tiles)
 * bytes, 4-byte aligned.  rrt_render_tile_list_device(n = n_tiles, d_count, d_tiles, ...) enqueued behind it on the same stream needs nothing from the host.
 * WHAT THE LIBRARY DOES NOT KNOW: what an edit can reach.  A test sees what a plane holds at a pixel.  A pixel that sees an edited surface only in a mirror, that
 * gains or loses a shadow, or whose sub-sample hits something new after a geometry edit is the caller's to include.  The worked example is a material edit:
 * keep the `material` plane of rrt_render_surface_device, call rrt_raytracer_set_materials, select with RRT_TILE_SET holding the edited material AND every material
 * with kr > 0 (a mirror may show the edited surface; materials do not move shadows), render the list into the old framebuffer: the result is the new frame, bit
 * for bit.
 * Device forms: everything but the structs in device memory of rt's device; one launch per test (and the compaction's three) enqueued on `stream` (hipStream_t,
 * NULL = default): no allocation, no copy, no synchronisation.  A kernel enqueued before the call on the same stream may write the planes.  Not ray calls:
 * rrt_last_stats, the tuning state and the coverage state stay as they were, as with the compaction.
 * Host forms: everything in host memory; blocking.  One device allocation of the call's own; only what the call reads is uploaded (the marks only with
 * RRT_TILE_KEEP), only what was asked for comes down.  rrt_select_tiles: `tiles` has room for n_tiles entries, the valid ones are tiles[0, *count); tiles or
 * count may be NULL, not both; it has no marks of the caller's, so a RRT_TILE_KEEP of tests[0] has nothing to join and is ignored.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving every output as it was: NULL rt, test(s) or marks; a bad frame size; a region with w == 0 or h == 0 or one
 * that sticks out of the frame; n_tests == 0 or > RRT_MAX_TILE_TESTS; an unknown test; elem_bytes other than 1, 4 or 8; per_pixel other than 1 or 4; RANGE or SET
 * with elem_bytes != 4; a NULL a, a NULL b for DIFFERS; a plane not aligned to elem_bytes; n_tiles > RRT_MAX_TILE_LIST; both list outputs NULL; a scratch that is
 * NULL or smaller than rrt_compact_scratch_bytes(n_tiles).
 * Not covered: growing a selection by a ring of tiles, a schedule-aware order of the list, a test on the coverage mask, counted forms, the rrt_multi_* path. */
enum { RRT_TILE_NONZERO = 0, RRT_TILE_RANGE = 1, RRT_TILE_SET = 2, RRT_TILE_DIFFERS = 3 };
#define RRT_TILE_KEEP      0x100u   /* or'ed into .test: join the marks already there */
#define RRT_MAX_TILE_TESTS 8
typedef uint32_t rrt_tile_set[8];   /* 256 bits: bit (x & 31) of word x >> 5 stands for the value x */
typedef struct {
    uint32_t test;          /* one of the four, optionally | RRT_TILE_KEEP */
    uint32_t elem_bytes;    /* 1, 4 or 8 */
    uint32_t per_pixel;     /* 1 (a framebuffer) or 4 (a sub-sample plane) */
    uint32_t lo, hi;        /* RANGE */
    rrt_tile_set set;       /* SET: uint32_t set[8] */
    uint32_t _pad;
    const void *a, *b;      /* planes [region.h][region.w][per_pixel]; b: DIFFERS only */
} rrt_tile_test;            /* 72 bytes */

int rrt_mark_tiles_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                          const rrt_tile_test *test, uint8_t *d_marks, void *stream);
int rrt_mark_tiles(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                   const rrt_tile_test *test, uint8_t *marks);
int rrt_select_tiles_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                            const rrt_tile_test *tests, uint32_t n_tests, uint8_t *d_marks,
                            uint32_t *d_tiles, uint32_t *d_count, void *d_scratch, size_t scratch_bytes, void *stream);
int rrt_select_tiles(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region,
                     const rrt_tile_test *tests, uint32_t n_tests, uint32_t *tiles, uint32_t *count);

/* The deferred stages over a tile list in DEVICE memory: visibility buffers, surface buffers, shading and ambient occlusion from kept buffers for the 8x8-pixel
 * tiles a list names -- what rrt_render_visibility_device, rrt_render_surface_device, rrt_shade_surface_device and rrt_ambient_surface_device do for a rectangle.
 * For the second round of an edit loop (the planes under a tex or bump edit repaired where rrt_select_tiles_device found the material, then shaded from the
 * repaired planes), for shading a selection without walking its primary rays again, for more ambient samples where an `occluded` plane shows disagreement.
 * PLANES.  Every plane, input and output, is a WHOLE-FRAME plane, tight: [height][width][4] (point and normal [height][width][4][3]); grey and d_fb are
 * [height][width].  They are exactly the planes the region call of the same name takes with region == NULL.
 * LIST.  n, d_count and d_tiles mean what they mean for rrt_render_tile_list_device: tiles numbered ty * tiles_x + tx; m = min(n, *d_count), read by the kernel
 * when it runs, in stream order; m = n for d_count == NULL.  d_tiles[j] is used as an index only after d_tiles[j] < tiles_x * tiles_y; any other value,
 * 0xFFFFFFFF included, is skipped.  Entries [m, n) are never read.  Duplicates are allowed.  The list and the bound are only ever read.
 * LAUNCH.  The grid is sized by n, four blocks of 64 threads per entry, one per quadrant; a block at or beyond m ends after one scalar load and a compare, before
 * it touches LDS or memory.  n == 0: RRT_OK, nothing is launched and rrt_last_stats stays as it was.  n > RRT_MAX_TILE_LIST: RRT_ERR_INVALID_ARG.  The caller's
 * order is the schedule (no XCD-aware block order).
 * WRITTEN.  For a tile in d_tiles[0, m) and a pixel of it inside the frame, every element of every requested output at that pixel holds what the region call
 * with region == NULL writes there, bit for bit, in every traversal variant -- the miss values of the pixels the reference never traces included.  No other
 * element of any output is read or written.
 * READ.  Shading and ambient occlusion read their input planes only at pixels of listed tiles.  A plane value is never used as an index; material >= n_mats is
 * a miss, as for the region calls.
 * Traversal variant, tuning state and coverage state as for the region calls.  rrt_last_stats as for rrt_render_tile_list_device: kernel_ms and filter_variant
 * of this launch, width / height = the frame size, rays_primary = 0 -- the library does not read the list.
 * RRT_ERR_INVALID_ARG, before any GPU work: what the region call of the same name refuses (NULL rt, a bad frame size, a NULL struct, no output requested, a
 * missing required plane, a NULL d_fb, a bad sample table), n > RRT_MAX_TILE_LIST, NULL d_tiles with n > 0.
 * Enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no synchronisation.  There are no host forms: a host that knows its tiles has regions.
 * Not covered: a coverage pass, counted or tile-list forms of rrt_resolve_hits, the rank/world tile partition, the rrt_multi_* path and the progressive path. */
int rrt_render_visibility_tile_list_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t *d_count,
                                           const uint32_t *d_tiles, const rrt_visibility *d_planes, void *stream);
int rrt_render_surface_tile_list_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t *d_count,
                                        const uint32_t *d_tiles, const rrt_visibility *d_vis /* may be NULL */, const rrt_surface *d_planes,
                                        void *stream);
int rrt_shade_surface_tile_list_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t *d_count,
                                       const uint32_t *d_tiles, const rrt_visibility *d_vis, const rrt_surface *d_planes, void *d_fb,
                                       void *stream);
int rrt_ambient_surface_tile_list_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t n, const uint32_t *d_count,
                                         const uint32_t *d_tiles, const rrt_surface *d_planes, const rrt_ambient_samples *samples,
                                         const rrt_ambient *d_out, void *stream);

/* Screen-tile partition for N GPUs (one process per GPU): the frame is cut into 8x8-pixel tiles, tile k (row-major)
 * belongs to rank k % world.  Renders this rank's tiles into d_tiles[rrt_tiles_per_rank][64] (tile-major, device).
 * After a gather (or all-gather) of the per-rank buffers (RCCL, done by the caller), rrt_detile_device turns
 * d_gathered[world][tiles_per_rank][64] into the row-major framebuffer d_fb[width*height]. */
uint32_t rrt_tiles_per_rank(uint32_t width, uint32_t height, uint32_t world);
int rrt_render_tiles_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t rank, uint32_t world,
                            void *d_tiles, void *stream);
int rrt_detile_device(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t world, const void *d_gathered,
                      void *d_fb, void *stream);

/* ------------------------------------------------------------------ the N GPUs of one node
 * The gather is inside the library: grouped RCCL point-to-point sends to rank 0 (every peer on its own xGMI link) and de-tiling on rank 0's GPU.
 * rrt_multi_create: ONE process drives all GPUs -- the Rust host creates one raytracer per device (rrt_raytracer_create(..., device = i, ...)) and
 *   hands them over; rts[0]'s device receives the frame.  Uses ncclCommInitAll; RCCL is loaded on first use (dlopen), not at link time.
 * rrt_dist_create: ONE process per GPU (MPI / torch.distributed style): rank 0 calls rrt_dist_unique_id, the caller ships the 128 bytes to every rank
 *   by its own means, every rank calls rrt_dist_create (collective: ncclCommInitRank).
 * frames_in_flight (1..8) sizes a ring of slots, each with its own streams and buffers: rrt_multi_enqueue returns as soon as trace -> gather ->
 * de-tile of the frame are enqueued, frame i + 1 is traced while frame i is gathered.  rrt_render_multi is the blocking host-framebuffer form of
 * Scene::draw_scene (engine.rs:186): out_fb as in rrt_render; processes that do not hold rank 0 pass NULL.
 * RRT_MULTI_LOOPBACK (rrt_multi_create with n = 1): rank 0's own tiles travel through ncclSend/ncclRecv too -- a one-GPU test of the transport. */
typedef struct rrt_multi rrt_multi;
#define RRT_MULTI_LOOPBACK 1u
int rrt_multi_create(rrt_raytracer *const *rts, uint32_t n, uint32_t frames_in_flight, uint32_t flags, rrt_multi **out);
int rrt_dist_unique_id(void *out128);
int rrt_dist_create(rrt_raytracer *rt, uint32_t rank, uint32_t world, const void *unique_id128, uint32_t frames_in_flight, rrt_multi **out);
void rrt_multi_destroy(rrt_multi *g);
int rrt_multi_enqueue(rrt_multi *g, uint32_t width, uint32_t height, void *d_fb /* device memory of rank 0's GPU; NULL elsewhere */);
int rrt_multi_sync(rrt_multi *g);
int rrt_render_multi(rrt_multi *g, uint32_t width, uint32_t height, uint32_t *out_fb);
/* HIP-event time, on rank 0's stream, from "rank 0's own tiles are traced" to "frame de-tiled" of the last enqueued frame: the wait for the slowest
 * peer + the gather + the de-tiling (-1 on processes without rank 0). */
int rrt_multi_last_gather_ms(rrt_multi *g, double *out_ms);

/* Scene::draw_scene with the reference's progressive display (engine.rs:196-253): the scene rows are traced in chunks of chunk_rows (0 = the
 * reference's 50) from y = -H/2 upward, i.e. from the BOTTOM of the canvas to the top (put_pixel, engine.rs:146-158); after each chunk its rows are
 * in out_fb (zero-initialised like Canvas::new, engine.rs:135) and on_update -- the stand-in for canvas.update(), engine.rs:253 -- is called on the
 * calling thread with the canvas rows [first_row, first_row + n_rows) that the chunk wrote (n_rows = 0 for a chunk that wrote none).  The finished
 * frame equals rrt_render's.  on_update may be NULL. */
typedef void (*rrt_update_fn)(void *user, const uint32_t *fb, uint32_t width, uint32_t height, uint32_t first_row, uint32_t n_rows);
int rrt_render_progressive(rrt_raytracer *rt, uint32_t width, uint32_t height, uint32_t *out_fb, uint32_t chunk_rows,
                           rrt_update_fn on_update, void *user);

/* Batched RayTracer::get_ray_colour (raytracer.rs:29): n rays, origins/dirs [n][3] host doubles -> colours[n] 0x00RRGGBB.
 * The two per-ray entry points take whatever rays the caller has, so unless a variant is forced they pick theirs by measurement too: the first batch of
 * at least 16384 rays is timed with all three variants on its first 65536 rays and the fastest is kept for later calls (smaller batches before that
 * run the frame variant).  rrt_last_stats after a per-ray call: kernel_ms and filter_variant of that launch, width = n, height = 1. */
int rrt_get_ray_colours(rrt_raytracer *rt, uint32_t n, const double *origins, const double *dirs, uint32_t *colours);

/* Batched Ray::intersect_with_octant_with_max_t(octree, 0, max_t) (ray.rs:104-168): hit[n] 0/1, t,u,v [n], tri[n] = index in
 * push order.  max_t may be NULL (= +inf, ray.rs:96-102). */
int rrt_intersect_rays(rrt_raytracer *rt, uint32_t n, const double *origins, const double *dirs, const double *max_t,
                       uint8_t *hit, double *t, double *u, double *v, uint32_t *tri);

/* Some/None of the same walk, for a host that asks "is this point lit from there" (light baking, ambient occlusion, a moved light's shadow mask, line of
 * sight): occluded[i] = 1 / 0 = hit[i] of rrt_intersect_rays for the same origin, direction and max_t, byte for byte.  It is the reference's
 * Ray::intersect_with_octant_with_max_t(octree, 0, max_t) reduced to Some/None, NOT "any triangle anywhere on the segment": max_t bounds the root's own
 * list and the final comparison only, children are entered with +inf, the first sorted child that returns Some ends the loop (ray.rs:104-168), and a NaN or
 * non-positive max_t gives 0.  max_t may be NULL (= +inf).  The walk stops at the first node that proves Some, computes no u, v or
 * triangle index and writes one byte per ray.
 * The reference's shadow query triangle_exists_between_points (raytracer.rs:164-188) forms its ray as origin = point + normal * surface_offset,
 * direction = target - origin (not normalised), max_t = |direction| (raytracer.rs:170-179) and returns `true` for None, i.e. for "lit": the negation of
 * occluded[i].  The library does not form these rays: like the other per-ray entry points this one takes the caller's own, and the default mode's
 * exactness band applies in the same way (RRT_FLAG_NO_CULL above: the guard is keyed to the current eye, secondary rays are not guarded).
 * Host arrays, blocking; the traversal variant is measured as for the two calls above (same thresholds, same kept variant). */
int rrt_occluded_rays(rrt_raytracer *rt, uint32_t n, const double *origins, const double *dirs, const double *max_t, uint8_t *occluded);

/* Device-resident ray batches: the three per-ray queries on device pointers of rt's device, enqueued on `stream` (hipStream_t, NULL = default), not
 * synchronised.  No device allocation, no free, no copy and no measurement is made: nothing on the path serialises the caller's stream.  Per ray the
 * results are exactly those of the host forms, the miss convention of rrt_intersect_rays included (hit 0, t = u = v = 0.0, tri = 0xFFFFFFFF).
 * rrt_intersect_rays_device: any of the five output pointers may be NULL (that array is not written), at least one is set; with d_u and d_v both NULL the
 * second Moller-Trumbore that yields u and v is skipped.  d_max_t NULL = +inf.
 * Traversal variant: the forced one; else the one kept for per-ray calls (by an earlier host batch of at least 16384 rays, or by rrt_tune_rays_device);
 * else the frame variant, which is what small host batches run.
 * RRT_ERR_INVALID_ARG, before any GPU work, here and in rrt_occluded_rays: NULL rt; NULL origins or dirs with n > 0; every output NULL with n > 0.  n = 0 is
 * RRT_OK with nothing enqueued.  rrt_last_stats afterwards: as after the host forms (width = n, height = 1), kernel_ms from events on the caller's stream. */
int rrt_intersect_rays_device(rrt_raytracer *rt, uint32_t n, const double *d_origins, const double *d_dirs, const double *d_max_t,
                              uint8_t *d_hit, double *d_t, double *d_u, double *d_v, uint32_t *d_tri, void *stream);
int rrt_get_ray_colours_device(rrt_raytracer *rt, uint32_t n, const double *d_origins, const double *d_dirs, uint32_t *d_colours, void *stream);
int rrt_occluded_rays_device(rrt_raytracer *rt, uint32_t n, const double *d_origins, const double *d_dirs, const double *d_max_t,
                             uint8_t *d_occluded, void *stream);
/* BLOCKING: measures the three traversal variants on a device-resident batch -- each twice on its first min(n, 65536) rays, closest-hit query, outputs into
 * memory the library owns, launched on the default stream (the rays must be complete in memory: synchronise the stream that wrote them first) -- and keeps
 * the fastest for later per-ray calls, host and device forms alike, replacing an earlier choice.  Any n >= 1 is measured; whether the sample stands for the
 * rays to come is the caller's business.  A raytracer with a forced variant does no GPU work and reports that variant.  variant_out may be NULL. */
int rrt_tune_rays_device(rrt_raytracer *rt, uint32_t n, const double *d_origins, const double *d_dirs, const double *d_max_t, uint32_t *variant_out);

/* Surface attributes and bounce rays of arbitrary rays: per ray of a batch the full surface record of its first hit -- what rrt_render_surface* gives for a
 * frame's primary rays -- and the reference's own next ray from there.  For the G-buffers of what a mirror shows, second-bounce ambient occlusion, baking and
 * probes from points that are not the eye, and any integrator that keeps its rays on the GPU: a whole reflection chain of get_ray_colour_recursive
 * (raytracer.rs:29-112) can be followed level by level, feeding next_origin / next_dir of one call to the next, without restating reference arithmetic outside
 * the library.
 * Per ray i with origin o, direction d and bound m = max_t[i] (max_t NULL = +inf):
 *   hit, t, u, v, tri = exactly what rrt_intersect_rays returns for (o, d, m), byte for byte, its miss convention (hit 0, t = u = v = 0.0, tri = 0xFFFFFFFF) and
 *              its max_t rule included: a NaN or non-positive max_t is a miss.  Such a ray takes part in no walk: it is the way to pass a dead ray in a batch
 *              of fixed size;
 *   albedo   = the colour-texture texel of the hit, 0x00RRGGBB, as the visibility planes define it; a miss gives 0x00FFFFFF, the reference's background;
 *   point    = o + d * t (raytracer.rs:39);
 *   normal, material = as rrt_surface defines them: the value of get_normal_at_intersection (raytracer.rs:114-162) and the index in the material table;
 *   lights   = as rrt_surface defines it, bit k for light k: 1 for an Ambient or Directional light; for a Point light the negation of what rrt_occluded_rays
 *              returns for origin = point + normal * surface_offset, direction = light - point, max_t = |direction|.  Every point light is tested, also those
 *              behind the reference's `break` (raytracer.rs:235-237).  Bits >= n_lights are 0;
 *   next_origin = point + normal * surface_offset (raytracer.rs:82): the origin of the reflection ray, and of the shadow and ambient rays of the hit;
 *   next_dir = normalised(d - (normal * 2.0) * dot(d, normal)) (raytracer.rs:78-79), the reflection ray's direction as a frame forms it.  It is written for
 *              every hit, whatever the material's kr: whether the reference would reflect there (kr > 0, depth below max_reflection_depth) is the caller's
 *              decision, taken from `material`.
 * A miss gives point = normal = next_origin = next_dir = (0.0, 0.0, 0.0), material = 0xFFFFFFFF, lights = 0.
 * Any of the twelve pointers may be NULL (that array is not written), at least one is set.  What is not asked for is not computed: without `lights` no shadow
 * ray is walked; without albedo, normal, material, lights, next_origin and next_dir no attribute of the hit is loaded; without those and u and v the second
 * Moller-Trumbore is skipped -- hit / t / tri alone run the one walk of rrt_intersect_rays_device and nothing else.  Inputs and outputs must not overlap.  A non-finite origin or
 * direction gives unspecified bits for that ray, and no fault.
 * Exactness: the first walk is rrt_intersect_rays' walk, its guard included (keyed to the current eye); the shadow walks are the frame kernels' shadow walks --
 * default mode, not guarded, the band documented under RRT_FLAG_NO_CULL.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer as it was: NULL rt; NULL struct; all twelve pointers NULL with n > 0; NULL origins or dirs
 * with n > 0.  n = 0 is RRT_OK with nothing enqueued.
 * rrt_last_stats afterwards: as after the other per-ray calls (width = n, height = 1, rays_primary = n; shadow rays are not counted).
 * rrt_surface_rays_device: rays and arrays in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no
 * synchronisation and no measurement; the traversal variant by the rule of rrt_intersect_rays_device.
 * rrt_surface_rays: rays and arrays in host memory; blocking.  One device allocation of the call's own; only the requested arrays are downloaded.  The traversal
 * variant is measured on a first large batch as for the other host forms (same thresholds, same kept variant).
 * rrt_raytracer_set_camera (the guard's eye), set_lights, set_materials and set_triangles[_device] apply to every call made after they return.
 * Not covered: the rank/world tile partition, the rrt_multi_* path and the progressive path. */
typedef struct {
    uint8_t *hit; double *t, *u, *v; uint32_t *tri, *albedo;   /* [n] each                */
    double *point, *normal;                                   /* [n][3]                  */
    uint32_t *material, *lights;                              /* [n]                     */
    double *next_origin, *next_dir;                           /* [n][3]                  */
} rrt_ray_surface;                                            /* 12 pointers, 96 bytes   */
int rrt_surface_rays(rrt_raytracer *rt, uint32_t n, const double *origins, const double *dirs, const double *max_t,
                     const rrt_ray_surface *out);
int rrt_surface_rays_device(rrt_raytracer *rt, uint32_t n, const double *d_origins, const double *d_dirs, const double *d_max_t,
                            const rrt_ray_surface *d_out, void *stream);

/* Shading of arbitrary rays from kept records: finishes the rays of a batch from the records rrt_surface_rays* wrote for them, with the lights and materials in
 * force NOW, without walking the rays again -- what rrt_shade_surface does for a frame's primary rays, for the caller's own.  For relighting and material edits of
 * the G-buffers of what a mirror shows, of probes and bake points that are not the eye, and for an integrator that keeps its rays on the GPU and follows a
 * reflection chain level by level with rrt_surface_rays_device: `local` and `kr` are what a level of get_ray_colour_recursive mixes the level below into
 * (raytracer.rs:89-101).
 * rec / d_rec is the struct the caller gave rrt_surface_rays[_device] for these n rays, in that layout.  READ: albedo, point, normal, material -- all four required
 * -- and lights, which may be NULL.  The other seven pointers are ignored.  dirs / d_dirs, [n][3], required: the rays' directions, the segment direction that
 * compute_lighting_intensity (as v = -d) and the reflection ray use.  Origins are not needed: the point is stored.
 * depth: the recursion depth of get_ray_colour_recursive at which the batch stands, one value for all rays: 0 for rays a caller would hand rrt_get_ray_colours,
 * k for the rays of level k of a chain.  Any value is valid; depth >= max_reflection_depth means direct lighting only.
 * WRITTEN, per ray i; any of the three pointers may be NULL (that array is not written), at least one is set:
 *   material[i] >= n_mats (0xFFFFFFFF, a miss or a dead ray, included): colour = 0x00FFFFFF, the reference's background (raytracer.rs:109-111), local = (0.0, 0.0, 0.0),
 *            kr = 0.0 -- the rule of rrt_shade_surface; no table is read out of bounds whatever the arrays hold, no value of them is used as an index, and only the
 *            low 24 bits of albedo count.  Otherwise the record is the hit of a segment standing at `depth`, as the reference holds it after
 *            get_normal_at_intersection.  With `lights`, the lights the segment's sum adds up are [0, min(ctz(~mask), n_lights)) and no shadow ray of this hit is
 *            walked; with `lights` NULL its shadow rays are formed and walked as a frame walks them, the `break` at the first occluded point light
 *            (raytracer.rs:235-237) included;
 *   local  = the f64 `local` colour of raytracer.rs:67-71 -- the albedo's channels times compute_lighting_intensity -- unquantised;
 *   kr     = the material's kr where the reference reflects at this hit (kr > 0 and depth < max_reflection_depth, raytracer.rs:76), else 0.0;
 *   colour = the reference's result for this segment, 0x00RRGGBB.  Where kr == 0.0: local, each channel clamped to [0, 255] and truncated.  Where kr > 0.0 the
 *            reflection chain is traced from point + normal * surface_offset along normalised(d - (normal * 2.0) * dot(d, normal)) up to max_reflection_depth,
 *            its shadow rays always walked, every level of the unwind quantised to u8 (raytracer.rs:85-101), exactly as rrt_shade_surface does from depth 0.
 * What is not asked for is not computed: with colour NULL no reflection ray is formed or walked; with colour NULL and `lights` given the launch walks nothing at
 * all.  With a mask, a wave of 64 consecutive rays none of which hits a mirror walks nothing either.
 * CONTRACT.  If the records are those rrt_surface_rays* wrote for the rays (o, d) in this scene, colour with depth = 0 is what rrt_get_ray_colours returns for
 * (o, d) with the lights and materials in force now, bit for bit.  Keeping the records valid is the caller's business:
 *
 *   change since the records were written                                             arrays that are stale
 *   rrt_raytracer_set_triangles[_device]                                              all
 *   set_lights: position of a Point light, kind or index of any light, list length    `lights` only (pass it as NULL)
 *   set_lights: intensities, or the vector of an Ambient or Directional light         none
 *   set_materials: `tex` of a material                                                `albedo`, `normal` (the bump texel is read at the colour texture's indices)
 *   set_materials: `bump`                                                             `normal`
 *   set_materials: ka, kd, ks, ns, kr                                                 none
 *   rrt_raytracer_set_camera                                                          none: the rays are the caller's
 *
 * Exactness: every walk of this call is a secondary walk of a frame -- default mode, not guarded, the band documented under RRT_FLAG_NO_CULL.
 * A non-finite direction, point or normal gives unspecified values for that ray, and no fault.  Inputs and outputs must not overlap.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer and the outputs as they were: NULL rt; NULL rec or out; all three outputs NULL with n > 0;
 * NULL dirs or a NULL required array with n > 0.  n = 0 is RRT_OK with nothing enqueued.
 * rrt_last_stats afterwards: as after the other per-ray calls (width = n, height = 1, rays_primary = n; shadow and reflection rays are not counted).
 * rrt_shade_rays_device: arrays in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no synchronisation and
 * no measurement; the traversal variant by the rule of rrt_intersect_rays_device.
 * rrt_shade_rays: arrays in host memory; blocking.  One device allocation of the call's own; dirs and the four or five arrays it reads are uploaded, only the
 * requested outputs downloaded.  It never measures the variants -- it has no origins to measure a walk on -- and picks its variant by the device form's rule.
 * rrt_raytracer_set_lights, set_materials and set_triangles[_device] apply to every call made after they return.
 * Not covered: per-ray depths, the rank/world tile partition, the rrt_multi_* path and the progressive path. */
typedef struct { uint32_t *colour; double *local; double *kr; } rrt_ray_shade;   /* 24 bytes; colour [n], local [n][3], kr [n] */
int rrt_shade_rays(rrt_raytracer *rt, uint32_t n, const double *dirs, const rrt_ray_surface *rec, uint32_t depth, const rrt_ray_shade *out);
int rrt_shade_rays_device(rrt_raytracer *rt, uint32_t n, const double *d_dirs, const rrt_ray_surface *d_rec, uint32_t depth, const rrt_ray_shade *d_out,
                          void *stream);

/* Ambient occlusion for arbitrary ray records: which of n hemisphere rays from every hit of a batch are blocked, from the records rrt_surface_rays* wrote for it, in
 * ONE launch that forms the rays in registers -- what rrt_ambient_surface does for a frame's first hits, for the caller's own rays, with a rotation of the sample
 * table per record.  For second-bounce ambient occlusion (the records of next_origin / next_dir), for probes and bake points that are not the eye, and for a
 * frame's own planes: flattened to [n] they are valid records, so this call also gives a frame a rotated fan.
 * rec / d_rec is the struct the caller gave rrt_surface_rays[_device] for these n rays, in that layout.  READ: point, normal and material, all three required; the
 * other nine pointers are ignored.  Origins and directions of the rays are not needed.
 * samples: the table of rrt_ambient_surface -- n directions (sx, sy, sz) in the tangent frame of a hit, sz along the normal, and one max_t for all rays (+inf is
 * valid).  It lies in HOST memory in both forms, is borrowed for the call and travels in the kernel arguments.
 * rot / d_rot: [n][2] doubles, (c, s) per record -- the cosine and sine of the angle by which the record's fan is turned about its normal -- or NULL.  It lies where
 * the records lie.  The library neither normalises (c, s) nor checks c*c + s*s = 1: a scaled or mirrored pair is the caller's business, as the camera basis is.
 * Per record i: material[i] >= n_mats (0xFFFFFFFF, a miss or a dead ray, included) is a miss -- the rule of rrt_shade_rays and rrt_ambient_surface; no value of the
 * caller's arrays is used as an index.  Otherwise, with point p and normal n exactly as stored and tg, bt the reference's tangent frame as rrt_ambient_surface
 * defines it, the ray of sample k = (sx, sy, sz) is
 *   origin = p + n * surface_offset;   max_t = samples->max_t;
 *   rot == NULL:          direction.c = (tg.c*sx + bt.c*sy) + n.c*sz  per component -- exactly the ray of rrt_ambient_surface;
 *   rot != NULL, (c, s) = rot[i]:   rx = sx*c - sy*s;  ry = sx*s + sy*c  -- six f64 operations, each rounded on its own -- and
 *                         direction.c = (tg.c*rx + bt.c*ry) + n.c*sz.
 * WRITTEN; either pointer may be NULL (that array is not written), not both; every element of every requested array is written:
 *   occluded[i]: bit k = what rrt_occluded_rays returns for exactly that ray, byte for byte; bits at and above n are 0.  A miss gives 0.
 *   open[i]:     samples->n - popcount(occluded[i]) for a hit; samples->n for a miss or a dead record -- the rule by which `grey` counts a miss as open.
 * A non-finite point, normal or rot pair gives unspecified bits for that record, and no fault.  Inputs and outputs must not overlap.
 * Exactness: as for rrt_ambient_surface: every walk of this call is a shadow walk of a frame -- default mode, not guarded, the band documented under
 * RRT_FLAG_NO_CULL.
 * Keeping the records valid is the caller's business; the table under rrt_shade_rays says when for point, normal and material.  A change of lights never matters,
 * rrt_raytracer_set_camera never matters.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer and the outputs as they were: NULL rt, rec, samples or out; with n > 0 a NULL required array
 * or both outputs NULL; and, whatever n is, every refusal rrt_ambient_surface makes for its table: n == 0 or n > RRT_MAX_AMBIENT_SAMPLES; NULL dirs; a non-finite
 * direction component; max_t NaN or <= 0.  n = 0 with valid structs is RRT_OK with nothing enqueued.
 * rrt_last_stats afterwards: as after the other per-ray calls (width = n, height = 1, rays_primary = n; the hemisphere rays are not counted).
 * rrt_ambient_rays_device: arrays in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no synchronisation and
 * no measurement; the traversal variant by the rule of rrt_intersect_rays_device.
 * rrt_ambient_rays: arrays in host memory; blocking.  One device allocation of the call's own; the three arrays it reads are uploaded, and rot if it is given;
 * only the requested outputs are downloaded.  It never measures the variants and picks its variant by the device form's rule, as rrt_shade_rays does.
 * Not covered: a max_t per ray, weights per sample (the mask lets the host weight), the rank/world tile partition, the rrt_multi_* path and the progressive path. */
typedef struct { uint32_t *occluded; uint32_t *open; } rrt_ray_ambient;   /* 16 bytes; [n] each; either may be NULL, not both */
int rrt_ambient_rays(rrt_raytracer *rt, uint32_t n, const rrt_ray_surface *rec, const double *rot /* [n][2], may be NULL */,
                     const rrt_ambient_samples *samples, const rrt_ray_ambient *out);
int rrt_ambient_rays_device(rrt_raytracer *rt, uint32_t n, const rrt_ray_surface *d_rec, const double *d_rot,
                            const rrt_ambient_samples *samples, const rrt_ray_ambient *d_out, void *stream);

/* Surface records from kept hits, with no primary walk: turns the compact answer of an earlier walk -- t, u, v, tri as rrt_intersect_rays*, rrt_surface_rays* or a
 * frame's rrt_render_visibility* wrote them -- into the shading record rrt_shade_rays* and rrt_ambient_rays* read, without walking the rays again.  For refreshing
 * albedo and normal after a changed `tex` or `bump` binding, or `lights` after a moved point light, and for a per-ray pipeline of library calls alone:
 * rrt_intersect_rays_device (the cheap kernel) -> rrt_compact_rays_device (RRT_SELECT_FLAG on the hit bytes; rrt_ray_set.rec carries t, u, v, tri) ->
 * rrt_resolve_hits_counted_device, whose shadow walks then run in full waves.
 * rec / d_rec is the struct the caller gave rrt_intersect_rays' arrays a place in, or rrt_surface_rays[_device], or one built from a frame's visibility planes, in
 * that layout.  READ: t, u, v, tri; `hit` is ignored.  WRITTEN: any of albedo, point, normal, material, lights, next_origin, next_dir; any of the seven may be
 * NULL (that array is not written), at least one is set.  origins / dirs, [n][3]: the rays the hits belong to.
 * Hit rule.  Entry i is a hit iff tri[i] < n_tris of the scene in force.  Anything else (0xFFFFFFFF, a miss or a dead entry, included) gets the miss values of
 * rrt_surface_rays -- albedo 0x00FFFFFF, the vectors (0.0, 0.0, 0.0), material 0xFFFFFFFF, lights 0 -- and takes part in no walk.  tri is the only value of the
 * caller's arrays that is ever used as an index, and only after that compare.  t, u and v are used as given: point = o + d * t (raytracer.rs:39), the attributes
 * at (u, v); a non-finite one gives unspecified bits for that entry, and no fault: the texel indices go through the saturating cast and the modulo of
 * raytracer.rs:52-53 as in every other call.
 * CONTRACT.  If t, u, v, tri are what rrt_intersect_rays[_device], rrt_surface_rays[_device] or rrt_render_visibility[_device] wrote for the rays (o, d) in the scene
 * in force, every requested output is what rrt_surface_rays writes for those rays with the same bound, byte for byte.  For a frame the rays are those of
 * rrt_frame_rays in RRT_ORDER_ROWS in the same pose.  The lights, the materials and the surface_offset in force NOW apply.
 * Required: origins, dirs, rec, rec->t and rec->tri always; rec->u and rec->v unless only point and / or material are asked for.
 * What is not asked for is not computed.  Without `lights` nothing is walked at all: the launch is a gather of one 128-byte attribute record and up to two texels
 * per hit, in ONE kernel whatever traversal variant is in force.  With `lights` the shadow walks are those of rrt_surface_rays: every point light tested, one per
 * turn, all hits of a wave together -- default mode, not guarded, the band documented under RRT_FLAG_NO_CULL; a wave of 64 consecutive entries without a hit walks
 * nothing.  Inputs and outputs must not overlap.
 * Keeping t, u, v, tri valid is the caller's business:
 *
 *   change since t, u, v, tri were written                                            what is stale
 *   rrt_raytracer_set_triangles[_device]                                              t, u, v, tri: nothing can be resolved from them
 *   rrt_raytracer_set_materials, rrt_raytracer_set_lights                             nothing: resolving again is what brings albedo, normal and lights up to date
 *   rrt_raytracer_set_camera                                                          nothing: the rays are the caller's
 *
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer and the outputs as they were: NULL rt; NULL rec; all seven outputs NULL with n > 0; NULL
 * origins, dirs or a NULL required array with n > 0.  n = 0 is RRT_OK with nothing enqueued.
 * rrt_last_stats afterwards: as after the other per-ray calls (width = n, height = 1, rays_primary = n; shadow rays are not counted).
 * rrt_resolve_hits_device: arrays in device memory of rt's device; enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no synchronisation and
 * no measurement; the traversal variant of the shadow walks by the rule of rrt_intersect_rays_device.
 * rrt_resolve_hits: arrays in host memory; blocking.  One device allocation of the call's own; only what is read is uploaded (u and v only where an output reads
 * them), only the requested outputs are downloaded.  It never measures the variants and picks its variant by the device form's rule, as rrt_shade_rays does.
 * Not covered: a region form (rrt_frame_rays in RRT_ORDER_ROWS serves a frame), the rank/world tile partition, the rrt_multi_* path and the progressive path. */
int rrt_resolve_hits(rrt_raytracer *rt, uint32_t n, const double *origins, const double *dirs, const rrt_ray_surface *rec);
int rrt_resolve_hits_device(rrt_raytracer *rt, uint32_t n, const double *d_origins, const double *d_dirs, const rrt_ray_surface *d_rec, void *stream);

/* Stable compaction of ray batches and records, and its inverse: between two stages of a per-ray pipeline (rrt_surface_rays_device -> rrt_shade_rays_device ->
 * rrt_ambient_rays_device) a batch thins out -- misses drop out, only mirror hits reflect, only hits have an ambient fan.  These calls move the survivors to the
 * front of a batch that KEEPS ITS LENGTH n and fill the tail with dead entries, on the device and without a read-back of the count: the next stage is enqueued with
 * the same n, a NaN max_t is a dead ray and material = 0xFFFFFFFF a dead record for every per-ray call, and a wave of 64 dead entries walks nothing.
 * d_src / d_dst: two rrt_ray_set -- the rays (origins, dirs [n][3]), their bounds (max_t [n]), the rotations of rrt_ambient_rays (rot [n][2]) and the twelve
 * arrays of an rrt_ray_surface, in the layouts of the calls that take them.  Any pointer may be NULL.  What is non-NULL in dst is gathered from the same array of
 * src, which must then be non-NULL -- except max_t: dst.max_t with src.max_t == NULL writes +inf for the survivors, so that a batch that had no bounds gets one
 * that can say "dead".  Arrays of src may alias each other: a record's next_origin / next_dir as src.origins / src.dirs is the intended use.  dst, index, count and
 * scratch must overlap neither src (or flag) nor each other.
 * select, sel[i] per entry i:
 *   RRT_SELECT_HIT     src.rec.material[i] < n_mats -- the hit rule of rrt_shade_rays and rrt_ambient_rays; src.rec.material is required;
 *   RRT_SELECT_MIRROR  that, and kr > 0.0 for that material in the table in force NOW (rrt_raytracer_set_materials before the call changes the selection).
 *                      Whether depth < max_reflection_depth stays the caller's decision; src.rec.material is required;
 *   RRT_SELECT_FLAG    flag[i] != 0; flag / d_flag [n] bytes is required (the other modes ignore it), and src and dst may both be NULL: only index and count
 *                      are wanted then.
 * RESULT, a stable partition:  count = the number of i with sel[i];  for j < count, index[j] = the j-th smallest such i and element j of every dst array is
 * element index[j] of the src array, copied byte for byte -- NaN payloads and -0.0 are preserved, no arithmetic touches a value;  for count <= j < n,
 * index[j] = 0xFFFFFFFF and element j of every dst array holds the dead value: max_t = NaN (0x7FF8000000000000), material = tri = 0xFFFFFFFF,
 * albedo = 0x00FFFFFF, hit = 0, lights = 0, rot = (1.0, 0.0), every other double 0.0 -- the miss values of rrt_surface_rays.  index and count may each be NULL;
 * with n > 0 at least one of index, count and the arrays of dst is set.  Every element of every requested output is written; the result is the same bits on
 * every run.
 * Scratch: rrt_compact_scratch_bytes(n) bytes of device memory, 4-byte aligned, whose contents before and after mean nothing: 0 for n == 0, never smaller for a
 * larger n, about 4 bytes per 1024 entries.  The device form refuses a smaller scratch_bytes, and a NULL d_scratch when the size is above 0.
 * rrt_compact_rays_device: everything but the structs themselves in device memory of rt's device; three small kernels enqueued on `stream` (hipStream_t, NULL =
 * default): no allocation, no copy to the host, no synchronisation, no measurement.  These are not ray calls: rrt_last_stats stays as it was, in both forms.
 * rrt_compact_rays: everything in host memory; blocking.  One device allocation of the call's own; only what the call reads is uploaded, only what was asked for
 * is downloaded.
 * rrt_scatter_rays[_device], the inverse, expands a stage's results back to source order: for j in [0, n), if index[j] < n then dst[index[j]] = src[j], elem_bytes
 * bytes each; every other entry, 0xFFFFFFFF included, is skipped.  Elements of dst that no j names are left as they were: the caller prefills them (0 for
 * `occluded`, samples->n for `open`).  elem_bytes is 1, 4, 8, 16 or 24, and the arrays are aligned to min(elem_bytes, 8).  An index that occurs twice gives one of
 * the values, and no fault.  src, dst and index [n elements each] must not overlap.  The host form is blocking and carries dst up and down.
 * RRT_ERR_INVALID_ARG, before any GPU work, before the handle is looked at, and leaving the outputs and the raytracer as they were: NULL rt; an unknown select; an
 * elem_bytes other than the five; and with n > 0: a NULL array the mode requires, an array of dst without its array of src (max_t excepted), every output NULL,
 * a scratch too small or NULL, a NULL index, src or dst of a scatter.  n == 0 is RRT_OK with nothing enqueued; rrt_compact_rays then writes *count = 0. */
enum { RRT_SELECT_HIT = 0, RRT_SELECT_MIRROR = 1, RRT_SELECT_FLAG = 2 };
typedef struct { double *origins, *dirs, *max_t, *rot; rrt_ray_surface rec; } rrt_ray_set;   /* 128 bytes; [n][3], [n][3], [n], [n][2], 12 record arrays; any may be NULL */
size_t rrt_compact_scratch_bytes(uint32_t n);
int rrt_compact_rays_device(rrt_raytracer *rt, uint32_t n, uint32_t select, const uint8_t *d_flag, const rrt_ray_set *d_src, const rrt_ray_set *d_dst,
                            uint32_t *d_index, uint32_t *d_count, void *d_scratch, size_t scratch_bytes, void *stream);
int rrt_compact_rays(rrt_raytracer *rt, uint32_t n, uint32_t select, const uint8_t *flag, const rrt_ray_set *src, const rrt_ray_set *dst,
                     uint32_t *index, uint32_t *count);
int rrt_scatter_rays_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_index, uint32_t elem_bytes, const void *d_src, void *d_dst, void *stream);
int rrt_scatter_rays(rrt_raytracer *rt, uint32_t n, const uint32_t *index, uint32_t elem_bytes, const void *src, void *dst);

/* Stable sort of ray batches and records by a coherence key: the other half of a wavefront pipeline.  Compaction removes the dead lanes and keeps the caller's
 * order; this call puts entries that start in the same part of the scene and head the same way next to each other, for batches that are not coherent to begin
 * with (probes, random rays, second-bounce records, the sources of rotated ambient fans).  The batch KEEPS ITS LENGTH n, dead entries go to the tail, and `index`
 * is what rrt_scatter_rays[_device] takes to bring a stage's results back to source order.
 * KEYS, one uint32 per entry; 0xFFFFFFFF means "dead" and sorts last.  key_mode:
 *   RRT_SORT_KEY_GIVEN   keys[i] as the caller wrote it; keys / d_keys [n] is required (the other modes ignore it), and src and dst may both be NULL;
 *   RRT_SORT_KEY_RAY     src.origins and src.dirs are required.  Dead if src.max_t is given and !(max_t[i] > 0.0) -- the dead-ray rule of the per-ray calls, NaN
 *                        counts as dead; otherwise p = origins[i], d = dirs[i];
 *   RRT_SORT_KEY_RECORD  src.rec.point, .normal and .material are required.  Dead if material[i] >= n_mats -- the hit rule of rrt_shade_rays and rrt_ambient_rays;
 *                        otherwise p = point[i], d = normal[i].
 * An alive key is formed with the root box lo, hi in force NOW (node 0 of rrt_raytracer_get_octree; rrt_raytracer_set_triangles may change it).  Per axis a
 * (x = 0, y = 1, z = 2): s_a = 512.0 / (hi.a - lo.a), one f64 division on the host;  q = (p.a - lo.a) * s_a, two f64 operations, each rounded;
 * cell_a = q >= 511.0 ? 511 : (q > 0.0 ? (uint32)q : 0), so that a NaN q gives 0, +inf 511 and -inf 0.  Key bit 3 b + a is bit b of cell_a for b = 0..8 (a Morton
 * code of 512^3 cells), key bit 27 + a is d.a < 0.0 (-0.0 and NaN give 0), bits 30 and 31 are 0.  No value of the caller's arrays is used as an index.
 * RESULT, a stable sort, ascending:  index is the permutation with key[index[j]] non-decreasing, entries with equal keys -- the dead ones among them, in the tail --
 * in source order;  keys_out[j] = key[index[j]];  count = the number of keys that are not 0xFFFFFFFF;  element j of every non-NULL array of dst is element index[j]
 * of the same array of src, copied byte for byte -- NaN payloads and -0.0 are preserved -- the tail like the rest: a pure permutation, nothing is filled in, and
 * every array of dst needs its array of src (there is no max_t exception here).  index, keys_out, count and the arrays of dst may each be NULL; with n > 0 at least
 * one of them is set.  Every element of every requested output is written; the result is the same bits on every run.  Arrays of src may alias each other; dst,
 * index, keys_out, count and scratch must overlap neither src (or keys) nor each other.
 * Scratch: rrt_sort_scratch_bytes(n) bytes of device memory, 4-byte aligned, whose contents before and after mean nothing: 0 for n == 0, a multiple of 4, never
 * smaller for a larger n, at most 20 n + 65536 (16 bytes per entry for two (key, index) buffer pairs, 1 KB of digit counts per 4096 entries, 1 KB of totals).  The
 * device form refuses a smaller scratch_bytes and a NULL d_scratch.
 * rrt_sort_rays_device: everything but the structs themselves in device memory of rt's device; the kernels of a four-pass radix sort enqueued on `stream`
 * (hipStream_t, NULL = default): no allocation, no copy to the host, no synchronisation, no measurement.  These are not ray calls: rrt_last_stats stays as it was,
 * in both forms.
 * rrt_sort_rays: everything in host memory; blocking.  One device allocation of the call's own; only what the call reads is uploaded, only what was asked for is
 * downloaded.
 * RRT_ERR_INVALID_ARG, before any GPU work, before the handle is looked at, and leaving the outputs and the raytracer as they were: NULL rt; an unknown key_mode;
 * and with n > 0: a NULL array the mode requires, an array of dst without its array of src, every output NULL, a scratch too small or NULL.  n == 0 is RRT_OK with
 * nothing enqueued; rrt_sort_rays then writes *count = 0. */
enum { RRT_SORT_KEY_GIVEN = 0, RRT_SORT_KEY_RAY = 1, RRT_SORT_KEY_RECORD = 2 };
size_t rrt_sort_scratch_bytes(uint32_t n);
int rrt_sort_rays_device(rrt_raytracer *rt, uint32_t n, uint32_t key_mode, const uint32_t *d_keys, const rrt_ray_set *d_src, const rrt_ray_set *d_dst,
                         uint32_t *d_index, uint32_t *d_keys_out, uint32_t *d_count, void *d_scratch, size_t scratch_bytes, void *stream);
int rrt_sort_rays(rrt_raytracer *rt, uint32_t n, uint32_t key_mode, const uint32_t *keys, const rrt_ray_set *src, const rrt_ray_set *dst,
                  uint32_t *index, uint32_t *keys_out, uint32_t *count);

/* The two ends of the per-ray pipeline, and a frame traced as ray generations.  rrt_surface_rays_device -> rrt_shade_rays_device -> rrt_compact_rays_device (->
 * rrt_sort_rays_device) take a batch of rays from a first hit to `local` and `kr` per level of a reflection chain.  These calls supply what stands before and behind
 * them: the rays a frame traces, as a batch; the finish of one level of the chain; the pixels.  rrt_render_wavefront strings all of it together.
 *
 * FRAME RAYS.  rrt_frame_rays[_device]: the primary rays of a region of a frame in the pose in force (rrt_camera; the vp_* options apply), as a batch of
 * n = rrt_frame_ray_count(width, height, region, order) entries.  region as rrt_region: NULL = the whole frame.  Entry e is sub-sample s (the order of rrt_visibility)
 * of canvas pixel (px, py), region = {x0, y0, w, h}:
 *   RRT_ORDER_ROWS   n = 4 * w * h;  e = ((py - y0) * w + (px - x0)) * 4 + s -- the element order of a [h][w][4] plane of the region calls;
 *   RRT_ORDER_TILES  n = 64 * tiles_w * tiles_h;  e = (((ty - y0 / 4) * tiles_w + (tx - x0 / 4)) * 16 + (py & 3) * 4 + (px & 3)) * 4 + s with tx = px / 4, ty = py / 4:
 *                    4x4-pixel tiles anchored at multiples of 4 of the FRAME, not of the region -- tiles_w = (x0 + w + 3) / 4 - x0 / 4, tiles_h likewise -- row-major
 *                    over that tile rectangle.  One aligned run of 64 entries is the 4x4 pixels x 4 sub-samples that one wave of the frame kernels holds, so a
 *                    per-ray stage (64 consecutive entries per wave) walks the frame's own waves; planes flattened in ROWS order cost 1.02-1.33x of that
 *                    (profiles/ambient_rays.json).
 * n is a multiple of 4.  A traced pixel's entry: origins[e] = the eye in force, dirs[e] = the direction the frame kernels form for it, bit for bit -- per component
 * (right.k*a + up.k*b) + forward.k*c, five operations each rounded on its own (rrt_camera) -- and max_t[e] = +inf.  A DEAD entry -- a pixel the reference never traces
 * (canvas row 0, row 1 of an odd height, the last column of an odd width) and, in TILES order, a pixel outside the region or the frame -- gets origins = dirs =
 * (0.0, 0.0, 0.0) and max_t = NaN (0x7FF8000000000000, the dead value of rrt_compact_rays): with max_t the batch can go to every per-ray call as it is, and a dead
 * ray takes part in no walk.  Any of the three arrays may be NULL (not written), at least one is set; WITHOUT max_t THE CALLER GETS NO DEAD MARKER -- a dead entry's
 * zero direction is then an ordinary (degenerate) ray to the per-ray calls.  Every element of every requested array is written; the same bits on every run.  The
 * arrays are 8-byte aligned; 16-byte aligned arrays (any device allocation) are written with 16-byte stores.
 * rrt_frame_ray_count: 0 for arguments the calls refuse, and for a region of more than 2^32 - 1 entries (refused too: n is the uint32 of the per-ray calls).
 * rrt_frame_rays_device: arrays in device memory of rt's device; one kernel enqueued on `stream` (hipStream_t, NULL = default): no allocation, no copy, no
 * synchronisation.  rrt_frame_rays: arrays in host memory; blocking, one device allocation of the call's own.  These are not ray calls: rrt_last_stats stays as it
 * was, in both forms (the precedent of rrt_compact_rays).
 * RRT_ERR_INVALID_ARG, before any GPU work and before the handle is looked at: NULL rt; a bad frame size; a region with w == 0 or h == 0 or one that sticks out of
 * the frame; an unknown order; all three arrays NULL.
 *
 * CHAIN RESOLVE.  rrt_mix_rays[_device]: one level of the unwind of get_ray_colour_recursive (raytracer.rs:89-108), in source order.  Per entry i of n:
 *   material[i] >= n_mats (the hit rule of rrt_shade_rays; a miss or a dead entry):          colour[i] = 0x00FFFFFF, the reference's background;
 *   a hit, and kr == NULL or reflected == NULL or !(kr[i] > 0.0):                             the three channels of local[i], each clamped to [0, 255] and truncated
 *                                                                                             (raytracer.rs:104-108; NaN gives 0), 0x00RRGGBB;
 *   a hit with kr[i] > 0.0, kr and reflected given:                                           per channel clamp(local * (1.0 - kr) + (double)channel(reflected[i]) * kr)
 *                                                                                             -- the f64 operations of raytracer.rs:89-101, each rounded on its own.
 * local [n][3] and kr [n] are what rrt_shade_rays* wrote for the level; reflected [n] holds the colours of the level BELOW in this level's order: the caller brings
 * them there with rrt_scatter_rays_device (4-byte elements) and the `index` of this level's compaction.  reflected[i] is read only for the entries that mix, and only
 * its low 24 bits count.  material may be NULL: every entry is then a hit.  No value of the caller's arrays is used as an index.  Inputs and output must not overlap.
 * RRT_ERR_INVALID_ARG, before any GPU work and before the handle is looked at: NULL rt; local or colour NULL with n > 0.  n == 0 is RRT_OK with nothing enqueued.
 * rrt_mix_rays_device: one kernel on `stream`, no allocation, no copy, no synchronisation; rrt_mix_rays: host arrays, blocking, one allocation of the call's own.
 * rrt_last_stats stays as it was.
 *
 * PIXELS.  rrt_mix_pixels[_device]: colours [rrt_frame_ray_count(...)] in the given order -> fb / out_fb [region.h][region.w] pixels, 0x00RRGGBB.  A traced pixel is
 * the reference's Color::mix (entities.rs:49-69) of its four sub-sample colours as the frame kernels compute it: channel sums, truncating / 4 (only the low 24 bits
 * of a colour count); a pixel the reference never traces is 0; every pixel of the region is written; dead entries are not read.  With region == NULL the layout is
 * the framebuffer of rrt_render_device.  Refusals as rrt_frame_rays, with "colours or the
 * framebuffer NULL" for its last one; the two forms as above; rrt_last_stats stays as it was.
 *
 * THE FRAME BY RAY GENERATIONS.  rrt_render_wavefront[_device]: CONTRACT -- the output is the same region of the frame rrt_render produces in the pose and with the
 * lights and materials in force, bit for bit -- traced level by level instead of ray by ray:
 *   1. the frame rays of the region in `order`, with max_t;
 *   2. for depth k = 0 .. max_reflection_depth: the surface records of the level's rays (rrt_surface_rays_device: albedo, point, normal, material, lights, and for
 *      k < max next_origin / next_dir); local and kr of the level (rrt_shade_rays_device at depth k, with the mask: this launch walks nothing); for k < max the
 *      compaction of the mirror hits' next rays into the rays of level k + 1 (rrt_compact_rays_device, RRT_SELECT_MIRROR, max_t synthesised), its index kept;
 *   3. back up, for k = max .. 0: the colours of level k + 1 scattered through the index of level k (rrt_scatter_rays_device), then rrt_mix_rays_device;
 *   4. rrt_mix_pixels_device.
 * Everything is enqueued on `stream`: no allocation, no copy to the host, no read-back of a count, no synchronisation.  Every launch has the grid of
 * n = rrt_frame_ray_count(...), because the host never learns a count; but from level 1 on the stages are the COUNTED forms below, bound by the count the level
 * above's compaction left in the work memory: surface, shade and compaction of level k by the count of level k - 1, the scatter of level k by the count of level k,
 * the mix of level k by the count of level k - 1.  The dead tail of a compacted level is neither read nor written, its blocks leave at once, and a level whose
 * predecessor left nothing alive costs its launches and nothing else.  Level 0, its mix and the pixels run uncounted.  The launches are those of the calls named
 * above and of their counted forms -- no kernel of its own.
 * Traversal variant: the rule of rrt_intersect_rays_device -- the forced one, else the one kept for per-ray calls, else the frame variant; nothing is measured, and the
 * call does not count as a frame of that size for the frame variant's measurement (RRT_FLAG_LANE_FILTER above).
 * Work memory: d_work = device memory of at least rrt_wavefront_work_bytes(rt, width, height, region, order) bytes, 256-byte aligned, whose contents before and after
 * mean nothing.  The size is 0 for arguments the call refuses, never smaller for a larger region, and at most
 *   n * (229 + 40 * (max_reflection_depth + 1)) + 16384   bytes, n = rrt_frame_ray_count(...)
 * -- per entry two generations of rays (2 x 56), one level's record arrays (104), two levels' colours and the scattered ones (12), the compaction's scratch, and per
 * level what the way back up needs: local, kr, material and index (40); one uint32 per level for the counts.  About 1.2 GB for a 1920 x 1080 frame at the default depth of 5.
 * rrt_last_stats afterwards: kernel_ms = the time between two events around the whole sequence, filter_variant = the variant used, width / height = the frame size,
 * rays_primary = 4 * the traced pixels inside the region.
 * RRT_ERR_INVALID_ARG, before any GPU work and leaving the raytracer as it was: the refusals of rrt_frame_rays for rt, the frame size, the region and the order; a
 * NULL framebuffer; a d_work that is NULL, not 256-byte aligned or smaller than rrt_wavefront_work_bytes says.
 * rrt_render_wavefront: framebuffer in host memory; blocking; it owns and frees its work memory and downloads the region's pixels.
 * rrt_raytracer_set_camera, set_lights, set_materials and set_triangles[_device] apply to every call made after they return, and must not overlap one in flight.
 * Not covered, as for the other region calls: the rank/world tile partition, the rrt_multi_* path and the progressive path; sorting between levels. */
enum { RRT_ORDER_ROWS = 0, RRT_ORDER_TILES = 1 };
uint32_t rrt_frame_ray_count(uint32_t width, uint32_t height, const rrt_region *region, uint32_t order);   /* 0 for bad arguments */
int rrt_frame_rays_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order,
                          double *d_origins, double *d_dirs, double *d_max_t, void *stream);
int rrt_frame_rays(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order,
                   double *origins, double *dirs, double *max_t);
int rrt_mix_rays_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_material, const double *d_local, const double *d_kr,
                        const uint32_t *d_reflected, uint32_t *d_colour, void *stream);
int rrt_mix_rays(rrt_raytracer *rt, uint32_t n, const uint32_t *material, const double *local, const double *kr,
                 const uint32_t *reflected, uint32_t *colour);
int rrt_mix_pixels_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order,
                          const uint32_t *d_colours, void *d_fb, void *stream);
int rrt_mix_pixels(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order,
                   const uint32_t *colours, uint32_t *out_fb);
size_t rrt_wavefront_work_bytes(const rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order);
int rrt_render_wavefront_device(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order,
                                void *d_fb, void *d_work, size_t work_bytes, void *stream);
int rrt_render_wavefront(rrt_raytracer *rt, uint32_t width, uint32_t height, const rrt_region *region, uint32_t order, uint32_t *out_fb);

/* COUNTED DEVICE FORMS.  A batch whose length was decided on the GPU -- the `count` of a compaction, the survivors of a kernel of the caller's -- need not be padded
 * with dead entries that every later stage pays for, nor read back (which synchronises).  Each of the ten calls below is the `_device` call of the same name with
 * ONE more argument, `const uint32_t *d_count`, directly after n: a launch bound that lives in device memory.
 * CONTRACT, the same for all ten:
 *   - d_count points to one uint32 in device memory of rt's device, 4-byte aligned.  The host never reads it; the kernels read it when they run, in stream order.  It
 *     may therefore be the `count` output of a compaction enqueued earlier on the same stream, with nothing in between.  It is only ever read.
 *   - Let m = min(n, *d_count): a *d_count above n is n.  Entries [0, m) are processed exactly as the uncounted call with n = m processes them, byte for byte.
 *     Entries [m, n) of every input and of every output are neither read nor written.  m == 0 writes nothing.
 *   - The arrays still hold n entries and the grid is still sized by n, because the host does not know m.  A block whose first entry is at or beyond m ends after one
 *     scalar load and one compare, before it touches LDS, a barrier or memory.  No atomics, no block that waits on another: the same bits on every run.
 *   - d_count == NULL: the call IS the uncounted one, through the same kernels.
 *   - Refusals are those of the uncounted form, made at the same point: before any GPU work, and for compaction, scatter and mix before the handle is looked at.
 *     n == 0 is RRT_OK with nothing enqueued.
 *   - rrt_last_stats after a counted ray call (intersect, get_ray_colours, occluded, surface, shade, ambient, resolve): as after the uncounted one, with
 *     width = rays_primary = n -- the host does not know m.  Counted compaction, scatter and mix leave it alone, as the uncounted ones do.
 * rrt_compact_rays_counted_device, in addition: the selection is evaluated over [0, m) only; *d_count_out, d_index and the arrays of d_dst are those of the uncounted
 * call with n = m -- survivors in [0, count_out), the dead fill in [count_out, m), nothing in [m, n); with m == 0 the output count is 0 and nothing else is written.
 * scratch_bytes is still checked against rrt_compact_scratch_bytes(n), and all of that scratch may be written.  d_count and d_count_out must not be the same word:
 * equal non-NULL pointers are refused with RRT_ERR_INVALID_ARG (neighbouring words of one allocation are fine).
 * rrt_scatter_rays_counted_device: j runs over [0, m); d_index[j] for j >= m is not read.  An index is a position in the caller's arrays of n elements, so the rule
 * for one that is skipped stays "at or above n" (NOT m): the index of a counted compaction names source positions up to its own bound, which may exceed its count.
 * rrt_mix_rays_counted_device: entries [0, m).
 * NOT covered: rrt_sort_rays_device (a counted sort needs a rule for the tail that a pure permutation has not got), the region calls (their size is the host's), and
 * rrt_tune_rays_device (it measures, and synchronises to do so).  There are no host forms: a host caller knows its n. */
int rrt_intersect_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const double *d_origins, const double *d_dirs, const double *d_max_t,
                                      uint8_t *d_hit, double *d_t, double *d_u, double *d_v, uint32_t *d_tri, void *stream);
int rrt_get_ray_colours_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const double *d_origins, const double *d_dirs, uint32_t *d_colours,
                                       void *stream);
int rrt_occluded_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const double *d_origins, const double *d_dirs, const double *d_max_t,
                                     uint8_t *d_occluded, void *stream);
int rrt_surface_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const double *d_origins, const double *d_dirs, const double *d_max_t,
                                    const rrt_ray_surface *d_out, void *stream);
int rrt_shade_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const double *d_dirs, const rrt_ray_surface *d_rec, uint32_t depth,
                                  const rrt_ray_shade *d_out, void *stream);
int rrt_ambient_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const rrt_ray_surface *d_rec, const double *d_rot,
                                    const rrt_ambient_samples *samples, const rrt_ray_ambient *d_out, void *stream);
int rrt_resolve_hits_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const double *d_origins, const double *d_dirs,
                                    const rrt_ray_surface *d_rec, void *stream);
int rrt_compact_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, uint32_t select, const uint8_t *d_flag, const rrt_ray_set *d_src,
                                    const rrt_ray_set *d_dst, uint32_t *d_index, uint32_t *d_count_out, void *d_scratch, size_t scratch_bytes, void *stream);
int rrt_scatter_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const uint32_t *d_index, uint32_t elem_bytes, const void *d_src,
                                    void *d_dst, void *stream);
int rrt_mix_rays_counted_device(rrt_raytracer *rt, uint32_t n, const uint32_t *d_count, const uint32_t *d_material, const double *d_local, const double *d_kr,
                                const uint32_t *d_reflected, uint32_t *d_colour, void *stream);

/* The octree of a raytracer whose set-up ran on the GPU (the default), read back from its device: same layout as rrt_model_get_octree; info (may be
 * NULL) as rrt_model_get_info.  Any pointer may be NULL.  RRT_ERR_UNSUPPORTED for a RRT_FLAG_HOST_SETUP raytracer (ask the model). */
int rrt_raytracer_get_octree(const rrt_raytracer *rt, rrt_model_info *info, double *aabb, uint32_t *first_child, uint32_t *tri_count,
                             uint32_t *own_off, uint32_t *own_idx);
/* Test / developer introspection: the bytes of one scene buffer in HBM.  out == NULL asks for the size only.
 * RRT_BUF_TRI_SLOT: uint32 [n_tris], the table rrt_resolve_hits reads -- per triangle the lowest slot of RRT_BUF_ATTR / RRT_BUF_SLOT_TRI that is the triangle's
 * (0xFFFFFFFF for a triangle outside the tree); kept by both set-up paths, the same bits on every run. */
enum { RRT_BUF_NODES = 0, RRT_BUF_GEOM, RRT_BUF_ATTR, RRT_BUF_SUPERS, RRT_BUF_CBOXES, RRT_BUF_CHILD_BOXES, RRT_BUF_TBOXES, RRT_BUF_SUSPECTS,
       RRT_BUF_OCT_BOX, RRT_BUF_OCT_FIRST_CHILD, RRT_BUF_OCT_TRI_COUNT, RRT_BUF_OCT_OWN_OFF, RRT_BUF_OCT_OWN_IDX, RRT_BUF_SLOT_TRI, RRT_BUF_SLOT_POS, RRT_BUF_CHAINS,
       RRT_BUF_TRI_SLOT };
int rrt_raytracer_get_buffer(const rrt_raytracer *rt, uint32_t which, void *out, size_t capacity, size_t *bytes);

/* Chain records of this raytracer's scene (see RRT_FLAG_NO_CHAIN_SHORTCUT): the number of chains that have one and the number of chain nodes they
 * cover.  Both 0 when the shortcut cannot apply (RRT_FLAG_NO_CULL, a triangle poking out of the root box, 2^24 nodes or more); the flag that turns
 * the shortcut off does not change them.  Either pointer may be NULL. */
int rrt_raytracer_get_chain_info(const rrt_raytracer *rt, uint32_t *n_chains, uint32_t *n_chain_nodes);

/* The coverage pass of this raytracer's LAST frame launch (see RRT_FLAG_NO_COVERAGE).  state: RRT_COVERAGE_ON when that frame ran with a mask, else why not.
 * n_waves: the 4x4-pixel waves of that frame (0 without a mask).  n_proved_empty: how many of them the mask proved empty -- asked for with a non-NULL
 * pointer only, and then BLOCKING: it waits for that frame and reads its mask back (the launch path never does).  Any pointer may be NULL. */
#define RRT_COVERAGE_ON 0u
#define RRT_COVERAGE_OFF_NO_FRAME 1u     /* no frame has been launched yet */
#define RRT_COVERAGE_OFF_FLAG 2u         /* RRT_FLAG_NO_COVERAGE */
#define RRT_COVERAGE_OFF_NO_CULL 3u      /* RRT_FLAG_NO_CULL, or an index without padding: there are no boxes to trust */
#define RRT_COVERAGE_OFF_SUSPECTS 4u     /* rrt_stats.origin_plane_triangles != 0: some primary rays run unfiltered */
#define RRT_COVERAGE_OFF_EYE_RANGE 5u    /* the eye, or a primary direction of the frame, lies outside the range of the index filters */
#define RRT_COVERAGE_OFF_CAMERA 6u       /* a view basis that is singular, ill-conditioned (condition above 256) or not finite, or a viewport depth <= 0 */
#define RRT_COVERAGE_OFF_POOL 7u         /* more than eight frames of this raytracer in flight on different streams */
#define RRT_COVERAGE_OFF_NOT_WHOLE 8u    /* a rank's tiles (rrt_render_tiles_device) or a progressive frame */
#define RRT_COVERAGE_OFF_SMALL_FRAME 9u  /* the pass would cost more than it saves: fewer than 49 152 waves (1024 x 768 pixels), or more than four triangle slots per wave (RRT_FLAG_COVERAGE_ALWAYS lifts both) */
int rrt_raytracer_get_coverage_info(const rrt_raytracer *rt, uint32_t *state, uint64_t *n_waves, uint64_t *n_proved_empty);
/* The mask itself of that frame, BLOCKING like n_proved_empty: n_words = (tiles_x * tiles_y + 7) / 8 words of 32 bits, tiles_x = (width + 7) / 8 and tiles_y =
 * (height + 7) / 8 of the frame.  Wave (bx, by) -- the pixels [4 bx, 4 bx + 3] x [4 by, 4 by + 3] -- is bit ((((by / 2) * tiles_x + bx / 2) * 4) | ((by & 1) * 2) |
 * (bx & 1)), counted from bit 0 of word 0; a set bit means the wave walked, a clear bit that it was proved empty.  The bits of the last word beyond the frame's
 * waves are 0.  RRT_ERR_INVALID_ARG for a NULL pointer, and for an n_words that is not that frame's.  When the last frame ran without a mask (state !=
 * RRT_COVERAGE_ON) nothing is written and the call returns RRT_OK.  A developer's and tests' view: no launch reads it back. */
int rrt_raytracer_get_coverage_mask(const rrt_raytracer *rt, uint32_t *words, uint64_t n_words);
/* The wide boxes of that frame (see RRT_FLAG_NO_WIDE_COVER), BLOCKING like n_proved_empty: n_wide = the boxes the pass listed (at most 16), n_simple_waves = the
 * waves that only listed boxes reach, whose primary rays the bundle-filter kernel tests against those triangles instead of walking.  Both 0 when the last frame ran without a mask
 * or with RRT_FLAG_NO_WIDE_COVER, and when some box reaches the whole frame (a corner not certainly in front of the eye): every wave is then ordinary and the
 * list, whatever the pass had put into it by then, is not used.  Either pointer may be NULL. */
int rrt_raytracer_get_wide_cover_info(const rrt_raytracer *rt, uint32_t *n_wide, uint64_t *n_simple_waves);

int rrt_last_stats(const rrt_raytracer *rt, rrt_stats *out);
/* Time of the set-up stages that run once per scene (the reference does all of them inside parse_obj_file_lines, utils.rs:139-213, before its one
 * frame): model side = file read, .obj/.mtl parse, texture decode; raytracer side = octree build (octree.rs:41-241), own-list index build, upload to
 * HBM.  With the default GPU set-up octree_ms and index_ms are HIP-event times on the build stream and upload_ms is the rest of
 * rrt_raytracer_create's wall time (pinned-staging uploads of triangles and textures, allocations, synchronisation); with RRT_FLAG_HOST_SETUP they
 * are host wall times (octree_ms: the model's host build).  hip_init_ms = bringing the device's HIP context up at the start of
 * rrt_raytracer_create (a one-off of the process, near 0 for every later raytracer); create_ms = wall time of the whole rrt_raytracer_create;
 * gpu_setup = 1.0 / 0.0.  Either handle may be NULL (its fields stay 0). */
typedef struct { double read_ms, parse_ms, texture_ms, octree_ms, index_ms, upload_ms, hip_init_ms, create_ms, gpu_setup; } rrt_setup_times;
int rrt_get_setup_times(const rrt_model *m, const rrt_raytracer *rt, rrt_setup_times *out);
int rrt_device_count(int *count);
const char *rrt_strerror(int status);
const char *rrt_last_error_detail(void);   /* thread-local text of the last failure */
const char *rrt_build_info(void);          /* offload arch, fp-contract mode */

#ifdef __cplusplus
}
#endif
#endif
