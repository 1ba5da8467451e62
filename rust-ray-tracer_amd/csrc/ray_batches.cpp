// ray_batches.cpp -- ray batches between two per-ray stages, behind include/rrt.h: compaction of batches and records and its inverse (compact.hip), their sort
// by a coherence key (sort.hip), the two ends of that pipeline -- a frame's primary rays as a batch, the unwind of one level, the pixels (wavefront.hip) -- and
// the frame by ray generations that strings the stages together.  No ray is traced by the first three groups: they go past timed_launch and record.
// Their host forms share with_call_planes (launches.hpp); the two ray sets of a compaction or a sort become planes in ray_set_planes (host_planes.hpp).
#include <algorithm>
#include <cstring>

#include "launches.hpp"

namespace {

using namespace rrt;

// ---- compaction of ray batches and records, and its inverse (rrt.h: rrt_compact_rays, rrt_scatter_rays).  These are not ray calls: no timed_launch, no record.
// The sixteen arrays of an rrt_ray_set in its order, as bytes per entry and as an array of pointers: host_planes.hpp (kRaySetElem, RaySetArrays); here, as the
// kernels' argument
static_assert(sizeof(RaySetPtrs) == sizeof(rrt_ray_set), "RaySetPtrs mirrors rrt_ray_set");
RaySetPtrs ray_set_ptrs(const RaySetArrays& a) {
    RaySetPtrs q;
    std::memcpy(&q, a.p, sizeof q);
    return q;
}
size_t compact_scratch_bytes(uint32_t n) { return n ? sizeof(uint32_t) * ((size_t)compact_tiles(n) + 1) : 0; }
// every check of a compaction but the scratch's, before any GPU work and before the handle is looked at
void check_compact(const rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* flag, const RaySetArrays& src, const RaySetArrays& dst,
                   const uint32_t* index, const uint32_t* count) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (select > RRT_SELECT_FLAG) throw Error{RRT_ERR_INVALID_ARG, "unknown select: want RRT_SELECT_HIT, RRT_SELECT_MIRROR or RRT_SELECT_FLAG"};
    if (n == 0) return;
    if (select == RRT_SELECT_FLAG ? !flag : !src.p[kRaySetMaterial])
        throw Error{RRT_ERR_INVALID_ARG, select == RRT_SELECT_FLAG ? "null flag array: RRT_SELECT_FLAG reads it" : "null src.rec.material: RRT_SELECT_HIT and RRT_SELECT_MIRROR read it"};
    bool any_output = index || count;
    for (size_t k = 0; k < kRaySetArrays; k++) {
        if (dst.p[k] && !src.p[k] && k != kRaySetMaxT) throw Error{RRT_ERR_INVALID_ARG, "an array of dst without its array of src (only max_t may be synthesised)"};
        any_output = any_output || dst.p[k];
    }
    if (!any_output) throw Error{RRT_ERR_INVALID_ARG, "no output requested: index, count and every array of dst are null"};
}
// the kernels' argument from arrays in device memory (checked)
CompactParams compact_params(const rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* d_flag, const RaySetArrays& d_src, const RaySetArrays& d_dst,
                             uint32_t* d_index, void* d_scratch) {
    CompactParams q{};
    q.src = ray_set_ptrs(d_src); q.dst = ray_set_ptrs(d_dst);
    q.flag = d_flag; q.mats = rt->scene.mats;
    q.index = d_index; q.tiles = static_cast<uint32_t*>(d_scratch);
    q.n = n; q.select = select; q.n_mats = rt->scene.n_mats;
    for (void* p : d_dst.p) if (p) q.any_dst = 1u;
    return q;
}
// Host form (checked): what the call reads up -- the src array of every dst array, the materials or the flags -- the three launches on the null stream, the
// requested outputs down; blocking (with_call_planes: the scratch is its first plane).  A host array that src names twice (the intended use: next_origin as
// origins, next_dir as dirs) goes up once: the later entry is no plane of the list and reads the device copy of the earlier one, from[k].
int compact_from_host(rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* flag, const RaySetArrays& src, const RaySetArrays& dst, uint32_t* index, uint32_t* count) {
    if (n == 0) { if (count) *count = 0; return RRT_OK; }
    DeviceGuard guard(rt->device);
    const size_t N = n;
    enum : size_t { kScratch, kSrc, kDst = kSrc + kRaySetArrays, kFlag = kDst + kRaySetArrays, kIndex, kCount, kEnd };
    HostPlane pl[kEnd];
    pl[kScratch] = HostPlane{rt, 1, compact_scratch_bytes(n), kCarve};     // (only carved: a host pointer that is not null says it is wanted)
    size_t from[kRaySetArrays];
    bool read[kRaySetArrays];
    for (size_t k = 0; k < kRaySetArrays; k++) read[k] = dst.p[k] || (k == kRaySetMaterial && select != RRT_SELECT_FLAG);
    ray_set_planes(pl, kSrc, kDst, src, dst, read, N, from);
    pl[kFlag] = plane_up(select == RRT_SELECT_FLAG ? flag : nullptr, 1, N); pl[kIndex] = plane_down(index, 4, N); pl[kCount] = plane_down(count, 4, 1);
    with_call_planes(pl, [&] {
        RaySetArrays d_src{}, d_dst{};
        for (size_t k = 0; k < kRaySetArrays; k++) { d_src.p[k] = pl[from[k]].dev; d_dst.p[k] = pl[kDst + k].dev; }
        const CompactParams q = compact_params(rt, n, select, (const uint8_t*)pl[kFlag].dev, d_src, d_dst, (uint32_t*)pl[kIndex].dev, pl[kScratch].dev);
        HIP_TRY((hipError_t)launch_compact(q, nullptr, (uint32_t*)pl[kCount].dev, nullptr));
    });
    return RRT_OK;
}
// every check of a scatter, before any GPU work and before the handle is looked at
void check_scatter(const rrt_raytracer* rt, uint32_t n, const uint32_t* index, uint32_t elem_bytes, const void* src, const void* dst) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16 && elem_bytes != 24) throw Error{RRT_ERR_INVALID_ARG, "bad elem_bytes: want 1, 4, 8, 16 or 24"};
    if (n && (!index || !src || !dst)) throw Error{RRT_ERR_INVALID_ARG, "null array: a scatter takes index, src and dst"};
}

// ---- stable sort of ray batches and records by a coherence key (rrt.h: rrt_sort_rays; sort.hip).  Not ray calls either.
size_t sort_scratch_bytes(uint32_t n) { return sizeof(uint32_t) * sort_scratch_words(n); }
// the arrays of src the key mode reads
bool sort_key_reads(uint32_t key_mode, size_t k) {
    if (key_mode == RRT_SORT_KEY_RAY) return k == kRaySetOrigins || k == kRaySetDirs || k == kRaySetMaxT;
    if (key_mode == RRT_SORT_KEY_RECORD) return k == kRaySetPoint || k == kRaySetNormal || k == kRaySetMaterial;
    return false;
}
// every check of a sort but the scratch's, before any GPU work and before the handle is looked at
void check_sort(const rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* keys, const RaySetArrays& src, const RaySetArrays& dst, const uint32_t* index,
                const uint32_t* keys_out, const uint32_t* count) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (key_mode > RRT_SORT_KEY_RECORD) throw Error{RRT_ERR_INVALID_ARG, "unknown key mode: want RRT_SORT_KEY_GIVEN, RRT_SORT_KEY_RAY or RRT_SORT_KEY_RECORD"};
    if (n == 0) return;
    if (key_mode == RRT_SORT_KEY_GIVEN && !keys) throw Error{RRT_ERR_INVALID_ARG, "null keys: RRT_SORT_KEY_GIVEN reads them"};
    if (key_mode == RRT_SORT_KEY_RAY && (!src.p[kRaySetOrigins] || !src.p[kRaySetDirs])) throw Error{RRT_ERR_INVALID_ARG, "null src.origins or src.dirs: RRT_SORT_KEY_RAY reads them"};
    if (key_mode == RRT_SORT_KEY_RECORD && (!src.p[kRaySetPoint] || !src.p[kRaySetNormal] || !src.p[kRaySetMaterial]))
        throw Error{RRT_ERR_INVALID_ARG, "null src.rec.point, .normal or .material: RRT_SORT_KEY_RECORD reads them"};
    bool any_output = index || keys_out || count;
    for (size_t k = 0; k < kRaySetArrays; k++) {
        if (dst.p[k] && !src.p[k]) throw Error{RRT_ERR_INVALID_ARG, "an array of dst without its array of src"};
        any_output = any_output || dst.p[k];
    }
    if (!any_output) throw Error{RRT_ERR_INVALID_ARG, "no output requested: index, keys_out, count and every array of dst are null"};
}
// the kernels' argument from arrays in device memory (checked): the key is formed with the root box in force now
SortParams sort_params(const rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* d_keys, const RaySetArrays& d_src, const RaySetArrays& d_dst,
                       uint32_t* d_index, uint32_t* d_keys_out, uint32_t* d_count, void* d_scratch) {
    SortParams q{};
    q.src = ray_set_ptrs(d_src); q.dst = ray_set_ptrs(d_dst);
    q.keys = d_keys; q.index = d_index; q.keys_out = d_keys_out; q.count = d_count; q.scratch = static_cast<uint32_t*>(d_scratch);
    q.n = n; q.key_mode = key_mode; q.n_mats = rt->scene.n_mats;
    for (int a = 0; a < 3; a++) { q.lo[a] = rt->root.lo[a]; q.scale[a] = 512.0 / (rt->root.hi[a] - rt->root.lo[a]); }
    return q;
}
// Host form (checked): what the call reads up -- the src array of every dst array, the arrays the key mode reads, the given keys -- the launches on the null stream,
// the requested outputs down; blocking (with_call_planes: the scratch is its first plane).
int sort_from_host(rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* keys, const RaySetArrays& src, const RaySetArrays& dst, uint32_t* index,
                   uint32_t* keys_out, uint32_t* count) {
    if (n == 0) { if (count) *count = 0; return RRT_OK; }
    DeviceGuard guard(rt->device);
    const size_t N = n;
    enum : size_t { kScratch, kSrc, kDst = kSrc + kRaySetArrays, kKeys = kDst + kRaySetArrays, kIndex, kKeysOut, kCount, kEnd };
    HostPlane pl[kEnd];
    pl[kScratch] = HostPlane{rt, 1, sort_scratch_bytes(n), kCarve};        // (only carved: a host pointer that is not null says it is wanted)
    size_t from[kRaySetArrays];
    bool read[kRaySetArrays];
    for (size_t k = 0; k < kRaySetArrays; k++) read[k] = dst.p[k] || sort_key_reads(key_mode, k);
    ray_set_planes(pl, kSrc, kDst, src, dst, read, N, from);
    pl[kKeys] = plane_up(key_mode == RRT_SORT_KEY_GIVEN ? keys : nullptr, 4, N);
    pl[kIndex] = plane_down(index, 4, N); pl[kKeysOut] = plane_down(keys_out, 4, N); pl[kCount] = plane_down(count, 4, 1);
    with_call_planes(pl, [&] {
        RaySetArrays d_src{}, d_dst{};
        for (size_t k = 0; k < kRaySetArrays; k++) { d_src.p[k] = pl[from[k]].dev; d_dst.p[k] = pl[kDst + k].dev; }
        const SortParams q = sort_params(rt, n, key_mode, (const uint32_t*)pl[kKeys].dev, d_src, d_dst, (uint32_t*)pl[kIndex].dev, (uint32_t*)pl[kKeysOut].dev,
                                         (uint32_t*)pl[kCount].dev, pl[kScratch].dev);
        HIP_TRY((hipError_t)launch_sort(q, nullptr));
    });
    return RRT_OK;
}

// ---- the two ends of the per-ray pipeline (rrt.h: rrt_frame_rays, rrt_mix_rays, rrt_mix_pixels; wavefront.hip) and the frame by ray generations that closes it
// (rrt_render_wavefront).  The first three are not ray calls: no timed_launch, no record.
// A region of a frame as a batch of entries: the region in force, the rectangle of 4x4-pixel tiles of the FRAME it touches, and the number of entries in the order.
// every check of a call that takes a frame, a region and an order, before any GPU work
FrameBatch check_frame_batch(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    check_frame(rt, width, height);
    return frame_batch(width, height, region, order);
}
// the kernels' arguments (checked): the frame as launch_frame forms it, the eye in force
FrameRaysParams frame_rays_params(const rrt_raytracer* rt, uint32_t width, uint32_t height, const FrameBatch& b, double* d_origins, double* d_dirs, double* d_max_t) {
    const FrameParams f = frame_params(rt, width, height, 0, 1, false);
    FrameRaysParams q{};
    q.width = width; q.height = height; q.x_scale = f.x_scale; q.y_scale = f.y_scale; q.z_value = f.z_value;
    for (int k = 0; k < 3; k++) { q.right[k] = f.right[k]; q.up[k] = f.up[k]; q.forward[k] = f.forward[k]; q.eye[k] = rt->scene.origin[k]; }
    q.x0 = b.r.x0; q.y0 = b.r.y0; q.w = b.r.w; q.h = b.r.h;
    q.tile_x0 = b.tile_x0; q.tile_y0 = b.tile_y0; q.tiles_w = b.tiles_w; q.order = b.order;
    q.n = (uint32_t)b.n;
    q.origins = d_origins; q.dirs = d_dirs; q.max_t = d_max_t;
    return q;
}
MixPixelsParams mix_pixels_params(uint32_t width, uint32_t height, const FrameBatch& b, const uint32_t* d_colours, void* d_fb) {
    return MixPixelsParams{width, height, b.r.x0, b.r.y0, b.r.w, b.r.h, b.tile_x0, b.tile_y0, b.tiles_w, b.order, d_colours, static_cast<uint32_t*>(d_fb)};
}
void check_mix_rays(const rrt_raytracer* rt, uint32_t n, const double* local, const uint32_t* colour) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (n && (!local || !colour)) throw Error{RRT_ERR_INVALID_ARG, "null array: a mix takes local and writes colour"};
}

// The frame by ray generations.  Its work memory, as byte offsets into the caller's allocation, every array in a slot of its own (slots.hpp: slot_bytes):
// the rays of the level in hand and of the next one (origins, dirs, max_t, twice), the record arrays a level's surface launch writes and its shade launch reads, the
// colours of two levels and the scattered colours of the level below, the compaction's scratch -- 228 bytes per entry -- and, KEPT PER LEVEL for the way back up,
// local, kr, material and the compaction's index: 40 bytes per entry and level.  The compactions' counts, a uint32 per level, share the scratch's slot.
constexpr uint32_t kMaxLevels = RRT_MAX_REFLECT + 1;
struct WavefrontWork {
    size_t origins[2], dirs[2], max_t[2];
    size_t albedo, point, normal, lights, next_origin, next_dir;
    size_t colour[2], reflected, scratch;
    size_t local[kMaxLevels], kr[kMaxLevels], material[kMaxLevels], index[kMaxLevels];
    size_t counts;                          // one uint32 per level, behind the scratch in its slot: c[k], the count of level k's compaction -- the bound of level k + 1
    size_t bytes;
};
WavefrontWork wavefront_work(uint64_t n, uint32_t levels) {
    WavefrontWork w{};
    size_t used = 0;
    auto take = [&](size_t bytes) { const size_t at = used; used += slot_bytes(bytes ? bytes : 1); return at; };
    for (int i = 0; i < 2; i++) { w.origins[i] = take(24 * n); w.dirs[i] = take(24 * n); w.max_t[i] = take(8 * n); w.colour[i] = take(4 * n); }
    w.albedo = take(4 * n); w.point = take(24 * n); w.normal = take(24 * n); w.lights = take(4 * n); w.next_origin = take(24 * n); w.next_dir = take(24 * n);
    w.reflected = take(4 * n);
    const size_t scratch = compact_scratch_bytes((uint32_t)n);                 // (a multiple of 4: the counts behind it, in its slot, are aligned)
    w.scratch = take(scratch + sizeof(uint32_t) * kMaxLevels); w.counts = w.scratch + scratch;
    for (uint32_t k = 0; k < levels; k++) { w.local[k] = take(24 * n); w.kr[k] = take(8 * n); w.material[k] = take(4 * n); w.index[k] = take(4 * n); }
    w.bytes = used;
    return w;
}
uint32_t wavefront_levels(const rrt_raytracer* rt) { return std::min(rt->scene.max_reflection_depth, (uint32_t)RRT_MAX_REFLECT) + 1; }

// every check but the work memory's, before any GPU work
FrameBatch check_wavefront(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, const void* fb) {
    const FrameBatch b = check_frame_batch(rt, width, height, region, order);
    if (!fb) throw Error{RRT_ERR_INVALID_ARG, "null framebuffer"};
    return b;
}
// The pipeline of batch b (checked) on `stream`, with d_work (checked) carved as wavefront_work says: generate; per level surface -> shade (local and kr only, with
// the mask: it walks nothing) -> compaction of the mirror hits' next rays into the next level's rays; back up, per level the colours of the level below scattered
// into source order and mixed in; the pixels.  Every launch has the grid of n, but from level 1 on each is COUNTED (rrt.h: COUNTED DEVICE FORMS) by a count the
// pipeline itself left in the work memory, c[k] = the count of level k's compaction: surface, shade and compaction of level k by c[k - 1] (the compaction writes
// c[k]), the scatter of level k by c[k], the mix of level k by c[k - 1].  Blocks beyond a bound leave at once, and what lies beyond it in the arrays is neither
// written nor read: a level whose predecessor left nothing alive costs its launches and nothing else.  Level 0, its mix and the pixels run uncounted.  Only
// launchers that the per-ray entry points use are called; one pair of events around all of it, one record.
void launch_wavefront(rrt_raytracer* rt, uint32_t width, uint32_t height, const FrameBatch& b, void* d_fb, void* d_work, void* stream) {
    const uint32_t n = (uint32_t)b.n, levels = wavefront_levels(rt), last = levels - 1;
    const WavefrontWork w = wavefront_work(n, levels);
    char* base = static_cast<char*>(d_work);
    auto f64 = [&](size_t at) { return reinterpret_cast<double*>(base + at); };
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t*>(base + at); };
    uint32_t* const counts = u32(w.counts);
    const int variant = device_rays_variant(rt);
    timed_launch(rt, stream, [&]() -> int {
        HIP_TRY((hipError_t)launch_frame_rays(frame_rays_params(rt, width, height, b, f64(w.origins[0]), f64(w.dirs[0]), f64(w.max_t[0])), stream));
        for (uint32_t k = 0; k <= last; k++) {
            const uint32_t cur = k & 1u, nxt = cur ^ 1u;
            rrt_ray_surface rec{};
            rec.albedo = u32(w.albedo); rec.point = f64(w.point); rec.normal = f64(w.normal); rec.material = u32(w.material[k]); rec.lights = u32(w.lights);
            if (k < last) { rec.next_origin = f64(w.next_origin); rec.next_dir = f64(w.next_dir); }
            const uint32_t* alive = k ? counts + (k - 1) : nullptr;          // the entries of this level: c[k - 1]; all n at level 0
            HIP_TRY((hipError_t)launch_surface_rays(rt->scene, n, f64(w.origins[cur]), f64(w.dirs[cur]), f64(w.max_t[cur]), ray_surface_params(rec), alive, stream, variant));
            const ShadeRaysParams shade = shade_rays_params(f64(w.dirs[cur]), rec, k, rrt_ray_shade{nullptr, f64(w.local[k]), f64(w.kr[k])});
            HIP_TRY((hipError_t)launch_shade_rays(rt->scene, n, shade, alive, stream, variant));
            if (k == last) break;
            RaySetArrays src{}, dst{};                                     // the next rays of the mirror hits become the rays of level k + 1; max_t is synthesised
            src.p[kRaySetOrigins] = rec.next_origin; src.p[kRaySetDirs] = rec.next_dir; src.p[kRaySetMaterial] = rec.material;
            dst.p[kRaySetOrigins] = f64(w.origins[nxt]); dst.p[kRaySetDirs] = f64(w.dirs[nxt]); dst.p[kRaySetMaxT] = f64(w.max_t[nxt]);
            HIP_TRY((hipError_t)launch_compact(compact_params(rt, n, RRT_SELECT_MIRROR, nullptr, src, dst, u32(w.index[k]), base + w.scratch), alive, counts + k, stream));
        }
        for (uint32_t k = levels; k-- > 0;) {                              // the unwind, innermost level first (raytracer.rs:85-101)
            const uint32_t* reflected = nullptr;
            if (k < last) {
                HIP_TRY((hipError_t)launch_scatter(n, counts + k, u32(w.index[k]), 4, u32(w.colour[(k + 1) & 1u]), u32(w.reflected), stream));
                reflected = u32(w.reflected);
            }
            HIP_TRY((hipError_t)launch_mix_rays(MixRaysParams{u32(w.material[k]), f64(w.local[k]), f64(w.kr[k]), reflected, u32(w.colour[k & 1u]), n, rt->scene.n_mats},
                                                k ? counts + (k - 1) : nullptr, stream));
        }
        return launch_mix_pixels(mix_pixels_params(width, height, b, u32(w.colour[0]), d_fb), stream);
    });
    record(rt, width, height, 4 * traced_pixels_in(b.r, width, height), variant);
}

}  // namespace

extern "C" {

size_t rrt_compact_scratch_bytes(uint32_t n) { return compact_scratch_bytes(n); }

int rrt_compact_rays(rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* flag, const rrt_ray_set* src, const rrt_ray_set* dst, uint32_t* index, uint32_t* count) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(src), d = ray_set_arrays(dst);
        check_compact(rt, n, select, flag, s, d, index, count);
        return compact_from_host(rt, n, select, flag, s, d, index, count);
    });
}

// (d_bound: the bound of the counted form, d_count_out: the call's output; the uncounted entry point gives a null bound)
int rrt_compact_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_bound, uint32_t select, const uint8_t* d_flag, const rrt_ray_set* d_src,
                                    const rrt_ray_set* d_dst, uint32_t* d_index, uint32_t* d_count_out, void* d_scratch, size_t scratch_bytes, void* stream) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(d_src), d = ray_set_arrays(d_dst);
        check_compact(rt, n, select, d_flag, s, d, d_index, d_count_out);
        if (d_bound && d_bound == d_count_out) throw Error{RRT_ERR_INVALID_ARG, "the bound and the output count are the same word: the scan would overwrite what later blocks read"};
        if (n == 0) return (int)RRT_OK;
        if (scratch_bytes < compact_scratch_bytes(n) || !d_scratch) throw Error{RRT_ERR_INVALID_ARG, "scratch too small or null: want rrt_compact_scratch_bytes(n) bytes of device memory"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_compact(compact_params(rt, n, select, d_flag, s, d, d_index, d_scratch), d_bound, d_count_out, stream));
        return (int)RRT_OK;
    });
}
int rrt_compact_rays_device(rrt_raytracer* rt, uint32_t n, uint32_t select, const uint8_t* d_flag, const rrt_ray_set* d_src, const rrt_ray_set* d_dst,
                            uint32_t* d_index, uint32_t* d_count, void* d_scratch, size_t scratch_bytes, void* stream) {
    return rrt_compact_rays_counted_device(rt, n, nullptr, select, d_flag, d_src, d_dst, d_index, d_count, d_scratch, scratch_bytes, stream);
}

int rrt_scatter_rays(rrt_raytracer* rt, uint32_t n, const uint32_t* index, uint32_t elem_bytes, const void* src, void* dst) {
    return guarded([&]() -> int {
        check_scatter(rt, n, index, elem_bytes, src, dst);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_up(index, 4, n), plane_up(src, elem_bytes, n), HostPlane{dst, elem_bytes, n, kUp | kDown}};   // (dst up too: the entries no index names keep their values)
        with_call_planes(pl, [&] { HIP_TRY((hipError_t)launch_scatter(n, nullptr, (const uint32_t*)pl[0].dev, elem_bytes, pl[1].dev, pl[2].dev, nullptr)); });
        return (int)RRT_OK;
    });
}

int rrt_scatter_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const uint32_t* d_index, uint32_t elem_bytes, const void* d_src, void* d_dst,
                                    void* stream) {
    return guarded([&]() -> int {
        check_scatter(rt, n, d_index, elem_bytes, d_src, d_dst);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_scatter(n, d_count, d_index, elem_bytes, d_src, d_dst, stream));
        return (int)RRT_OK;
    });
}
int rrt_scatter_rays_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_index, uint32_t elem_bytes, const void* d_src, void* d_dst, void* stream) {
    return rrt_scatter_rays_counted_device(rt, n, nullptr, d_index, elem_bytes, d_src, d_dst, stream);
}

size_t rrt_sort_scratch_bytes(uint32_t n) { return sort_scratch_bytes(n); }

int rrt_sort_rays(rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* keys, const rrt_ray_set* src, const rrt_ray_set* dst, uint32_t* index,
                  uint32_t* keys_out, uint32_t* count) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(src), d = ray_set_arrays(dst);
        check_sort(rt, n, key_mode, keys, s, d, index, keys_out, count);
        return sort_from_host(rt, n, key_mode, keys, s, d, index, keys_out, count);
    });
}

int rrt_sort_rays_device(rrt_raytracer* rt, uint32_t n, uint32_t key_mode, const uint32_t* d_keys, const rrt_ray_set* d_src, const rrt_ray_set* d_dst,
                         uint32_t* d_index, uint32_t* d_keys_out, uint32_t* d_count, void* d_scratch, size_t scratch_bytes, void* stream) {
    return guarded([&]() -> int {
        const RaySetArrays s = ray_set_arrays(d_src), d = ray_set_arrays(d_dst);
        check_sort(rt, n, key_mode, d_keys, s, d, d_index, d_keys_out, d_count);
        if (n == 0) return (int)RRT_OK;
        if (scratch_bytes < sort_scratch_bytes(n) || !d_scratch) throw Error{RRT_ERR_INVALID_ARG, "scratch too small or null: want rrt_sort_scratch_bytes(n) bytes of device memory"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_sort(sort_params(rt, n, key_mode, d_keys, s, d, d_index, d_keys_out, d_count, d_scratch), stream));
        return (int)RRT_OK;
    });
}

uint32_t rrt_frame_ray_count(uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    uint32_t n = 0;
    (void)guarded([&]() -> int { n = (uint32_t)frame_batch(width, height, region, order).n; return RRT_OK; });
    return n;
}

int rrt_frame_rays_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, double* d_origins, double* d_dirs, double* d_max_t,
                          void* stream) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!d_origins && !d_dirs && !d_max_t) throw Error{RRT_ERR_INVALID_ARG, "no array requested: origins, dirs and max_t are all null"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_frame_rays(frame_rays_params(rt, width, height, b, d_origins, d_dirs, d_max_t), stream));
        return RRT_OK;
    });
}

int rrt_frame_rays(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, double* origins, double* dirs, double* max_t) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!origins && !dirs && !max_t) throw Error{RRT_ERR_INVALID_ARG, "no array requested: origins, dirs and max_t are all null"};
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_down(origins, 24, b.n), plane_down(dirs, 24, b.n), plane_down(max_t, 8, b.n)};
        with_call_planes(pl, [&] {
            HIP_TRY((hipError_t)launch_frame_rays(frame_rays_params(rt, width, height, b, (double*)pl[0].dev, (double*)pl[1].dev, (double*)pl[2].dev), nullptr));
        });
        return RRT_OK;
    });
}

int rrt_mix_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const uint32_t* d_material, const double* d_local, const double* d_kr,
                                const uint32_t* d_reflected, uint32_t* d_colour, void* stream) {
    return guarded([&]() -> int {
        check_mix_rays(rt, n, d_local, d_colour);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_mix_rays(MixRaysParams{d_material, d_local, d_kr, d_reflected, d_colour, n, rt->scene.n_mats}, d_count, stream));
        return (int)RRT_OK;
    });
}
int rrt_mix_rays_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_material, const double* d_local, const double* d_kr, const uint32_t* d_reflected, uint32_t* d_colour,
                        void* stream) {
    return rrt_mix_rays_counted_device(rt, n, nullptr, d_material, d_local, d_kr, d_reflected, d_colour, stream);
}

int rrt_mix_rays(rrt_raytracer* rt, uint32_t n, const uint32_t* material, const double* local, const double* kr, const uint32_t* reflected, uint32_t* colour) {
    return guarded([&]() -> int {
        check_mix_rays(rt, n, local, colour);
        if (n == 0) return (int)RRT_OK;
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_up(material, 4, n), plane_up(local, 24, n), plane_up(kr, 8, n), plane_up(reflected, 4, n), plane_down(colour, 4, n)};
        with_call_planes(pl, [&] {
            HIP_TRY((hipError_t)launch_mix_rays(MixRaysParams{(const uint32_t*)pl[0].dev, (const double*)pl[1].dev, (const double*)pl[2].dev, (const uint32_t*)pl[3].dev,
                                                              (uint32_t*)pl[4].dev, n, rt->scene.n_mats}, nullptr, nullptr));
        });
        return (int)RRT_OK;
    });
}

int rrt_mix_pixels_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, const uint32_t* d_colours, void* d_fb, void* stream) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!d_colours || !d_fb) throw Error{RRT_ERR_INVALID_ARG, "null array: the pixels take colours and write a framebuffer"};
        DeviceGuard guard(rt->device);
        HIP_TRY((hipError_t)launch_mix_pixels(mix_pixels_params(width, height, b, d_colours, d_fb), stream));
        return RRT_OK;
    });
}

int rrt_mix_pixels(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, const uint32_t* colours, uint32_t* out_fb) {
    return guarded([&]() -> int {
        const FrameBatch b = check_frame_batch(rt, width, height, region, order);
        if (!colours || !out_fb) throw Error{RRT_ERR_INVALID_ARG, "null array: the pixels take colours and write a framebuffer"};
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {plane_up(colours, 4, b.n), plane_down(out_fb, 4, (size_t)b.r.w * b.r.h)};
        with_call_planes(pl, [&] { HIP_TRY((hipError_t)launch_mix_pixels(mix_pixels_params(width, height, b, (const uint32_t*)pl[0].dev, pl[1].dev), nullptr)); });
        return RRT_OK;
    });
}

size_t rrt_wavefront_work_bytes(const rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    size_t bytes = 0;
    (void)guarded([&]() -> int { bytes = wavefront_work(check_frame_batch(rt, width, height, region, order).n, wavefront_levels(rt)).bytes; return RRT_OK; });
    return bytes;
}

int rrt_render_wavefront_device(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, void* d_fb, void* d_work, size_t work_bytes,
                                void* stream) {
    return guarded([&]() -> int {
        const FrameBatch b = check_wavefront(rt, width, height, region, order, d_fb);
        if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 255u) || work_bytes < wavefront_work(b.n, wavefront_levels(rt)).bytes)
            throw Error{RRT_ERR_INVALID_ARG, "work memory null, not 256-byte aligned or too small: want rrt_wavefront_work_bytes(...) bytes of device memory"};
        DeviceGuard guard(rt->device);
        launch_wavefront(rt, width, height, b, d_fb, d_work, stream);
        return RRT_OK;
    });
}

int rrt_render_wavefront(rrt_raytracer* rt, uint32_t width, uint32_t height, const rrt_region* region, uint32_t order, uint32_t* out_fb) {
    return guarded([&]() -> int {
        const FrameBatch b = check_wavefront(rt, width, height, region, order, out_fb);
        DeviceGuard guard(rt->device);
        HostPlane pl[] = {HostPlane{rt, 1, wavefront_work(b.n, wavefront_levels(rt)).bytes, kCarve},   // (only carved: a host pointer that is not null says it is wanted)
                          plane_down(out_fb, 4, (size_t)b.r.w * b.r.h)};
        with_call_planes(pl, [&] { launch_wavefront(rt, width, height, b, pl[1].dev, pl[0].dev, nullptr); });
        return RRT_OK;
    });
}


}  // extern "C"
