// host_planes.hpp -- the pure part of the host forms: no HIP call; it needs include/rrt.h, the C++ library and two headers of one definition each (error.hpp,
// slots.hpp), so tests/host_planes_model.cpp compiles it alone with the host compiler.
//   A plane of the caller's in host memory and where it lives in one device allocation (HostPlane, planes_bytes, carve_planes).
//   The public pointer structs of rrt.h as plane lists: ONE table of bytes per entry for each, ONE routine that puts a struct's planes into a list
//   (mirror_planes) and gives the struct of device pointers back after the carving (mirrored); the two ray sets of a compaction or a sort (ray_set_planes).
//   A region of a frame: the region in force, the pixels traced in it, and the region as a batch of entries (frame_batch).
// The launches themselves, and the copies up and down, are in launches.hpp (with_kept_planes, with_call_planes) and the units behind it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/rrt.h"
#include "error.hpp"
#include "slots.hpp"

namespace rrt {

// ---- A plane of the caller's in host memory, and where it lives in a device allocation for one call.
enum : int { kSkip = -1, kCarve = 0, kUp = 1, kDown = 2 };   // copied host -> device before the launch, device -> host after it (kUp | kDown: both), or only carved;
                                                             // kSkip (a field of a struct only): not wanted, as a null pointer
struct HostPlane {
    void* host;              // the caller's pointer; null: the plane is not wanted, it gets no device memory and `dev` stays null
    size_t elem, count;      // bytes per element, elements
    int dir;
    void* dev = nullptr;
    size_t bytes() const { return elem * count; }
};
inline HostPlane plane_up(const void* host, size_t elem, size_t count) { return HostPlane{const_cast<void*>(host), elem, count, kUp}; }   // (an input is only read)
inline HostPlane plane_down(void* host, size_t elem, size_t count) { return HostPlane{host, elem, count, kDown}; }

// The two pure pieces of a host-form call: the device bytes the wanted planes of a list need, a slot each (slots.hpp: slot_bytes), and their carving out of
// `cap` bytes at `base` IN THE ORDER OF THE LIST.  (as DevArena::take: an empty plane still gets an address of its own)
template <size_t K> size_t planes_bytes(const HostPlane (&planes)[K]) {
    size_t need = 0;
    for (const HostPlane& p : planes) if (p.host) need += slot_bytes(p.bytes());
    return need;
}
template <size_t K> void carve_planes(HostPlane (&planes)[K], void* base, size_t cap) {
    size_t used = 0;
    for (HostPlane& p : planes) if (p.host) {
        const size_t bytes = slot_bytes(p.bytes() ? p.bytes() : 1);
        if (used + bytes > cap) throw Error{RRT_ERR_OOM, "internal: set-up arena too small"};
        p.dev = static_cast<char*>(base) + used; used += bytes;
    }
}

// ---- The public pointer structs: bytes per entry of every pointer, in field order.  (an entry: a sub-sample of a frame's plane, a ray of a batch)
constexpr size_t kVisibilityElem[] = {1, 8, 8, 8, 4, 4};                                        // hit, t, u, v, tri, albedo
constexpr size_t kSurfaceElem[] = {24, 24, 4, 4};                                               // point, normal, material, lights
constexpr size_t kAmbientElem[] = {4, 4};                                                       // occluded (per sub-sample), grey (PER PIXEL)
constexpr size_t kRaySurfaceElem[] = {1, 8, 8, 8, 4, 4, 24, 24, 4, 4, 24, 24};                  // the six of a visibility, the four of a surface, next_origin, next_dir
constexpr size_t kRayShadeElem[] = {4, 24, 8};                                                  // colour, local, kr
constexpr size_t kRayAmbientElem[] = {4, 4};                                                    // occluded, open
constexpr size_t kRaySetElem[] = {24, 24, 8, 16, 1, 8, 8, 8, 4, 4, 24, 24, 4, 4, 24, 24};       // origins, dirs, max_t, rot, the twelve of its record
template <size_t K> using ElemTable = const size_t (&)[K];
constexpr ElemTable<6> elem_table(const rrt_visibility*) { return kVisibilityElem; }
constexpr ElemTable<4> elem_table(const rrt_surface*) { return kSurfaceElem; }
constexpr ElemTable<2> elem_table(const rrt_ambient*) { return kAmbientElem; }
constexpr ElemTable<12> elem_table(const rrt_ray_surface*) { return kRaySurfaceElem; }
constexpr ElemTable<3> elem_table(const rrt_ray_shade*) { return kRayShadeElem; }
constexpr ElemTable<2> elem_table(const rrt_ray_ambient*) { return kRayAmbientElem; }
constexpr ElemTable<16> elem_table(const rrt_ray_set*) { return kRaySetElem; }
// the number of pointers of struct S
template <class S> constexpr size_t kFields = sizeof(elem_table((const S*)nullptr)) / sizeof(size_t);
static_assert(sizeof(rrt_visibility) == kFields<rrt_visibility> * sizeof(void*), "rrt_visibility is six pointers");
static_assert(sizeof(rrt_surface) == kFields<rrt_surface> * sizeof(void*), "rrt_surface is four pointers");
static_assert(sizeof(rrt_ambient) == kFields<rrt_ambient> * sizeof(void*), "rrt_ambient is two pointers");
static_assert(sizeof(rrt_ray_surface) == kFields<rrt_ray_surface> * sizeof(void*), "rrt_ray_surface is twelve pointers");
static_assert(sizeof(rrt_ray_shade) == kFields<rrt_ray_shade> * sizeof(void*), "rrt_ray_shade is three pointers");
static_assert(sizeof(rrt_ray_ambient) == kFields<rrt_ray_ambient> * sizeof(void*), "rrt_ray_ambient is two pointers");
static_assert(sizeof(rrt_ray_set) == kFields<rrt_ray_set> * sizeof(void*), "rrt_ray_set is sixteen pointers");
// the device bytes of all the planes of a struct, n entries each: a slot per plane
template <size_t K> constexpr size_t table_bytes(const size_t (&elem)[K], size_t n) {
    size_t bytes = 0;
    for (size_t k = 0; k < K; k++) bytes += slot_bytes(elem[k] * n);
    return bytes;
}

// The position of a field among the pointers of its struct, from its name: field_of(&rrt_surface::material) == 2.
template <class S, class T> size_t field_of(T S::*field) {
    const S s{};
    return (size_t)(reinterpret_cast<const char*>(&(s.*field)) - reinterpret_cast<const char*>(&s)) / sizeof(void*);
}
// A direction per field of S.  None is wanted at first; set(dir, &S::a, &S::b, ...) gives the named fields a direction, every(dir) all of them.
template <class S> struct FieldDirs {
    int dir[kFields<S>];
    FieldDirs() { std::fill(dir, dir + kFields<S>, (int)kSkip); }
    template <class... T> FieldDirs& set(int d, T S::*... field) { ((dir[field_of(field)] = d), ...); return *this; }
    static FieldDirs every(int d) { FieldDirs f; std::fill(f.dir, f.dir + kFields<S>, d); return f; }
};

// THE mirroring routine.  The planes of host struct `s` into pl[0, kFields<S>), field k's into pl[k]: count[k] entries (or n, for every field) of its table's
// bytes, in direction want.dir[k].  A field that is null or not wanted is no plane: it gets no device memory and its device pointer is null.
template <class S> void mirror_planes(HostPlane* pl, const S& s, const size_t (&count)[kFields<S>], const FieldDirs<S>& want) {
    void* host[kFields<S>];
    std::memcpy(host, &s, sizeof host);
    for (size_t k = 0; k < kFields<S>; k++)
        pl[k] = HostPlane{want.dir[k] == kSkip ? nullptr : host[k], elem_table(&s)[k], count[k], want.dir[k] == kSkip ? (int)kCarve : want.dir[k]};
}
template <class S> void mirror_planes(HostPlane* pl, const S& s, size_t n, const FieldDirs<S>& want) {
    size_t count[kFields<S>];
    std::fill(count, count + kFields<S>, n);
    mirror_planes(pl, s, count, want);
}
// ... and, after the carving, the struct of device pointers of the planes at pl[0, kFields<S>).  Of a struct whose planes lie in two runs of the list (a call's
// planes keep their order where it is not the struct's), each field is in one run at most: the one that carved it gives the pointer.
template <class S> S mirrored(const HostPlane* pl) {
    void* dev[kFields<S>];
    for (size_t k = 0; k < kFields<S>; k++) dev[k] = pl[k].dev;
    S d;
    std::memcpy(&d, dev, sizeof d);
    return d;
}
template <class S> S mirrored(const HostPlane* pl, const HostPlane* pl_more) {
    void* dev[kFields<S>];
    for (size_t k = 0; k < kFields<S>; k++) dev[k] = pl[k].dev ? pl[k].dev : pl_more[k].dev;
    S d;
    std::memcpy(&d, dev, sizeof d);
    return d;
}

// ---- The two ray sets of a compaction or a sort.  The sixteen arrays of an rrt_ray_set in its order (kRaySetElem): the positions the host code names ...
constexpr size_t kRaySetArrays = kFields<rrt_ray_set>;
constexpr size_t kRaySetOrigins = 0, kRaySetDirs = 1, kRaySetMaxT = 2, kRaySetPoint = 4 + 6, kRaySetNormal = 4 + 7, kRaySetMaterial = 4 + 8;
// ... and the struct as an array of pointers (a NULL struct: sixteen NULLs)
struct RaySetArrays { void* p[kRaySetArrays]; };
inline RaySetArrays ray_set_arrays(const rrt_ray_set* s) {
    RaySetArrays a{};
    if (s) std::memcpy(a.p, s, sizeof a.p);
    return a;
}
// The planes of two ray sets of N entries into pl[at_src, at_src + 16) and pl[at_dst, at_dst + 16): of src what the call reads (read[k], and the array is there) goes
// up, of dst what is set comes down.  A host array that src names twice goes up once: the later entry is no plane of the list and reads the device copy of the
// earlier one, from[k] (its own plane otherwise).
inline void ray_set_planes(HostPlane* pl, size_t at_src, size_t at_dst, const RaySetArrays& src, const RaySetArrays& dst, const bool (&read)[kRaySetArrays], size_t N,
                           size_t (&from)[kRaySetArrays]) {
    for (size_t k = 0; k < kRaySetArrays; k++) {
        const bool up = src.p[k] && read[k];
        from[k] = at_src + k;
        for (size_t e = 0; up && e < k; e++) if (pl[at_src + e].host == src.p[k] && kRaySetElem[e] == kRaySetElem[k]) from[k] = at_src + e;
        pl[at_src + k] = plane_up(up && from[k] == at_src + k ? src.p[k] : nullptr, kRaySetElem[k], N);
        pl[at_dst + k] = plane_down(dst.p[k], kRaySetElem[k], N);
    }
}

// ---- A region of a frame.  The region in force: the caller's, or the whole frame; the last check of every region call, after those of its own arguments.
inline rrt_region region_in_force(uint32_t width, uint32_t height, const rrt_region* region) {
    const rrt_region r = region ? *region : rrt_region{0, 0, width, height};
    if (r.w == 0 || r.h == 0) throw Error{RRT_ERR_INVALID_ARG, "empty region"};
    if ((uint64_t)r.x0 + r.w > width || (uint64_t)r.y0 + r.h > height) throw Error{RRT_ERR_INVALID_ARG, "region sticks out of the frame"};
    return r;
}
// traced pixels (render_kernel): columns [0, 2*(W/2)), rows [H - 2*(H/2) + 1, H) -- of a region, and of the whole frame
inline uint64_t traced_pixels_in(const rrt_region& r, uint32_t width, uint32_t height) {
    const uint64_t col_end = std::min<uint64_t>((uint64_t)r.x0 + r.w, 2ull * (width / 2)), row_begin = std::max<uint64_t>(r.y0, (uint64_t)height - 2ull * (height / 2) + 1);
    const uint64_t cols = col_end > r.x0 ? col_end - r.x0 : 0, rows = (uint64_t)r.y0 + r.h > row_begin ? (uint64_t)r.y0 + r.h - row_begin : 0;
    return cols * rows;
}
inline uint64_t traced_pixels(uint32_t width, uint32_t height) { return traced_pixels_in(rrt_region{0, 0, width, height}, width, height); }
// A region of a frame as a batch of entries: the region in force, the rectangle of 4x4-pixel tiles of the FRAME it touches, and the number of entries in the order.
struct FrameBatch { rrt_region r; uint32_t order, tile_x0, tile_y0, tiles_w; uint64_t n; };
// no handle is looked at; throws what the region calls throw, and for an unknown order or a batch beyond the uint32 n of the per-ray calls
inline FrameBatch frame_batch(uint32_t width, uint32_t height, const rrt_region* region, uint32_t order) {
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7FFFFFFFull) throw Error{RRT_ERR_INVALID_ARG, "bad frame size"};
    if (order > RRT_ORDER_TILES) throw Error{RRT_ERR_INVALID_ARG, "unknown order: want RRT_ORDER_ROWS or RRT_ORDER_TILES"};
    FrameBatch b{};
    b.r = region_in_force(width, height, region);
    b.order = order; b.tile_x0 = b.r.x0 / 4; b.tile_y0 = b.r.y0 / 4;
    b.tiles_w = (b.r.x0 + b.r.w + 3) / 4 - b.tile_x0;
    const uint32_t tiles_h = (b.r.y0 + b.r.h + 3) / 4 - b.tile_y0;
    b.n = order == RRT_ORDER_ROWS ? 4ull * b.r.w * b.r.h : 64ull * b.tiles_w * tiles_h;
    if (b.n > 0xFFFFFFFFull) throw Error{RRT_ERR_INVALID_ARG, "the region has more entries than a ray batch can hold (2^32 - 1)"};
    return b;
}

}  // namespace rrt
