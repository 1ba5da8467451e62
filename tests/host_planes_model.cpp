// Stand-alone check of csrc/host_planes.hpp, the pure part of the host forms (built and run by tests/test_host_planes_model.py; never loaded into Python).
//   host_planes_model  ->  one line "checks=... failures=..."; exit status 0 iff no check failed.
// No device: planes are carved out of a FAKE arena address that is never dereferenced, and host pointers are addresses inside one local buffer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "host_planes.hpp"

namespace {

using namespace rrt;

unsigned g_checks = 0, g_failures = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failures++; std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

char* const kArena = reinterpret_cast<char*>(uintptr_t{0x7000000000});   // 256-byte aligned; never dereferenced
char g_host[64 * 64];                                                       // host "arrays": distinct addresses, never read through a plane
void* host_array(size_t k) { return g_host + 64 * k; }

// ---- 1. the tables against rrt.h.  field k of S: `components` values of the type rrt.h declares for it per entry
template <class S, class T> void check_field(T* S::*field, size_t k, size_t components) {
    CHECK(field_of(field) == k);
    CHECK(k < kFields<S> && elem_table((const S*)nullptr)[k] == components * sizeof(std::remove_const_t<T>));
}
template <class S> void check_size() { CHECK(sizeof(S) == kFields<S> * sizeof(void*)); }
void check_record_fields() {   // (twice: as rrt_ray_surface, and behind the four arrays of an rrt_ray_set)
    using R = rrt_ray_surface;
    check_field(&R::hit, 0, 1); check_field(&R::t, 1, 1); check_field(&R::u, 2, 1); check_field(&R::v, 3, 1); check_field(&R::tri, 4, 1); check_field(&R::albedo, 5, 1);
    check_field(&R::point, 6, 3); check_field(&R::normal, 7, 3); check_field(&R::material, 8, 1); check_field(&R::lights, 9, 1);
    check_field(&R::next_origin, 10, 3); check_field(&R::next_dir, 11, 3);
}
void check_tables() {
    check_size<rrt_visibility>(); check_size<rrt_surface>(); check_size<rrt_ambient>(); check_size<rrt_ray_surface>();
    check_size<rrt_ray_shade>(); check_size<rrt_ray_ambient>(); check_size<rrt_ray_set>();
    using V = rrt_visibility;
    check_field(&V::hit, 0, 1); check_field(&V::t, 1, 1); check_field(&V::u, 2, 1); check_field(&V::v, 3, 1); check_field(&V::tri, 4, 1); check_field(&V::albedo, 5, 1);
    using S = rrt_surface;
    check_field(&S::point, 0, 3); check_field(&S::normal, 1, 3); check_field(&S::material, 2, 1); check_field(&S::lights, 3, 1);
    check_field(&rrt_ambient::occluded, 0, 1); check_field(&rrt_ambient::grey, 1, 1);
    check_record_fields();
    check_field(&rrt_ray_shade::colour, 0, 1); check_field(&rrt_ray_shade::local, 1, 3); check_field(&rrt_ray_shade::kr, 2, 1);
    check_field(&rrt_ray_ambient::occluded, 0, 1); check_field(&rrt_ray_ambient::open, 1, 1);
    using Q = rrt_ray_set;
    check_field(&Q::origins, 0, 3); check_field(&Q::dirs, 1, 3); check_field(&Q::max_t, 2, 1); check_field(&Q::rot, 3, 2);
    CHECK(field_of(&Q::rec) == 4 && kRaySetArrays == 4 + kFields<rrt_ray_surface>);
    for (size_t k = 0; k < kFields<rrt_ray_surface>; k++) CHECK(kRaySetElem[4 + k] == kRaySurfaceElem[k]);
    CHECK(kRaySetOrigins == field_of(&Q::origins) && kRaySetDirs == field_of(&Q::dirs) && kRaySetMaxT == field_of(&Q::max_t));
    CHECK(kRaySetPoint == 4 + field_of(&rrt_ray_surface::point) && kRaySetNormal == 4 + field_of(&rrt_ray_surface::normal) &&
          kRaySetMaterial == 4 + field_of(&rrt_ray_surface::material));
    CHECK(table_bytes(kVisibilityElem, 4) == 6 * 256);                 // (rrt_pick: six slots)
}

// ---- 2. planes_bytes and carve_planes
void check_carving() {
    HostPlane pl[] = {plane_up(host_array(0), 24, 100), plane_down(nullptr, 8, 100), plane_down(host_array(1), 1, 7), HostPlane{host_array(2), 4, 0, kCarve},
                      plane_up(host_array(3), 8, 32), plane_up(nullptr, 4, 0), plane_down(host_array(4), 4, 64)};
    const size_t need = planes_bytes(pl);
    size_t sum = 0;
    for (const HostPlane& p : pl) if (p.host) sum += slot_bytes(p.bytes());
    CHECK(need == sum && need == 2560 + 256 + 0 + 256 + 256);
    carve_planes(pl, kArena, need + 256);                              // (the empty plane takes a slot of its own)
    CHECK(!pl[1].dev && !pl[5].dev);                                   // null planes take nothing
    char* at = kArena;
    for (const HostPlane& p : pl) if (p.host) {                        // wanted planes in list order, at multiples of 256
        CHECK(p.dev == at && (reinterpret_cast<uintptr_t>(p.dev) & 255u) == 0);
        at += slot_bytes(p.bytes() ? p.bytes() : 1);
    }
    CHECK(pl[3].dev && pl[3].dev != pl[4].dev && pl[4].dev == static_cast<char*>(pl[3].dev) + 256);   // a plane of 0 bytes has an address of its own
    // a list without an empty plane fits planes_bytes exactly, and one byte less is refused
    HostPlane two[] = {plane_up(host_array(0), 24, 100), plane_down(host_array(1), 4, 65)};
    CHECK(planes_bytes(two) == 2560 + 512);
    carve_planes(two, kArena, 2560 + 512);
    CHECK(two[0].dev == kArena && two[1].dev == kArena + 2560);
    bool refused = false;
    try { carve_planes(two, kArena, 2560 + 511); } catch (const Error& e) { refused = e.status == RRT_ERR_OOM; }
    CHECK(refused);
}

// ---- 3. the mirrored device struct: the full set, and each field alone
template <class S> void check_mirror_case(const S& host, const FieldDirs<S>& want, const size_t (&count)[kFields<S>]) {
    constexpr size_t K = kFields<S>;
    HostPlane pl[K + 2];                                               // between two loose planes, as in a call's list
    pl[0] = plane_up(host_array(40), 24, 5);
    mirror_planes(pl + 1, host, count, want);
    pl[K + 1] = plane_down(host_array(41), 4, 5);
    carve_planes(pl, kArena, planes_bytes(pl));
    const S dev = mirrored<S>(pl + 1);
    void *h[K], *d[K];
    std::memcpy(h, &host, sizeof h); std::memcpy(d, &dev, sizeof d);
    char* at = kArena + slot_bytes(24 * 5);
    for (size_t k = 0; k < K; k++) {
        const bool wanted = h[k] && want.dir[k] != kSkip;
        CHECK(pl[1 + k].elem == elem_table(&host)[k] && pl[1 + k].count == count[k]);
        CHECK(pl[1 + k].host == (wanted ? h[k] : nullptr));
        CHECK(!wanted || pl[1 + k].dir == want.dir[k]);
        CHECK(d[k] == (wanted ? at : nullptr) && d[k] == pl[1 + k].dev);
        if (wanted) at += slot_bytes(elem_table(&host)[k] * count[k]);
    }
    CHECK(pl[K + 1].dev == at);
}
template <class S> void check_mirror(size_t n, size_t n_last) {        // n entries per field; n_last for the last one (rrt_ambient: grey is per pixel)
    constexpr size_t K = kFields<S>;
    void* h[K];
    size_t count[K];
    for (size_t k = 0; k < K; k++) { h[k] = host_array(k); count[k] = k + 1 == K ? n_last : n; }
    S full;
    std::memcpy(&full, h, sizeof full);
    const int dirs[] = {kUp, kDown, kUp | kDown, kCarve};
    for (int dir : dirs) check_mirror_case(full, FieldDirs<S>::every(dir), count);
    for (size_t one = 0; one < K; one++) {
        FieldDirs<S> only;                                             // the full struct, one field wanted ...
        only.dir[one] = kDown;
        check_mirror_case(full, only, count);
        void* single[K] = {};                                          // ... and every field wanted of a struct with one field set
        single[one] = h[one];
        S s;
        std::memcpy(&s, single, sizeof s);
        check_mirror_case(s, FieldDirs<S>::every(kUp), count);
    }
    // the form with one count for every field
    HostPlane a[K], b[K];
    size_t same[K];
    for (size_t k = 0; k < K; k++) same[k] = n;
    mirror_planes(a, full, n, FieldDirs<S>::every(kDown));
    mirror_planes(b, full, same, FieldDirs<S>::every(kDown));
    for (size_t k = 0; k < K; k++) CHECK(a[k].host == b[k].host && a[k].elem == b[k].elem && a[k].count == b[k].count && a[k].dir == b[k].dir);
}
// a struct whose planes lie in two runs of the list (rrt_shade_surface, rrt_shade_rays): each field from the run that carved it
void check_two_runs() {
    using R = rrt_ray_surface;
    constexpr size_t K = kFields<R>;
    void* h[K];
    for (size_t k = 0; k < K; k++) h[k] = host_array(k);
    R rec;
    std::memcpy(&rec, h, sizeof rec);
    HostPlane pl[2 * K];
    mirror_planes(pl, rec, 10, FieldDirs<R>().set(kUp, &R::point, &R::normal, &R::material));
    mirror_planes(pl + K, rec, 10, FieldDirs<R>().set(kUp, &R::albedo, &R::lights));
    carve_planes(pl, kArena, planes_bytes(pl));
    const R d = mirrored<R>(pl, pl + K);
    CHECK((char*)d.point == kArena && (char*)d.normal == kArena + 256 && (char*)d.material == kArena + 512 && (char*)d.albedo == kArena + 768 && (char*)d.lights == kArena + 1024);
    CHECK(!d.hit && !d.t && !d.u && !d.v && !d.tri && !d.next_origin && !d.next_dir);
    CHECK(planes_bytes(pl) == 5 * 256);
}

// ---- 4. the two ray sets of a compaction or a sort: an array named twice goes up once
size_t uploads(const HostPlane* pl, size_t at, size_t n) { size_t c = 0; for (size_t k = 0; k < n; k++) c += pl[at + k].host && (pl[at + k].dir & kUp); return c; }
void check_ray_sets() {
    enum : size_t { kScratch, kSrc, kDst = kSrc + kRaySetArrays, kEnd = kDst + kRaySetArrays };
    const size_t kNextOrigin = 4 + field_of(&rrt_ray_surface::next_origin), kNextDir = 4 + field_of(&rrt_ray_surface::next_dir);
    {   // the use rrt.h names: src.origins == src.rec.next_origin, src.dirs == src.rec.next_dir
        rrt_ray_set src{}, dst{};
        src.origins = src.rec.next_origin = static_cast<double*>(host_array(0));
        src.dirs = src.rec.next_dir = static_cast<double*>(host_array(1));
        dst.origins = static_cast<double*>(host_array(2)); dst.dirs = static_cast<double*>(host_array(3));
        dst.rec.next_origin = static_cast<double*>(host_array(4)); dst.rec.next_dir = static_cast<double*>(host_array(5));
        const RaySetArrays s = ray_set_arrays(&src), d = ray_set_arrays(&dst);
        bool read[kRaySetArrays];
        for (size_t k = 0; k < kRaySetArrays; k++) read[k] = d.p[k] != nullptr;
        HostPlane pl[kEnd];
        pl[kScratch] = HostPlane{g_host, 1, 8, kCarve};
        size_t from[kRaySetArrays];
        ray_set_planes(pl, kSrc, kDst, s, d, read, 50, from);
        CHECK(uploads(pl, kSrc, kRaySetArrays) == 2);                  // two uploads, not four
        CHECK(from[kNextOrigin] == kSrc + kRaySetOrigins && from[kNextDir] == kSrc + kRaySetDirs);
        CHECK(!pl[kSrc + kNextOrigin].host && !pl[kSrc + kNextDir].host);
        for (size_t k = 0; k < kRaySetArrays; k++) if (k != kNextOrigin && k != kNextDir) CHECK(from[k] == kSrc + k);
        carve_planes(pl, kArena, planes_bytes(pl));
        CHECK(pl[from[kNextOrigin]].dev == pl[kSrc + kRaySetOrigins].dev && pl[from[kNextOrigin]].dev != nullptr && !pl[kSrc + kNextOrigin].dev);
        CHECK(uploads(pl, kDst, kRaySetArrays) == 0 && pl[kDst + kNextOrigin].host == host_array(4) && pl[kDst + kNextOrigin].dir == kDown);
        CHECK(planes_bytes(pl) == 256 + 2 * slot_bytes(24 * 50) + 4 * slot_bytes(24 * 50));
        const RaySetArrays none = ray_set_arrays(nullptr);             // a NULL struct: sixteen NULLs
        for (void* p : none.p) CHECK(!p);
    }
    {   // equal pointers whose element sizes differ do not alias: max_t (8 bytes) and rot (16)
        rrt_ray_set src{};
        src.max_t = src.rot = static_cast<double*>(host_array(6));
        src.rec.t = static_cast<double*>(host_array(6));               // (8 bytes, as max_t: this one does alias)
        const RaySetArrays s = ray_set_arrays(&src), d = ray_set_arrays(nullptr);
        bool read[kRaySetArrays];
        for (size_t k = 0; k < kRaySetArrays; k++) read[k] = true;
        HostPlane pl[kEnd];
        pl[kScratch] = HostPlane{g_host, 1, 8, kCarve};
        size_t from[kRaySetArrays];
        ray_set_planes(pl, kSrc, kDst, s, d, read, 50, from);
        const size_t kRot = field_of(&rrt_ray_set::rot), kT = 4 + field_of(&rrt_ray_surface::t);
        CHECK(from[kRot] == kSrc + kRot && pl[kSrc + kRot].host == host_array(6) && pl[kSrc + kRaySetMaxT].host == host_array(6));
        CHECK(from[kT] == kSrc + kRaySetMaxT && !pl[kSrc + kT].host);
        CHECK(uploads(pl, kSrc, kRaySetArrays) == 2);
    }
    {   // an array that is there but not read is no plane, and nothing aliases it
        rrt_ray_set src{};
        src.origins = src.rec.next_origin = static_cast<double*>(host_array(0));
        const RaySetArrays s = ray_set_arrays(&src), d = ray_set_arrays(nullptr);
        bool read[kRaySetArrays] = {};
        read[kNextOrigin] = true;
        HostPlane pl[kEnd];
        pl[kScratch] = HostPlane{g_host, 1, 8, kCarve};
        size_t from[kRaySetArrays];
        ray_set_planes(pl, kSrc, kDst, s, d, read, 50, from);
        CHECK(!pl[kSrc + kRaySetOrigins].host && from[kNextOrigin] == kSrc + kNextOrigin && pl[kSrc + kNextOrigin].host == host_array(0));
    }
}

// ---- 5. a region of a frame, against the numbers of tests/test_gpu_launch_paths.py: W, H = 24, 17, region (3, 2, 9, 7)
template <class F> bool refuses(F&& f) { try { f(); } catch (const Error& e) { return e.status == RRT_ERR_INVALID_ARG; } return false; }
void check_regions() {
    const uint32_t W = 24, H = 17;
    const rrt_region R{3, 2, 9, 7};
    CHECK(traced_pixels(W, H) == 24 * 15 && traced_pixels_in(rrt_region{0, 0, W, H}, W, H) == 24 * 15);   // rows 0 and 1 are never traced
    CHECK(traced_pixels_in(R, W, H) == 9 * 7);
    CHECK(traced_pixels_in(rrt_region{12, 9, 1, 1}, W, H) == 1 && traced_pixels_in(rrt_region{0, 0, 1, 1}, W, H) == 0);
    CHECK(traced_pixels(25, 17) == 24 * 15 && traced_pixels(24, 16) == 24 * 15 && traced_pixels_in(rrt_region{24, 0, 1, 17}, 25, 17) == 0);   // an odd width's last column
    const rrt_region whole = region_in_force(W, H, nullptr), given = region_in_force(W, H, &R);
    CHECK(whole.x0 == 0 && whole.y0 == 0 && whole.w == W && whole.h == H);
    CHECK(given.x0 == 3 && given.y0 == 2 && given.w == 9 && given.h == 7);
    const FrameBatch rows = frame_batch(W, H, &R, RRT_ORDER_ROWS), tiles = frame_batch(W, H, &R, RRT_ORDER_TILES);
    CHECK(rows.n == 4 * 9 * 7 && rows.order == RRT_ORDER_ROWS && rows.r.x0 == 3 && rows.r.h == 7);
    CHECK(tiles.n == 64 * 3 * 3 && tiles.tile_x0 == 0 && tiles.tile_y0 == 0 && tiles.tiles_w == 3 && tiles.order == RRT_ORDER_TILES);
    CHECK(frame_batch(W, H, nullptr, RRT_ORDER_ROWS).n == 4 * 24 * 17 && frame_batch(W, H, nullptr, RRT_ORDER_TILES).n == 64 * 6 * 5);
    const rrt_region inner{9, 6, 4, 3};                                // tiles 2..3 x 1..2 of the frame
    const FrameBatch in = frame_batch(W, H, &inner, RRT_ORDER_TILES);
    CHECK(in.tile_x0 == 2 && in.tile_y0 == 1 && in.tiles_w == 2 && in.n == 64 * 2 * 2);
    // the refusals: an empty region, a protruding one, an unknown order, a bad frame size, more entries than a batch holds
    const rrt_region empty_w{3, 2, 0, 7}, empty_h{3, 2, 9, 0}, wide{16, 2, 9, 7}, tall{3, 11, 9, 7}, far{0xFFFFFFFFu, 0, 2, 1};
    for (const rrt_region* bad : {&empty_w, &empty_h, &wide, &tall, &far}) {
        CHECK(refuses([&] { (void)region_in_force(W, H, bad); }));
        CHECK(refuses([&] { (void)frame_batch(W, H, bad, RRT_ORDER_ROWS); }));
    }
    CHECK(refuses([&] { (void)frame_batch(W, H, &R, RRT_ORDER_TILES + 1); }));
    CHECK(refuses([&] { (void)frame_batch(0, H, nullptr, RRT_ORDER_ROWS); }) && refuses([&] { (void)frame_batch(W, 0, nullptr, RRT_ORDER_ROWS); }));
    CHECK(refuses([&] { (void)frame_batch(65536, 32768, nullptr, RRT_ORDER_ROWS); }));          // 2^31 pixels
    CHECK(refuses([&] { (void)frame_batch(46340, 46340, nullptr, RRT_ORDER_ROWS); }));          // a frame that is allowed, 4 entries per pixel: beyond 2^32 - 1
    CHECK(frame_batch(32768, 32767, nullptr, RRT_ORDER_ROWS).n == 4ull * 32768 * 32767);      // ... and the largest that fits
}

}  // namespace

int main() {
    check_tables();
    check_carving();
    check_mirror<rrt_visibility>(36, 36); check_mirror<rrt_surface>(36, 36); check_mirror<rrt_ambient>(36, 9); check_mirror<rrt_ray_surface>(100, 100);
    check_mirror<rrt_ray_shade>(100, 100); check_mirror<rrt_ray_ambient>(100, 100); check_mirror<rrt_ray_set>(50, 50);
    check_two_runs();
    check_ray_sets();
    check_regions();
    std::printf("checks=%u failures=%u\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
