// ray_queries.cpp -- per-ray queries behind include/rrt.h: intersections, colours, occlusion, surface records, shading and ambient occlusion of ray records,
// records from kept hits, and the measurement of the variants on a resident batch (rrt_tune_rays_device).
// Every per-ray launch that does not measure is timed and recorded in one place (recorded_ray_launch); the device forms share device_ray_query, the host forms
// host_ray_query or, where a call has no rays of its own to measure on, a plane list of their own for with_call_planes (launches.hpp) over the mirrored structs
// (host_planes.hpp: mirror_planes).
#include <algorithm>
#include <cstring>

#include "launches.hpp"

namespace rrt {

// The device forms (rrt_intersect_rays_device, ...) never measure: the forced variant, else the one kept for per-ray calls, else the frame variant.
int device_rays_variant(const rrt_raytracer* rt) {
    if (rt->variant_forced) return rt->walk;
    return rt->walk_rays >= 0 ? rt->walk_rays : rt->walk;
}
// an rrt_ray_surface of arrays in device memory as the kernels' argument
static_assert(sizeof(RaySurfaceParams) == sizeof(rrt_ray_surface), "RaySurfaceParams mirrors rrt_ray_surface");
RaySurfaceParams ray_surface_params(const rrt_ray_surface& o) {
    return RaySurfaceParams{o.hit, o.t, o.u, o.v, o.tri, o.albedo, o.point, o.normal, o.material, o.lights, o.next_origin, o.next_dir};
}
// the kernels' argument from arrays in device memory
ShadeRaysParams shade_rays_params(const double* d_dirs, const rrt_ray_surface& d_rec, uint32_t depth, const rrt_ray_shade& d_out) {
    return ShadeRaysParams{d_dirs, d_rec.point, d_rec.normal, d_rec.material, d_rec.albedo, d_rec.lights, d_out.colour, d_out.local, d_out.kr, depth, 0u};
}

}  // namespace rrt

namespace {

using namespace rrt;

// every check of a per-ray call, before any GPU work; n == 0 is a no-op
void check_rays(const rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, bool outputs_ok) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (n && (!origins || !dirs)) throw Error{RRT_ERR_INVALID_ARG, "null ray origins or directions"};
    if (n && !outputs_ok) throw Error{RRT_ERR_INVALID_ARG, "null output: a device form and rrt_surface_rays need one output pointer at least, the other host forms every one of their outputs"};
}

// ---- per-ray queries.  The one recorded per-ray launch that does not measure: launch(variant) of n rays on `stream`, in the variant of the device forms.
template <class Launch> void recorded_ray_launch(rrt_raytracer* rt, uint32_t n, void* stream, Launch&& launch) {
    const int variant = device_rays_variant(rt);
    timed_launch(rt, stream, [&] { return launch(variant); });
    record(rt, n, 1, n, variant);
}
// The device forms (rrt.h: rrt_intersect_rays_device, ...): no allocation, no copy, no synchronisation; launch(variant) on the caller's stream.
// (device_ray_launch: the same for a call that has made its own checks -- rrt_shade_rays_device has no origins for check_rays)
template <class Launch> int device_ray_launch(rrt_raytracer* rt, uint32_t n, void* stream, Launch&& launch) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    recorded_ray_launch(rt, n, stream, launch);
    return RRT_OK;
}
template <class Launch> int device_ray_query(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, bool any_output, void* stream, Launch&& launch) {
    check_rays(rt, n, d_origins, d_dirs, any_output);
    return device_ray_launch(rt, n, stream, launch);
}
// The host forms: rays and the optional max_t up, launch(m, d_origins, d_dirs, d_max_t, d_out, variant) on the null stream (the variant by rays_variant, measured on a
// first large batch), every output down; blocking (with_call_planes).  out[k]: the caller's array of output k as a plane of n elements (plane_down).
// kEveryOutput: the call wants each of its outputs; kAnyOutput (rrt_surface_rays): one at least -- a null output gets no device memory, d_out[k] is null for the
// launch and nothing is downloaded for it.
enum OutputRule { kEveryOutput, kAnyOutput };
template <size_t K, class Launch>
int host_ray_query(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t, const HostPlane (&out)[K], Launch&& launch,
                   OutputRule rule = kEveryOutput) {
    bool every_output = true, any_output = false;
    for (const HostPlane& o : out) { every_output = every_output && o.host; any_output = any_output || o.host; }
    check_rays(rt, n, origins, dirs, rule == kAnyOutput ? any_output : every_output);
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    enum : size_t { kOrigins, kDirs, kMaxT, kOut };
    HostPlane pl[kOut + K] = {plane_up(origins, 24, n), plane_up(dirs, 24, n), plane_up(max_t, 8, n)};
    std::copy(out, out + K, pl + kOut);
    with_call_planes(pl, [&] {
        const double *d_o = (const double*)pl[kOrigins].dev, *d_d = (const double*)pl[kDirs].dev, *d_m = (const double*)pl[kMaxT].dev;
        void* d_out[K];
        for (size_t k = 0; k < K; k++) d_out[k] = pl[kOut + k].dev;
        const int variant = rays_variant(rt, n, [&](uint32_t m, int v) { return launch(m, d_o, d_d, d_m, d_out, v); });
        timed_launch(rt, nullptr, [&] { return launch(n, d_o, d_d, d_m, d_out, variant); });
        record(rt, n, 1, n, variant);
    });
    return RRT_OK;
}

// ---- the surface record of arbitrary rays (rrt.h: rrt_surface_rays).  The twelve arrays of an rrt_ray_surface in its order: host_planes.hpp, kRaySurfaceElem.
constexpr size_t kRec = kFields<rrt_ray_surface>;
using RecDirs = FieldDirs<rrt_ray_surface>;
// every check of the struct, before any GPU work; true: an array is asked for
bool ray_surface_wanted(const rrt_raytracer* rt, const rrt_ray_surface* out) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!out) throw Error{RRT_ERR_INVALID_ARG, "null ray surface struct"};
    return out->hit || out->t || out->u || out->v || out->tri || out->albedo || out->point || out->normal || out->material || out->lights || out->next_origin || out->next_dir;
}

// ---- shading of arbitrary rays from kept records (rrt.h: rrt_shade_rays).  every check, before any GPU work; n == 0 is a no-op for valid handles and structs
void check_shade_rays(const rrt_raytracer* rt, uint32_t n, const double* dirs, const rrt_ray_surface* rec, const rrt_ray_shade* out) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!rec || !out) throw Error{RRT_ERR_INVALID_ARG, "null struct: shading rays reads the ray surface struct and writes the ray shade struct"};
    if (n && !out->colour && !out->local && !out->kr) throw Error{RRT_ERR_INVALID_ARG, "no output requested: colour, local and kr are all null"};
    if (n && !dirs) throw Error{RRT_ERR_INVALID_ARG, "null ray directions"};
    if (n && (!rec->albedo || !rec->point || !rec->normal || !rec->material)) throw Error{RRT_ERR_INVALID_ARG, "null array: albedo, point, normal and material are all required"};
}
// Host form (checked), for a call without origins: the directions and the four or five arrays it reads up, one launch on the null stream in the variant of the
// device forms -- nothing is measured: there are no origins to measure a walk on -- the requested outputs down; blocking (with_call_planes).  The list keeps the
// order point, normal, material, albedo, lights: the record lies in two runs of it.
int shade_rays_from_host(rrt_raytracer* rt, uint32_t n, const double* dirs, const rrt_ray_surface& rec, uint32_t depth, const rrt_ray_shade& out) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    const size_t N = n;
    enum : size_t { kDirs, kRecA, kRecB = kRecA + kRec, kOut = kRecB + kRec, kEnd = kOut + kFields<rrt_ray_shade> };
    HostPlane pl[kEnd];
    pl[kDirs] = plane_up(dirs, 24, N);
    mirror_planes(pl + kRecA, rec, N, RecDirs().set(kUp, &rrt_ray_surface::point, &rrt_ray_surface::normal, &rrt_ray_surface::material));
    mirror_planes(pl + kRecB, rec, N, RecDirs().set(kUp, &rrt_ray_surface::albedo, &rrt_ray_surface::lights));
    mirror_planes(pl + kOut, out, N, FieldDirs<rrt_ray_shade>::every(kDown));
    with_call_planes(pl, [&] {
        const ShadeRaysParams q = shade_rays_params((const double*)pl[kDirs].dev, mirrored<rrt_ray_surface>(pl + kRecA, pl + kRecB), depth, mirrored<rrt_ray_shade>(pl + kOut));
        recorded_ray_launch(rt, n, nullptr, [&](int variant) { return launch_shade_rays(rt->scene, n, q, nullptr, nullptr, variant); });
    });
    return RRT_OK;
}

// ---- ambient occlusion for ray records (rrt.h: rrt_ambient_rays).  every check, before any GPU work; the structs and the table are checked for n == 0 too
void check_ambient_rays(const rrt_raytracer* rt, uint32_t n, const rrt_ray_surface* rec, const rrt_ambient_samples* samples, const rrt_ray_ambient* out) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!rec || !samples || !out) throw Error{RRT_ERR_INVALID_ARG, "null struct: ambient occlusion of rays takes the ray surface struct, the sample table and the ray ambient struct"};
    if (n && (!rec->point || !rec->normal || !rec->material)) throw Error{RRT_ERR_INVALID_ARG, "null array: point, normal and material are all required"};
    if (n && !out->occluded && !out->open) throw Error{RRT_ERR_INVALID_ARG, "no output requested: occluded and open are both null"};
    check_ambient_samples(*samples);
}
// the kernels' argument from arrays in device memory.  The sample table is copied into it here: no device memory holds it.
AmbientRaysParams ambient_rays_params(const rrt_ray_surface& d_rec, const double* d_rot, const rrt_ambient_samples& samples, const rrt_ray_ambient& d_out) {
    AmbientRaysParams q{};
    q.point = d_rec.point; q.normal = d_rec.normal; q.material = d_rec.material;
    q.rot = d_rot;
    q.occluded = d_out.occluded; q.open = d_out.open;
    q.n_samples = samples.n; q.max_t = samples.max_t;
    std::memcpy(q.dirs, samples.dirs, sizeof(double) * 3 * samples.n);
    return q;
}
// Host form (checked): the three arrays and the optional rotations up, one launch on the null stream in the variant of the device forms -- nothing is measured --
// the requested outputs down; blocking (with_call_planes).
int ambient_rays_from_host(rrt_raytracer* rt, uint32_t n, const rrt_ray_surface& rec, const double* rot, const rrt_ambient_samples& samples, const rrt_ray_ambient& out) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    const size_t N = n;
    enum : size_t { kRecAt, kRot = kRecAt + kRec, kOut, kEnd = kOut + kFields<rrt_ray_ambient> };
    HostPlane pl[kEnd];
    mirror_planes(pl + kRecAt, rec, N, RecDirs().set(kUp, &rrt_ray_surface::point, &rrt_ray_surface::normal, &rrt_ray_surface::material));
    pl[kRot] = plane_up(rot, 16, N);
    mirror_planes(pl + kOut, out, N, FieldDirs<rrt_ray_ambient>::every(kDown));
    with_call_planes(pl, [&] {
        const AmbientRaysParams q = ambient_rays_params(mirrored<rrt_ray_surface>(pl + kRecAt), (const double*)pl[kRot].dev, samples, mirrored<rrt_ray_ambient>(pl + kOut));
        recorded_ray_launch(rt, n, nullptr, [&](int variant) { return launch_ambient_rays(rt->scene, n, q, nullptr, nullptr, variant); });
    });
    return RRT_OK;
}

// ---- surface records from kept hits (rrt.h: rrt_resolve_hits).  u and v are read for everything but point and material
bool resolve_reads_uv(const rrt_ray_surface& rec) { return rec.albedo || rec.normal || rec.lights || rec.next_origin || rec.next_dir; }
// every check, before any GPU work; n == 0 is a no-op for a valid handle and struct
void check_resolve_hits(const rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const rrt_ray_surface* rec) {
    if (!rt) throw Error{RRT_ERR_INVALID_ARG, "null raytracer"};
    if (!rec) throw Error{RRT_ERR_INVALID_ARG, "null struct: resolving hits reads t, u, v and tri of the ray surface struct and writes its other arrays"};
    if (n && !rec->albedo && !rec->point && !rec->normal && !rec->material && !rec->lights && !rec->next_origin && !rec->next_dir)
        throw Error{RRT_ERR_INVALID_ARG, "no output requested: albedo, point, normal, material, lights, next_origin and next_dir are all null"};
    if (n && (!origins || !dirs)) throw Error{RRT_ERR_INVALID_ARG, "null ray origins or directions"};
    if (n && (!rec->t || !rec->tri)) throw Error{RRT_ERR_INVALID_ARG, "null array: t and tri are required"};
    if (n && resolve_reads_uv(*rec) && (!rec->u || !rec->v)) throw Error{RRT_ERR_INVALID_ARG, "null array: u and v are required for every output but point and material"};
}
// the kernels' argument from arrays in device memory, with the triangle -> slot table of the scene in force
ResolveParams resolve_params(const rrt_raytracer* rt, const double* d_origins, const double* d_dirs, const rrt_ray_surface& d_rec) {
    const BuiltScene& G = rt->built;
    return ResolveParams{d_origins, d_dirs, d_rec.t, d_rec.u, d_rec.v, d_rec.tri, G.tri_slot, G.n_tris, G.n_slots_total,
                         d_rec.albedo, d_rec.point, d_rec.normal, d_rec.material, d_rec.lights, d_rec.next_origin, d_rec.next_dir};
}
// Host form (checked): the rays, t, tri and -- where something asked for reads them -- u and v up, one launch on the null stream in the variant of the device
// forms -- nothing is measured -- the requested outputs down; blocking (with_call_planes).
int resolve_hits_from_host(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const rrt_ray_surface& rec) {
    if (n == 0) return RRT_OK;
    DeviceGuard guard(rt->device);
    const size_t N = n;
    const bool uv = resolve_reads_uv(rec);
    enum : size_t { kOrigins, kDirs, kRecAt, kEnd = kRecAt + kRec };
    HostPlane pl[kEnd];
    pl[kOrigins] = plane_up(origins, 24, N); pl[kDirs] = plane_up(dirs, 24, N);
    mirror_planes(pl + kRecAt, rec, N, RecDirs::every(kDown).set(kSkip, &rrt_ray_surface::hit).set(kUp, &rrt_ray_surface::t, &rrt_ray_surface::tri)
                                                           .set(uv ? kUp : kSkip, &rrt_ray_surface::u, &rrt_ray_surface::v));
    with_call_planes(pl, [&] {
        const ResolveParams q = resolve_params(rt, (const double*)pl[kOrigins].dev, (const double*)pl[kDirs].dev, mirrored<rrt_ray_surface>(pl + kRecAt));
        recorded_ray_launch(rt, n, nullptr, [&](int variant) { return launch_resolve_hits(rt->scene, n, q, nullptr, nullptr, variant); });
    });
    return RRT_OK;
}

}  // namespace

extern "C" {

int rrt_get_ray_colours(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, uint32_t* colours) {
    return guarded([&]() -> int {
        const HostPlane out[] = {plane_down(colours, 4, n)};
        return host_ray_query(rt, n, origins, dirs, nullptr, out, [&](uint32_t m, const double* o, const double* d, const double*, void* const* x, int variant) {
            return launch_ray_colours(rt->scene, m, o, d, (uint32_t*)x[0], nullptr, nullptr, variant);
        });
    });
}

// (the host form wants all five outputs; rrt_intersect_rays_device writes the ones it is given)
int rrt_intersect_rays(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t,
                       uint8_t* hit, double* t, double* u, double* v, uint32_t* tri) {
    return guarded([&]() -> int {
        const HostPlane out[] = {plane_down(hit, 1, n), plane_down(t, 8, n), plane_down(u, 8, n), plane_down(v, 8, n), plane_down(tri, 4, n)};
        return host_ray_query(rt, n, origins, dirs, max_t, out, [&](uint32_t m, const double* o, const double* d, const double* mt, void* const* x, int variant) {
            return launch_intersect(rt->scene, m, o, d, mt, (uint8_t*)x[0], (double*)x[1], (double*)x[2], (double*)x[3], (uint32_t*)x[4], nullptr, nullptr, variant);
        });
    });
}

int rrt_occluded_rays(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t, uint8_t* occluded) {
    return guarded([&]() -> int {
        const HostPlane out[] = {plane_down(occluded, 1, n)};
        return host_ray_query(rt, n, origins, dirs, max_t, out, [&](uint32_t m, const double* o, const double* d, const double* mt, void* const* x, int variant) {
            return launch_occlusion(rt->scene, m, o, d, mt, (uint8_t*)x[0], nullptr, nullptr, variant);
        });
    });
}

// The device forms of the per-ray calls, and behind them their counted forms (rrt.h: COUNTED DEVICE FORMS): ONE body per call, the uncounted entry point gives it a
// null bound.  The bound is never looked at on the host: the same checks, the same grid, the same record.
int rrt_intersect_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const double* d_max_t,
                                      uint8_t* d_hit, double* d_t, double* d_u, double* d_v, uint32_t* d_tri, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, d_hit || d_t || d_u || d_v || d_tri, stream, [&](int variant) {
            return launch_intersect(rt->scene, n, d_origins, d_dirs, d_max_t, d_hit, d_t, d_u, d_v, d_tri, d_count, stream, variant);
        });
    });
}
int rrt_intersect_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t,
                              uint8_t* d_hit, double* d_t, double* d_u, double* d_v, uint32_t* d_tri, void* stream) {
    return rrt_intersect_rays_counted_device(rt, n, nullptr, d_origins, d_dirs, d_max_t, d_hit, d_t, d_u, d_v, d_tri, stream);
}

int rrt_get_ray_colours_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, uint32_t* d_colours, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, d_colours != nullptr, stream, [&](int variant) {
            return launch_ray_colours(rt->scene, n, d_origins, d_dirs, d_colours, d_count, stream, variant);
        });
    });
}
int rrt_get_ray_colours_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, uint32_t* d_colours, void* stream) {
    return rrt_get_ray_colours_counted_device(rt, n, nullptr, d_origins, d_dirs, d_colours, stream);
}

int rrt_occluded_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const double* d_max_t,
                                     uint8_t* d_occluded, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, d_occluded != nullptr, stream, [&](int variant) {
            return launch_occlusion(rt->scene, n, d_origins, d_dirs, d_max_t, d_occluded, d_count, stream, variant);
        });
    });
}
int rrt_occluded_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, uint8_t* d_occluded, void* stream) {
    return rrt_occluded_rays_counted_device(rt, n, nullptr, d_origins, d_dirs, d_max_t, d_occluded, stream);
}

int rrt_surface_rays(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const double* max_t, const rrt_ray_surface* out) {
    return guarded([&]() -> int {
        (void)ray_surface_wanted(rt, out);                                 // (whether one is asked for is host_ray_query's own check: kAnyOutput)
        HostPlane arrays[kRec];
        mirror_planes(arrays, *out, n, RecDirs::every(kDown));
        return host_ray_query(rt, n, origins, dirs, max_t, arrays, [&](uint32_t m, const double* o, const double* d, const double* mt, void* const* x, int variant) {
            rrt_ray_surface dev;
            std::memcpy(&dev, x, sizeof dev);
            return launch_surface_rays(rt->scene, m, o, d, mt, ray_surface_params(dev), nullptr, nullptr, variant);
        }, kAnyOutput);
    });
}

int rrt_surface_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const double* d_max_t,
                                    const rrt_ray_surface* d_out, void* stream) {
    return guarded([&]() -> int {
        return device_ray_query(rt, n, d_origins, d_dirs, ray_surface_wanted(rt, d_out), stream, [&](int variant) {
            return launch_surface_rays(rt->scene, n, d_origins, d_dirs, d_max_t, ray_surface_params(*d_out), d_count, stream, variant);
        });
    });
}
int rrt_surface_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, const rrt_ray_surface* d_out, void* stream) {
    return rrt_surface_rays_counted_device(rt, n, nullptr, d_origins, d_dirs, d_max_t, d_out, stream);
}

int rrt_shade_rays(rrt_raytracer* rt, uint32_t n, const double* dirs, const rrt_ray_surface* rec, uint32_t depth, const rrt_ray_shade* out) {
    return guarded([&]() -> int {
        check_shade_rays(rt, n, dirs, rec, out);
        return shade_rays_from_host(rt, n, dirs, *rec, depth, *out);
    });
}

int rrt_shade_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_dirs, const rrt_ray_surface* d_rec, uint32_t depth,
                                  const rrt_ray_shade* d_out, void* stream) {
    return guarded([&]() -> int {
        check_shade_rays(rt, n, d_dirs, d_rec, d_out);
        return device_ray_launch(rt, n, stream, [&](int variant) {
            return launch_shade_rays(rt->scene, n, shade_rays_params(d_dirs, *d_rec, depth, *d_out), d_count, stream, variant);
        });
    });
}
int rrt_shade_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_dirs, const rrt_ray_surface* d_rec, uint32_t depth, const rrt_ray_shade* d_out, void* stream) {
    return rrt_shade_rays_counted_device(rt, n, nullptr, d_dirs, d_rec, depth, d_out, stream);
}

int rrt_ambient_rays(rrt_raytracer* rt, uint32_t n, const rrt_ray_surface* rec, const double* rot, const rrt_ambient_samples* samples, const rrt_ray_ambient* out) {
    return guarded([&]() -> int {
        check_ambient_rays(rt, n, rec, samples, out);
        return ambient_rays_from_host(rt, n, *rec, rot, *samples, *out);
    });
}

int rrt_ambient_rays_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const rrt_ray_surface* d_rec, const double* d_rot,
                                    const rrt_ambient_samples* samples, const rrt_ray_ambient* d_out, void* stream) {
    return guarded([&]() -> int {
        check_ambient_rays(rt, n, d_rec, samples, d_out);
        return device_ray_launch(rt, n, stream, [&](int variant) {
            return launch_ambient_rays(rt->scene, n, ambient_rays_params(*d_rec, d_rot, *samples, *d_out), d_count, stream, variant);
        });
    });
}
int rrt_ambient_rays_device(rrt_raytracer* rt, uint32_t n, const rrt_ray_surface* d_rec, const double* d_rot, const rrt_ambient_samples* samples,
                            const rrt_ray_ambient* d_out, void* stream) {
    return rrt_ambient_rays_counted_device(rt, n, nullptr, d_rec, d_rot, samples, d_out, stream);
}

int rrt_resolve_hits(rrt_raytracer* rt, uint32_t n, const double* origins, const double* dirs, const rrt_ray_surface* rec) {
    return guarded([&]() -> int {
        check_resolve_hits(rt, n, origins, dirs, rec);
        return resolve_hits_from_host(rt, n, origins, dirs, *rec);
    });
}

int rrt_resolve_hits_counted_device(rrt_raytracer* rt, uint32_t n, const uint32_t* d_count, const double* d_origins, const double* d_dirs, const rrt_ray_surface* d_rec,
                                    void* stream) {
    return guarded([&]() -> int {
        check_resolve_hits(rt, n, d_origins, d_dirs, d_rec);
        return device_ray_launch(rt, n, stream, [&](int variant) {
            return launch_resolve_hits(rt->scene, n, resolve_params(rt, d_origins, d_dirs, *d_rec), d_count, stream, variant);
        });
    });
}
int rrt_resolve_hits_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const rrt_ray_surface* d_rec, void* stream) {
    return rrt_resolve_hits_counted_device(rt, n, nullptr, d_origins, d_dirs, d_rec, stream);
}

// Blocking: measure_rays on the first kTuneSample rays of a batch that is already on the device, whatever its size; the result replaces an earlier one.  The
// outputs go to an allocation of the raytracer's own, kept between calls.  The launches run on the null stream: the rays must be complete in memory.
int rrt_tune_rays_device(rrt_raytracer* rt, uint32_t n, const double* d_origins, const double* d_dirs, const double* d_max_t, uint32_t* variant_out) {
    return guarded([&]() -> int {
        check_rays(rt, n, d_origins, d_dirs, true);
        if (n && !rt->variant_forced) {
            DeviceGuard guard(rt->device);
            const uint32_t m = std::min(n, kTuneSample);
            constexpr size_t kBytes = (size_t)kTuneSample * (1 + 8 + 8 + 8 + 4);   // hit, t, u, v, tri of the largest sample (each a multiple of 256 bytes)
            DevArena arena{static_cast<char*>(rt->tune_buf.at_least(kBytes)), kBytes, 0};
            uint8_t* hit = arena.take<uint8_t>(m); double *t = arena.take<double>(m), *u = arena.take<double>(m), *v = arena.take<double>(m); uint32_t* tri = arena.take<uint32_t>(m);
            measure_rays(rt, [&](int variant) { return launch_intersect(rt->scene, m, d_origins, d_dirs, d_max_t, hit, t, u, v, tri, nullptr, nullptr, variant); });
        }
        if (variant_out) *variant_out = (uint32_t)device_rays_variant(rt);
        return (int)RRT_OK;
    });
}

}  // extern "C"
