// wavefront.hip -- the two ends of the per-ray pipeline (rrt.h: rrt_frame_rays_device, rrt_mix_rays_device, rrt_mix_pixels_device): the primary rays of a frame as a
// ray batch, one level of the reflection chain's unwind, and Color::mix of the sub-sample colours into pixels.  The stages between them are render.hip's per-ray
// kernels, compact.hip and sort.hip; ray_batches.cpp strings all of them into rrt_render_wavefront_device.
//
// Three bandwidth kernels, one lane per entry (mix_pixels_kernel: per pixel), no LDS, no atomics, no block that waits on another: the same bits on every run.
// They live here and not in render.hip because a helper shared with the frame kernels changes their register allocation (render.hip, above region_lane); the dozen
// lines of primary_direction and the four of the unwind are therefore RESTATED below, each under a comment that names the original, and
// tests/test_gpu_wavefront.py pins the two texts to each other bit for bit.  Compiled with the plain flags of compact.hip / sort.hip; floating-point contraction is
// off as everywhere (Makefile: FLAGS), and the bits depend on it.
#include <hip/hip_runtime.h>

#include "device_scene.hpp"

namespace rrt {

namespace {

constexpr uint32_t kBlock = 256;                   // entries (pixels) per block: four waves
constexpr uint64_t kNaNBits = 0x7FF8000000000000ull, kInfBits = 0x7FF0000000000000ull;   // max_t of a dead entry (compaction's dead value) and of a traced one
constexpr uint32_t kWhite = 0x00FFFFFFu;           // the reference's background (raytracer.rs:109-111)

static_assert(sizeof(FrameRaysParams) < 4096 && sizeof(MixRaysParams) < 4096 && sizeof(MixPixelsParams) < 4096, "the arguments must fit the 4 KB kernel-argument segment");

// ---- frame rays.  Entry e of the batch -> its canvas pixel and sub-sample (rrt.h: RRT_ORDER_ROWS / RRT_ORDER_TILES).  traced: the pixel lies in the region and is one
// of those the reference traces (render.hip: render_kernel); every other entry is dead.  x, y: the pixel's scene coordinates as render_kernel forms them.
struct Entry { bool traced; uint32_t sub; int32_t x, y; };
__device__ __forceinline__ Entry entry_of(const FrameRaysParams& P, uint32_t e) {
    const uint32_t sub = e & 3u, q = e >> 2;
    uint32_t px, py;
    bool in_region = true;
    if (P.order == 0u) {                            // rows: q = (py - y0) * w + (px - x0)
        const uint32_t ry = q / P.w;
        px = P.x0 + (q - ry * P.w); py = P.y0 + ry;
    } else {                                        // tiles: q = (tile of the tile rectangle, row-major) * 16 + (py & 3) * 4 + (px & 3)
        const uint32_t pix = q & 15u, tile = q >> 4, tyr = tile / P.tiles_w;
        px = (P.tile_x0 + (tile - tyr * P.tiles_w)) * 4u + (pix & 3u); py = (P.tile_y0 + tyr) * 4u + (pix >> 2);
        in_region = px >= P.x0 && px < P.x0 + P.w && py >= P.y0 && py < P.y0 + P.h;     // (the region lies inside the frame)
    }
    const int32_t W = (int32_t)P.width, H = (int32_t)P.height;
    const bool traced = in_region && (int32_t)px < 2 * (W / 2) && (int32_t)py >= H - 2 * (H / 2) + 1;   // render.hip: render_kernel, `traced`
    return Entry{traced, sub, (int32_t)px - W / 2, (H - H / 2) - (int32_t)py};
}
__device__ __forceinline__ double pick3(const double (&v)[3], uint32_t k) { return k == 0u ? v[0] : (k == 1u ? v[1] : v[2]); }
// Component k of the direction of a traced entry.  RESTATES render.hip: primary_direction -- the sub-samples (x,y),(x+.5,y),(x,y+.5),(x+.5,y+.5) of engine.rs:207-236,
// then (right*a + up*b) + forward*c, five operations, each rounded on its own (rrt.h: rrt_camera).
__device__ __forceinline__ double direction_component(const FrameRaysParams& P, const Entry& E, uint32_t k) {
    const double xd = (E.sub & 1u) ? ((double)E.x + 0.5) : (double)E.x;
    const double yd = (E.sub & 2u) ? ((double)E.y + 0.5) : (double)E.y;
    const double sa = xd * P.x_scale, sb = yd * P.y_scale, sc = P.z_value;
    return (pick3(P.right, k) * sa + pick3(P.up, k) * sb) + pick3(P.forward, k) * sc;
}
__device__ __forceinline__ double origin_value(const FrameRaysParams& P, const Entry& E, uint32_t k) { return E.traced ? pick3(P.eye, k) : 0.0; }
__device__ __forceinline__ double direction_value(const FrameRaysParams& P, const Entry& E, uint32_t k) { return E.traced ? direction_component(P, E, k) : 0.0; }
__device__ __forceinline__ uint64_t bound_bits(const Entry& E) { return E.traced ? kInfBits : kNaNBits; }

// A block covers kBlock consecutive entries: 3 * kBlock consecutive doubles of `origins` and of `dirs`, kBlock of `max_t`.  Every value is a function of its index
// alone, so no lane needs another lane's result to store wide.
// kWide (every requested array 16-byte aligned): the block's doubles are taken as 16-byte pairs and thread t stores the pairs t and t + kBlock of origins / dirs and
// the pair t of max_t -- a wave's store instruction covers 1 KB of consecutive bytes, against 8 bytes per lane at a 24-byte stride.  n is a multiple of 4 (rrt.h), so a
// pair lies inside the arrays with both doubles or with neither.
// !kWide (some array only 8-byte aligned): thread t stores the seven doubles of entry t.
// Which arrays are present is uniform across the launch (kernel arguments).
template <bool kWide> __global__ __launch_bounds__(kBlock) void frame_rays_kernel(const FrameRaysParams P) {
    const uint64_t first = (uint64_t)blockIdx.x * kBlock;                  // the block's first entry
    if constexpr (kWide) {
        if (P.origins || P.dirs) {
            for (uint32_t pair = threadIdx.x; pair < 3u * kBlock / 2u; pair += kBlock) {
                const uint32_t j = 2u * pair, ea = j / 3u, ka = j - 3u * ea, eb = (j + 1u) / 3u, kb = (j + 1u) - 3u * eb;   // the doubles j, j + 1 of the block
                if (first + ea >= P.n) break;
                const Entry A = entry_of(P, (uint32_t)(first + ea)), B = entry_of(P, (uint32_t)(first + eb));
                const size_t at = 3u * (size_t)first + j;
                if (P.origins) *reinterpret_cast<double2*>(P.origins + at) = make_double2(origin_value(P, A, ka), origin_value(P, B, kb));
                if (P.dirs) *reinterpret_cast<double2*>(P.dirs + at) = make_double2(direction_value(P, A, ka), direction_value(P, B, kb));
            }
        }
        if (P.max_t && threadIdx.x < kBlock / 2u) {
            const uint64_t e = first + 2u * threadIdx.x;
            if (e < P.n) {
                const ulonglong2 v = make_ulonglong2(bound_bits(entry_of(P, (uint32_t)e)), bound_bits(entry_of(P, (uint32_t)e + 1u)));
                *reinterpret_cast<ulonglong2*>(P.max_t + e) = v;
            }
        }
    } else {
        const uint64_t e = first + threadIdx.x;
        if (e >= P.n) return;
        const Entry E = entry_of(P, (uint32_t)e);
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) {
            if (P.origins) P.origins[3u * (size_t)e + k] = origin_value(P, E, k);
            if (P.dirs) P.dirs[3u * (size_t)e + k] = direction_value(P, E, k);
        }
        if (P.max_t) reinterpret_cast<uint64_t*>(P.max_t)[e] = bound_bits(E);
    }
}

// ---- one level of the unwind.  RESTATES render.hip: clamp_u8 -- clamp(0.0, 255.0) as u8 (raytracer.rs:97-108); NaN gives 0
__device__ __forceinline__ uint32_t clamp_u8(double x) {
    if (x < 0.0) x = 0.0;
    if (x > 255.0) x = 255.0;
    if (!(x > 0.0)) return 0;
    return (uint32_t)x;
}
// One lane per entry (rrt.h: rrt_mix_rays_device).  material: null = every entry is a hit; kr, reflected: either null = nothing mixes.  `reflected` is read only where
// an entry mixes, `local` and `kr` only for hits; no value of the caller's arrays is an index.
// kCounted (rrt.h: COUNTED DEVICE FORMS): ONE more argument, the bound -- a pack of no or one `const uint32_t*`, so the uncounted instantiation keeps the argument list it
// had.  The length becomes min(n, *bound), one scalar load, and a block whose first entry lies at or beyond it leaves at once.  The bound is only ever read.
template <bool kCounted = false, class... Bound>
__global__ __launch_bounds__(kBlock) void mix_rays_kernel(const MixRaysParams P, Bound... bound) {
    static_assert(sizeof...(Bound) == (kCounted ? 1 : 0), "a counted kernel takes one bound");
    uint32_t n = P.n;
    if constexpr (kCounted) {
        const uint32_t c = *(bound, ...);                                 // uniform: a kernel-argument pointer
        n = c < n ? c : n;
        if ((uint64_t)blockIdx.x * kBlock >= n) return;
    }
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t c = kWhite;
    if (!P.material || P.material[i] < P.n_mats) {                         // the hit rule of rrt_shade_rays
        const double lx = P.local[3u * i], ly = P.local[3u * i + 1u], lz = P.local[3u * i + 2u];
        const double kr = (P.kr && P.reflected) ? P.kr[i] : 0.0;
        if (kr > 0.0) {
            // RESTATES render.hip: shade_unwind, one level (raytracer.rs:89-101): the level below is a u8 colour; local * (1 - kr) + reflected * kr per channel
            const uint32_t below = P.reflected[i];
            const double fx = lx * (1.0 - kr) + (double)((below >> 16) & 255u) * kr;
            const double fy = ly * (1.0 - kr) + (double)((below >> 8) & 255u) * kr;
            const double fz = lz * (1.0 - kr) + (double)(below & 255u) * kr;
            c = (clamp_u8(fx) << 16) | (clamp_u8(fy) << 8) | clamp_u8(fz);
        } else {
            c = (clamp_u8(lx) << 16) | (clamp_u8(ly) << 8) | clamp_u8(lz);   // render.hip: trace_colour, raytracer.rs:104-108
        }
    }
    P.colour[i] = c;
}

// ---- pixels.  One lane per pixel of the region, row-major as the framebuffer: a wave stores 256 consecutive bytes.  The pixel's four sub-sample colours are four
// consecutive elements in either order -- in rows order the wave reads 1 KB of consecutive bytes, in tiles order sixteen 64-byte runs (four pixels of a tile's row) --
// and the compiler takes them with one 16-byte load (global_load_dwordx4 in the listing; the hardware does not need it aligned).  Color::mix (entities.rs:49-69) as
// render_kernel computes it: channel sums, truncating / 4.
__global__ __launch_bounds__(kBlock) void mix_pixels_kernel(const MixPixelsParams P) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)P.w * P.h) return;
    const uint32_t ry = (uint32_t)(i / P.w), px = P.x0 + (uint32_t)(i - (size_t)ry * P.w), py = P.y0 + ry;
    const int32_t W = (int32_t)P.width, H = (int32_t)P.height;
    uint32_t mixed = 0u;                                                   // a pixel the reference never traces (Canvas::new, engine.rs:135)
    if ((int32_t)px < 2 * (W / 2) && (int32_t)py >= H - 2 * (H / 2) + 1) {  // render.hip: render_kernel, `traced`
        const size_t q = P.order == 0u ? i : ((size_t)((py >> 2) - P.tile_y0) * P.tiles_w + ((px >> 2) - P.tile_x0)) * 16u + (py & 3u) * 4u + (px & 3u);
        uint32_t r = 0, g = 0, b = 0;
#pragma unroll
        for (uint32_t s = 0; s < 4u; s++) {
            const uint32_t c = P.colours[4u * q + s];
            r += (c >> 16) & 255u; g += (c >> 8) & 255u; b += c & 255u;
        }
        mixed = ((r >> 2) << 16) | ((g >> 2) << 8) | (b >> 2);             // Into<u32>, entities.rs:32-36
    }
    P.fb[i] = mixed;
}

uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + kBlock - 1) / kBlock); }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }   // (null is aligned)

}  // namespace

int launch_frame_rays(const FrameRaysParams& q, void* stream) {
    if (q.n == 0) return 0;
    if ((q.n & 1u) == 0 && aligned16(q.origins) && aligned16(q.dirs) && aligned16(q.max_t)) hipLaunchKernelGGL(frame_rays_kernel<true>, dim3(blocks_for(q.n)), dim3(kBlock), 0, (hipStream_t)stream, q);
    else hipLaunchKernelGGL(frame_rays_kernel<false>, dim3(blocks_for(q.n)), dim3(kBlock), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

int launch_mix_rays(const MixRaysParams& q, const uint32_t* d_bound, void* stream) {
    if (q.n == 0) return 0;
    if (d_bound) hipLaunchKernelGGL((mix_rays_kernel<true, const uint32_t*>), dim3(blocks_for(q.n)), dim3(kBlock), 0, (hipStream_t)stream, q, d_bound);
    else hipLaunchKernelGGL(mix_rays_kernel<>, dim3(blocks_for(q.n)), dim3(kBlock), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

int launch_mix_pixels(const MixPixelsParams& q, void* stream) {
    const uint64_t pixels = (uint64_t)q.w * q.h;
    if (pixels == 0) return 0;
    hipLaunchKernelGGL(mix_pixels_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

}  // namespace rrt
