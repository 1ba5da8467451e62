// compact.hip -- stable compaction of ray batches and records on the device, and its inverse (rrt.h: rrt_compact_rays_device, rrt_scatter_rays_device).
//
// Three kernels, enqueued one behind the other on the caller's stream:
//   count_kernel   a block evaluates the selection over its tile of kCompactTile consecutive entries (wave ballot + popcount, the wave totals summed through
//                  LDS) and writes one count per tile to the scratch;
//   scan_kernel    ONE block turns the tile counts into exclusive offsets in place, in chunks of kScanBlock with a running carry, and writes the total behind
//                  them and to *count;
//   place_kernel   thread i evaluates the selection of entry i again; its slot is tile offset + wave offset (LDS) + the number of selected lanes below its own
//                  (mbcnt of the ballot).  It writes index[slot] = i and copies entry i of every requested array to slot `slot`.  The same thread writes the dead
//                  values and index = 0xFFFFFFFF to slot i if i >= total: survivors fill [0, total), dead entries [total, n), so no slot is written twice.
// No block waits on another block and no atomic decides a position: the result is the same bits on every run.  Values are moved as 1-, 4- and 8-byte integers;
// no arithmetic touches them, so NaN payloads and -0.0 survive.  Which arrays are present is uniform across a launch (kernel arguments).
//
// The counted forms (rrt.h: COUNTED DEVICE FORMS): count_kernel, place_kernel and scatter_kernel have a kCounted instantiation with ONE more argument, the bound -- a
// pack of no or one `const uint32_t*`, so the uncounted instantiation keeps the argument list it had.  The length of the batch becomes m = min(n, *bound), one scalar
// load, and a block whose first entry lies at or beyond m leaves before its first barrier and before it touches LDS or the arrays -- the whole block, because m is
// uniform.  The grids stay those of n, so scan_kernel is as it was: a count block beyond m still writes its tile's zero.  The bound is only ever read.
#include <hip/hip_runtime.h>

#include "batch_words.hpp"
#include "device_scene.hpp"

namespace rrt {

namespace {

constexpr uint32_t kWaves = kCompactTile / 64;     // waves of a count / place block
constexpr uint32_t kScanBlock = 256;               // tile counts per pass of the one scan block
constexpr uint32_t kDeadIndex = 0xFFFFFFFFu;
constexpr uint64_t kNaNBits = 0x7FF8000000000000ull, kInfBits = 0x7FF0000000000000ull, kOneBits = 0x3FF0000000000000ull;

static_assert(kCompactTile % 64 == 0 && kCompactTile <= 1024 && kWaves <= 64, "a tile is a whole number of waves of one block");
static_assert(sizeof(CompactParams) < 4096, "the arguments of the compaction kernels must fit the 4 KB kernel-argument segment");

// (lanes_below and move_words: batch_words.hpp, shared with sort.hip)
// sel[i] of rrt.h, for i < n
__device__ __forceinline__ bool selected(const CompactParams& P, size_t i) {
    if (P.select == 2u) return P.flag[i] != 0;
    const uint32_t m = P.src.material[i];
    if (m >= P.n_mats) return false;
    return P.select == 0u || P.mats[m].kr > 0.0;
}

// m of a counted launch
__device__ __forceinline__ uint32_t counted_length(uint32_t n, const uint32_t* __restrict__ bound) {
    const uint32_t c = *bound;                                            // uniform: a kernel-argument pointer
    return c < n ? c : n;
}

template <int K> __device__ __forceinline__ void fill_words(double* dst, size_t to, uint64_t first, uint64_t rest) {
    uint64_t* d = reinterpret_cast<uint64_t*>(dst) + (size_t)K * to;
#pragma unroll
    for (int k = 0; k < K; k++) d[k] = k == 0 ? first : rest;
}

template <bool kCounted = false, class... Bound>
__global__ __launch_bounds__(kCompactTile) void count_kernel(const CompactParams P, Bound... bound) {
    static_assert(sizeof...(Bound) == (kCounted ? 1 : 0), "a counted kernel takes one bound");
    uint32_t n = P.n;
    if constexpr (kCounted) {
        n = counted_length(n, bound...);
        if ((uint64_t)blockIdx.x * kCompactTile >= n) {                    // a tile wholly beyond the bound: its zero for scan_kernel, nothing else
            if (threadIdx.x == 0) P.tiles[blockIdx.x] = 0;
            return;
        }
    }
    __shared__ uint32_t wave_count[kWaves];
    const size_t i = (size_t)blockIdx.x * kCompactTile + threadIdx.x;
    const bool s = i < n && selected(P, i);
    const unsigned long long ballot = __ballot(s);
    if ((threadIdx.x & 63u) == 0) wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) sum += wave_count[w];
        P.tiles[blockIdx.x] = sum;
    }
}

// tiles[0, n_tiles): counts -> exclusive offsets; tiles[n_tiles] = total; *count = total
__global__ __launch_bounds__(kScanBlock) void scan_kernel(uint32_t* tiles, uint32_t n_tiles, uint32_t* count) {
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += kScanBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_tiles ? tiles[t] : 0u;
        uint32_t incl = v;                              // inclusive scan inside the wave
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanBlock / 64; w++) { const uint32_t s = wave_sum[w]; if (w < wave) before += s; all += s; }
        if (t < n_tiles) tiles[t] = carry + before + (incl - v);
        carry += all;
        __syncthreads();                                // wave_sum is written again in the next pass
    }
    if (threadIdx.x == 0) {
        tiles[n_tiles] = carry;
        if (count) *count = carry;
    }
}

template <bool kCounted = false, class... Bound>
__global__ __launch_bounds__(kCompactTile) void place_kernel(const CompactParams P, Bound... bound) {
    static_assert(sizeof...(Bound) == (kCounted ? 1 : 0), "a counted kernel takes one bound");
    uint32_t n = P.n;
    if constexpr (kCounted) {
        n = counted_length(n, bound...);
        if ((uint64_t)blockIdx.x * kCompactTile >= n) return;              // neither a survivor nor a dead slot below the bound in this tile
    }
    __shared__ uint32_t wave_count[kWaves];
    const size_t i = (size_t)blockIdx.x * kCompactTile + threadIdx.x;
    const bool in = i < n;
    const bool s = in && selected(P, i);
    const unsigned long long ballot = __ballot(s);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t wave_off = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++) if (w < wave) wave_off += wave_count[w];
    const uint32_t total = P.tiles[gridDim.x];
    const RaySetPtrs& S = P.src;
    const RaySetPtrs& D = P.dst;
    if (s) {
        const size_t to = (size_t)P.tiles[blockIdx.x] + wave_off + lanes_below(ballot);
        if (P.index) P.index[to] = (uint32_t)i;
        if (D.origins) move_words<3>(S.origins, i, D.origins, to);
        if (D.dirs) move_words<3>(S.dirs, i, D.dirs, to);
        if (D.max_t) { if (S.max_t) move_words<1>(S.max_t, i, D.max_t, to); else fill_words<1>(D.max_t, to, kInfBits, 0); }
        if (D.rot) move_words<2>(S.rot, i, D.rot, to);
        if (D.hit) D.hit[to] = S.hit[i];
        if (D.t) move_words<1>(S.t, i, D.t, to);
        if (D.u) move_words<1>(S.u, i, D.u, to);
        if (D.v) move_words<1>(S.v, i, D.v, to);
        if (D.tri) D.tri[to] = S.tri[i];
        if (D.albedo) D.albedo[to] = S.albedo[i];
        if (D.point) move_words<3>(S.point, i, D.point, to);
        if (D.normal) move_words<3>(S.normal, i, D.normal, to);
        if (D.material) D.material[to] = S.material[i];
        if (D.lights) D.lights[to] = S.lights[i];
        if (D.next_origin) move_words<3>(S.next_origin, i, D.next_origin, to);
        if (D.next_dir) move_words<3>(S.next_dir, i, D.next_dir, to);
    }
    if (in && i >= total) {                             // the dead entry of slot i: rrt_surface_rays' miss values, a NaN bound, the identity rotation
        if (P.index) P.index[i] = kDeadIndex;
        if (D.origins) fill_words<3>(D.origins, i, 0, 0);
        if (D.dirs) fill_words<3>(D.dirs, i, 0, 0);
        if (D.max_t) fill_words<1>(D.max_t, i, kNaNBits, 0);
        if (D.rot) fill_words<2>(D.rot, i, kOneBits, 0);
        if (D.hit) D.hit[i] = 0;
        if (D.t) fill_words<1>(D.t, i, 0, 0);
        if (D.u) fill_words<1>(D.u, i, 0, 0);
        if (D.v) fill_words<1>(D.v, i, 0, 0);
        if (D.tri) D.tri[i] = 0xFFFFFFFFu;
        if (D.albedo) D.albedo[i] = 0x00FFFFFFu;
        if (D.point) fill_words<3>(D.point, i, 0, 0);
        if (D.normal) fill_words<3>(D.normal, i, 0, 0);
        if (D.material) D.material[i] = 0xFFFFFFFFu;
        if (D.lights) D.lights[i] = 0;
        if (D.next_origin) fill_words<3>(D.next_origin, i, 0, 0);
        if (D.next_dir) fill_words<3>(D.next_dir, i, 0, 0);
    }
}

// dst[index[j]] = src[j] for every j -- of a counted launch: every j below the bound -- whose index is below n; kBytes per element
template <int kBytes> __device__ __forceinline__ void scatter_one(const void* src, size_t j, void* dst, size_t to) {
    if constexpr (kBytes == 1) static_cast<uint8_t*>(dst)[to] = static_cast<const uint8_t*>(src)[j];
    else if constexpr (kBytes == 4) static_cast<uint32_t*>(dst)[to] = static_cast<const uint32_t*>(src)[j];
    else move_words<kBytes / 8>(static_cast<const double*>(src), j, static_cast<double*>(dst), to);
}
template <bool kCounted = false, class... Bound>
__global__ __launch_bounds__(256) void scatter_kernel(uint32_t n, const uint32_t* index, uint32_t elem_bytes, const void* src, void* dst, Bound... bound) {
    static_assert(sizeof...(Bound) == (kCounted ? 1 : 0), "a counted kernel takes one bound");
    uint32_t m = n;                                     // j runs below m; an index is a position in the caller's arrays of n
    if constexpr (kCounted) {
        m = counted_length(n, bound...);
        if ((uint64_t)blockIdx.x * 256 >= m) return;
    }
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t to = index[j];
    if (to >= n) return;
    switch (elem_bytes) {                               // uniform across the launch
        case 1: scatter_one<1>(src, j, dst, to); break;
        case 4: scatter_one<4>(src, j, dst, to); break;
        case 8: scatter_one<8>(src, j, dst, to); break;
        case 16: scatter_one<16>(src, j, dst, to); break;
        case 24: scatter_one<24>(src, j, dst, to); break;
        default: break;
    }
}

}  // namespace

int launch_compact(const CompactParams& q, const uint32_t* d_bound, uint32_t* d_count, void* stream) {
    if (q.n == 0) return 0;
    const uint32_t n_tiles = compact_tiles(q.n);
    const bool place = q.index || q.any_dst;
    if (d_bound) hipLaunchKernelGGL((count_kernel<true, const uint32_t*>), dim3(n_tiles), dim3(kCompactTile), 0, (hipStream_t)stream, q, d_bound);
    else hipLaunchKernelGGL(count_kernel<>, dim3(n_tiles), dim3(kCompactTile), 0, (hipStream_t)stream, q);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanBlock), 0, (hipStream_t)stream, q.tiles, n_tiles, d_count);
    if (place && d_bound) hipLaunchKernelGGL((place_kernel<true, const uint32_t*>), dim3(n_tiles), dim3(kCompactTile), 0, (hipStream_t)stream, q, d_bound);
    else if (place) hipLaunchKernelGGL(place_kernel<>, dim3(n_tiles), dim3(kCompactTile), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

int launch_scatter(uint32_t n, const uint32_t* d_bound, const uint32_t* d_index, uint32_t elem_bytes, const void* d_src, void* d_dst, void* stream) {
    if (n == 0) return 0;
    const dim3 grid((uint32_t)(((uint64_t)n + 255) / 256));
    if (d_bound) hipLaunchKernelGGL((scatter_kernel<true, const uint32_t*>), grid, dim3(256), 0, (hipStream_t)stream, n, d_index, elem_bytes, d_src, d_dst, d_bound);
    else hipLaunchKernelGGL(scatter_kernel<>, grid, dim3(256), 0, (hipStream_t)stream, n, d_index, elem_bytes, d_src, d_dst);
    return (int)hipGetLastError();
}

}  // namespace rrt
