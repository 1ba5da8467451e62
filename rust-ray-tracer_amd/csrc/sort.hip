// sort.hip -- stable sort of ray batches and records by a 32-bit coherence key on the device (rrt.h: rrt_sort_rays_device).
//
// An LSD radix sort over 8-bit digits, every kernel enqueued behind the last on the caller's stream:
//   key_kernel          entry i gets its key -- the caller's (GIVEN), or 27 bits of Morton code of its position in the root box and 3 sign bits of its direction
//                       (RAY, RECORD), 0xFFFFFFFF for a dead entry -- and the pair (key, i) goes to buffer 0 of the scratch;
//   four passes, digit = bits [8 p, 8 p + 8) of the key, from buffer p & 1 to the other one:
//     hist_kernel       a block counts the 256 digits of its tile of kSortTile consecutive entries: hist[digit][tile];
//     scan_rows_kernel  block d turns row d of hist into exclusive offsets in place, in chunks of 256 tiles with a running carry, and writes the row's total;
//     scan_totals_kernel one block turns the 256 totals into the digits' first slots;
//     place_kernel      a block walks its tile again in kRounds rounds of 1024 entries.  The slot of an entry with digit d is the digit's first slot + the row
//                       offset of the tile + the entries with d in earlier rounds and in earlier waves of this round (wave counts through LDS, summed in wave
//                       order by thread d) + the lanes with d below its own: the match mask is 8 ballots, one per digit bit, and the rank its mbcnt;
//   gather_kernel       slot j takes (key, i) of the sorted buffer: index[j] = i, keys_out[j] = key, element i of every requested array of src to element j of
//                       dst; the one thread that sees the last alive key in front of a dead one (or the end) writes *count.
// No block waits on another block and no atomic decides a position or a count: the result is the same bits on every run.  Lanes at or beyond n execute every ballot
// and are kept out of every mask.  Values are moved as 1-, 4- and 8-byte integers.  Which arrays are present is uniform across a launch (kernel arguments).
#include <hip/hip_runtime.h>

#include "batch_words.hpp"
#include "device_scene.hpp"

namespace rrt {

namespace {

constexpr uint32_t kThreads = 1024;                     // of a hist / place block
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kRounds = kSortTile / kThreads;
constexpr uint32_t kPasses = 4, kDigitBits = 8;
constexpr uint32_t kDeadKey = 0xFFFFFFFFu;
constexpr uint32_t kFlatBlock = 256;                    // of the key and gather kernels, and of the scans: one thread per digit

static_assert(kSortTile % kThreads == 0 && kSortDigits == (1u << kDigitBits) && kPasses * kDigitBits == 32 && kSortDigits <= kThreads && kFlatBlock == kSortDigits,
              "a tile is a whole number of rounds of one block, a key four digits, and thread d of a block owns digit d");
static_assert(sizeof(SortParams) < 4096, "the arguments of the sort kernels must fit the 4 KB kernel-argument segment");

// bit b of c to bit 3 b, for the nine bits of a cell number
__device__ __forceinline__ uint32_t spread3(uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t b = 0; b < 9; b++) r |= ((c >> b) & 1u) << (3 * b);
    return r;
}

// The key of an alive entry at p heading along d (rrt.h): per axis the cell of 512 of the root box that p falls into -- two rounded f64 operations, clamped; NaN and
// -inf give 0, +inf gives 511 -- interleaved, and the three signs above them.
__device__ __forceinline__ uint32_t coherence_key(const SortParams& P, const double* p, const double* d) {
    uint32_t key = 0;
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) {
        const double q = (p[a] - P.lo[a]) * P.scale[a];
        const uint32_t cell = q >= 511.0 ? 511u : (q > 0.0 ? (uint32_t)q : 0u);
        key |= spread3(cell) << a;
        key |= (d[a] < 0.0 ? 1u : 0u) << (27 + a);
    }
    return key;
}

__global__ __launch_bounds__(kFlatBlock) void key_kernel(const SortParams P, uint32_t* key, uint32_t* idx) {
    const size_t i = (size_t)blockIdx.x * kFlatBlock + threadIdx.x;
    if (i >= P.n) return;
    uint32_t k;
    if (P.key_mode == 0u) {
        k = P.keys[i];
    } else if (P.key_mode == 1u) {
        const bool dead = P.src.max_t && !(P.src.max_t[i] > 0.0);
        k = dead ? kDeadKey : coherence_key(P, P.src.origins + 3 * i, P.src.dirs + 3 * i);
    } else {
        const bool dead = P.src.material[i] >= P.n_mats;
        k = dead ? kDeadKey : coherence_key(P, P.src.point + 3 * i, P.src.normal + 3 * i);
    }
    key[i] = k;
    idx[i] = (uint32_t)i;
}

// The lanes of this wave that are `in` and hold the digit d: eight ballots, executed by all 64 lanes.  (the value is only meaningful for a lane that is `in`)
__device__ __forceinline__ unsigned long long match_mask(uint32_t d, bool in) {
    unsigned long long m = __ballot(in);
#pragma unroll
    for (uint32_t b = 0; b < kDigitBits; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long has = __ballot(bit);
        m &= bit ? has : ~has;
    }
    return m;
}

// One round of a block over its tile, for the calling thread's entry with digit d (in: the entry exists): the wave's count of every digit present goes to
// cnt[wave][digit] -- the first lane of a match mask writes it; cnt is zero on entry.  Returns the thread's rank among its wave's lanes with the same digit.  No
// barrier inside.
__device__ __forceinline__ uint32_t count_round(uint32_t (*cnt)[kSortDigits], uint32_t d, bool in) {
    const unsigned long long mask = match_mask(d, in);
    const uint32_t below = lanes_below(mask);
    if (in && below == 0) cnt[threadIdx.x >> 6][d] = (uint32_t)__popcll(mask);
    return below;
}

__global__ __launch_bounds__(kThreads) void hist_kernel(const uint32_t* key, uint32_t n, uint32_t shift, uint32_t* hist, uint32_t n_tiles) {
    __shared__ uint32_t cnt[kWaves][kSortDigits];
    for (uint32_t k = threadIdx.x; k < kWaves * kSortDigits; k += kThreads) (&cnt[0][0])[k] = 0;
    __syncthreads();
    uint32_t sum = 0;                                   // thread d: digit d's count in the tile so far
    for (uint32_t r = 0; r < kRounds; r++) {
        const size_t i = (size_t)blockIdx.x * kSortTile + r * kThreads + threadIdx.x;
        const bool in = i < n;
        count_round(cnt, in ? (key[i] >> shift) & (kSortDigits - 1) : 0u, in);
        __syncthreads();
        if (threadIdx.x < kSortDigits) {
#pragma unroll
            for (uint32_t w = 0; w < kWaves; w++) { sum += cnt[w][threadIdx.x]; cnt[w][threadIdx.x] = 0; }
        }
        __syncthreads();                                // cnt is written again in the next round
    }
    if (threadIdx.x < kSortDigits) hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = sum;
}

// Exclusive scan of one value per thread of a kFlatBlock block: returns the sum of the values of the threads below, `all` = the block's sum.  Two barriers.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* wave_sum, uint32_t& all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;                                  // inclusive scan inside the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kFlatBlock / 64; w++) { const uint32_t s = wave_sum[w]; if (w < wave) before += s; all += s; }
    __syncthreads();                                    // wave_sum is written again by the next call
    return before + (incl - v);
}

// block d: hist[d][0, n_tiles): counts -> exclusive offsets inside the row; totals[d] = the row's sum
__global__ __launch_bounds__(kFlatBlock) void scan_rows_kernel(uint32_t* hist, uint32_t n_tiles, uint32_t* totals) {
    __shared__ uint32_t wave_sum[kFlatBlock / 64];
    uint32_t* row = hist + (size_t)blockIdx.x * n_tiles;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += kFlatBlock) {
        const uint32_t t = base + threadIdx.x;
        uint32_t all;
        const uint32_t before = block_exclusive(t < n_tiles ? row[t] : 0u, wave_sum, all);
        if (t < n_tiles) row[t] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// totals[0, 256): the digits' counts -> the digits' first slots
__global__ __launch_bounds__(kFlatBlock) void scan_totals_kernel(uint32_t* totals) {
    __shared__ uint32_t wave_sum[kFlatBlock / 64];
    uint32_t all;
    totals[threadIdx.x] = block_exclusive(totals[threadIdx.x], wave_sum, all);
}

__global__ __launch_bounds__(kThreads) void place_kernel(const uint32_t* key, const uint32_t* idx, uint32_t* key_to, uint32_t* idx_to, uint32_t n, uint32_t shift,
                                                         const uint32_t* hist, const uint32_t* totals, uint32_t n_tiles) {
    __shared__ uint32_t cnt[kWaves][kSortDigits], off[kWaves][kSortDigits];
    for (uint32_t k = threadIdx.x; k < kWaves * kSortDigits; k += kThreads) (&cnt[0][0])[k] = 0;
    uint32_t next = 0;                                  // thread d: the slot of the tile's next entry with digit d
    if (threadIdx.x < kSortDigits) next = totals[threadIdx.x] + hist[(size_t)threadIdx.x * n_tiles + blockIdx.x];
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t r = 0; r < kRounds; r++) {
        const size_t i = (size_t)blockIdx.x * kSortTile + r * kThreads + threadIdx.x;
        const bool in = i < n;
        const uint32_t k = in ? key[i] : 0u;
        const uint32_t d = (k >> shift) & (kSortDigits - 1);
        const uint32_t below = count_round(cnt, d, in);
        __syncthreads();
        if (threadIdx.x < kSortDigits) {                // the waves' first slots of digit d in this round, in wave order
#pragma unroll
            for (uint32_t w = 0; w < kWaves; w++) { off[w][threadIdx.x] = next; next += cnt[w][threadIdx.x]; cnt[w][threadIdx.x] = 0; }
        }
        __syncthreads();                                // (off is written again only behind the next round's first barrier: every thread has read it by then)
        if (in) {
            const uint32_t to = off[wave][d] + below;
            if (to < n) { key_to[to] = k; idx_to[to] = idx[i]; }   // (always: the counts of a pass add up to n)
        }
    }
}

__global__ __launch_bounds__(kFlatBlock) void gather_kernel(const SortParams P, const uint32_t* key, const uint32_t* idx) {
    const size_t j = (size_t)blockIdx.x * kFlatBlock + threadIdx.x;
    if (j >= P.n) return;
    const uint32_t k = key[j];
    const size_t i = idx[j];
    if (P.count) {                                      // the sorted keys end in the dead ones: one thread sees the border
        if (k != kDeadKey && (j + 1 == P.n || key[j + 1] == kDeadKey)) *P.count = (uint32_t)(j + 1);
        if (j == 0 && k == kDeadKey) *P.count = 0;
    }
    if (i >= P.n) return;                               // (never: idx is a permutation of [0, n))
    if (P.index) P.index[j] = (uint32_t)i;
    if (P.keys_out) P.keys_out[j] = k;
    const RaySetPtrs& S = P.src;
    const RaySetPtrs& D = P.dst;
    if (D.origins) move_words<3>(S.origins, i, D.origins, j);
    if (D.dirs) move_words<3>(S.dirs, i, D.dirs, j);
    if (D.max_t) move_words<1>(S.max_t, i, D.max_t, j);
    if (D.rot) move_words<2>(S.rot, i, D.rot, j);
    if (D.hit) D.hit[j] = S.hit[i];
    if (D.t) move_words<1>(S.t, i, D.t, j);
    if (D.u) move_words<1>(S.u, i, D.u, j);
    if (D.v) move_words<1>(S.v, i, D.v, j);
    if (D.tri) D.tri[j] = S.tri[i];
    if (D.albedo) D.albedo[j] = S.albedo[i];
    if (D.point) move_words<3>(S.point, i, D.point, j);
    if (D.normal) move_words<3>(S.normal, i, D.normal, j);
    if (D.material) D.material[j] = S.material[i];
    if (D.lights) D.lights[j] = S.lights[i];
    if (D.next_origin) move_words<3>(S.next_origin, i, D.next_origin, j);
    if (D.next_dir) move_words<3>(S.next_dir, i, D.next_dir, j);
}

}  // namespace

int launch_sort(const SortParams& q, void* stream_v) {
    if (q.n == 0) return 0;
    const hipStream_t stream = (hipStream_t)stream_v;
    const uint32_t n = q.n, n_tiles = sort_tiles(n), flat = (uint32_t)(((uint64_t)n + kFlatBlock - 1) / kFlatBlock);
    uint32_t* key[2] = {q.scratch, q.scratch + 2 * (size_t)n};
    uint32_t* idx[2] = {q.scratch + (size_t)n, q.scratch + 3 * (size_t)n};
    uint32_t* hist = q.scratch + 4 * (size_t)n;
    uint32_t* totals = hist + (size_t)kSortDigits * n_tiles;
    hipLaunchKernelGGL(key_kernel, dim3(flat), dim3(kFlatBlock), 0, stream, q, key[0], idx[0]);
    for (uint32_t p = 0; p < kPasses; p++) {
        const uint32_t a = p & 1u, b = a ^ 1u, shift = p * kDigitBits;
        hipLaunchKernelGGL(hist_kernel, dim3(n_tiles), dim3(kThreads), 0, stream, key[a], n, shift, hist, n_tiles);
        hipLaunchKernelGGL(scan_rows_kernel, dim3(kSortDigits), dim3(kFlatBlock), 0, stream, hist, n_tiles, totals);
        hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kFlatBlock), 0, stream, totals);
        hipLaunchKernelGGL(place_kernel, dim3(n_tiles), dim3(kThreads), 0, stream, key[a], idx[a], key[b], idx[b], n, shift, hist, totals, n_tiles);
    }
    hipLaunchKernelGGL(gather_kernel, dim3(flat), dim3(kFlatBlock), 0, stream, q, key[kPasses & 1u], idx[kPasses & 1u]);
    return (int)hipGetLastError();
}

}  // namespace rrt
