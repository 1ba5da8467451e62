// coverage.hip -- the coverage pass of a whole frame: one bit per 4x4-pixel wave of render_kernel, set when some padded triangle box of the scene can reach
// the wave (coverage_rule.hpp has the rule, its margin and why a cleared bit means sixteen WHITE pixels).  One small kernel for every whole
// single-GPU frame, computed anew from the camera and scene in force at the frame's call; nothing is kept from one frame to the next.  Where it runs is the host's
// choice (frames.cpp: launch_whole_frame): in front of render_kernel on the frame's stream when that stream is idle, else on the raytracer's side stream, beside
// the frame before, with the frame's render_kernel behind an event -- then outside the frame's two events.  Plain flags: no traversal here.
#include <hip/hip_runtime.h>

#include <atomic>

#include "coverage_rule.hpp"
#include "device_scene.hpp"

namespace rrt {
namespace {

// The mask: bit coverage_wave_index of word [0, n_words), then one word that says "some box reaches the whole frame: every bit is, or is being, set".
// A word of the mask holds the four quadrant bits of eight consecutive tiles.  One item of a box = word `j` of tile row `row` of its rectangle: word_bits gives
// the word's index and the bits of the rectangle in it (0: nothing to mark).
// Behind the mask (coverage_rule.hpp, "wide boxes"): the mask `fine` of the same layout, the count of wide boxes and their records.
__device__ __forceinline__ uint32_t word_bits(const CoverageRect& r, uint32_t tiles_x, uint32_t row, uint32_t j, uint32_t& w) {
    const uint32_t ty = ((uint32_t)r.by0 >> 1) + row;
    const uint32_t t0 = ty * tiles_x + ((uint32_t)r.bx0 >> 1), t1 = ty * tiles_x + ((uint32_t)r.bx1 >> 1);   // first and last tile of the row
    w = (t0 >> 3) + j;
    if (w > (t1 >> 3)) return 0u;
    // the rows of the tile row inside [by0, by1]: quadrant bits 0, 1 are the upper waves (by even), 2, 3 the lower; the same in all eight tiles of the word
    uint32_t bits = (((int32_t)(2u * ty) >= r.by0 && (int32_t)(2u * ty) <= r.by1 ? 0x3u : 0u) | ((int32_t)(2u * ty + 1u) >= r.by0 && (int32_t)(2u * ty + 1u) <= r.by1 ? 0xCu : 0u)) * 0x11111111u;
    // the first and the last word lose the tiles outside [t0, t1], and the outer column of an end tile that the rectangle enters halfway: quadrant bits 0, 2 are
    // the left waves (bx even), 1, 3 the right
    if (w == (t0 >> 3)) { const uint32_t s = 4u * (t0 & 7u); bits &= 0xFFFFFFFFu << s; if (r.bx0 & 1) bits &= ~(0x5u << s); }
    if (w == (t1 >> 3)) { const uint32_t s = 4u * (t1 & 7u); bits &= 0xFFFFFFFFu >> (28u - s); if (!(r.bx1 & 1)) bits &= ~(0xAu << s); }
    return bits;
}

// One lane per box, kBlock boxes per block.  The boxes of a scene fall on few words again and again (the slots are in the order of the octree's nodes: neighbours in
// space), so a block first ORs into a copy in its LDS and then sends each non-zero word of the copy to memory once (reduce per block, then one atomic per
// destination).  A box of at most kOwnItems items is marked by its lane, 64 boxes of a wave side by side; a larger one -- a large oblique triangle can reach
// most of the frame: thousands of items -- is queued and then dealt over the whole block, one box at a time.  A box that reaches the whole frame sets every word of
// both masks and the flag behind the first; blocks that start later see the flag and leave.  lds_words: n_words, or 0 for a frame whose mask does not fit the LDS --
// the ORs then go to memory directly.
// The LDS copy is the copy of `fine`: every box that is not LISTED goes into it, and a non-zero word of it is flushed to BOTH masks (a bit of `fine` is a bit of
// the mask).  A listed box -- a handful per frame (coverage_rule.hpp: at most kMaxWide) -- appends its record with one atomic and marks its words of the mask in
// memory; two LDS copies would not fit the raised limit at 3840 x 2160.  root_end: the slots [0, root_end) are the root's own list; 0: nothing is listed.
constexpr uint32_t kBlock = 256, kOwnItems = 64;
constexpr uint32_t kLdsWords = 15296, kLdsWordsRaised = 30720;   // 64 KB less the queue (4096 B: sixteen bytes per entry, no more) and the block's four words; 120 KB of the 160 KB of a gfx950 CU, where the runtime grants it
__global__ __launch_bounds__(kBlock) void coverage_kernel(const CoverageFrame F, const DevClusterBox* __restrict__ boxes, uint32_t n_boxes, uint32_t n_words, uint32_t lds_words,
                                                           uint32_t root_end, uint32_t* __restrict__ mask) {
    extern __shared__ uint32_t block_mask[];
    __shared__ CoverageRect queue[kBlock];                                 // (a queued rectangle holds a wave, so bx0 >= 0: its bit 31 says "listed")
    __shared__ uint32_t seen_whole, block_whole, first, n_queued;
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kBlock + tid;
    uint32_t* const whole = mask + n_words;
    uint32_t* const fine = mask + coverage_fine_offset(n_words);
    if (tid == 0) { seen_whole = __hip_atomic_load(whole, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); block_whole = 0u; n_queued = 0u; }
    for (uint32_t w = tid; w < lds_words; w += kBlock) block_mask[w] = 0u;
    __syncthreads();
    if (seen_whole) return;                                               // (block-uniform, and not written again)
    CoverageRect r{0, -1, 0, -1};
    if (i < n_boxes) { const DevClusterBox B = boxes[i]; r = coverage_rect(F, B.c, B.h); }
    bool some = r.bx0 <= r.bx1 && r.by0 <= r.by1;
    if (some && coverage_is_whole_frame(F, r)) { block_whole = 1u; some = false; }   // (any number of lanes store the same value; the block fills the masks below)
    bool listed = false;
    if (some && coverage_is_wide(F, r, i, root_end)) {
        const uint32_t k = atomicAdd(mask + coverage_wide_count_offset(n_words), 1u);
        if (k < kMaxWide) {                                               // (else: the list is full, an ordinary box)
            reinterpret_cast<WideRecord*>(mask + coverage_wide_records_offset(n_words))[k] = WideRecord{i, r.bx0, r.bx1, r.by0, r.by1};
            listed = true;
        }
    }
    const uint32_t tile_rows = some ? (uint32_t)(r.by1 >> 1) - (uint32_t)(r.by0 >> 1) + 1u : 0u;
    const uint32_t words_per_row = some ? (((uint32_t)(r.bx1 >> 1) - (uint32_t)(r.bx0 >> 1)) >> 3) + 2u : 1u;   // (a run of n tiles touches at most (n - 1) / 8 + 2 words)
    const bool own = tile_rows * words_per_row <= kOwnItems;
    if (some && !own) queue[atomicAdd(&n_queued, 1u)] = CoverageRect{(int32_t)((uint32_t)r.bx0 | (listed ? 0x80000000u : 0u)), r.bx1, r.by0, r.by1};   // (at most one entry per lane)
    auto mark_all = [&](auto put) {                                       // (once per destination of an unlisted box: LDS ORs, or global atomics)
        if (own) for (uint32_t row = 0; row < tile_rows; row++) for (uint32_t j = 0; j < words_per_row; j++) put(r, listed, row, j);
        __syncthreads();
        for (uint32_t k = 0; k < n_queued; k++) {                         // the threads of the block as rows x words, the words of a row rounded up to a power of two
            CoverageRect q = queue[k];
            const bool q_listed = q.bx0 < 0;
            q.bx0 &= 0x7FFFFFFF;
            const uint32_t q_rows = (uint32_t)(q.by1 >> 1) - (uint32_t)(q.by0 >> 1) + 1u, q_words = (((uint32_t)(q.bx1 >> 1) - (uint32_t)(q.bx0 >> 1)) >> 3) + 2u;
            const uint32_t shift = q_words >= kBlock ? 8u : 32u - (uint32_t)__builtin_clz(q_words - 1u);       // 2^shift >= q_words (q_words >= 2), at most kBlock
            for (uint32_t row = tid >> shift; row < q_rows; row += kBlock >> shift)
                for (uint32_t j = tid & ((1u << shift) - 1u); j < q_words; j += 1u << shift) put(q, q_listed, row, j);
        }
    };
    if (lds_words) mark_all([&](const CoverageRect& q, bool q_listed, uint32_t row, uint32_t j) {
        uint32_t w; const uint32_t bits = word_bits(q, F.tiles_x, row, j, w);
        if (bits) { if (q_listed) atomicOr(mask + w, bits); else atomicOr(block_mask + w, bits); }
    });
    else mark_all([&](const CoverageRect& q, bool q_listed, uint32_t row, uint32_t j) {
        uint32_t w; const uint32_t bits = word_bits(q, F.tiles_x, row, j, w);
        if (bits) { atomicOr(mask + w, bits); if (!q_listed) atomicOr(fine + w, bits); }
    });
    __syncthreads();
    if (block_whole) {                                                   // the first block to say so fills both masks: every wave walks
        if (tid == 0) first = atomicExch(whole, 1u) == 0u;
        __syncthreads();
        if (first) for (uint32_t w = tid; w < n_words; w += kBlock) { atomicOr(mask + w, 0xFFFFFFFFu); atomicOr(fine + w, 0xFFFFFFFFu); }
        return;
    }
    for (uint32_t w = tid; w < lds_words; w += kBlock) { const uint32_t bits = block_mask[w]; if (bits) { atomicOr(mask + w, bits); atomicOr(fine + w, bits); } }
}

}  // namespace

uint32_t coverage_mask_words(uint32_t tiles_x, uint32_t tiles_y) { return coverage_words_of(tiles_x, tiles_y); }

// Clear and fill `mask` (coverage_buffer_words(coverage_mask_words) words: the mask, `whole`, `fine`, the wide boxes' count and records) for the frame F over
// boxes[0, n_boxes), of which [0, root_end) are the root's own list (0: no box is listed), on `stream`.  Returns hipError_t as int; nothing is synchronised.
int launch_coverage(const CoverageFrame& F, const DevClusterBox* boxes, uint32_t n_boxes, uint32_t root_end, uint32_t* mask, void* stream) {
    const uint32_t n_words = coverage_mask_words(F.tiles_x, F.tiles_y);
    const hipError_t e = hipMemsetAsync(mask, 0, sizeof(uint32_t) * (size_t)coverage_buffer_words(n_words), (hipStream_t)stream);
    if (e != hipSuccess || n_boxes == 0) return (int)e;
    // (a 1920 x 1080 frame has 4050 words, a 3840 x 2160 frame 16200: beyond the default limit of dynamic LDS, which is raised for this kernel once per device;
    // a mask beyond the raised limit, or a device that refuses it, takes the kernel's path without LDS)
    uint32_t lds_words = n_words <= kLdsWords ? n_words : 0u;
    if (!lds_words && n_words <= kLdsWordsRaised) {
        static std::atomic<uint8_t> raised[64];                               // per device: 0 not asked yet, 1 granted, 2 refused
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); dev = -1; }
        uint8_t state = dev >= 0 ? raised[dev].load(std::memory_order_relaxed) : 2;
        if (state == 0) {
            state = hipFuncSetAttribute(reinterpret_cast<const void*>(&coverage_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(uint32_t) * kLdsWordsRaised)) == hipSuccess ? 1 : 2;
            if (state == 2) (void)hipGetLastError();
            raised[dev].store(state, std::memory_order_relaxed);
        }
        if (state == 1) lds_words = n_words;
    }
    hipLaunchKernelGGL(coverage_kernel, dim3((n_boxes + kBlock - 1u) / kBlock), dim3(kBlock), sizeof(uint32_t) * lds_words, (hipStream_t)stream, F, boxes, n_boxes, n_words, lds_words, root_end, mask);
    return (int)hipGetLastError();
}

}  // namespace rrt
