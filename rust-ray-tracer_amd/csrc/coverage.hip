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
// A word of the mask holds the four quadrant bits of eight consecutive tiles.  One item of a box = word `j` of tile row `row` of its rectangle.
// `dst` is the block's copy of the mask in LDS, or the mask itself for a frame whose mask does not fit there; an OR without a returned value either way.
__device__ __forceinline__ void mark_word(const CoverageRect& r, uint32_t tiles_x, uint32_t row, uint32_t j, uint32_t* dst) {
    const uint32_t ty = ((uint32_t)r.by0 >> 1) + row;
    const uint32_t t0 = ty * tiles_x + ((uint32_t)r.bx0 >> 1), t1 = ty * tiles_x + ((uint32_t)r.bx1 >> 1);   // first and last tile of the row
    const uint32_t w = (t0 >> 3) + j;
    if (w > (t1 >> 3)) return;
    // the rows of the tile row inside [by0, by1]: quadrant bits 0, 1 are the upper waves (by even), 2, 3 the lower; the same in all eight tiles of the word
    uint32_t bits = (((int32_t)(2u * ty) >= r.by0 && (int32_t)(2u * ty) <= r.by1 ? 0x3u : 0u) | ((int32_t)(2u * ty + 1u) >= r.by0 && (int32_t)(2u * ty + 1u) <= r.by1 ? 0xCu : 0u)) * 0x11111111u;
    // the first and the last word lose the tiles outside [t0, t1], and the outer column of an end tile that the rectangle enters halfway: quadrant bits 0, 2 are
    // the left waves (bx even), 1, 3 the right
    if (w == (t0 >> 3)) { const uint32_t s = 4u * (t0 & 7u); bits &= 0xFFFFFFFFu << s; if (r.bx0 & 1) bits &= ~(0x5u << s); }
    if (w == (t1 >> 3)) { const uint32_t s = 4u * (t1 & 7u); bits &= 0xFFFFFFFFu >> (28u - s); if (!(r.bx1 & 1)) bits &= ~(0xAu << s); }
    if (bits) atomicOr(dst + w, bits);
}

// One lane per box, kBlock boxes per block.  The boxes of a scene fall on few words again and again (the slots are in the order of the octree's nodes: neighbours in
// space), so a block first ORs into a copy of the mask in its LDS and then sends each non-zero word of the copy to memory once (reduce per block, then one atomic
// per destination).  A box of at most kOwnItems items is marked by its lane, 64 boxes of a wave side by side; a larger one -- a large oblique triangle can reach
// most of the frame: thousands of items -- is queued and then dealt over the whole block, one box at a time.  A box that reaches the whole frame sets every word and
// the flag behind them; blocks that start later see the flag and leave.  lds_words: n_words, or 0 for a frame whose mask does not fit the LDS -- the ORs then go to
// memory directly.
constexpr uint32_t kBlock = 256, kOwnItems = 64;
constexpr uint32_t kLdsWords = 15296, kLdsWordsRaised = 30720;   // 64 KB less the queue and the block's four words; 120 KB of the 160 KB of a gfx950 CU, where the runtime grants it
__global__ __launch_bounds__(kBlock) void coverage_kernel(const CoverageFrame F, const DevClusterBox* __restrict__ boxes, uint32_t n_boxes, uint32_t n_words, uint32_t lds_words,
                                                           uint32_t* __restrict__ mask) {
    extern __shared__ uint32_t block_mask[];
    __shared__ CoverageRect queue[kBlock];
    __shared__ uint32_t seen_whole, block_whole, first, n_queued;
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kBlock + tid;
    uint32_t* const whole = mask + n_words;
    if (tid == 0) { seen_whole = __hip_atomic_load(whole, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); block_whole = 0u; n_queued = 0u; }
    for (uint32_t w = tid; w < lds_words; w += kBlock) block_mask[w] = 0u;
    __syncthreads();
    if (seen_whole) return;                                               // (block-uniform, and not written again)
    CoverageRect r{0, -1, 0, -1};
    if (i < n_boxes) { const DevClusterBox B = boxes[i]; r = coverage_rect(F, B.c, B.h); }
    bool some = r.bx0 <= r.bx1 && r.by0 <= r.by1;
    if (some && coverage_is_whole_frame(F, r)) { block_whole = 1u; some = false; }   // (any number of lanes store the same value; the block fills the mask below)
    const uint32_t tile_rows = some ? (uint32_t)(r.by1 >> 1) - (uint32_t)(r.by0 >> 1) + 1u : 0u;
    const uint32_t words_per_row = some ? (((uint32_t)(r.bx1 >> 1) - (uint32_t)(r.bx0 >> 1)) >> 3) + 2u : 1u;   // (a run of n tiles touches at most (n - 1) / 8 + 2 words)
    const bool own = tile_rows * words_per_row <= kOwnItems;
    if (some && !own) queue[atomicAdd(&n_queued, 1u)] = r;                // (at most one entry per lane)
    auto mark_all = [&](auto* dst) {                                      // (once per address space: LDS ORs, or global atomics)
        if (own) for (uint32_t row = 0; row < tile_rows; row++) for (uint32_t j = 0; j < words_per_row; j++) mark_word(r, F.tiles_x, row, j, dst);
        __syncthreads();
        for (uint32_t k = 0; k < n_queued; k++) {                         // the threads of the block as rows x words, the words of a row rounded up to a power of two
            const CoverageRect q = queue[k];
            const uint32_t q_rows = (uint32_t)(q.by1 >> 1) - (uint32_t)(q.by0 >> 1) + 1u, q_words = (((uint32_t)(q.bx1 >> 1) - (uint32_t)(q.bx0 >> 1)) >> 3) + 2u;
            const uint32_t shift = q_words >= kBlock ? 8u : 32u - (uint32_t)__builtin_clz(q_words - 1u);       // 2^shift >= q_words (q_words >= 2), at most kBlock
            for (uint32_t row = tid >> shift; row < q_rows; row += kBlock >> shift)
                for (uint32_t j = tid & ((1u << shift) - 1u); j < q_words; j += 1u << shift) mark_word(q, F.tiles_x, row, j, dst);
        }
    };
    if (lds_words) mark_all(block_mask); else mark_all(mask);
    __syncthreads();
    if (block_whole) {                                                   // the first block to say so fills the mask
        if (tid == 0) first = atomicExch(whole, 1u) == 0u;
        __syncthreads();
        if (first) for (uint32_t w = tid; w < n_words; w += kBlock) atomicOr(mask + w, 0xFFFFFFFFu);
        return;
    }
    for (uint32_t w = tid; w < lds_words; w += kBlock) { const uint32_t bits = block_mask[w]; if (bits) atomicOr(mask + w, bits); }
}

}  // namespace

uint32_t coverage_mask_words(uint32_t tiles_x, uint32_t tiles_y) { return (uint32_t)(((uint64_t)tiles_x * tiles_y + 7u) / 8u); }

// Clear and fill `mask` (coverage_mask_words + 1 words) for the frame F over boxes[0, n_boxes), on `stream`.  Returns hipError_t as int; nothing is synchronised.
int launch_coverage(const CoverageFrame& F, const DevClusterBox* boxes, uint32_t n_boxes, uint32_t* mask, void* stream) {
    const uint32_t n_words = coverage_mask_words(F.tiles_x, F.tiles_y);
    const hipError_t e = hipMemsetAsync(mask, 0, sizeof(uint32_t) * ((size_t)n_words + 1), (hipStream_t)stream);
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
    hipLaunchKernelGGL(coverage_kernel, dim3((n_boxes + kBlock - 1u) / kBlock), dim3(kBlock), sizeof(uint32_t) * lds_words, (hipStream_t)stream, F, boxes, n_boxes, n_words, lds_words, mask);
    return (int)hipGetLastError();
}

}  // namespace rrt
