// tiles.hip -- from a plane of a frame to one byte per 8x8-pixel tile (rrt.h: rrt_mark_tiles_device, rrt_select_tiles_device): the producer of the list that
// render_tile_list_kernel (render.hip) consumes.  The step from the marks to the list is the compaction that exists (compact.hip: RRT_SELECT_FLAG over the marks).
//
// One kernel, one launch per test.  A plane is [region.h][region.w][per_pixel] elements of elem_bytes, read as unsigned integers: no arithmetic touches them, so
// -0.0 is not zero and a NaN equals itself.  A tile row is R = 8 * per_pixel * elem_bytes bytes: 8, 32, 64, 128 or 256.
//   The wave.  A wave takes the 8 rows of a STRETCH of S = max(R, 128) bytes of the frame's rows, that is G = S / R neighbouring tiles of one tile row: 16, 4, 2, 1, 1.
//   Stretches are laid from column 0 of the FRAME, so tile tx belongs to stretch tx / G whatever the region is.  A lane takes 16-byte chunks: chunk c of the
//   8 * S / 16 = 64 (or 128: two passes) of its wave is bytes [16 (c % (S / 16)), + 16) of row c / (S / 16), so one load instruction of a wave covers whole 128-byte
//   stretches of 8 (or 4) rows.  Every element is read once, by one lane.
//   The two paths.  kVec: one 16-byte load per chunk.  The host chooses it, once per launch, where every chunk is aligned and wholly inside or wholly outside the
//   region: the plane's address, its row pitch region.w * per_pixel * elem_bytes and the byte offset of the region's first column in a row of the frame are all
//   multiples of 16 (a whole frame: the address and the pitch).  Otherwise the element path: the same chunks, element by element, each element loaded only if it
//   lies inside the region.  A chunk or an element outside the region is not loaded and votes 0; bounds are decided in BYTES of the region's row, which
//   is exact because a pixel is a whole number of elements.
//   The verdict.  Each lane holds the verdict of the two 8-byte halves of its chunk(s); only for R = 8 do the halves belong to different tiles.  One ballot per half
//   gives the wave all of them; lane j < G masks out the lanes of tile j and stores ITS byte: one store per tile, one writer per byte, no atomic, no LDS, no
//   barrier, no block that waits on another -- the same bits on every run.  The grid covers every tile of the frame, so without KEEP a tile the region does not
//   touch gets its 0 (from a wave that loads nothing); with KEEP only a selected tile's byte is written, and a wave whose stretch misses the region leaves at once.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_scene.hpp"

namespace rrt {

namespace {

constexpr uint32_t kBlock = 256;                       // four waves, each with a stretch of its own

static_assert(sizeof(TileTestParams) < 4096, "the argument of mark_tiles_kernel must fit the 4 KB kernel-argument segment");

// element x passes the test (RANGE and SET: 4-byte elements only, the host checks)
__device__ __forceinline__ bool passes_u32(const TileTestParams& P, uint32_t x) {
    if (P.test == 1u) return P.lo <= x && x < P.hi;
    // SET: the word of x by selects, not by an index into the kernel argument (that would put the table into scratch)
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) word = (x >> 5) == k ? P.set[k] : word;
    return x < 256u && ((word >> (x & 31u)) & 1u) != 0u;
}

// The verdicts of the two 8-byte halves of the 16-byte chunk at byte `rel` of region row `row` (both inside the region, checked by the caller for kVec; per element here).
template <uint32_t kElem, bool kVec>
__device__ __forceinline__ void chunk_verdict(const TileTestParams& P, size_t row_bytes_at, int64_t rel, int64_t pitch, bool& lo, bool& hi) {
    const char* const a = static_cast<const char*>(P.a) + row_bytes_at;
    const char* const b = static_cast<const char*>(P.b) + row_bytes_at;     // (DIFFERS only: never dereferenced otherwise)
    const bool range_or_set = P.test == 1u || P.test == 2u;
    const bool differs = P.test == 3u;
    if constexpr (kVec) {
        if (rel < 0 || rel + 16 > pitch) return;
        uint4 x = *reinterpret_cast<const uint4*>(a + rel);
        if (differs) {
            const uint4 y = *reinterpret_cast<const uint4*>(b + rel);
            x.x ^= y.x; x.y ^= y.y; x.z ^= y.z; x.w ^= y.w;
        }
        if (range_or_set) {
            lo = lo || passes_u32(P, x.x) || passes_u32(P, x.y);
            hi = hi || passes_u32(P, x.z) || passes_u32(P, x.w);
        } else {                                        // NONZERO, and DIFFERS after the xor: any bit, whatever the element width
            lo = lo || (x.x | x.y) != 0u;
            hi = hi || (x.z | x.w) != 0u;
        }
    } else {
        using Elem = std::conditional_t<kElem == 1, uint8_t, std::conditional_t<kElem == 4, uint32_t, uint64_t>>;
#pragma unroll
        for (uint32_t k = 0; k < 16 / kElem; k++) {
            const int64_t at = rel + (int64_t)(k * kElem);
            if (at < 0 || at >= pitch) continue;
            const Elem x = *reinterpret_cast<const Elem*>(a + at);
            bool pass;
            if (differs) pass = x != *reinterpret_cast<const Elem*>(b + at);
            else if (range_or_set) pass = passes_u32(P, (uint32_t)x);
            else pass = x != 0;
            if (k * kElem < 8) lo = lo || pass; else hi = hi || pass;
        }
    }
}

// kElem: elem_bytes; kPix: per_pixel
template <uint32_t kElem, uint32_t kPix, bool kVec>
__global__ __launch_bounds__(kBlock) void mark_tiles_kernel(const TileTestParams P) {
    constexpr uint32_t R = 8 * kPix * kElem;            // bytes of a tile row
    constexpr uint32_t S = R < 128 ? 128 : R;           // ... of a stretch
    constexpr uint32_t G = S / R;                       // tiles of a stretch
    constexpr uint32_t kChunksPerRow = S / 16, kPasses = 8 * kChunksPerRow / 64;
    static_assert(kPasses == 1 || kPasses == 2, "a stretch is 64 or 128 chunks");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stretches_x = (P.tiles_x + G - 1) / G;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (wave >= (uint64_t)stretches_x * P.tiles_y) return;
    const uint32_t ty = (uint32_t)(wave / stretches_x), sx = (uint32_t)(wave % stretches_x);
    // the stretch against the region, in pixels: uniform
    const uint32_t px0 = sx * (8 * G), py0 = ty * 8;
    const bool touches = px0 < P.x0 + P.w && px0 + 8 * G > P.x0 && py0 < P.y0 + P.h && py0 + 8 > P.y0;
    bool lo = false, hi = false;
    if (touches) {
        const int64_t pitch = (int64_t)P.w * (kPix * kElem);
        const int64_t first = (int64_t)px0 * (kPix * kElem) - (int64_t)P.x0 * (kPix * kElem);   // byte of the region's row at which the stretch begins (may be negative)
#pragma unroll
        for (uint32_t pass = 0; pass < kPasses; pass++) {
            const uint32_t chunk = pass * 64 + lane;
            const uint32_t y = py0 + chunk / kChunksPerRow;
            if (y < P.y0 || y >= P.y0 + P.h) continue;
            chunk_verdict<kElem, kVec>(P, (size_t)(y - P.y0) * (size_t)pitch, first + (int64_t)(16 * (chunk % kChunksPerRow)), pitch, lo, hi);
        }
    } else if (P.keep) {
        return;                                         // nothing can be selected here, and KEEP writes nothing else
    }
    // the lanes of tile j of the stretch: for R >= 16 the R / 16 chunks of each row (both halves), for R = 8 one half of chunk j / 2
    unsigned long long mine;
    if constexpr (R == 8) {
        const unsigned long long ballot_lo = __ballot(lo), ballot_hi = __ballot(hi);
        mine = ((lane & 1u) ? ballot_hi : ballot_lo) & (0x0101010101010101ull << ((lane >> 1) & 7u));
    } else {
        constexpr uint32_t kChunksPerTile = R / 16 > 8 ? 8 : R / 16;      // (R = 256: one tile, every lane)
        const unsigned long long ballot = __ballot(lo || hi);
        mine = ballot & (0x0101010101010101ull * (unsigned long long)((1u << kChunksPerTile) - 1u) << ((lane * kChunksPerTile) & 7u));
    }
    const uint32_t tx = sx * G + lane;
    if (lane < G && tx < P.tiles_x) {
        const bool selected = mine != 0ull;
        if (selected || !P.keep) P.marks[(size_t)ty * P.tiles_x + tx] = selected ? 1 : 0;
    }
}

template <uint32_t kElem, uint32_t kPix> void launch_one(const TileTestParams& q, dim3 grid, hipStream_t stream) {
    if (q.vec) hipLaunchKernelGGL((mark_tiles_kernel<kElem, kPix, true>), grid, dim3(kBlock), 0, stream, q);
    else hipLaunchKernelGGL((mark_tiles_kernel<kElem, kPix, false>), grid, dim3(kBlock), 0, stream, q);
}

}  // namespace

int launch_mark_tiles(const TileTestParams& q, void* stream) {
    const uint32_t row_bytes = 8 * q.per_pixel * q.elem_bytes, tiles_per_wave = row_bytes < 128 ? 128 / row_bytes : 1;
    const uint64_t waves = (uint64_t)((q.tiles_x + tiles_per_wave - 1) / tiles_per_wave) * q.tiles_y;
    if (waves == 0) return 0;
    const dim3 grid((uint32_t)((waves + kBlock / 64 - 1) / (kBlock / 64)));
    const hipStream_t s = (hipStream_t)stream;
    switch (q.elem_bytes * 8 + q.per_pixel) {           // (elem_bytes 1, 4 or 8 and per_pixel 1 or 4: checked by the caller)
        case 1 * 8 + 1: launch_one<1, 1>(q, grid, s); break;
        case 1 * 8 + 4: launch_one<1, 4>(q, grid, s); break;
        case 4 * 8 + 1: launch_one<4, 1>(q, grid, s); break;
        case 4 * 8 + 4: launch_one<4, 4>(q, grid, s); break;
        case 8 * 8 + 1: launch_one<8, 1>(q, grid, s); break;
        case 8 * 8 + 4: launch_one<8, 4>(q, grid, s); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace rrt
