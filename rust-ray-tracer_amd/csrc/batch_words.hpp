// batch_words.hpp -- what the kernels that reorder ray batches share (compact.hip, sort.hip): a lane's rank inside its wave's ballot, and the move of one element of
// an array as 8-byte integers, so that no arithmetic touches a value and NaN payloads and -0.0 survive.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rrt {

// the number of set lanes of this wave's ballot below the calling lane
__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// element `from` of src to element `to` of dst, K 8-byte words each
template <int K> __device__ __forceinline__ void move_words(const double* src, size_t from, double* dst, size_t to) {
    const uint64_t* s = reinterpret_cast<const uint64_t*>(src) + (size_t)K * from;
    uint64_t* d = reinterpret_cast<uint64_t*>(dst) + (size_t)K * to;
    uint64_t w[K];
#pragma unroll
    for (int k = 0; k < K; k++) w[k] = s[k];
#pragma unroll
    for (int k = 0; k < K; k++) d[k] = w[k];
}

}  // namespace rrt
