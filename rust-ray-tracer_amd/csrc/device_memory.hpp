// device_memory.hpp -- owners of HIP handles, the device buffer kept and grown between calls, and the bump allocator that carves one device allocation into buffers.
#pragma once
#include <cstddef>

#include "hip_check.hpp"
#include "model.hpp"
#include "slots.hpp"

namespace rrt {

// Move-only owner of one HIP handle (a device allocation, a stream); an empty one owns nothing.
template <class T, hipError_t (*Destroy)(T)> struct HipOwned {
    T h{};
    HipOwned() = default;
    explicit HipOwned(T handle) : h(handle) {}
    HipOwned(HipOwned&& o) noexcept : h(o.h) { o.h = T{}; }
    HipOwned& operator=(HipOwned&& o) noexcept { if (this != &o) { reset(); h = o.h; o.h = T{}; } return *this; }
    HipOwned(const HipOwned&) = delete; HipOwned& operator=(const HipOwned&) = delete;
    ~HipOwned() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = T{}; }
};
using DevBuf = HipOwned<void*, hipFree>;
using OwnedStream = HipOwned<hipStream_t, hipStreamDestroy>;
inline DevBuf dev_alloc(size_t bytes) { void* p = nullptr; HIP_TRY(hipMalloc(&p, bytes)); return DevBuf(p); }
// A device allocation kept between calls and grown when a larger request comes: the old one is freed first, and after a failed allocation it holds nothing.
struct KeptBuf {
    DevBuf mem; size_t bytes = 0;
    void* at_least(size_t need) {
        if (bytes < need) { mem.reset(); bytes = 0; mem = dev_alloc(need); bytes = need; }
        return mem.h;
    }
};

// Scene buffers are carved out of ONE device allocation (a hipMalloc per buffer costs milliseconds each: 15 of them were most of the teapot's
// upload time).  Every buffer starts on a 256-byte boundary (slots.hpp: slot_bytes); an empty one still gets an address of its own.  The arena does not own `base`.
struct DevArena {
    char* base = nullptr; size_t cap = 0, used = 0;
    template <class T> T* take(size_t count) {
        const size_t bytes = slot_bytes(sizeof(T) * (count ? count : 1));
        if (used + bytes > cap) throw Error{RRT_ERR_OOM, "internal: set-up arena too small"};
        T* p = reinterpret_cast<T*>(base + used); used += bytes; return p;
    }
};

}  // namespace rrt
