// slots.hpp -- the size rule of every buffer carved out of a device allocation (device_memory.hpp: DevArena; host_planes.hpp: carve_planes).  No HIP.
#pragma once
#include <cstddef>

namespace rrt {

// what a buffer of `bytes` bytes occupies: a whole number of 256-byte slots
constexpr size_t slot_bytes(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace rrt
