// hip_check.hpp -- the library's one HIP error: what a failed HIP call throws, anywhere in the host code.  `guarded` (api_internal.hpp) is the
// only place that turns it into a status code (RRT_ERR_OOM / RRT_ERR_NO_DEVICE / RRT_ERR_HIP) and an error-detail string.
#pragma once
#include <hip/hip_runtime.h>

namespace rrt {
struct HipFail { hipError_t e; const char* what; };
}  // namespace rrt

#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) throw ::rrt::HipFail{_e, #expr}; } while (0)
