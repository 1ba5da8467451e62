// error.hpp -- the library's one refusal: what a failed check throws, anywhere in the host code.  `guarded` (api_internal.hpp) turns it into its status code
// and an error-detail string.  No HIP: the pure host code (host_planes.hpp) throws it too.
#pragma once
#include <string>

namespace rrt {
struct Error { int status; std::string detail; };
}  // namespace rrt
