// staging.hpp -- process-wide transfer infrastructure: one ring of page-locked chunks and two non-blocking streams per device, shared by the
// scene set-up's uploads (scene_build.hip, raytracer.cpp) and by every download of a frame or of its planes into host memory (frames.cpp; launches.hpp: with_kept_planes).  A failed HIP call throws HipFail.
#pragma once
#include <cstddef>

namespace rrt {

// Pinned-staging upload of a host buffer (pageable or not) to device memory on `stream`: worker threads fill a ring of page-locked chunks while
// the DMA engine drains it.  Returns after the last chunk has been ENQUEUED; dst is ready after a stream sync.  Pageable `src` has been copied
// out of by then and may be freed at once.  `src` that is already page-locked goes up as ONE asynchronous DMA straight from where it lies: it
// must stay valid and unchanged until `stream` has drained (every caller here synchronises the stream before its source goes away).
void staged_upload(void* dst, const void* src, size_t bytes, void* stream);
void staged_upload_warm();    // allocates the current device's ring and set-up streams (called from the warm-up thread so that the first upload does not pay for it)
// Device memory -> host memory on `stream`: page-locked `dst` as ONE asynchronous DMA, pageable `dst` through the same ring (chunk DMAs run ahead of the
// copies out of the ring).  The data is in `dst` once the caller has synchronised `stream`; for pageable `dst` it is already there on return.
void staged_download(void* dst, const void* src_dev, size_t bytes, void* stream);
// The current device's shared non-blocking stream (hipStream_t) for set-up work and blocking host-framebuffer renders: creating a stream costs
// milliseconds, the reference's whole frame takes less.  Owned by the library; never destroyed.
void* setup_stream();
void* upload_stream();    // a second one, for uploads that run beside work on setup_stream() (textures beside the scene build)

}  // namespace rrt
