// cover_pool.hpp -- which buffer of the raytracer's small pool takes the coverage mask of the next whole frame on a stream, and whether its last frame has to be
// waited for first?  (frames.cpp: take_cover_buffer, launch_whole_frame; api_internal.hpp: CoverBuf; DESIGN.md section 4, "coverage pass".)  Plain host logic over
// what the caller found out about the buffers, no HIP in it, so that a stand-alone host program can drive it through scripted sequences
// (tests/cover_pool_model.cpp, tests/test_cover_pool_model.py).
//
// WHY TWO PER STREAM.  The pass of a frame (clear, coverage_kernel) runs on a side stream, beside the render_kernel of the frame BEFORE it on the caller's stream.
// That frame is still reading its own mask, so the pass needs another buffer: a stream alternates between two.  The pass of frame k+1 then waits, at most, for
// render_kernel of frame k-1 (the buffer's `done`), which has long ended when frame k runs: it never waits for the newest frame.  Two is also the bound: a host
// that enqueues hundreds of frames ahead of the GPU gets two masks of run-ahead per stream, not the whole pool, and the other streams keep their buffers.
//
// THE CHOICE, in this order:
//  1. a buffer this stream used last whose frame has completed (the least recently used of them);
//  2. while the stream holds fewer than kCoverPerStream buffers: a buffer never used, else one of ANOTHER stream whose frame has completed (the least recently
//     used: it is taken away from that stream);
//  3. the stream's own least recently used buffer, still busy: `wait` is set, and the pass is enqueued behind that buffer's `done`;
//  4. none (-1): the stream holds nothing and everything else is busy.  The frame renders without a mask (RRT_COVERAGE_OFF_POOL).
// Nothing here blocks the host, and nothing is keyed on a scene or a camera: a buffer is a place, not a cache.
#pragma once
#include <cstdint>

namespace rrt {

constexpr int kCoverPerStream = 2;

// What the choice reads of one buffer.  stream: the stream of the frame it served last; completed: that frame's `done` has completed (hipEventQuery);
// age: the pool's launch counter when it was handed out last -- larger is more recent.  stream, completed and age mean nothing while !used.
struct CoverSlot { const void* stream; bool used; bool completed; uint64_t age; };
struct CoverPick { int index; bool wait; };

inline CoverPick pick_cover_buffer(const CoverSlot* slots, int n, const void* stream, int per_stream = kCoverPerStream) {
    int own_free = -1, own_busy = -1, never = -1, other_free = -1, held = 0;
    const auto older = [&](int i, int than) { return than < 0 || slots[i].age < slots[than].age; };
    for (int i = 0; i < n; i++) {
        const CoverSlot& s = slots[i];
        if (!s.used) { if (never < 0) never = i; continue; }
        if (s.stream == stream) {
            held++;
            if (s.completed) { if (older(i, own_free)) own_free = i; }
            else if (older(i, own_busy)) own_busy = i;
        } else if (s.completed && older(i, other_free)) other_free = i;
    }
    if (own_free >= 0) return {own_free, false};
    if (held < per_stream) {
        if (never >= 0) return {never, false};
        if (other_free >= 0) return {other_free, false};
    }
    if (own_busy >= 0) return {own_busy, true};
    return {-1, false};
}

}  // namespace rrt
