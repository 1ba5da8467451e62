// staging.cpp -- the process-wide transfer infrastructure: one pinned staging ring and two set-up streams per device (staging.hpp).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "hip_check.hpp"
#include "model.hpp"
#include "parallel.hpp"
#include "staging.hpp"

namespace rrt {
namespace {

// ---- pinned staging: one ring of page-locked chunks per device, shared by every upload and every pageable-framebuffer download of the process.
// A slot's event says when the DMA that last used it has finished; a slot is waited for right before it is reused, never at the end of a call.
struct StagingRing {
    static constexpr int kSlots = 8; static constexpr size_t kSlotBytes = (size_t)4 << 20;
    char* mem = nullptr; hipEvent_t ev[kSlots] = {}; bool busy[kSlots] = {}; size_t next = 0; hipStream_t stream = nullptr, stream2 = nullptr;
    void ensure() {
        if (mem) return;
        HIP_TRY(hipHostMalloc((void**)&mem, kSlots * kSlotBytes, hipHostMallocDefault));
        for (auto& e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));   // the device's set-up stream (creating one costs ~3 ms: done once, by the warm-up thread when it runs)
        HIP_TRY(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));  // uploads beside the build (upload_stream)
    }
    int acquire() {                                                     // next slot, free to be written
        const int s = (int)(next++ % kSlots);
        if (busy[s]) { HIP_TRY(hipEventSynchronize(ev[s])); busy[s] = false; }
        return s;
    }
    void release(int s, hipStream_t st) { HIP_TRY(hipEventRecord(ev[s], st)); busy[s] = true; }
};
constexpr int kMaxDevices = 64;
std::mutex g_ring_mu;
StagingRing g_rings[kMaxDevices];
StagingRing& ring_of_current_device() {                                 // (caller holds g_ring_mu)
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) throw Error{RRT_ERR_INVALID_ARG, "device index beyond the staging table"};
    g_rings[dev].ensure();
    return g_rings[dev];
}
// parallel memcpy on the host pool (copies out of the ring on the frame path: one core moves ~10 GB/s)
void copy_bytes(char* dst, const char* src, size_t len) {
    if (len < ((size_t)2 << 20)) { std::memcpy(dst, src, len); return; }
    parallel_ranges(len, (len + 3) / 4, [&](size_t b, size_t e, size_t) { std::memcpy(dst + b, src + b, e - b); });
}

}  // namespace

void staged_upload_warm() { try { std::lock_guard<std::mutex> lk(g_ring_mu); (void)ring_of_current_device(); } catch (...) { (void)hipGetLastError(); } }

void* setup_stream() { std::lock_guard<std::mutex> lk(g_ring_mu); return ring_of_current_device().stream; }
void* upload_stream() { std::lock_guard<std::mutex> lk(g_ring_mu); return ring_of_current_device().stream2; }

void staged_upload(void* dst, const void* src, size_t bytes, void* stream_) {
    if (!bytes) return;
    hipStream_t stream = (hipStream_t)stream_;
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost) {   // already page-locked: one DMA, read from src until the stream has drained (staging.hpp)
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        return;
    }
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(g_ring_mu);
    StagingRing& R = ring_of_current_device();
    const size_t S = StagingRing::kSlotBytes, n_chunks = (bytes + S - 1) / S;
    // One task per ring slot (host pool), each an independent pipeline: wait for the slot's last DMA, fill the slot from `src`, enqueue its DMA, take the next
    // chunk -- so the copies into page-locked memory (the slow part: one core moves ~10 GB/s) run on several cores while the DMA engine drains
    // the finished slots.  Chunks land at disjoint destinations: their order on the stream does not matter.
    const unsigned workers = (unsigned)std::min<size_t>(std::min<size_t>(StagingRing::kSlots, n_chunks), host_threads());
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::atomic<size_t> next_chunk{0};
    std::vector<int> err(workers, 0);
    auto run = [&](unsigned w) {
        if (hipSetDevice(dev) != hipSuccess) { err[w] = (int)hipGetLastError(); return; }        // (HIP's current device is per thread, and a pool worker keeps its last one)
        char* stage = R.mem + (size_t)w * S;
        for (size_t c; (c = next_chunk.fetch_add(1)) < n_chunks;) {
            const size_t off = c * S, len = std::min(S, bytes - off);
            hipError_t e = hipSuccess;
            if (R.busy[w]) { e = hipEventSynchronize(R.ev[w]); R.busy[w] = false; }
            if (e == hipSuccess) { std::memcpy(stage, static_cast<const char*>(src) + off, len); e = hipMemcpyAsync(static_cast<char*>(dst) + off, stage, len, hipMemcpyHostToDevice, stream); }
            if (e == hipSuccess) { e = hipEventRecord(R.ev[w], stream); R.busy[w] = true; }
            if (e != hipSuccess) { err[w] = (int)e; return; }
        }
    };
    parallel_ranges(workers, 1, [&](size_t b, size_t e, size_t) { for (size_t w = b; w < e; w++) run((unsigned)w); });
    for (int e : err) if (e) throw HipFail{(hipError_t)e, "staged_upload (pinned-staging host-to-device copy)"};
    // src has been read completely: it may be freed.  dst is complete once `stream` has drained; the slots guard themselves (busy + event).
}

// Device -> host memory, page-locked or not.  A page-locked `dst` (rrt_host_buffer_register, hipHostMalloc, ...) gets ONE asynchronous DMA.  A pageable one goes
// through the ring: chunk DMAs run ahead while the finished chunks are copied out (a pageable hipMemcpy stages through the runtime's own bounce buffers
// serially; a frame-sized pinned buffer of the caller's own costs milliseconds to allocate -- more than the reference's one frame takes to trace), which
// waits for everything enqueued on `stream` before the call.  Either way dst is complete once the caller has synchronised `stream` (staging.hpp).
void staged_download(void* dst, const void* src_dev, size_t bytes, void* stream_) {
    if (!bytes) return;
    hipStream_t stream = (hipStream_t)stream_;
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, dst) == hipSuccess && attr.type == hipMemoryTypeHost) {
        HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, stream));
        return;
    }
    (void)hipGetLastError();                                              // ("not registered" is sticky)
    std::lock_guard<std::mutex> lk(g_ring_mu);
    StagingRing& R = ring_of_current_device();
    size_t chunk = (bytes / 8 + 0xFFFFF) & ~(size_t)0xFFFFF;              // about 8 chunks per frame, whole MiB, at most a slot
    chunk = std::min(std::max(chunk, (size_t)1 << 20), StagingRing::kSlotBytes);
    const size_t n_chunks = (bytes + chunk - 1) / chunk;
    int slot_of[StagingRing::kSlots];
    size_t issued = 0;
    auto issue = [&](size_t c) {
        const int slot = R.acquire();
        const size_t off = c * chunk, len = std::min(chunk, bytes - off);
        HIP_TRY(hipMemcpyAsync(R.mem + (size_t)slot * StagingRing::kSlotBytes, static_cast<const char*>(src_dev) + off, len, hipMemcpyDeviceToHost, stream));
        R.release(slot, stream);
        slot_of[c % StagingRing::kSlots] = slot;
    };
    for (; issued < n_chunks && issued < (size_t)StagingRing::kSlots; issued++) issue(issued);
    for (size_t c = 0; c < n_chunks; c++) {
        const int slot = slot_of[c % StagingRing::kSlots];
        HIP_TRY(hipEventSynchronize(R.ev[slot])); R.busy[slot] = false;
        const size_t off = c * chunk, len = std::min(chunk, bytes - off);
        copy_bytes(static_cast<char*>(dst) + off, R.mem + (size_t)slot * StagingRing::kSlotBytes, len);
        if (issued < n_chunks) issue(issued++);
    }
}

}  // namespace rrt
