// cover_pool_model.cpp -- the buffer choice of the coverage pass (csrc/cover_pool.hpp: pick_cover_buffer) driven through scripted sequences on the host, with a
// small model of what the GPU does around it: every stream renders its frames in order, a frame completes when the script says so, and a buffer's `completed`
// is "the frame that used it last has completed".  Stand-alone: built and run by tests/test_cover_pool_model.py, plainly and with the sanitizers.
//
// Checked after EVERY pick, whatever the scenario:
//   * the index is -1 or inside the pool; `wait` is set exactly when the buffer's last frame is still in flight;
//   * a busy buffer is only ever handed to the stream that used it last (its `done` is then enqueued on the side stream; another stream's frame never shares it);
//   * a buffer handed out busy is the OLDEST in-flight frame of that stream, so with two frames in flight it is never the newest;
//   * no stream holds more than kCoverPerStream buffers unless it was given them while they were free, and -1 only comes when the stream holds nothing and no
//     buffer is free.
// Scenarios: one stream hundreds of frames ahead of the GPU, one stream with the GPU keeping up, twelve streams over eight buffers, completions in every order
// of a small set-up (all permutations), random interleavings of launches and completions, and an exhausted pool.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

#include "cover_pool.hpp"

using namespace rrt;

namespace {

int failures = 0;
long picks = 0, waits = 0, refusals = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Frame { int stream; int buf; bool done; };

// The pool and the frames in flight.  A stream is a small integer; its address in `ids` is the `const void*` the header compares.
struct Model {
    int n;
    std::vector<CoverSlot> slots;
    std::vector<int> last_frame;           // per buffer: index into frames of the frame that used it last, or -1
    std::vector<Frame> frames;
    std::vector<std::deque<int>> queue;    // per stream: its frames in flight, oldest first (a stream runs in order)
    std::vector<char> ids;
    uint64_t clock = 0;
    Model(int n_bufs, int n_streams) : n(n_bufs), slots(n_bufs, CoverSlot{nullptr, false, false, 0}), last_frame(n_bufs, -1), queue(n_streams), ids(n_streams) {}
    const void* id(int s) const { return &ids[(size_t)s]; }
    void refresh() { for (int i = 0; i < n; i++) if (slots[i].used) slots[i].completed = frames[(size_t)last_frame[i]].done; }
    int held(int s) const { int c = 0; for (int i = 0; i < n; i++) c += slots[i].used && slots[i].stream == id(s); return c; }
    // one whole frame on stream s: the pick, the checks, the bookkeeping of take_cover_buffer.  Returns the pick.
    CoverPick launch(int s, int per_stream = kCoverPerStream) {
        refresh();
        const int held_before = held(s);
        bool any_free = false;
        for (int i = 0; i < n; i++) any_free = any_free || !slots[i].used || slots[i].completed;
        const CoverPick p = pick_cover_buffer(slots.data(), n, id(s), per_stream);
        picks++;
        CHECK(p.index >= -1 && p.index < n, "index %d", p.index);
        if (p.index < 0) {
            refusals++;
            CHECK(!p.wait, "wait with no buffer");
            CHECK(held_before == 0 && !any_free, "refused with %d held, free %d", held_before, (int)any_free);
            frames.push_back(Frame{s, -1, false}); queue[(size_t)s].push_back((int)frames.size() - 1);
            return p;
        }
        const CoverSlot& b = slots[(size_t)p.index];
        const bool busy = b.used && !b.completed;
        CHECK(p.wait == busy, "buffer %d: wait %d, busy %d", p.index, (int)p.wait, (int)busy);
        if (busy) {
            waits++;
            CHECK(b.stream == id(s), "a busy buffer of another stream was handed to stream %d", s);
            CHECK(held_before >= per_stream || !any_free, "stream %d waits with %d held although a buffer is free", s, held_before);
            // the oldest frame of this stream that still holds a mask
            int oldest = -1;
            for (int f : queue[(size_t)s]) if (frames[(size_t)f].buf >= 0 && last_frame[(size_t)frames[(size_t)f].buf] == f) { oldest = f; break; }
            CHECK(oldest == last_frame[(size_t)p.index], "stream %d waits for frame %d, its oldest with a mask is %d", s, last_frame[(size_t)p.index], oldest);
            if (held_before >= 2) CHECK(queue[(size_t)s].back() != last_frame[(size_t)p.index], "stream %d waits for its newest frame", s);
        } else if (b.used && b.stream != id(s)) {
            CHECK(held_before < per_stream, "stream %d took a buffer of another stream while holding %d", s, held_before);
        }
        if (!busy && held_before >= per_stream) CHECK(b.used && b.stream == id(s), "stream %d grew beyond %d buffers", s, per_stream);
        frames.push_back(Frame{s, p.index, false});
        const int f = (int)frames.size() - 1;
        queue[(size_t)s].push_back(f);
        slots[(size_t)p.index] = CoverSlot{id(s), true, false, ++clock};
        last_frame[(size_t)p.index] = f;
        return p;
    }
    // the oldest frame in flight on stream s completes; false when there is none
    bool complete(int s) {
        if (queue[(size_t)s].empty()) return false;
        frames[(size_t)queue[(size_t)s].front()].done = true;
        queue[(size_t)s].pop_front();
        return true;
    }
};

// One stream far ahead of the GPU: after the first two frames every launch waits, alternates between the same two buffers, and waits for the frame before the newest.
void one_stream_far_ahead() {
    Model m(8, 1);
    int a = -1, b = -1;
    for (int k = 0; k < 400; k++) {
        const CoverPick p = m.launch(0);
        if (k == 0) a = p.index;
        if (k == 1) b = p.index;
        CHECK(p.index == (k % 2 ? b : a), "frame %d took buffer %d, the stream alternates %d and %d", k, p.index, a, b);
        CHECK(p.wait == (k >= 2), "frame %d: wait %d", k, (int)p.wait);
        if (k == 1) CHECK(a != b && a >= 0 && b >= 0, "the first two frames took %d and %d", a, b);
        if (k >= 2) CHECK(m.frames[(size_t)m.last_frame[(size_t)p.index]].stream == 0, "own");
    }
    CHECK(m.held(0) == 2, "run-ahead of %d masks", m.held(0));
    // the GPU catches up by one frame between launches: still two buffers, and no wait -- the frame two back has completed
    Model g(8, 1);
    for (int k = 0; k < 100; k++) {
        const CoverPick p = g.launch(0);
        CHECK(!p.wait, "frame %d waits although the frame two back has completed", k);
        if (k >= 1) g.complete(0);
    }
    CHECK(g.held(0) == 2, "a stream that is one frame ahead holds %d buffers", g.held(0));
    // one buffer per stream (the deliberately slow form): correct, but every launch waits for the newest frame -- this is what the second buffer is for
    Model one(8, 1);
    for (int k = 0; k < 10; k++) {
        const CoverPick p = one.launch(0, 1);
        CHECK(p.wait == (k >= 1) && p.index >= 0 && one.last_frame[(size_t)p.index] == k, "one per stream, frame %d: buffer %d, wait %d", k, p.index, (int)p.wait);
    }
    CHECK(one.held(0) == 1, "one per stream holds %d", one.held(0));
}

// Twelve streams over eight buffers, nothing completing: the first eight launches get a buffer each, the other four streams none; a second round gives the eight
// their own buffer again (with a wait) and the four nothing; once everything has completed the four are served from the others' buffers.
void twelve_streams() {
    Model m(8, 12);
    for (int k = 0; k < 12; k++) {
        const CoverPick p = m.launch((k * 5) % 12);
        CHECK((p.index >= 0) == (k < 8), "launch %d got %d", k, p.index);
        CHECK(!p.wait, "launch %d waits", k);
    }
    for (int k = 0; k < 12; k++) {
        const CoverPick p = m.launch((k * 5) % 12);
        CHECK((p.index >= 0) == (k < 8) && p.wait == (k < 8), "second round, launch %d: %d wait %d", k, p.index, (int)p.wait);
    }
    for (int s = 0; s < 12; s++) while (m.complete(s)) {}
    for (int k = 8; k < 12; k++) {
        const CoverPick p = m.launch((k * 5) % 12);
        CHECK(p.index >= 0 && !p.wait, "after completion, launch %d: %d wait %d", k, p.index, (int)p.wait);
    }
    int with = 0;
    for (int s = 0; s < 12; s++) with += m.held(s) > 0;
    CHECK(with == 8, "%d streams hold a buffer", with);
}

// Completions in every order: four streams with two frames each in flight over eight buffers; for every permutation of which stream completes next, every
// stream launches again after each completion.
void completions_in_every_order() {
    std::vector<int> order = {0, 0, 1, 1, 2, 2, 3, 3};
    long perms = 0;
    do {
        Model m(8, 4);
        for (int round = 0; round < 2; round++) for (int s = 0; s < 4; s++) m.launch(s);
        for (int s : order) {
            m.complete(s);
            for (int t = 0; t < 4; t++) m.launch(t);
        }
        perms++;
    } while (std::next_permutation(order.begin(), order.end()));
    CHECK(perms == 2520, "%ld permutations", perms);
}

void random_interleavings(unsigned n_runs) {
    std::mt19937 rng(12345);
    for (unsigned run = 0; run < n_runs; run++) {
        const int n_bufs = 1 + (int)(rng() % 8), n_streams = 1 + (int)(rng() % 12);
        Model m(n_bufs, n_streams);
        const unsigned bias = rng() % 4;                                   // how eager the GPU is
        for (int step = 0; step < 200; step++) {
            const int s = (int)(rng() % (unsigned)n_streams);
            if (rng() % 4 < bias) m.complete(s); else m.launch(s);
        }
    }
}

void pool_exhausted() {
    Model m(8, 9);
    for (int s = 0; s < 8; s++) CHECK(m.launch(s).index >= 0, "stream %d", s);
    const CoverPick p = m.launch(8);
    CHECK(p.index == -1 && !p.wait, "ninth stream got %d", p.index);
    m.complete(3);
    const CoverPick q = m.launch(8);
    CHECK(q.index >= 0 && !q.wait && m.frames[(size_t)3].done, "after stream 3 completed the ninth got %d", q.index);
    Model empty(0, 1);
    CHECK(empty.launch(0).index == -1, "a pool of no buffers");
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned n_runs = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 2000u;
    one_stream_far_ahead();
    twelve_streams();
    completions_in_every_order();
    random_interleavings(n_runs);
    pool_exhausted();
    std::printf("picks=%ld waits=%ld refusals=%ld failures=%d\n", picks, waits, refusals, failures);
    return failures ? 1 : 0;
}
