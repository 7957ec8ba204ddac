// streams_plan.h -- live feeds: the planning of one push, host arithmetic only.  No HIP: the file and
// streams_plan.cpp compile alone (tools/streams_plan_check.cpp runs them under the host sanitizers).
//
// A feed at rate fs has (L, M, H) of resample_ratio(fs), T = 2 H; a feed at 44 100 Hz has L = M = 1 and H = 0.  After n input
// samples its ring has received the 44.1 kHz samples y[0 .. emitted(n)) of the offline resampler on everything pushed:
//   emitted(n) = 0 for n <= H, else ceil((n - H) L / M)
// and the most it may hold while emitted <= X is H + floor(X M / L) input samples.
#pragma once
#include <cstdint>
#include <vector>

namespace hpfw {

struct RingRun {
    int64_t src, dst, count; // `count` staged samples from src + `src` to slab + `dst`: one run inside one ring
};
struct RingWindow {
    int64_t base, start; // a window's ring at slab + base, its first sample at ring position start < capacity
};
// One feed's part in a push at another rate than 44.1 kHz (ring_resample_append_kernel): outputs m0 <= m < m1 of the feed,
// output m0 + j at slab + base + pos0 + j for j < first and at slab + base + (j - first) behind the ring's end.
struct RingRsRun {
    int64_t src;              // the chunk's first sample in the staged PCM
    int64_t n_old, count;     // input samples before the push, and in it
    int64_t m0, m1;           // emitted(n_old), emitted(n_old + count)
    int64_t base, pos0;       // the ring in the slab; m0 mod capacity
    int64_t first;            // min(m1 - m0, capacity - pos0): the outputs in front of the ring's end
    int64_t hist_rd, hist_wr; // the feed's history of T - 1 samples (inputs n_old - (T - 1) .. n_old - 1) and where the new one goes
};

// a feed's state on the host
struct RingFeed {
    int32_t rate = 44100, L = 1, M = 1, H = 0;
    int64_t n = 0, e = 0; // input samples received, windows handed out
    int64_t hist = 0;     // its two history buffers at hist and hist + hist_len in the set's history slab
    int64_t hist_len = 0; // T - 1 rounded up to 8 samples; 0 at 44.1 kHz
    int32_t cur = 0;      // which of the two is current
};

int64_t ring_emitted(int64_t n, int32_t L, int32_t M, int32_t H);
// the input samples a feed can take now: H + floor((e hop + capacity) M / L) - n
int64_t ring_room(const RingFeed &f, int64_t hop, int64_t capacity);

struct RingPushPlan {
    std::vector<RingRun> copy; // the 44.1 kHz feeds: one run per chunk, or two when it passes the ring's end
    int64_t copy_longest = 0;
    struct Group {
        int32_t rate, first, n; // runs rs[first .. first + n) are the feeds at `rate` that take part
        int64_t most;           // the most outputs of one of them
    };
    std::vector<RingRsRun> rs; // grouped by rate, the rates in order of their first feed
    std::vector<Group> groups;
    int64_t total = 0; // samples of all chunks
};

// counts [feeds.size()] >= 0, chunks back to back in feed order.  Returns -1 and the plan, or the first feed whose chunk does
// not fit its ring (the plan is then not meaningful).  A feed with count 0 takes no part.
int ring_plan_push(const std::vector<RingFeed> &feeds, const int64_t *counts, int64_t hop, int64_t capacity, RingPushPlan *plan);

} // namespace hpfw
