// k_combiner.hip -- AudioCombiner (reference include/hpfw/audioproblems/combiner/combiner.h:90-132) on the device:
// the exact-hash inverted index over uint16 hashprints and the offset-vote search, integer work only, bitwise
// deterministic (no atomics: every bin is written by one thread per launch).
//
// Index (build_db, :90-97).  A stable radix sort of (value, global position) gives the postings of every value in
// ascending position = (recording, offset); val_start[v] is the first posting of value v (a lower bound in the sorted
// values).  Appending recordings re-sorts everything: the result is the rebuild by construction.
//
// Search (find, :100-132).  The events of a query in stream order are (frame c ascending, then the postings of Q[c] in
// index order, the excluded recording's contiguous sub-range of each list skipped).  Per frame its number of events; an
// exclusive scan of those numbers over a batch of queries gives every event its stream index, so events are generated
// already in stream order, in chunks of a bounded number of events (a chunk may end inside a frame).  An event of
// recording j at d = c - o falls into bin (q, j, d) of a dense per-query array: row j holds C_q + L_j - 1 bins
// (d = -(L_j - 1) .. C_q - 1).  Inside a bin, stream order is c order and one frame touches a bin at most once, so a
// stable sort of the chunk's events by bin gives every event its rank among the chunk's events of its bin;
// count = (the bin's total over earlier chunks) + rank + 1, and the bin's total is then advanced.  One wave per query
// applies the reference's rule to the counts in stream order: ballot(count > confidence), the first set lane updates the
// result, the ballot is taken again from the lane after it -- O(events / 64 + updates), state carried across chunks.
//
// Alignment: after the last chunk the bins hold the complete per-offset event counts; a segmented argmax per (query,
// recording) row (ties to the smallest d) and a top-k over recordings by (peak desc, rec asc).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "combiner.h"

namespace hpfw {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kNone = 0xffffffffu;

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// last index i in [0, n) with a[i] <= x (a ascending, a[0] <= x)
template <class T, class U>
__device__ __forceinline__ int64_t last_le(const T *a, int64_t n, U x)
{
    int64_t lo = 0, hi = n; // answer in [lo, hi)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((U)a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- index -----------------------------------------------------------------------------------------------------------
__global__ void iota_kernel(uint32_t *v, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

// val_start[v] = first i with keys[i] >= v, v = 0 .. 65536
__global__ void val_start_kernel(const uint16_t *keys, int64_t n, uint32_t *val_start)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v > 65536) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int)keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    val_start[v] = (uint32_t)lo;
}

// posting i: its global position -> (recording, offset); rec_off [n_rec + 1] (empty recordings repeat an offset: the
// last recording whose start is <= the position is the non-empty one holding it)
__global__ void postings_kernel(const uint32_t *pos, int64_t n, const uint32_t *rec_off, int64_t n_rec, uint2 *post)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pos[i];
    const int64_t j = last_le(rec_off, n_rec + 1, p);
    post[i] = make_uint2((uint32_t)j, p - rec_off[j]);
}

// ---- search ----------------------------------------------------------------------------------------------------------
// per query of a batch (uploaded together): frame start in the batch, bin base, source offset in the queries, exclusion
struct QueryTab {
    uint32_t frame0;   // first frame of the query in the batch; frame0 of the next query ends it
    uint32_t bin0;     // first bin of the query in the batch
    int32_t exclude;   // recording skipped, -1 = none
    uint32_t q_global; // index of the query in the call
    int64_t src;       // first hashprint of the query in d_q
};

// per frame of the batch: its posting list (minus the excluded range) and the query it belongs to
struct FrameTab {
    uint32_t begin;    // first posting of Q[c]
    uint32_t skip_at;  // events before the excluded range
    uint32_t skip;     // postings of the excluded recording
    uint32_t q;        // query in the batch
};

__global__ void frames_kernel(const uint16_t *q_hp, const QueryTab *qt, int nq, int64_t n_frames, const uint32_t *val_start,
                              const uint2 *post, FrameTab *ft, int64_t *len)
{
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f > n_frames) return;
    if (f == n_frames) { // the scan's last element: the stream index one past the last event
        len[f] = 0;
        return;
    }
    // the query holding frame f: the last whose frame0 <= f (queries without frames repeat a frame0)
    int lo = 0, hi = nq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (qt[mid].frame0 <= (uint32_t)f) lo = mid;
        else hi = mid;
    }
    const QueryTab t = qt[lo];
    const uint16_t v = q_hp[t.src + (f - t.frame0)];
    const uint32_t b = val_start[v], e = val_start[v + 1];
    uint32_t xa = e, xb = e;
    if (t.exclude >= 0) { // the excluded recording's postings: a contiguous sub-range (recordings ascend in a list)
        const uint32_t ex = (uint32_t)t.exclude;
        uint32_t l = b, r = e;
        while (l < r) {
            const uint32_t m = (l + r) >> 1;
            if (post[m].x < ex) l = m + 1;
            else r = m;
        }
        xa = l;
        r = e;
        while (l < r) {
            const uint32_t m = (l + r) >> 1;
            if (post[m].x <= ex) l = m + 1;
            else r = m;
        }
        xb = l;
    }
    ft[f] = FrameTab{b, xa - b, xb - xa, (uint32_t)lo};
    len[f] = (int64_t)(e - b) - (int64_t)(xb - xa);
}

// rows of a query's bin array: row j starts at j (C_q - 1) + rec_off[j] and holds C_q - 1 + L_j bins
__device__ __forceinline__ uint32_t row_base(uint32_t j, uint32_t cq1, const uint32_t *rec_off) { return j * cq1 + rec_off[j]; }

// events [e0, e0 + n) of the batch's stream: bin key, recording and chunk index
__global__ void events_kernel(const int64_t *ev_start, int64_t n_frames, const FrameTab *ft, const QueryTab *qt,
                              const uint2 *post, const uint32_t *rec_off, int64_t e0, int64_t n, uint32_t *keys, uint32_t *recs,
                              uint32_t *vals)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t e = e0 + i;
    const int64_t f = last_le(ev_start, n_frames, e); // the last frame starting at or before e is the non-empty one
    const FrameTab fr = ft[f];
    const QueryTab t = qt[fr.q];
    const uint32_t cq1 = qt[fr.q + 1].frame0 - t.frame0 - 1;
    const uint32_t k = (uint32_t)(e - ev_start[f]);
    const uint2 p = post[fr.begin + k + (k >= fr.skip_at ? fr.skip : 0u)];
    const uint32_t c = (uint32_t)(f - t.frame0);
    // d = c - o at index d + L_j - 1 of row j: row_base(j) + L_j - 1 + c - o = j (C_q - 1) + rec_off[j + 1] - 1 + c - o
    keys[i] = t.bin0 + p.x * cq1 + rec_off[p.x + 1] - 1u + c - p.y;
    recs[i] = p.x;
    vals[i] = (uint32_t)i;
}

// count of the event at sorted position p: the bin's total before this chunk + its rank in the bin's run + 1
__global__ void counts_kernel(const uint32_t *keys_s, const uint32_t *vals_s, int64_t n, const uint32_t *bins, uint32_t *cnt)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t key = keys_s[p];
    // the run's first position: gallop back, then bisect (runs are short but may be long for skewed hashes)
    int64_t lo = p, step = 1;
    while (lo - step >= 0 && keys_s[lo - step] == key) {
        lo -= step;
        step <<= 1;
    }
    int64_t a = std::max<int64_t>(lo - step + 1, 0), b = lo;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (keys_s[m] == key) b = m;
        else a = m + 1;
    }
    cnt[vals_s[p]] = bins[key] + (uint32_t)(p - a) + 1u;
}

// the last event of every run advances its bin to its own count
__global__ void carry_kernel(const uint32_t *keys_s, const uint32_t *vals_s, int64_t n, const uint32_t *cnt, uint32_t *bins)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t key = keys_s[p];
    if (p + 1 == n || keys_s[p + 1] != key) bins[key] = cnt[vals_s[p]];
}

__global__ void find_init_kernel(hpfw_combine_result *out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = hpfw_combine_result{kNone, 0, 0, 0, 0};
}

// the reference's rule over the chunk's events of every query, in stream order; one wave (block of 64) per query
__global__ __launch_bounds__(64) void rule_kernel(const int64_t *ev_start, const QueryTab *qt, const uint32_t *keys,
                                                  const uint32_t *recs, const uint32_t *cnt, int64_t e0, int64_t n,
                                                  const uint32_t *rec_off, hpfw_combine_result *out)
{
    const int qb = blockIdx.x;
    const int lane = threadIdx.x;
    const QueryTab t = qt[qb];
    const uint32_t frames = qt[qb + 1].frame0 - t.frame0;
    const int64_t qa = ev_start[t.frame0], qe = ev_start[t.frame0 + frames];
    const int64_t b = (qa > e0 ? qa : e0) - e0, e = (qe < e0 + n ? qe : e0 + n) - e0;
    if (b >= e) return;
    const uint32_t cq1 = frames - 1;
    hpfw_combine_result r = out[t.q_global];
    for (int64_t base = b; base < e; base += 64) {
        const int64_t i = base + lane;
        const bool valid = i < e;
        const uint32_t c = valid ? cnt[i] : 0u, key = valid ? keys[i] : 0u, rec = valid ? recs[i] : 0u;
        uint64_t pending = __ballot(valid);
        while (true) {
            const uint64_t m = __ballot((int64_t)c > r.confidence) & pending;
            if (!m) break;
            const int L = __ffsll((unsigned long long)m) - 1;
            pending &= L == 63 ? 0ull : (~0ull << (L + 1));
            const uint32_t cl = (uint32_t)__shfl((int)c, L), kl = (uint32_t)__shfl((int)key, L);
            const uint32_t j = (uint32_t)__shfl((int)rec, L);
            // the bin's offset within row j (events_kernel's key inverted): one load, no search in the serial part
            const int64_t d = (int64_t)(kl - t.bin0) - (int64_t)j * cq1 - (int64_t)rec_off[j + 1] + 1;
            if (j != r.rec) r = hpfw_combine_result{j, 0, (int64_t)cl, 1, d};
            else r = hpfw_combine_result{j, 0, (int64_t)cl, r.confidence + 1, d};
        }
    }
    if (lane == 0) out[t.q_global] = r;
}

// per (query, recording) row: peak = max bin, offset = smallest d reaching it; one block per row
__global__ void peaks_kernel(const QueryTab *qt, const uint32_t *bins, const uint32_t *rec_off, int64_t n_rec, uint64_t *peaks)
{
    const int64_t row = blockIdx.x;
    const int qb = (int)(row / n_rec);
    const uint32_t j = (uint32_t)(row % n_rec);
    const QueryTab t = qt[qb];
    const uint32_t frames = qt[qb + 1].frame0 - t.frame0;
    __shared__ uint64_t red[kThreads / 64];
    uint64_t best = 0; // (count << 32) | ~index: the largest count, then the smallest index
    if (frames > 0 && (int32_t)j != t.exclude) {
        const uint32_t lj = rec_off[j + 1] - rec_off[j], len = frames - 1 + lj;
        const uint32_t *rowp = bins + t.bin0 + row_base(j, frames - 1, rec_off);
        for (uint32_t i = threadIdx.x; i < len; i += kThreads) {
            const uint32_t v = rowp[i];
            if (v) best = std::max(best, ((uint64_t)v << 32) | (uint64_t)(~i));
        }
    }
    for (int s = 32; s >= 1; s >>= 1) best = std::max(best, (uint64_t)__shfl_xor((unsigned long long)best, s));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) best = std::max(best, red[w]);
        peaks[row] = best;
    }
}

// top-k recordings of every query by (peak desc, rec asc); one block per query
__global__ void align_topk_kernel(const QueryTab *qt, const uint64_t *peaks, const uint32_t *rec_off, int64_t n_rec, int k,
                                  hpfw_align_hit *out)
{
    const int qb = blockIdx.x;
    const QueryTab t = qt[qb];
    const uint64_t *pk = peaks + (int64_t)qb * n_rec;
    __shared__ uint64_t red[kThreads / 64];
    uint64_t below = ~0ull; // keys (peak << 32) | ~rec are distinct: each round takes the largest one below the last
    for (int r = 0; r < k; ++r) {
        uint64_t best = 0;
        for (int64_t j = threadIdx.x; j < n_rec; j += kThreads) {
            const uint32_t peak = (uint32_t)(pk[j] >> 32);
            const uint64_t key = ((uint64_t)peak << 32) | (uint32_t)~(uint32_t)j;
            if (peak && key < below) best = std::max(best, key);
        }
        for (int s = 32; s >= 1; s >>= 1) best = std::max(best, (uint64_t)__shfl_xor((unsigned long long)best, s));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
        __syncthreads();
        for (int w = 0; w < kThreads / 64; ++w) best = std::max(best, red[w]);
        __syncthreads();
        if (threadIdx.x == 0) {
            hpfw_align_hit hit{kNone, 0, 0};
            if (best) {
                const uint32_t j = ~(uint32_t)best;
                const uint32_t idx = ~(uint32_t)pk[j];
                hit = hpfw_align_hit{j, (uint32_t)(best >> 32), (int64_t)idx - (int64_t)(rec_off[j + 1] - rec_off[j]) + 1};
            }
            out[(int64_t)t.q_global * k + r] = hit;
        }
        if (!best) below = 0;
        else below = best;
    }
}

__global__ void align_pad_kernel(hpfw_align_hit *out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = hpfw_align_hit{kNone, 0, 0};
}

int hip_fail(hipError_t e, const char *what, std::string &err)
{
    err = std::string(what) + ": " + hipGetErrorString(e);
    return HPFW_E_HIP;
}

#define CB_TRY(expr)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return hip_fail(e_, #expr, err);                                                          \
    } while (0)
#define CB_LAUNCH(name)                                                                                                 \
    do {                                                                                                                \
        hipError_t e_ = hipGetLastError();                                                                              \
        if (e_ != hipSuccess) return hip_fail(e_, "launch of " name, err);                                              \
    } while (0)

int bits_for(uint64_t n) // key bits of values < n
{
    int b = 1;
    while (b < 32 && (1ull << b) < n) ++b;
    return b;
}

// HPFW_COMBINER_WORKSPACE_MB: bins + event chunk per pass (default 1 GiB; at most 8 GiB: bin keys are 32-bit)
size_t workspace_cap()
{
    const char *v = std::getenv("HPFW_COMBINER_WORKSPACE_MB");
    long long mb = v && *v ? std::atoll(v) : 1024;
    mb = std::max<long long>(1, std::min<long long>(mb, 8192));
    return (size_t)mb << 20;
}

constexpr size_t kEventBytes = 36;          // keys, values and their sorted copies, recordings, counts, the sort's own double buffer
constexpr int64_t kMaxHashprints = 0x7fffffff; // the index sort takes an int item count
constexpr int64_t kMinChunk = (int64_t)1 << 16;
constexpr int64_t kMaxBatch = 1024;         // queries per pass (bounds the peak table: kMaxBatch x n_rec)

// a scratch buffer of at least `bytes` (256 at least: never a null one, which hipcub takes for a size query)
hipError_t grow(DevBuf &b, size_t bytes) { return b.ensure(std::max<size_t>(bytes, 256)); }

} // namespace

void Combiner::clear() { rec_off_.assign(1, 0); } // (the device tables are rebuilt by the next add)

int Combiner::add(const uint16_t *hp, bool device, const int64_t *offsets, int64_t n_rec, hipStream_t s, std::string &err)
{
    if (n_rec < 0 || (n_rec > 0 && (!hp || !offsets))) {
        err = "bad argument";
        return HPFW_E_INVALID;
    }
    for (int64_t i = 0; i < n_rec; ++i)
        if (offsets[i + 1] < offsets[i]) {
            err = "offsets must be non-decreasing";
            return HPFW_E_INVALID;
        }
    if (n_rec == 0) return 0;
    const int64_t have = rec_off_.back(), add = offsets[n_rec] - offsets[0];
    if (have + add > kMaxHashprints || size() + n_rec >= (int64_t)0x7fffffff) {
        err = "combiner index: more than 2^31 - 1 hashprints";
        return HPFW_E_INVALID;
    }
    if ((size_t)(have + add) * 2 > hp_.capacity()) { // grow by doubling, keeping what is there
        DevBuf nd;
        CB_TRY(nd.alloc(std::max<size_t>((size_t)(have + add) * 2, hp_.capacity() * 2)));
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess && have) e = hipMemcpy(nd.get(), hp_.get(), (size_t)have * 2, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return hip_fail(e, "growing the combiner index", err);
        hp_ = std::move(nd); // (the old buffer goes with nd)
    }
    uint16_t *dst = (uint16_t *)hp_.get() + have;
    if (add) {
        if (device) CB_TRY(hipMemcpyAsync(dst, hp + offsets[0], (size_t)add * 2, hipMemcpyDeviceToDevice, s));
        else CB_TRY(hipMemcpy(dst, hp + offsets[0], (size_t)add * 2, hipMemcpyHostToDevice));
    }
    const size_t keep = rec_off_.size();
    for (int64_t i = 0; i < n_rec; ++i) rec_off_.push_back(have + (offsets[i + 1] - offsets[0]));
    const int rc = rebuild(s, err);
    if (rc) rec_off_.resize(keep); // the index stays what it was (stale_: rebuilt before it is read again)
    return rc;
}

int Combiner::rebuild(hipStream_t s, std::string &err)
{
    stale_ = true; // until the tables below are complete
    const int64_t n = rec_off_.back(), n_rec = size();
    std::vector<uint32_t> ro(rec_off_.begin(), rec_off_.end());
    CB_TRY(grow(rec_off_d_, ro.size() * 4));
    CB_TRY(grow(val_start_, 65537 * 4));
    CB_TRY(grow(post_, (size_t)n * 8));
    CB_TRY(grow(sort_keys_, (size_t)n * 2));
    CB_TRY(grow(sort_vals_, (size_t)n * 4));
    CB_TRY(grow(sort_vals_out_, (size_t)n * 4));
    CB_TRY(hipMemcpyAsync(rec_off_d_.get(), ro.data(), ro.size() * 4, hipMemcpyHostToDevice, s));
    size_t tb = 0;
    CB_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint16_t *)hp_.get(), (uint16_t *)sort_keys_.get(),
                                              (const uint32_t *)sort_vals_.get(), (uint32_t *)sort_vals_out_.get(), (int)n, 0, 16, s));
    CB_TRY(grow(temp_, tb));
    if (n) {
        iota_kernel<<<grid_of(n), kThreads, 0, s>>>((uint32_t *)sort_vals_.get(), n);
        CB_LAUNCH("combiner iota");
        tb = temp_.capacity();
        CB_TRY(hipcub::DeviceRadixSort::SortPairs(temp_.get(), tb, (const uint16_t *)hp_.get(), (uint16_t *)sort_keys_.get(),
                                                  (const uint32_t *)sort_vals_.get(), (uint32_t *)sort_vals_out_.get(), (int)n, 0, 16, s));
        postings_kernel<<<grid_of(n), kThreads, 0, s>>>((const uint32_t *)sort_vals_out_.get(), n, (const uint32_t *)rec_off_d_.get(),
                                                        n_rec, (uint2 *)post_.get());
        CB_LAUNCH("combiner postings");
    }
    val_start_kernel<<<grid_of(65537), kThreads, 0, s>>>((const uint16_t *)sort_keys_.get(), n, (uint32_t *)val_start_.get());
    CB_LAUNCH("combiner val_start");
    // the host vector ro dies here: the copy above must have left it
    CB_TRY(hipStreamSynchronize(s));
    stale_ = false;
    return 0;
}

int Combiner::get(int64_t *val_start, uint32_t *rec, uint32_t *off, int64_t cap, std::string &err)
{
    const int64_t n = rec_off_.back();
    if (!val_start || ((rec || off) && cap < n)) {
        err = !val_start ? "null val_start" : "posting buffers smaller than the index";
        return HPFW_E_INVALID;
    }
    CB_TRY(hipDeviceSynchronize());
    if (!val_start_.get() || n == 0) { // nothing added since the last clear (the device tables are those of before)
        std::fill(val_start, val_start + 65537, 0);
        return 0;
    }
    if (stale_) { // an append whose rebuild failed was rolled back: the tables are rebuilt for the index as it stands
        const int rc = rebuild(nullptr, err);
        if (rc) return rc;
    }
    std::vector<uint32_t> vs(65537);
    CB_TRY(hipMemcpy(vs.data(), val_start_.get(), 65537 * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < 65537; ++i) val_start[i] = vs[(size_t)i];
    if ((rec || off) && n) {
        std::vector<uint32_t> p((size_t)n * 2);
        CB_TRY(hipMemcpy(p.data(), post_.get(), (size_t)n * 8, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            if (rec) rec[i] = p[(size_t)i * 2];
            if (off) off[i] = p[(size_t)i * 2 + 1];
        }
    }
    return 0;
}

int Combiner::search(const uint16_t *d_q, const int64_t *q_off, const int32_t *exclude, int64_t n_q, hpfw_combine_result *d_find,
                     int k, hpfw_align_hit *d_align, hipStream_t s, std::string &err)
{
    if (n_q < 0 || !q_off || (d_align && (k < 1 || k > 64))) {
        err = "bad argument";
        return HPFW_E_INVALID;
    }
    if (n_q == 0) return 0;
    const int64_t n_rec = size(), n = rec_off_.back();
    int64_t total_frames = 0;
    for (int64_t q = 0; q < n_q; ++q) {
        if (q_off[q + 1] < q_off[q]) {
            err = "q_off must be non-decreasing";
            return HPFW_E_INVALID;
        }
        if (exclude && exclude[q] < -1) {
            err = "exclude must be a recording id or -1";
            return HPFW_E_INVALID;
        }
        total_frames += q_off[q + 1] - q_off[q];
    }
    if (total_frames && !d_q) {
        err = "null queries";
        return HPFW_E_INVALID;
    }
    if (d_find) {
        find_init_kernel<<<grid_of(n_q), kThreads, 0, s>>>(d_find, n_q);
        CB_LAUNCH("combiner find_init");
    }
    if (d_align) {
        align_pad_kernel<<<grid_of(n_q * k), kThreads, 0, s>>>(d_align, n_q * k);
        CB_LAUNCH("combiner align_pad");
    }
    if (n == 0) return 0; // an empty index: no events, no peaks
    if (stale_) { // see get()
        const int rc = rebuild(s, err);
        if (rc) return rc;
    }
    const size_t cap = workspace_cap();
    // queries per pass: also bounded by the peak table, [queries][n_rec] uint64
    const int64_t max_batch = std::max<int64_t>(1, std::min<int64_t>(kMaxBatch, ((int64_t)1 << 24) / std::max<int64_t>(n_rec, 1)));
    for (int64_t q0 = 0; q0 < n_q;) {
        // a batch: queries while their bins stay within half the workspace (one query may take all of it)
        std::vector<QueryTab> qt;
        uint64_t bins = 0, frames = 0;
        int64_t q1 = q0;
        for (; q1 < n_q && q1 - q0 < max_batch; ++q1) {
            const int64_t cq = q_off[q1 + 1] - q_off[q1];
            const uint64_t qb = cq > 0 ? (uint64_t)n_rec * (uint64_t)(cq - 1) + (uint64_t)n : 0;
            if (qb * 4 > cap) {
                err = "combiner: the bin array of query " + std::to_string(q1) + " (" + std::to_string(qb * 4 >> 20) +
                      " MiB) exceeds the workspace cap HPFW_COMBINER_WORKSPACE_MB = " + std::to_string(cap >> 20);
                return HPFW_E_INVALID;
            }
            if (q1 > q0 && (bins + qb) * 4 > cap / 2) break;
            if (frames + cq >= 0xffffffffull) break;
            const int32_t ex = exclude ? exclude[q1] : -1;
            qt.push_back(QueryTab{(uint32_t)frames, (uint32_t)bins, ex, (uint32_t)q1, q_off[q1]});
            bins += qb;
            frames += (uint64_t)cq;
        }
        qt.push_back(QueryTab{(uint32_t)frames, (uint32_t)bins, -1, 0, 0}); // sentinel: ends the last query
        const int nq = (int)(q1 - q0);
        const int64_t nf = (int64_t)frames;
        CB_TRY(grow(q_tab_, qt.size() * sizeof(QueryTab)));
        CB_TRY(grow(fr_len_, (size_t)(nf + 1) * 8 * 2)); // lengths, then their exclusive scan
        CB_TRY(grow(fr_tab_, (size_t)std::max<int64_t>(nf, 1) * sizeof(FrameTab)));
        CB_TRY(grow(bins_, (size_t)std::max<uint64_t>(bins, 1) * 4));
        CB_TRY(hipMemcpyAsync(q_tab_.get(), qt.data(), qt.size() * sizeof(QueryTab), hipMemcpyHostToDevice, s));
        CB_TRY(hipMemsetAsync(bins_.get(), 0, (size_t)std::max<uint64_t>(bins, 1) * 4, s));
        const QueryTab *d_qt = (const QueryTab *)q_tab_.get();
        int64_t *len = (int64_t *)fr_len_.get(), *ev_start = len + nf + 1;
        frames_kernel<<<grid_of(nf + 1), kThreads, 0, s>>>(d_q, d_qt, nq, nf, (const uint32_t *)val_start_.get(), (const uint2 *)post_.get(),
                                                           (FrameTab *)fr_tab_.get(), len);
        CB_LAUNCH("combiner frames");
        size_t tb = 0;
        CB_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, len, ev_start, nf + 1, s));
        CB_TRY(grow(temp_, tb));
        tb = temp_.capacity();
        CB_TRY(hipcub::DeviceScan::ExclusiveSum(temp_.get(), tb, len, ev_start, nf + 1, s));
        int64_t n_ev = 0;
        CB_TRY(hipMemcpyAsync(&n_ev, ev_start + nf, 8, hipMemcpyDeviceToHost, s));
        CB_TRY(hipStreamSynchronize(s));
        // event chunks: what the bins leave of the workspace, at least kMinChunk events
        const size_t left = cap > bins * 4 ? cap - bins * 4 : 0;
        const int64_t chunk = std::min<int64_t>(std::max<int64_t>((int64_t)(left / kEventBytes), kMinChunk), (int64_t)1 << 30);
        const int64_t ec = std::min(chunk, std::max<int64_t>(n_ev, 1));
        CB_TRY(grow(ev_keys_, (size_t)ec * 4));
        CB_TRY(grow(ev_keys_s_, (size_t)ec * 4));
        CB_TRY(grow(ev_vals_, (size_t)ec * 4));
        CB_TRY(grow(ev_vals_s_, (size_t)ec * 4));
        CB_TRY(grow(ev_rec_, (size_t)ec * 4));
        CB_TRY(grow(ev_cnt_, (size_t)ec * 4));
        const int kb = bits_for(std::max<uint64_t>(bins, 1));
        tb = 0;
        CB_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t *)ev_keys_.get(), (uint32_t *)ev_keys_s_.get(),
                                                  (const uint32_t *)ev_vals_.get(), (uint32_t *)ev_vals_s_.get(), (int)ec, 0, kb, s));
        CB_TRY(grow(temp_, tb));
        uint32_t *keys = (uint32_t *)ev_keys_.get(), *keys_s = (uint32_t *)ev_keys_s_.get(), *vals = (uint32_t *)ev_vals_.get(),
                 *vals_s = (uint32_t *)ev_vals_s_.get(), *cnt = (uint32_t *)ev_cnt_.get(), *bin = (uint32_t *)bins_.get();
        const uint32_t *rof = (const uint32_t *)rec_off_d_.get();
        for (int64_t e0 = 0; e0 < n_ev; e0 += chunk) {
            const int64_t m = std::min(chunk, n_ev - e0);
            events_kernel<<<grid_of(m), kThreads, 0, s>>>(ev_start, nf, (const FrameTab *)fr_tab_.get(), d_qt, (const uint2 *)post_.get(), rof,
                                                          e0, m, keys, (uint32_t *)ev_rec_.get(), vals);
            CB_LAUNCH("combiner events");
            tb = temp_.capacity();
            CB_TRY(hipcub::DeviceRadixSort::SortPairs(temp_.get(), tb, (const uint32_t *)keys, keys_s, (const uint32_t *)vals, vals_s,
                                                      (int)m, 0, kb, s));
            counts_kernel<<<grid_of(m), kThreads, 0, s>>>(keys_s, vals_s, m, bin, cnt);
            CB_LAUNCH("combiner counts");
            carry_kernel<<<grid_of(m), kThreads, 0, s>>>(keys_s, vals_s, m, cnt, bin);
            CB_LAUNCH("combiner carry");
            if (d_find) {
                rule_kernel<<<nq, 64, 0, s>>>(ev_start, d_qt, keys, (const uint32_t *)ev_rec_.get(), cnt, e0, m, rof, d_find);
                CB_LAUNCH("combiner rule");
            }
        }
        if (d_align && n_rec > 0) {
            CB_TRY(grow(peaks_, (size_t)nq * n_rec * 8));
            peaks_kernel<<<(unsigned)(nq * n_rec), kThreads, 0, s>>>(d_qt, bin, rof, n_rec, (uint64_t *)peaks_.get());
            CB_LAUNCH("combiner peaks");
            align_topk_kernel<<<nq, kThreads, 0, s>>>(d_qt, (const uint64_t *)peaks_.get(), rof, n_rec, k, d_align);
            CB_LAUNCH("combiner align_topk");
        }
        // the next batch reuses the tables uploaded from host vectors above
        CB_TRY(hipStreamSynchronize(s));
        q0 = q1;
    }
    return 0;
}

} // namespace hpfw
