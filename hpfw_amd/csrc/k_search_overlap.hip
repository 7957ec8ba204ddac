// k_search_overlap.hip -- the overlap search (include/hpfw_gpu.h): a query may overhang either end of
// a clip, and every alignment is rated by its mismatches per overlapping hashprint.
//
// Lag d puts query position j on clip position d + j.  Over the L(d) = min(k, n - d) - max(0, -d) positions both have,
// dist(d) = sum popcount(q[j] ^ r[d + j]).  A lag with L >= min_overlap is a candidate; candidates are ordered by dist / L
// as an exact rational (cross-multiplied: dist <= 64 L, L <= 16000, products below 2^34), then larger L, then smaller d.
// No floating point takes part in the order.
//
// (a) overlap_mfma_kernel is hamming_mfma_kernel (k_search_mfma.hip) with the clip's window zero-filled on both sides: with
// hashprint bits as fp4 +-1 and fp4 0 outside the query and outside the clip, the accumulator of (query row, lag) is
// 64 L - 2 dist.  A workgroup = 32 queries x 1024 lags of one clip per chunk; the lags of a clip start at
// min_overlap - (the group's longest query) and end at n - min_overlap.
// (b) overlap_popc_kernel computes the same by xor/popcount: queries whose window does not fit the LDS, and the second
// opinion on the device (HPFW_OVERLAP_POPC).
//
// Both write one 16-byte entry {dist, L, lag, 0} per (query, clip, split) with ordinary stores: a clip's chunks are dealt
// round robin to `splits` workgroups, each of which owns its entry (no atomics, nothing depends on the order workgroups
// run in).  overlap_select_kernel folds the splits and picks the k best clips per query.
#include "kernels.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int kOvThreads = 512;                          // 8 waves
constexpr int kOvTiles = 4;                              // lag tiles of 32 per wave
constexpr int kOvWaveLags = 32 * kOvTiles;               // 128
constexpr int kOvWgLags = kOvWaveLags * (kOvThreads / 64); // 1024 lags per chunk (kOverlapChunk)
constexpr int kOvChunk = 16;                             // positions j per staged chunk of the A operand, as kSmChunk
static_assert(kOvWgLags == kOverlapChunk, "kernels.h states the chunk");

constexpr unsigned kNoDist = 1u << 21; // above every distance (64 * 16000 < 2^20); with L = 1 a rate above every rate
constexpr unsigned kLMax = 16383;      // L <= 16000 < 2^14

// 8 bits -> 8 E2M1 nibbles, bit i in nibble i: 0 -> +1.0 (0x2), 1 -> -1.0 (0xA)  (as k_search_mfma.hip)
__device__ __forceinline__ uint32_t ov_expand8(uint32_t x)
{
    uint32_t t = (x | (x << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return 0x22222222u | (t << 3);
}

__device__ __forceinline__ v4i ov_expand32(uint32_t w)
{
    v4i r;
    r.x = (int)ov_expand8(w & 0xff);
    r.y = (int)ov_expand8((w >> 8) & 0xff);
    r.z = (int)ov_expand8((w >> 16) & 0xff);
    r.w = (int)ov_expand8(w >> 24);
    return r;
}

// dist1 / L1 against dist2 / L2: the operands are below 2^24, so the products are two 24-bit multiplies each
__device__ __forceinline__ uint64_t ov_mul(unsigned a, unsigned b) { return (uint64_t)(a & 0xffffffu) * (uint64_t)(b & 0xffffffu); }

// Inside a chunk a candidate is two words: dist, and w = (kLMax - L) << 10 | lag inside the chunk -- at equal rates the
// smaller w has the larger L, then the smaller lag.  "none" is (kNoDist, L = 1).
constexpr unsigned kNoW = ((kLMax - 1) << 10) | 0x3ffu;
__device__ __forceinline__ bool ov_less(unsigned d1, unsigned w1, unsigned d2, unsigned w2)
{
    const uint64_t a = ov_mul(d1, kLMax - (w2 >> 10)), b = ov_mul(d2, kLMax - (w1 >> 10));
    return a < b || (a == b && w1 < w2);
}

// a workgroup's best so far over the chunks it has done (in rising order of lag), in one thread per query row
struct OvBest {
    unsigned dist = kNoDist, L = 1;
    int lag = 0;
    // a candidate of a later chunk: a larger lag, so it wins on a smaller rate or, at the same rate, a larger L
    __device__ void offer(unsigned d, unsigned l, int g)
    {
        const uint64_t a = ov_mul(d, L), b = ov_mul(dist, l);
        if (a < b || (a == b && l > L)) {
            dist = d;
            L = l;
            lag = g;
        }
    }
    __device__ void store(uint4 *e) const
    {
        if (dist != kNoDist) *e = make_uint4(dist, L, (unsigned)lag, 0u);
    }
};
} // namespace

struct OverlapArgs {
    const uint64_t *db;
    const int64_t *db_off;
    int n_clips;
    const uint64_t *q;    // the call's hashprints (xor/popcount kernel)
    const int64_t *q_off; // [n_q + 1] (device), this launch's first query at q_off[0]
    int n_q;
    const v4i *qa;        // expanded queries of this launch (expand_queries_kernel's image)
    int kt_pad;
    const int *gk;        // [g]: longest query of group g
    int min_overlap, splits;
    uint4 *tab;           // [n_q][n_clips][splits], every byte preset to 0xff
};

__global__ __launch_bounds__(kOvThreads, 4) void overlap_mfma_kernel(OverlapArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lane = lane & 31, h = lane >> 5;
    const int clip = blockIdx.x / a.splits, split = blockIdx.x - clip * a.splits, g = blockIdx.y;
    const int64_t r0 = a.db_off[clip];
    const int n = (int)(a.db_off[clip + 1] - r0);
    const int kt = a.gk[g], mo = a.min_overlap;
    if (n < mo || kt < mo) return; // no row of the group has a candidate in this clip
    const int d_lo = mo - kt, d_hi = n - mo;
    const int n_wg_chunks = (d_hi - d_lo) / kOvWgLags + 1;

    const int win = kOvWgLags + kt;                      // window slots (one spare)
    v4i *ldsB = reinterpret_cast<v4i *>(smem_raw);       // [2][win]: plane h = bits [32 h, 32 h + 32) of each hashprint
    v4i *ldsA = ldsB + 2 * win;                          // [2][kOvChunk][64]
    int *kq_s = reinterpret_cast<int *>(ldsA + 2 * kOvChunk * 64); // [32] lengths of the group's queries (0: no candidate)
    uint2 *red = reinterpret_cast<uint2 *>(ldsA);        // [8 waves][32 queries], over the A operand once the sums are done

    if (tid < 32) {
        const int qi = g * 32 + tid;
        int k = 0;
        if (qi < a.n_q) k = (int)(a.q_off[qi + 1] - a.q_off[qi]);
        kq_s[tid] = k >= mo ? k : 0;
    }
    const v4i *qa = a.qa + (int64_t)g * a.kt_pad * 64;
    const int n_chunks = (kt + kOvChunk - 1) / kOvChunk;
    const int one = 0x7f7f7f7f; // E8M0 scale 2^0
    const v4i *bp = ldsB + h * win + wave * kOvWaveLags + n_lane;
    OvBest best; // (threads below 32)

    for (int wc = split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kOvWgLags;
        __syncthreads(); // the chunk before this one has read its window and its candidates
        // clip positions d0 .. d0 + win - 1, expanded; fp4 zeros before the clip's start and past its end
        for (int i = tid; i < win; i += kOvThreads) {
            const int gi = d0 + i;
            v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
            if (gi >= 0 && gi < n) {
                const uint64_t w = a.db[r0 + gi];
                lo = ov_expand32((uint32_t)w);
                hi = ov_expand32((uint32_t)(w >> 32));
            }
            ldsB[i] = lo;
            ldsB[win + i] = hi;
        }
        v4i st0 = qa[tid], st1 = qa[tid + kOvThreads]; // 16 steps x 64 lanes = 1024 entries: two per thread
        ldsA[tid] = st0;
        ldsA[tid + kOvThreads] = st1;
        __syncthreads();

        f32x16 acc[kOvTiles];
#pragma unroll
        for (int t = 0; t < kOvTiles; ++t) acc[t] = f32x16{0};
        // a wave whose 128 lags all lie past n - min_overlap (the clip's last chunk) multiplies nothing: it only helps staging
        const bool live = d0 + wave * kOvWaveLags <= d_hi;
        for (int c = 0; c < n_chunks; ++c) {
            const bool more = c + 1 < n_chunks;
            if (more) { // next chunk of A into registers while this one multiplies
                st0 = qa[(c + 1) * (kOvChunk * 64) + tid];
                st1 = qa[(c + 1) * (kOvChunk * 64) + tid + kOvThreads];
            }
            const v4i *ap = ldsA + (c & 1) * (kOvChunk * 64) + lane;
            const int jn = min(kOvChunk, kt - c * kOvChunk);
            const v4i *bj = bp + c * kOvChunk;
            for (int j = 0; live && j < jn; ++j) {
                const v4i a4 = ap[j * 64];
                const v8i av = {a4.x, a4.y, a4.z, a4.w, 0, 0, 0, 0};
#pragma unroll
                for (int t = 0; t < kOvTiles; ++t) {
                    const v4i b4 = bj[j + 32 * t];
                    const v8i bv = {b4.x, b4.y, b4.z, b4.w, 0, 0, 0, 0};
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[t], 4, 4, 0, one, 0, one);
                }
            }
            if (more) {
                v4i *dst = ldsA + ((c + 1) & 1) * (kOvChunk * 64);
                dst[tid] = st0;
                dst[tid + kOvThreads] = st1;
            }
            __syncthreads();
        }

        // acc[t][reg]: query row m = (reg & 3) + 8 (reg >> 2) + 4 h, lag d0 + wave 128 + t 32 + n_lane
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int k = kq_s[m];
            unsigned bd = kNoDist, bw = kNoW;
#pragma unroll
            for (int t = 0; t < kOvTiles; ++t) {
                const int lo = wave * kOvWaveLags + t * 32 + n_lane;
                const int d = d0 + lo;
                const int L = min(k, n - d) + min(0, d); // L >= min_overlap: min_overlap - k <= d <= n - min_overlap
                const unsigned dist = (unsigned)((64 * L - (int)acc[t][reg]) >> 1);
                const unsigned w = ((kLMax - (unsigned)L) << 10) | (unsigned)lo;
                if (k > 0 && L >= mo && ov_less(dist, w, bd, bw)) {
                    bd = dist;
                    bw = w;
                }
            }
#pragma unroll
            for (int s = 16; s >= 1; s >>= 1) { // the best of the 32 lag columns of this half-wave
                const unsigned od = (unsigned)__shfl_xor((int)bd, s), ow = (unsigned)__shfl_xor((int)bw, s);
                if (ov_less(od, ow, bd, bw)) {
                    bd = od;
                    bw = ow;
                }
            }
            if (n_lane == 0) red[wave * 32 + m] = make_uint2(bd, bw);
        }
        __syncthreads();
        if (tid < 32) {
            uint2 b = red[tid];
            for (int w = 1; w < kOvThreads / 64; ++w) {
                const uint2 o = red[w * 32 + tid];
                if (ov_less(o.x, o.y, b.x, b.y)) b = o;
            }
            if (b.x != kNoDist) best.offer(b.x, kLMax - (b.y >> 10), d0 + (int)(b.y & 0x3ffu));
        }
    }
    if (tid < 32 && g * 32 + tid < a.n_q)
        best.store(a.tab + ((int64_t)(g * 32 + tid) * a.n_clips + clip) * a.splits + split);
}

// one workgroup per (query, clip, split): a thread takes four lags of a chunk and walks their overlaps
__global__ __launch_bounds__(256) void overlap_popc_kernel(OverlapArgs a)
{
    __shared__ uint2 red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int clip = blockIdx.x / a.splits, split = blockIdx.x - clip * a.splits, qi = blockIdx.y;
    const int64_t r0 = a.db_off[clip], q0 = a.q_off[qi];
    const int n = (int)(a.db_off[clip + 1] - r0), k = (int)(a.q_off[qi + 1] - q0), mo = a.min_overlap;
    if (n < mo || k < mo) return;
    const uint64_t *q = a.q + q0, *r = a.db + r0;
    const int d_lo = mo - k, d_hi = n - mo;
    const int n_wg_chunks = (d_hi - d_lo) / kOvWgLags + 1;
    OvBest best; // (thread 0)
    for (int wc = split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kOvWgLags;
        unsigned bd = kNoDist, bw = kNoW;
        for (int e = 0; e < kOvWgLags / 256; ++e) {
            const int lo = tid + 256 * e, d = d0 + lo;
            if (d > d_hi) break;
            const int j0 = max(0, -d), j1 = min(k, n - d); // d_lo <= d <= d_hi: j1 - j0 >= min_overlap
            unsigned dist = 0;
            for (int j = j0; j < j1; ++j) dist += (unsigned)__popcll(q[j] ^ r[d + j]);
            const unsigned w = ((kLMax - (unsigned)(j1 - j0)) << 10) | (unsigned)lo;
            if (ov_less(dist, w, bd, bw)) {
                bd = dist;
                bw = w;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned od = (unsigned)__shfl_xor((int)bd, s), ow = (unsigned)__shfl_xor((int)bw, s);
            if (ov_less(od, ow, bd, bw)) {
                bd = od;
                bw = ow;
            }
        }
        __syncthreads(); // (the chunk before has been read)
        if (lane == 0) red[wave] = make_uint2(bd, bw);
        __syncthreads();
        if (tid == 0) {
            uint2 b = red[0];
            for (int w = 1; w < 4; ++w)
                if (ov_less(red[w].x, red[w].y, b.x, b.y)) b = red[w];
            if (b.x != kNoDist) best.offer(b.x, kLMax - (b.y >> 10), d0 + (int)(b.y & 0x3ffu));
        }
    }
    if (tid == 0) best.store(a.tab + ((int64_t)qi * a.n_clips + clip) * a.splits + split);
}

namespace {
struct OverlapHitDev {
    uint32_t dist, clip;
    int32_t lag;
    uint32_t overlap;
};

// clips of one query: dist / L, then larger L, then the smaller clip id.  "none" is (kNoDist, 1, 0x7fffffff).
struct OvPick {
    unsigned dist, L, clip;
};
__device__ __forceinline__ bool ov_pick_less(const OvPick &x, const OvPick &y)
{
    const uint64_t a = ov_mul(x.dist, y.L), b = ov_mul(y.dist, x.L);
    return a < b || (a == b && (x.L > y.L || (x.L == y.L && x.clip < y.clip)));
}
} // namespace

// one workgroup per query: the splits of every clip folded into the clip's first entry, then k rounds of "the smallest
// clip above the one before"
__global__ __launch_bounds__(256) void overlap_select_kernel(uint4 *__restrict__ tab, int n_clips, int splits,
                                                             const int32_t *__restrict__ exclude, int k, uint32_t clip_base,
                                                             OverlapHitDev *__restrict__ out)
{
    __shared__ OvPick red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qi = blockIdx.x;
    uint4 *row = tab + (int64_t)qi * n_clips * splits;
    const int ex = exclude ? exclude[qi] : -1;
    if (splits > 1) {
        for (int c = tid; c < n_clips; c += 256) {
            uint4 b = row[(int64_t)c * splits];
            for (int s = 1; s < splits; ++s) {
                const uint4 e = row[(int64_t)c * splits + s];
                if (e.x == 0xffffffffu) continue;
                const uint64_t x = ov_mul(e.x, b.y), y = ov_mul(b.x, e.y);
                if (b.x == 0xffffffffu || x < y || (x == y && (e.y > b.y || (e.y == b.y && (int)e.z < (int)b.z)))) b = e;
            }
            row[(int64_t)c * splits] = b;
        }
        __syncthreads();
    }
    const OvPick none = {kNoDist, 1u, 0x7fffffffu};
    OvPick prev = none;
    for (int r = 0; r < k; ++r) {
        OvPick mine = none;
        if (r == 0 || prev.dist != kNoDist) {
            for (int c = tid; c < n_clips; c += 256) {
                const uint4 e = row[(int64_t)c * splits];
                if (e.x == 0xffffffffu || c == ex) continue;
                const OvPick p = {e.x, e.y, (unsigned)c};
                if ((r == 0 || ov_pick_less(prev, p)) && ov_pick_less(p, mine)) mine = p;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const OvPick o = {(unsigned)__shfl_xor((int)mine.dist, s), (unsigned)__shfl_xor((int)mine.L, s),
                              (unsigned)__shfl_xor((int)mine.clip, s)};
            if (ov_pick_less(o, mine)) mine = o;
        }
        __syncthreads(); // (the round before has been read)
        if (lane == 0) red[wave] = mine;
        __syncthreads();
        OvPick sel = red[0];
        for (int w = 1; w < 4; ++w)
            if (ov_pick_less(red[w], sel)) sel = red[w];
        if (tid == 0) {
            OverlapHitDev hit = {0xffffffffu, 0xffffffffu, 0, 0u};
            if (sel.dist != kNoDist) hit = {sel.dist, clip_base + sel.clip, (int32_t)row[(int64_t)sel.clip * splits].z, sel.L};
            out[(int64_t)qi * k + r] = hit;
        }
        prev = sel;
    }
}

void launch_overlap_mfma(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const int64_t *d_q_off, int n_q, const void *d_qa,
                         int kt_pad, const int *d_gk, int k_max, int min_overlap, int splits, void *d_tab, hipStream_t s)
{
    static PerDeviceOnce attr_set;
    if (attr_set.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(overlap_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        attr_set.mark();
    }
    OverlapArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.q_off = d_q_off;
    a.n_q = n_q;
    a.qa = reinterpret_cast<const v4i *>(d_qa);
    a.kt_pad = kt_pad;
    a.gk = d_gk;
    a.min_overlap = min_overlap;
    a.splits = splits;
    a.tab = reinterpret_cast<uint4 *>(d_tab);
    // (the candidates lie over the A operand: hamming_mfma_lds_bytes covers this kernel too)
    const dim3 grid((unsigned)n_clips * (unsigned)splits, (unsigned)((n_q + 31) / 32));
    hipLaunchKernelGGL(overlap_mfma_kernel, grid, dim3(kOvThreads), hamming_mfma_lds_bytes(k_max), s, a);
}

void launch_overlap_popc(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const uint64_t *d_q, const int64_t *d_q_off, int n_q,
                         int min_overlap, int splits, void *d_tab, hipStream_t s)
{
    OverlapArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.q = d_q;
    a.q_off = d_q_off;
    a.n_q = n_q;
    a.min_overlap = min_overlap;
    a.splits = splits;
    a.tab = reinterpret_cast<uint4 *>(d_tab);
    const dim3 grid((unsigned)n_clips * (unsigned)splits, (unsigned)n_q);
    hipLaunchKernelGGL(overlap_popc_kernel, grid, dim3(256), 0, s, a);
}

void launch_overlap_select(void *d_tab, int n_q, int n_clips, int splits, const int32_t *d_exclude, int k, uint32_t clip_base, void *d_out,
                           hipStream_t s)
{
    hipLaunchKernelGGL(overlap_select_kernel, dim3(n_q), dim3(256), 0, s, reinterpret_cast<uint4 *>(d_tab), n_clips, splits, d_exclude, k,
                       clip_base, reinterpret_cast<OverlapHitDev *>(d_out));
}

} // namespace hpfw
