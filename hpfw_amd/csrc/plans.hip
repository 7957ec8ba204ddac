// plans.hip -- the per-length tables (plan.h's host half, generated or uploaded to the device) and their cache, the
// handle's pool of device memory, and the workspaces that may take memory back from that pool.
#include "handle.h"

// HPFW_PLAN_TIMING=1: where the first use of a clip length spends the host's time (printed when the handle goes)
struct PlanTiming {
    double host_wait = 0, host_build = 0, upload = 0, device_tables = 0, alloc = 0, evict = 0, total = 0;
    long plans = 0, copies = 0;
    size_t copied = 0;
};

namespace {
thread_local size_t g_uploaded = 0; // bytes uploaded by upload() since get_plan last reset it

hpfw::RadixList to_radix(const std::vector<int> &r)
{
    hpfw::RadixList rl;
    std::memset(&rl, 0, sizeof(rl));
    rl.n = (int)r.size();
    for (size_t i = 0; i < r.size(); ++i) rl.r[i] = r[i];
    return rl;
}

DevBuf pool_take(hpfw_gpu *h, size_t bytes);
void pool_give(hpfw_gpu *h, DevBuf b);
void pool_release(hpfw_gpu *h);

constexpr size_t kPlanChunk = (size_t)4 << 20;

thread_local PlanTiming *g_plan_timing = nullptr;
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct PlanTimer {
    double *acc, t0;
    explicit PlanTimer(double PlanTiming::*m) : acc(g_plan_timing ? &(g_plan_timing->*m) : nullptr), t0(acc ? now_s() : 0.0) {}
    ~PlanTimer()
    {
        if (acc) *acc += now_s() - t0;
    }
};
hipError_t plan_h2d(hpfw_gpu *h, void *dst, const void *src, size_t bytes); // (below: needs the handle)

int plan_flush(DevPlan *dp)
{
    size_t i = 0;
    while (i < dp->staged.size()) {
        size_t off = dp->staged[i].first, end = off + dp->staged[i].second;
        // (a run = tables in adjacent 256-byte slots; a table the device fills itself, in between, ends the run)
        for (++i; i < dp->staged.size() && dp->staged[i].first == (end + 255) / 256 * 256; ++i) end = dp->staged[i].first + dp->staged[i].second;
        HIP_TRY(plan_h2d(dp->owner, dp->chunk_base + off, dp->stage.data() + off, end - off));
    }
    dp->staged.clear();
    return 0;
}

int plan_alloc(DevPlan *dp, size_t bytes, void **out)
{
    PlanTimer t(&PlanTiming::alloc);
    bytes = (bytes + 255) / 256 * 256;
    if (bytes >= kPlanChunk / 4) { // a block of its own, in 64 KB steps (equal sizes recur: lengths near each other share n1 and n2)
        DevBuf b = pool_take(dp->owner, (bytes + 65535) / 65536 * 65536);
        if (!b) return fail(HPFW_E_HIP, "out of device memory for the tables of a clip length");
        *out = b.get();
        dp->blocks.push_back(std::move(b));
        return 0;
    }
    if (dp->left < bytes) {
        int rc = plan_flush(dp);
        if (rc) return rc;
        DevBuf b = pool_take(dp->owner, kPlanChunk);
        if (!b) return fail(HPFW_E_HIP, "out of device memory for the tables of a clip length");
        dp->cur = dp->chunk_base = b.as<char>();
        dp->blocks.push_back(std::move(b));
        dp->left = kPlanChunk;
        dp->stage.resize(kPlanChunk);
    }
    *out = dp->cur;
    dp->cur += bytes;
    dp->left -= bytes;
    return 0;
}

template <class T>
int upload(const std::vector<T> &v, const T **out, DevPlan *dp)
{
    g_uploaded += v.size() * sizeof(T);
    if (v.empty()) {
        *out = nullptr;
        return 0;
    }
    void *d = nullptr;
    const size_t bytes = v.size() * sizeof(T);
    int rc = plan_alloc(dp, bytes, &d);
    if (rc) return rc;
    const bool in_chunk = dp->chunk_base && static_cast<char *>(d) >= dp->chunk_base && static_cast<char *>(d) < dp->chunk_base + kPlanChunk &&
                          bytes < kPlanChunk / 4;
    if (in_chunk) {
        const size_t off = (size_t)(static_cast<char *>(d) - dp->chunk_base);
        std::memcpy(dp->stage.data() + off, v.data(), bytes);
        dp->staged.emplace_back(off, bytes);
    } else {
        HIP_TRY(plan_h2d(dp->owner, d, v.data(), bytes));
    }
    *out = reinterpret_cast<const T *>(d);
    return 0;
}

constexpr size_t kPinRing = (size_t)48 << 20;

hipError_t plan_h2d(hpfw_gpu *h, void *dst, const void *src, size_t bytes)
{
    PlanTimer t(&PlanTiming::upload);
    if (g_plan_timing) {
        ++g_plan_timing->copies;
        g_plan_timing->copied += bytes;
    }
    if (!h->cache.pin_ring && h->cache.pin_ring.alloc(kPinRing) != hipSuccess) (void)hipGetLastError();
    const hipStream_t ps = h->cache.plan_stream.get();
    if (!h->cache.pin_ring || bytes > h->cache.pin_ring.capacity() / 2) { // (a table beyond the ring: the runtime stages it; rare -- clips of many minutes)
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ps);
        return e != hipSuccess ? e : hipStreamSynchronize(ps);
    }
    if (h->cache.pin_off + bytes > h->cache.pin_ring.capacity()) { // wrap: what was copied out of the ring before has to be gone
        hipError_t e = hipStreamSynchronize(ps);
        if (e != hipSuccess) return e;
        h->cache.pin_off = 0;
    }
    char *slot = h->cache.pin_ring.as<char>() + h->cache.pin_off;
    std::memcpy(slot, src, bytes);
    hipError_t e = hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, ps);
    h->cache.pin_off += (bytes + 255) / 256 * 256;
    return e;
}

// The pool: blocks of evicted plans and the temporaries of table generation, kept (up to 4 GiB, on top of the plan cache's
// HPFW_PLAN_CACHE_GB) so that a corpus of distinct lengths does not pay a hipMalloc / hipFree -- a device-wide
// synchronisation -- per file.  A request takes the smallest block that holds it with at most a quarter to spare (block
// sizes of distinct lengths rarely recur exactly); whoever fails to allocate -- the pool itself, the workspaces -- gives the
// whole pool back first.
void pool_release(hpfw_gpu *h)
{
    h->cache.dev_pool.clear();
    h->cache.dev_pool_bytes = 0;
}

// a block of at least `bytes` (its capacity() is its real size), empty when there is no device memory for it
DevBuf pool_take(hpfw_gpu *h, size_t bytes)
{
    auto it = h->cache.dev_pool.lower_bound(bytes);
    if (it != h->cache.dev_pool.end() && it->first <= bytes + bytes / 4) {
        DevBuf b = std::move(it->second);
        h->cache.dev_pool_bytes -= it->first;
        h->cache.dev_pool.erase(it);
        return b;
    }
    DevBuf b;
    if (b.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        pool_release(h);
        (void)b.alloc(bytes);
    }
    return b;
}

// (a block beyond the pool's bound is freed here)
void pool_give(hpfw_gpu *h, DevBuf b)
{
    const size_t bytes = b.capacity();
    if (h && h->cache.dev_pool_bytes + bytes <= ((size_t)4 << 30)) {
        h->cache.dev_pool.emplace(bytes, std::move(b));
        h->cache.dev_pool_bytes += bytes;
    }
}
} // namespace

// a workspace of at least `need` bytes (its contents are not kept when it grows)
int ensure(DevBuf &b, size_t need, hpfw_gpu *pool_owner)
{
    if (b.capacity() >= need) return 0;
    hipError_t e = b.alloc(need);
    if (e != hipSuccess && pool_owner) { // the handle's pool of table blocks may be holding what is missing
        (void)hipGetLastError();
        pool_release(pool_owner);
        e = b.alloc(need);
    }
    if (e != hipSuccess) return fail(HPFW_E_HIP, std::string("device memory for a workspace: ") + hipGetErrorString(e));
    return 0;
}

DevPlan::~DevPlan()
{
    for (DevBuf &b : blocks) pool_give(owner, std::move(b));
}

int get_plan(hpfw_gpu *h, int64_t n, DevPlan **out)
{
    auto it = h->cache.plans.find(n);
    if (it != h->cache.plans.end()) {
        it->second->last_use = ++h->cache.plan_clock;
        *out = it->second.get();
        return 0;
    }
    g_uploaded = 0;
    g_plan_timing = h->cache.plan_timing.get();
    PlanTimer whole(&PlanTiming::total);
    if (g_plan_timing) ++g_plan_timing->plans;
    auto dp = std::make_unique<DevPlan>();
    dp->owner = h;
    std::string why;
    bool have_host = false;
    {
        PlanTimer t(&PlanTiming::host_wait);
        // the host half may have been prepared (or be in preparation) by a reader thread: take it, or wait for it
        std::unique_lock<std::mutex> lock(h->cache.host_mtx);
        auto ready = h->cache.host_ready.find(n);
        if (ready != h->cache.host_ready.end()) {
            h->cache.host_cv.wait(lock, [&] { return h->cache.host_ready.find(n)->second != nullptr; });
            ready = h->cache.host_ready.find(n);
            have_host = ready->second->n == n;     // (a failed preparation leaves an empty plan: rebuilt below for its message)
            if (have_host) dp->hp = std::move(*ready->second);
            h->cache.host_ready.erase(ready);
        }
        h->cache.host_seen.insert(n);
    }
    // HPFW_FORCE_BLUESTEIN=1 (tests): the chirp-z forward transform for 7-smooth lengths too
    if (!have_host) {
        PlanTimer t(&PlanTiming::host_build);
        if (!hpfw::build_plan(n, dp->hp, why, false, std::getenv("HPFW_FORCE_BLUESTEIN") != nullptr, h->conventions, false))
            return fail(HPFW_E_UNSUPPORTED, "clip length " + std::to_string(n) + ": " + why);
    }
    const hpfw::HostPlan &p = dp->hp;
    using hpfw::cf;
    int rc;
    static_assert(sizeof(hpfw::HostCf) == sizeof(cf), "complex layout");
    hpfw::RowsArgs &ra = dp->rows;
    std::memset(&ra, 0, sizeof(ra));
    ra.n1 = p.n1;
    ra.n2 = p.n2;
    ra.h = p.h;
    ra.hpad = (p.h + 31) / 32 * 32;
    ra.pair_stride = 1;
    ra.groups.n = (int)p.groups.size();
    for (size_t g = 0; g < p.groups.size(); ++g) {
        ra.groups.r1[g] = p.groups[g].first;
        ra.groups.r2[g] = p.groups[g].second;
        ra.groups.tw_off[g] = p.rows_gtw_off[g];
    }
    if ((rc = upload(p.rows_gtw, reinterpret_cast<const hpfw::HostCf **>(&ra.gtw), dp.get()))) return rc;
    if ((rc = upload(p.pos_n2, &ra.pos_n2, dp.get()))) return rc;
    if ((rc = upload(p.kb_last, &ra.kb_last, dp.get()))) return rc;
    if (hpfw::fwd_rows_lds_bytes(ra) > 160 * 1024) return fail(HPFW_E_UNSUPPORTED, "n2 exceeds the LDS");
    hpfw::BzArgs &bz = dp->bz;
    std::memset(&bz, 0, sizeof(bz));
    if (p.bluestein) {
        PlanTimer t_dev(&PlanTiming::device_tables);
        bz.n1 = p.n1;
        bz.n2 = p.n2;
        bz.n2pad = (p.n2 + 31) / 32 * 32;
        bz.kmin = p.kmin;
        bz.kmax = p.kmax;
        {
            const hpfw::BzShape s = hpfw::bz_shape(p.n1, p.n2, p.kmin, p.kmax); // (plan.h)
            bz.a = s.a;
            bz.n_tiles1 = s.n_tiles1;
            bz.k1lo = s.k1lo;
            bz.k1n = s.k1n;
            bz.nt2 = s.nt2;
            bz.n_tiles2 = s.n_tiles2;
        }
        // coefficient images of the column transforms (the first one's two stages; the second one's rows that hold
        // consumed bins), packed on the device
        // temporaries of this block (T_n1, the generation scratch) come from the handle's pool and go back to it: hipFree
        // waits for every stream of the device, which would stop a caller that extracts on a stream of its own from
        // preparing the next length while the previous file's kernels run
        const cf *d_tw_n1 = nullptr;
        struct PoolTmp {
            hpfw_gpu *h;
            std::vector<DevBuf> v;
            ~PoolTmp() { for (DevBuf &b : v) pool_give(h, std::move(b)); }
            void *take(size_t bytes)
            {
                DevBuf b = pool_take(h, (bytes + 65535) / 65536 * 65536);
                if (!b) return nullptr;
                v.push_back(std::move(b));
                return v.back().get();
            }
        } tmp{h, {}};
        {
            void *d = tmp.take(p.tw_n1.size() * sizeof(cf));
            if (!d) return fail(HPFW_E_HIP, "out of device memory for the tables of a clip length");
            HIP_TRY(plan_h2d(h, d, p.tw_n1.data(), p.tw_n1.size() * sizeof(cf)));
            d_tw_n1 = static_cast<const cf *>(d);
        }
        {
            const size_t bytes[3] = {(size_t)bz.a * bz.n_tiles1 * 64 * sizeof(float), (size_t)bz.a * 16 * 64 * sizeof(float),
                                     (size_t)p.n1 * bz.n_tiles2 * 64 * sizeof(float)};
            const float **slot[3] = {&bz.apack1, &bz.apack3, &bz.apack2};
            for (int i = 0; i < 3; ++i) {
                void *d = nullptr;
                if ((rc = plan_alloc(dp.get(), bytes[i], &d))) return rc;
                g_uploaded += bytes[i];
                *slot[i] = static_cast<const float *>(d);
            }
            if ((rc = plan_flush(dp.get()))) return rc; // the row transform's tables are used by the kernels below
            hpfw::launch_bz_pack_stages(bz, d_tw_n1, const_cast<float *>(bz.apack1), const_cast<float *>(bz.apack3), h->cache.plan_stream.get());
            hpfw::launch_bz_pack_coefficients(p.n1, bz.k1lo, bz.k1n, d_tw_n1, bz.n_tiles2, const_cast<float *>(bz.apack2), h->cache.plan_stream.get());
        }
        // chirp, T_L, w[k] / L and Bhat are generated on the device (k_bluestein.hip): a corpus of
        // real recordings brings a new length with every file
        const size_t big_l = (size_t)p.n1 * p.n2, plane = hpfw::bz_plane_bytes(bz, 1);
        {
            const size_t bytes[4] = {big_l * sizeof(cf), big_l * sizeof(cf), big_l * sizeof(cf), (size_t)(p.kmax - p.kmin) * sizeof(cf)};
            const void **slot[4] = {reinterpret_cast<const void **>(&bz.wp), reinterpret_cast<const void **>(&bz.tl),
                                    reinterpret_cast<const void **>(&bz.bhat), reinterpret_cast<const void **>(&bz.wk)};
            for (int i = 0; i < 4; ++i) {
                void *d = nullptr;
                if ((rc = plan_alloc(dp.get(), bytes[i], &d))) return rc;
                g_uploaded += bytes[i];
                *slot[i] = d;
            }
        }
        void *scratch = tmp.take(big_l * 8 + plane); // back to the pool with T_n1 when this block ends, after the synchronisation below
        if (!scratch) return fail(HPFW_E_HIP, "out of device memory for the tables of a clip length");
        hpfw::launch_bz_make_tables(ra, bz, n, static_cast<float *>(scratch), static_cast<float *>(scratch) + 2 * big_l, h->cache.plan_stream.get());
        // (no host wait: the temporaries go back to the pool, whose next user is ordered after these kernels on the handle's
        // table stream like every table generation and upload; the stream that extracts waits for the event recorded below)
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess) return fail(HPFW_E_HIP, std::string("chirp-z tables: ") + hipGetErrorString(launched));
    }
    // S6 (7-smooth lengths): the column stage's twiddle digits, digit-offset correction and inter-stage twiddles
    hpfw::ColsQArgs &ca = dp->cols;
    std::memset(&ca, 0, sizeof(ca));
    dp->rows_out = hpfw::Rows2Out{p.n1, p.hq, p.q2lo, p.q2w, nullptr, nullptr, (p.n2 + 3) / 4, 5 /* kZBlock / 4 = 2^5 pieces */,
                                  (long long)2 * p.hq * hpfw::kZBlock, hpfw::kZBlock, hpfw::z_floats_per_clip(p.hq, p.n2)};
    static_assert(hpfw::kZBlock == 128, "Rows2Out::zshift4 above");
    // HPFW_PRUNE bit 0: the row stage leaves out the last group's outputs that neither consumed window reads, when those it needs
    // are among the first and last two of a block
    dp->rows_out.last_edges = (h->prune & 1u) && !p.bluestein && !p.groups.empty() &&
                              hpfw::rows_last_edges_ok(p.rows_last_mask, p.groups.back().first * p.groups.back().second);
    if (!p.bluestein) {
        ca.n1 = p.n1;
        ca.n2 = p.n2;
        ca.hq = p.hq;
        ca.mt = p.cols_mt;
        ca.ks = p.cols_ks;
        ca.zclip = hpfw::z_floats_per_clip(p.hq, p.n2);
        const int8_t *img = nullptr;
        if ((rc = upload(p.cols_image, &img, dp.get()))) return rc;
        ca.image = img;
        if (!p.cols2_image.empty()) {
            ca.mt2 = p.cols2_mt;
            ca.ks2 = p.cols2_ks;
            if ((rc = upload(p.cols2_image, &img, dp.get()))) return rc;
            ca.image2 = img;
        }
        if ((rc = upload(p.cols_corr, &ca.corr, dp.get()))) return rc;
        if ((rc = upload(p.ts_seed, reinterpret_cast<const hpfw::HostCf **>(&dp->rows_out.seed), dp.get()))) return rc;
        if ((rc = upload(p.ts_step, reinterpret_cast<const hpfw::HostCf **>(&dp->rows_out.step), dp.get()))) return rc;
    }
    hpfw::CqPlanDev &c = dp->cq;
    c.kmin = p.kmin;
    c.nk = p.kmax - p.kmin;
    c.c = p.c;
    if (p.bluestein) { // natural order from kmin on
        c.xn1 = 1;
        c.xw = 0;
        c.xq0 = p.kmin;
        c.xclip = c.nk;
        c.xmagic = 0;
    } else {           // x[k mod n1][k / n1 - q2lo], rows of q2w
        c.xn1 = p.n1;
        c.xw = p.q2w;
        c.xq0 = p.q2lo;
        c.xclip = (int64_t)p.n1 * p.q2w;
        c.xmagic = ((1ull << 40) + (unsigned long long)p.n1 - 1) / (unsigned long long)p.n1;
    }
    std::vector<int> start(p.start, p.start + 121), lg(p.lg, p.lg + 121);
    if ((rc = upload(start, &c.start, dp.get()))) return rc;
    if ((rc = upload(lg, &c.lg, dp.get()))) return rc;
    if ((rc = upload(p.g_off, &c.g_off, dp.get()))) return rc;
    // the window table itself is generated on the device, behind the uploads (below): S5, k_cq_tables.hip
    {
        void *d = nullptr;
        if ((rc = plan_alloc(dp.get(), (size_t)std::max<int64_t>(p.g_total, 1) * sizeof(cf), &d))) return rc;
        g_uploaded += (size_t)p.g_total * sizeof(cf);
        c.g = static_cast<const cf *>(d);
    }
    int g2_max_entries = 0;
    c.g2 = nullptr;
    c.g2_off = nullptr;
    c.q2a = c.nq2 = nullptr;
    c.nq2_magic = nullptr;
    c.rows_min = 4; // (measured on one box: 0..8 alike, 16 and above slower; element by element throughout +0.4 ms per 1000 clips)
    if (!p.bluestein) { // the windows once more, in the order the rows layout of the forward bins is read (kernels.h XsBandRows)
        std::vector<int> q2a(121), nq2(121);
        std::vector<unsigned> magic(121);
        std::vector<int64_t> g2_off(121);
        int64_t total = 0;
        for (int j = 0; j < 121; ++j) {
            q2a[j] = p.start[j] / p.n1;
            nq2[j] = (p.start[j] + p.lg[j] - 1) / p.n1 - q2a[j] + 1;
            magic[j] = nq2[j] >= 2 ? (unsigned)(((1ull << 32) + (unsigned)nq2[j] - 1) / (unsigned)nq2[j]) : 0u;
            g2_off[j] = total;
            total += (int64_t)p.n1 * nq2[j];
        }
        for (int j = 0; j < 121; ++j) g2_max_entries = std::max(g2_max_entries, p.n1 * nq2[j]);
        {
            void *d = nullptr;
            if ((rc = plan_alloc(dp.get(), (size_t)std::max<int64_t>(total, 1) * sizeof(cf), &d))) return rc;
            g_uploaded += (size_t)total * sizeof(cf);
            c.g2 = static_cast<const cf *>(d);
        }
        if ((rc = upload(g2_off, &c.g2_off, dp.get()))) return rc;
        if ((rc = upload(q2a, &c.q2a, dp.get()))) return rc;
        if ((rc = upload(nq2, &c.nq2, dp.get()))) return rc;
        if ((rc = upload(magic, &c.nq2_magic, dp.get()))) return rc;
    }
    for (const hpfw::BluesteinClass &bc : p.classes) {
        hpfw::CqClassDev cd;
        cd.p = bc.p;
        cd.n_bands = (int)bc.bands.size();
        cd.radix = to_radix(bc.radix);
        if ((rc = upload(bc.tw, reinterpret_cast<const hpfw::HostCf **>(&cd.tw), dp.get()))) return rc;
        if ((rc = upload(bc.gtw, reinterpret_cast<const hpfw::HostCf **>(&cd.gtw.tab), dp.get()))) return rc;
        for (int g = 0; g < 4; ++g) cd.gtw.off[g] = bc.goff[g];
        cd.gtw.mid_off = bc.mid_off;
        if ((rc = upload(bc.vrev, reinterpret_cast<const hpfw::HostCf **>(&cd.vrev), dp.get()))) return rc;
        if ((rc = upload(bc.bands, &cd.band, dp.get()))) return rc;
        cd.len0 = bc.len0;
        cd.outer = bc.outer;
        dp->cls.push_back(cd);
    }
    if ((size_t)p.n2 * sizeof(cf) > 150 * 1024) return fail(HPFW_E_UNSUPPORTED, "n2 exceeds the LDS");
    // the tables live on the device now: drop the host copies (only the sizes are read from here on)
    {
        hpfw::HostPlan &hp = dp->hp;
        std::vector<hpfw::HostCf>().swap(hp.rows_gtw);
        std::vector<hpfw::HostCf>().swap(hp.tw_n2);
        std::vector<hpfw::HostCf>().swap(hp.tw_n1);
        std::vector<hpfw::HostCf>().swap(hp.ts_seed);
        std::vector<int8_t>().swap(hp.cols_image);
        std::vector<int8_t>().swap(hp.cols2_image);
        std::vector<hpfw::HostCf>().swap(hp.g);
        for (hpfw::BluesteinClass &bc : hp.classes) {
            std::vector<hpfw::HostCf>().swap(bc.tw);
            std::vector<hpfw::HostCf>().swap(bc.gtw);
            std::vector<hpfw::HostCf>().swap(bc.vrev);
        }
    }
    dp->bytes = g_uploaded;
    dp->last_use = ++h->cache.plan_clock;
    // a corpus of files of many different lengths would otherwise keep one set of tables per length
    // (14 MB for 30 s clips, growing with the length): bound the cache (HPFW_PLAN_CACHE_GB, default 16) by
    // evicting the least recently used plans; work already queued may still read their tables, hence the sync
    size_t budget = (size_t)16 << 30;
    if (const char *e = std::getenv("HPFW_PLAN_CACHE_GB")) budget = (size_t)(std::max(0.0, std::atof(e)) * 1073741824.0);
    if (h->cache.plan_bytes + dp->bytes > budget && !h->cache.plans.empty()) {
        PlanTimer t(&PlanTiming::evict);
        // Plans known to be idle go one at a time, as many as the new one needs: their blocks pass through the pool to the
        // next length's tables (sizes of neighbouring lengths recur), no hipMalloc, no hipFree.  A plan that queued work may
        // still read costs a device-wide wait first: then room for a quarter of the budget is made at once, so that a corpus
        // of distinct lengths larger than the cache does not pay that wait with every file.
        size_t goal = budget;
        while (h->cache.plan_bytes + dp->bytes > goal && !h->cache.plans.empty()) {
            auto lru = h->cache.plans.begin();
            for (auto q = h->cache.plans.begin(); q != h->cache.plans.end(); ++q)
                if (q->second->last_use < lru->second->last_use) lru = q;
            if (lru->second->last_use > h->cache.idle_clock) {
                HIP_TRY(hipDeviceSynchronize());
                h->cache.idle_clock = h->cache.plan_clock;
                goal = budget - budget / 4;
            }
            h->cache.plan_bytes -= lru->second->bytes;
            {
                // an evicted length may be prepared ahead again by the reader threads the next time a file brings it
                std::scoped_lock lock(h->cache.host_mtx);
                h->cache.host_seen.erase(lru->first);
            }
            h->cache.plans.erase(lru);
        }
    }
    if ((rc = plan_flush(dp.get()))) return rc;
    std::vector<char>().swap(dp->stage);
    // the constant-Q windows, generated behind the uploads of the band tables they read (S5, k_cq_tables.hip)
    {
        PlanTimer t(&PlanTiming::device_tables);
        hpfw::CqWindowBands wb;
        int lg_max = 0;
        for (int j = 0; j < 121; ++j) {
            wb.scale[j] = hpfw::cq_window_scale(h->conventions, p.big_m, p.psize[j]);
            wb.hann_den[j] = (int)hpfw::cq_hann_den(h->conventions, p.lg[j]);
            lg_max = std::max(lg_max, p.lg[j]);
        }
        hpfw::launch_cq_windows(c, wb, p.big_m, lg_max, const_cast<cf *>(c.g), h->cache.plan_stream.get());
        if (c.g2) hpfw::launch_cq_windows_rows(c, p.n1, g2_max_entries, const_cast<cf *>(c.g2), h->cache.plan_stream.get());
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess) return fail(HPFW_E_HIP, std::string("constant-Q window tables: ") + hipGetErrorString(launched));
    }
    // every table of the length is on its way on the table stream: whoever uses them first waits for this (ordered_call)
    HIP_TRY(hipEventRecord(h->cache.plan_ev.get(), h->cache.plan_stream.get()));
    h->cache.plan_ev_pending = true;
    h->cache.plan_bytes += dp->bytes;
    *out = dp.get();
    h->cache.plans[n] = std::move(dp);
    return 0;
}

hipError_t init_plans(hpfw_gpu *h)
{
    if (std::getenv("HPFW_PLAN_TIMING")) h->cache.plan_timing = std::make_unique<PlanTiming>();
    const hipError_t e = h->cache.plan_ev.create();
    return e != hipSuccess ? e : h->cache.plan_stream.create();
}

void clear_plans(hpfw_gpu *h)
{
    h->cache.plans.clear();
    h->cache.plan_bytes = 0;
    std::unique_lock<std::mutex> lock(h->cache.host_mtx);
    h->cache.host_cv.wait(lock, [&] { // (preparations in flight finish first: their threads write into the map)
        for (auto &kv : h->cache.host_ready)
            if (!kv.second) return false;
        return true;
    });
    h->cache.host_ready.clear();
    h->cache.host_seen.clear();
}

hpfw_gpu::PlanCache::PlanCache() = default;
hpfw_gpu::PlanCache::~PlanCache()
{
    if (!plan_timing || !plan_timing->plans) return;
    const PlanTiming &t = *plan_timing;
    std::fprintf(stderr, "hpfw plan timing: %ld lengths, %.1f ms in get_plan = %.3f ms each: wait for the host half %.3f, host build %.3f, "
                         "uploads %.3f (%ld copies, %.2f MB per length), device tables (incl. their uploads) %.3f, device memory %.3f, "
                         "evictions %.3f\n",
                 t.plans, t.total * 1e3, t.total * 1e3 / t.plans, t.host_wait * 1e3 / t.plans, t.host_build * 1e3 / t.plans,
                 t.upload * 1e3 / t.plans, t.copies, t.copied / 1e6 / t.plans, t.device_tables * 1e3 / t.plans, t.alloc * 1e3 / t.plans,
                 t.evict * 1e3 / t.plans);
}

extern "C" {

// (legacy.cpp, after it has waited for the stream that carried everything it queued on the handle)
void hpfw_internal_note_idle(hpfw_gpu *h)
{
    if (h) h->cache.idle_clock = h->cache.plan_clock;
}

int hpfw_gpu_geometry(hpfw_gpu *h, int64_t n_samples, hpfw_geometry *out)
{
    if (!h || !out) return fail(HPFW_E_INVALID, "null argument");
    // The sizes alone: from the cached plan or from the host half a reader thread prepared, else by the geometry part of
    // the plan (microseconds).  No device table is built for the question -- a caller that asks for the geometry of every
    // file of a window before extracting the first would otherwise build all their tables with the GPU idle.
    auto fill = [&](const hpfw::HostPlan &p) { *out = {p.n, p.n1, p.n2, p.kmin, p.kmax, p.m, p.c, p.n_frames, p.n_hp}; };
    auto it = h->cache.plans.find(n_samples);
    if (it != h->cache.plans.end()) {
        fill(it->second->hp);
        return 0;
    }
    {
        std::scoped_lock lock(h->cache.host_mtx);
        auto ready = h->cache.host_ready.find(n_samples);
        if (ready != h->cache.host_ready.end() && ready->second && ready->second->n == n_samples) {
            fill(*ready->second);
            return 0;
        }
    }
    hpfw::HostPlan hp;
    std::string why;
    if (!hpfw::build_plan(n_samples, hp, why, true, std::getenv("HPFW_FORCE_BLUESTEIN") != nullptr, h->conventions))
        return fail(HPFW_E_UNSUPPORTED, "clip length " + std::to_string(n_samples) + ": " + why);
    // what get_plan would refuse later is refused here (callers size their buffers from this answer)
    if ((size_t)hp.n2 * sizeof(hpfw::cf) > 150 * 1024)
        return fail(HPFW_E_UNSUPPORTED, "clip length " + std::to_string(n_samples) + ": n2 exceeds the LDS");
    fill(hp);
    return 0;
}

// Host half of the tables of a clip length, built on the CALLING thread and kept for the next entry point that meets
// the length (which then only generates / uploads the device tables).  Thread-safe against every other call on the
// handle: the collectors' reader threads call it for each file they have decoded.
int hpfw_gpu_prepare_length(hpfw_gpu *h, int64_t n_samples)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    {
        std::scoped_lock lock(h->cache.host_mtx);
        if (!h->cache.host_seen.insert(n_samples).second) return 0; // known already
        h->cache.host_ready[n_samples] = nullptr;                   // in preparation
    }
    auto hp = std::make_unique<hpfw::HostPlan>();
    std::string why;
    bool ok;
    {
        hpfw::PlanSerial serial;
        ok = hpfw::build_plan(n_samples, *hp, why, false, std::getenv("HPFW_FORCE_BLUESTEIN") != nullptr, h->conventions, false);
    }
    if (!ok) *hp = hpfw::HostPlan(); // n = 0: get_plan builds it again and reports why
    {
        std::scoped_lock lock(h->cache.host_mtx);
        h->cache.host_ready[n_samples] = std::move(hp);
        if (!ok) h->cache.host_seen.erase(n_samples); // an unsupported length says so every time it is asked for
    }
    h->cache.host_cv.notify_all();
    return ok ? 0 : fail(HPFW_E_UNSUPPORTED, "clip length " + std::to_string(n_samples) + ": " + why);
}

// ---- diagnostic: the device-generated tables of the chirp-z forward transform ------------------
int hpfw_gpu_chirpz_table(hpfw_gpu *h, int64_t n_samples, int which, float *out, int64_t capacity, int64_t *count)
{
    if (!h || !count) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, n_samples, &dp);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->cache.plan_stream.get())); // the tables are generated on the handle's table stream
    if (which == 4) { // the constant-Q stage's windows (every length): bands concatenated
        *count = 2 * dp->hp.g_total;
        if (!out) return 0;
        if (capacity < *count) return fail(HPFW_E_INVALID, "table buffer too small");
        HIP_TRY(hipMemcpy(out, dp->cq.g, (size_t)*count * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    if (!dp->hp.bluestein) return fail(HPFW_E_INVALID, "clip length takes the mixed-radix transform: no chirp-z tables");
    const hpfw::BzArgs &bz = dp->bz;
    const void *tab[4] = {bz.wp, bz.tl, bz.bhat, bz.wk};
    if (which < 0 || which > 3) return fail(HPFW_E_INVALID, "table index out of range");
    *count = 2 * (which == 3 ? (int64_t)(bz.kmax - bz.kmin) : (int64_t)bz.n1 * bz.n2);
    if (!out) return 0;
    if (capacity < *count) return fail(HPFW_E_INVALID, "table buffer too small");
    if (which == 0) { // the chirp lies in two planes on the device
        std::vector<float> planar((size_t)*count);
        HIP_TRY(hipMemcpy(planar.data(), tab[0], planar.size() * sizeof(float), hipMemcpyDeviceToHost));
        const size_t big_l = planar.size() / 2;
        for (size_t j = 0; j < big_l; ++j) {
            out[2 * j] = planar[j];
            out[2 * j + 1] = planar[big_l + j];
        }
        return 0;
    }
    HIP_TRY(hipMemcpy(out, tab[which], (size_t)*count * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

} // extern "C"
