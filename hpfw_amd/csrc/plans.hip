// plans.hip -- the per-length tables (plan.h's host half, generated or uploaded to the device) and their cache, the
// handle's pool of device memory, and the workspaces that may take memory back from that pool.
#include "handle.h"
#include "plan_cache.h"

// HPFW_PLAN_TIMING=1: where the first use of a clip length spends the host's time (printed when the handle goes)
struct PlanTiming {
    double host_wait = 0, host_build = 0, upload = 0, device_tables = 0, alloc = 0, evict = 0, total = 0;
    long plans = 0, copies = 0;
    size_t copied = 0;
};

namespace {
using hpfw::cf;
static_assert(sizeof(hpfw::HostCf) == sizeof(cf), "complex layout");

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

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// adds its lifetime to one part of the handle's PlanTiming (nothing without HPFW_PLAN_TIMING)
struct PlanTimer {
    double *acc, t0;
    PlanTimer(hpfw_gpu *h, double PlanTiming::*m) : acc(h->cache.plan_timing ? &(h->cache.plan_timing.get()->*m) : nullptr), t0(acc ? now_s() : 0.0) {}
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
    PlanTimer t(dp->owner, &PlanTiming::alloc);
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
    dp->bytes += v.size() * sizeof(T);
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

// room for a table that the device generates, counted like an uploaded one (an empty table still gets a valid pointer)
template <class T>
int device_table(DevPlan *dp, size_t bytes, const T **out)
{
    void *d = nullptr;
    dp->bytes += bytes;
    const int rc = plan_alloc(dp, std::max<size_t>(bytes, 1), &d);
    *out = static_cast<const T *>(d);
    return rc;
}

constexpr size_t kPinRing = (size_t)48 << 20;

hipError_t plan_h2d(hpfw_gpu *h, void *dst, const void *src, size_t bytes)
{
    PlanTimer t(h, &PlanTiming::upload);
    if (PlanTiming *pt = h->cache.plan_timing.get()) {
        ++pt->copies;
        pt->copied += bytes;
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

// ---- the tables of a new clip length: get_plan's steps, in its order ------------------------------
namespace {
// HPFW_FORCE_BLUESTEIN=1 (tests): the chirp-z forward transform for 7-smooth lengths too.  Read whenever a plan is built.
bool force_bluestein() { return std::getenv("HPFW_FORCE_BLUESTEIN") != nullptr; }
// HPFW_PLAN_CACHE_GB (default 16): the bytes of tables the cache keeps.  Read whenever a plan is built.
size_t plan_cache_budget()
{
    const char *e = std::getenv("HPFW_PLAN_CACHE_GB");
    return e ? (size_t)(std::max(0.0, std::atof(e)) * 1073741824.0) : (size_t)16 << 30;
}
int unsupported(int64_t n, const std::string &why) { return fail(HPFW_E_UNSUPPORTED, "clip length " + std::to_string(n) + ": " + why); }
// the host plan of a clip length (geometry_only: its sizes alone, microseconds), or why the length is not supported
int host_plan(const hpfw_gpu *h, int64_t n, hpfw::HostPlan &hp, bool geometry_only)
{
    std::string why;
    return hpfw::build_plan(n, hp, why, geometry_only, force_bluestein(), h->conventions, false) ? 0 : unsupported(n, why);
}

// The host half may have been prepared (or be in preparation) by a reader thread: take it, or wait for it.  Registers the
// length as seen; false: there is no host half (a failed preparation leaves an empty plan: rebuilt for its message).
bool take_host_half(hpfw_gpu *h, DevPlan *dp, int64_t n)
{
    PlanTimer t(h, &PlanTiming::host_wait);
    bool have = false;
    std::unique_lock<std::mutex> lock(h->cache.host_mtx);
    auto ready = h->cache.host_ready.find(n);
    if (ready != h->cache.host_ready.end()) {
        h->cache.host_cv.wait(lock, [&] { return h->cache.host_ready.find(n)->second != nullptr; });
        ready = h->cache.host_ready.find(n);
        have = ready->second->n == n;
        if (have) dp->hp = std::move(*ready->second);
        h->cache.host_ready.erase(ready);
    }
    h->cache.host_seen.insert(n);
    return have;
}
// A get_plan that fails leaves the cache as it found it: the length is not seen any more, so hpfw_gpu_prepare_length builds
// (and an unsupported length says so) every time it is asked for.  The plan's blocks go back to the pool with the DevPlan.
struct SeenGuard {
    hpfw_gpu *h;
    int64_t n;
    bool dismissed = false;
    ~SeenGuard()
    {
        if (dismissed) return;
        std::scoped_lock lock(h->cache.host_mtx);
        h->cache.host_seen.erase(n);
    }
};

int build_host_half(hpfw_gpu *h, DevPlan *dp, int64_t n)
{
    PlanTimer t(h, &PlanTiming::host_build);
    return host_plan(h, n, dp->hp, false);
}

// the row transform's arguments, its tables not yet in place
hpfw::RowsArgs rows_args(const hpfw::HostPlan &p)
{
    hpfw::RowsArgs ra;
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
    return ra;
}

// what cannot run is refused before any device memory is taken: both bounds depend on the host plan alone
int refuse_unrunnable(hpfw_gpu *, DevPlan *dp)
{
    if (hpfw::fwd_rows_lds_bytes(rows_args(dp->hp)) > 160 * 1024 || !hpfw::row_fits_lds(dp->hp.n2))
        return fail(HPFW_E_UNSUPPORTED, "n2 exceeds the LDS");
    return 0;
}

int rows_tables(hpfw_gpu *, DevPlan *dp)
{
    const hpfw::HostPlan &p = dp->hp;
    hpfw::RowsArgs &ra = dp->rows;
    ra = rows_args(p);
    int rc;
    if ((rc = upload(p.rows_gtw, reinterpret_cast<const hpfw::HostCf **>(&ra.gtw), dp))) return rc;
    if ((rc = upload(p.pos_n2, &ra.pos_n2, dp))) return rc;
    return upload(p.kb_last, &ra.kb_last, dp);
}

// Temporaries of table generation (T_n1, the generation scratch) come from the handle's pool and go back to it: hipFree
// waits for every stream of the device, which would stop a caller that extracts on a stream of its own from preparing the
// next length while the previous file's kernels run.  (No host wait before they go back either: the pool's next user is
// ordered after the generating kernels on the handle's table stream like every table generation and upload; the stream that
// extracts waits for the event get_plan records.)
struct PoolTmp {
    hpfw_gpu *h;
    std::vector<DevBuf> v;
    ~PoolTmp() { for (DevBuf &b : v) pool_give(h, std::move(b)); }
    int take(size_t bytes, void **out)
    {
        DevBuf b = pool_take(h, (bytes + 65535) / 65536 * 65536);
        if (!b) return fail(HPFW_E_HIP, "out of device memory for the tables of a clip length");
        v.push_back(std::move(b));
        *out = v.back().get();
        return 0;
    }
};

// Clip lengths with a prime factor above 7: the coefficient images of the column transforms (the first one's two stages; the
// second one's rows that hold consumed bins) are packed on the device, and chirp, T_L, w[k] / L and Bhat are generated there
// (k_bluestein.hip): a corpus of real recordings brings a new length with every file.
int chirpz_tables(hpfw_gpu *h, DevPlan *dp)
{
    const hpfw::HostPlan &p = dp->hp;
    hpfw::BzArgs &bz = dp->bz;
    std::memset(&bz, 0, sizeof(bz));
    if (!p.bluestein) return 0;
    PlanTimer t(h, &PlanTiming::device_tables);
    const hipStream_t ps = h->cache.plan_stream.get();
    const hpfw::BzShape s = hpfw::bz_shape(p.n1, p.n2, p.kmin, p.kmax); // (plan.h)
    bz.n1 = p.n1;
    bz.n2 = p.n2;
    bz.n2pad = (p.n2 + 31) / 32 * 32;
    bz.kmin = p.kmin;
    bz.kmax = p.kmax;
    bz.a = s.a;
    bz.n_tiles1 = s.n_tiles1;
    bz.k1lo = s.k1lo;
    bz.k1n = s.k1n;
    bz.nt2 = s.nt2;
    bz.n_tiles2 = s.n_tiles2;
    int rc;
    PoolTmp tmp{h, {}};
    void *d_tw_n1 = nullptr, *scratch = nullptr;
    if ((rc = tmp.take(p.tw_n1.size() * sizeof(cf), &d_tw_n1))) return rc;
    HIP_TRY(plan_h2d(h, d_tw_n1, p.tw_n1.data(), p.tw_n1.size() * sizeof(cf)));
    if ((rc = device_table(dp, (size_t)bz.a * bz.n_tiles1 * 64 * sizeof(float), &bz.apack1))) return rc;
    if ((rc = device_table(dp, (size_t)bz.a * 16 * 64 * sizeof(float), &bz.apack3))) return rc;
    if ((rc = device_table(dp, (size_t)p.n1 * bz.n_tiles2 * 64 * sizeof(float), &bz.apack2))) return rc;
    if ((rc = plan_flush(dp))) return rc; // the row transform's tables are used by the kernels below
    hpfw::launch_bz_pack_stages(bz, static_cast<const cf *>(d_tw_n1), const_cast<float *>(bz.apack1), const_cast<float *>(bz.apack3), ps);
    hpfw::launch_bz_pack_coefficients(p.n1, bz.k1lo, bz.k1n, static_cast<const cf *>(d_tw_n1), bz.n_tiles2, const_cast<float *>(bz.apack2), ps);
    const size_t big_l = (size_t)p.n1 * p.n2;
    if ((rc = device_table(dp, big_l * sizeof(cf), &bz.wp))) return rc;
    if ((rc = device_table(dp, big_l * sizeof(cf), &bz.tl))) return rc;
    if ((rc = device_table(dp, big_l * sizeof(cf), &bz.bhat))) return rc;
    if ((rc = device_table(dp, (size_t)(p.kmax - p.kmin) * sizeof(cf), &bz.wk))) return rc;
    if ((rc = tmp.take(big_l * 8 + hpfw::bz_plane_bytes(bz, 1), &scratch))) return rc;
    hpfw::launch_bz_make_tables(dp->rows, bz, p.n, static_cast<float *>(scratch), static_cast<float *>(scratch) + 2 * big_l, ps);
    const hipError_t launched = hipGetLastError();
    return launched == hipSuccess ? 0 : fail(HPFW_E_HIP, std::string("chirp-z tables: ") + hipGetErrorString(launched));
}

// S6 (7-smooth lengths): the column stage's twiddle digits, digit-offset correction and inter-stage twiddles
int cols_tables(hpfw_gpu *h, DevPlan *dp)
{
    const hpfw::HostPlan &p = dp->hp;
    hpfw::ColsQArgs &ca = dp->cols;
    std::memset(&ca, 0, sizeof(ca));
    dp->rows_out = hpfw::Rows2Out{p.n1, p.hq, p.q2lo, p.q2w, nullptr, nullptr, (p.n2 + 3) / 4, 5 /* kZBlock / 4 = 2^5 pieces */,
                                  (long long)2 * p.hq * hpfw::kZBlock, hpfw::kZBlock, hpfw::z_floats_per_clip(p.hq, p.n2)};
    static_assert(hpfw::kZBlock == 128, "Rows2Out::zshift4 above");
    // HPFW_PRUNE bit 0: the row stage leaves out the last group's outputs that neither consumed window reads, when those it needs
    // are among the first and last two of a block
    dp->rows_out.last_edges = (h->prune & 1u) && !p.bluestein && !p.groups.empty() &&
                              hpfw::rows_last_edges_ok(p.rows_last_mask, p.groups.back().first * p.groups.back().second);
    if (p.bluestein) return 0;
    ca.n1 = p.n1;
    ca.n2 = p.n2;
    ca.hq = p.hq;
    ca.mt = p.cols_mt;
    ca.ks = p.cols_ks;
    ca.zclip = hpfw::z_floats_per_clip(p.hq, p.n2);
    int rc;
    const int8_t *img = nullptr;
    if ((rc = upload(p.cols_image, &img, dp))) return rc;
    ca.image = img;
    if (!p.cols2_image.empty()) {
        ca.mt2 = p.cols2_mt;
        ca.ks2 = p.cols2_ks;
        if ((rc = upload(p.cols2_image, &img, dp))) return rc;
        ca.image2 = img;
    }
    if ((rc = upload(p.cols_corr, &ca.corr, dp))) return rc;
    if ((rc = upload(p.ts_seed, reinterpret_cast<const hpfw::HostCf **>(&dp->rows_out.seed), dp))) return rc;
    return upload(p.ts_step, reinterpret_cast<const hpfw::HostCf **>(&dp->rows_out.step), dp);
}

// where the constant-Q stage finds the forward bins (plan_cache.h), its band tables, and room for the windows, which the
// device generates behind these uploads (generate_windows)
int cq_layout_tables(hpfw_gpu *, DevPlan *dp)
{
    const hpfw::HostPlan &p = dp->hp;
    hpfw::CqPlanDev &c = dp->cq;
    std::memset(&c, 0, sizeof(c)); // (g2 and its band tables stay null after the chirp-z forward transform)
    const hpfw::CqXLayout x = hpfw::cq_x_layout(p);
    c.kmin = p.kmin;
    c.nk = p.kmax - p.kmin;
    c.c = p.c;
    c.xn1 = x.xn1;
    c.xw = x.xw;
    c.xq0 = x.xq0;
    c.xclip = x.xclip;
    c.xmagic = x.xmagic;
    int rc;
    const std::vector<int> start(p.start, p.start + 121), lg(p.lg, p.lg + 121);
    if ((rc = upload(start, &c.start, dp))) return rc;
    if ((rc = upload(lg, &c.lg, dp))) return rc;
    if ((rc = upload(p.g_off, &c.g_off, dp))) return rc;
    if ((rc = device_table(dp, (size_t)p.g_total * sizeof(cf), &c.g))) return rc;
    c.rows_min = 4; // (measured on one box: 0..8 alike, 16 and above slower; element by element throughout +0.4 ms per 1000 clips)
    if (p.bluestein) return 0;
    // the windows once more, in the order the rows layout of the forward bins is read (kernels.h XsBandRows)
    const hpfw::CqRowsLayout r = hpfw::cq_rows_layout(p);
    dp->cq_rows_max = r.max_entries;
    if ((rc = device_table(dp, (size_t)r.total * sizeof(cf), &c.g2))) return rc;
    if ((rc = upload(r.g2_off, &c.g2_off, dp))) return rc;
    if ((rc = upload(r.q2a, &c.q2a, dp))) return rc;
    if ((rc = upload(r.nq2, &c.nq2, dp))) return rc;
    return upload(r.magic, &c.nq2_magic, dp);
}

// one chirp-z size class for all bands that share a transform length
int size_class_tables(hpfw_gpu *, DevPlan *dp)
{
    int rc;
    for (const hpfw::BluesteinClass &bc : dp->hp.classes) {
        hpfw::CqClassDev cd;
        cd.p = bc.p;
        cd.n_bands = (int)bc.bands.size();
        cd.radix = to_radix(bc.radix);
        if ((rc = upload(bc.tw, reinterpret_cast<const hpfw::HostCf **>(&cd.tw), dp))) return rc;
        if ((rc = upload(bc.gtw, reinterpret_cast<const hpfw::HostCf **>(&cd.gtw.tab), dp))) return rc;
        for (int g = 0; g < 4; ++g) cd.gtw.off[g] = bc.goff[g];
        cd.gtw.mid_off = bc.mid_off;
        if ((rc = upload(bc.vrev, reinterpret_cast<const hpfw::HostCf **>(&cd.vrev), dp))) return rc;
        if ((rc = upload(bc.bands, &cd.band, dp))) return rc;
        cd.len0 = bc.len0;
        cd.outer = bc.outer;
        dp->cls.push_back(cd);
    }
    return 0;
}

// the tables live on the device now (or in the staged image): drop the host copies; only the sizes are read from here on
int drop_host_copies(hpfw_gpu *, DevPlan *dp)
{
    hpfw::HostPlan &hp = dp->hp;
    for (auto *v : {&hp.rows_gtw, &hp.tw_n2, &hp.tw_n1, &hp.ts_seed, &hp.g}) std::vector<hpfw::HostCf>().swap(*v);
    for (auto *v : {&hp.cols_image, &hp.cols2_image}) std::vector<int8_t>().swap(*v);
    for (hpfw::BluesteinClass &bc : hp.classes)
        for (auto *v : {&bc.tw, &bc.gtw, &bc.vrev}) std::vector<hpfw::HostCf>().swap(*v);
    return 0;
}

// A corpus of files of many different lengths would otherwise keep one set of tables per length (14 MB for 30 s clips,
// growing with the length): the cache is bounded by evicting the least recently used plans.  Which ones, and where the
// device-wide wait falls (work already queued may still read a victim's tables), is plan_cache.h's choice.
int make_room(hpfw_gpu *h, DevPlan *dp)
{
    hpfw_gpu::PlanCache &c = h->cache;
    dp->last_use = ++c.plan_clock;
    const size_t budget = plan_cache_budget();
    if (c.plan_bytes + dp->bytes <= budget || c.plans.empty()) return 0;
    PlanTimer t(h, &PlanTiming::evict);
    std::vector<hpfw::CachedPlan> cached;
    cached.reserve(c.plans.size());
    for (const auto &kv : c.plans) cached.push_back({kv.first, kv.second->last_use, kv.second->bytes});
    const hpfw::Evictions ev = hpfw::choose_evictions(std::move(cached), c.plan_bytes, dp->bytes, budget, c.idle_clock);
    for (size_t i = 0; i < ev.victims.size(); ++i) {
        if ((int)i == ev.wait_before) {
            HIP_TRY(hipDeviceSynchronize());
            c.idle_clock = c.plan_clock;
        }
        auto victim = c.plans.find(ev.victims[i]);
        c.plan_bytes -= victim->second->bytes;
        {
            // an evicted length may be prepared ahead again by the reader threads the next time a file brings it
            std::scoped_lock lock(c.host_mtx);
            c.host_seen.erase(victim->first);
        }
        c.plans.erase(victim);
    }
    return 0;
}

// the constant-Q windows, generated behind the uploads of the band tables they read (S5, k_cq_tables.hip)
int generate_windows(hpfw_gpu *h, DevPlan *dp)
{
    int rc = plan_flush(dp);
    if (rc) return rc;
    std::vector<char>().swap(dp->stage);
    PlanTimer t(h, &PlanTiming::device_tables);
    const hpfw::HostPlan &p = dp->hp;
    const hpfw::CqPlanDev &c = dp->cq;
    hpfw::CqWindowBands wb;
    int lg_max = 0;
    for (int j = 0; j < 121; ++j) {
        wb.scale[j] = hpfw::cq_window_scale(h->conventions, p.big_m, p.psize[j]);
        wb.hann_den[j] = (int)hpfw::cq_hann_den(h->conventions, p.lg[j]);
        lg_max = std::max(lg_max, p.lg[j]);
    }
    hpfw::launch_cq_windows(c, wb, p.big_m, lg_max, const_cast<cf *>(c.g), h->cache.plan_stream.get());
    if (c.g2) hpfw::launch_cq_windows_rows(c, p.n1, dp->cq_rows_max, const_cast<cf *>(c.g2), h->cache.plan_stream.get());
    const hipError_t launched = hipGetLastError();
    return launched == hipSuccess ? 0 : fail(HPFW_E_HIP, std::string("constant-Q window tables: ") + hipGetErrorString(launched));
}
} // namespace

int get_plan(hpfw_gpu *h, int64_t n, DevPlan **out)
{
    auto it = h->cache.plans.find(n);
    if (it != h->cache.plans.end()) {
        it->second->last_use = ++h->cache.plan_clock;
        *out = it->second.get();
        return 0;
    }
    PlanTimer whole(h, &PlanTiming::total);
    if (h->cache.plan_timing) ++h->cache.plan_timing->plans;
    auto dp = std::make_unique<DevPlan>();
    dp->owner = h;
    const bool have_host = take_host_half(h, dp.get(), n);
    SeenGuard seen{h, n};
    int rc;
    if (!have_host && (rc = build_host_half(h, dp.get(), n))) return rc;
    // uploads and kernels queued on the table stream keep this order; the windows are generated behind the last flush
    using Step = int (*)(hpfw_gpu *, DevPlan *);
    static constexpr Step steps[] = {refuse_unrunnable, rows_tables,      chirpz_tables, cols_tables,     cq_layout_tables,
                                     size_class_tables, drop_host_copies, make_room,     generate_windows};
    for (Step step : steps)
        if ((rc = step(h, dp.get()))) return rc;
    // every table of the length is on its way on the table stream: whoever uses them first waits for this (ordered_call)
    HIP_TRY(hipEventRecord(h->cache.plan_ev.get(), h->cache.plan_stream.get()));
    h->cache.plan_ev_pending = true;
    h->cache.plan_bytes += dp->bytes;
    seen.dismissed = true;
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
    const int rc = host_plan(h, n_samples, hp, true);
    if (rc) return rc;
    // what get_plan would refuse later is refused here (callers size their buffers from this answer)
    if (!hpfw::row_fits_lds(hp.n2)) return unsupported(n_samples, "n2 exceeds the LDS");
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
    int rc;
    {
        hpfw::PlanSerial serial;
        rc = host_plan(h, n_samples, *hp, false);
    }
    if (rc) *hp = hpfw::HostPlan(); // n = 0: get_plan builds it again and reports why
    {
        std::scoped_lock lock(h->cache.host_mtx);
        h->cache.host_ready[n_samples] = std::move(hp);
        if (rc) h->cache.host_seen.erase(n_samples); // an unsupported length says so every time it is asked for
    }
    h->cache.host_cv.notify_all();
    return rc; // (the reason is the thread's last error already)
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
