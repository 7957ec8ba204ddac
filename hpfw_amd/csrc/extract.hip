// extract.hip -- PCM -> hashprints: the forward transform, the constant-Q and dB front end, the projection, the
// transposed and tempo variants, the stage entry points, the host-buffer round trips, resampling.
#include "handle.h"

#include <optional>

// nb: clips per front-end pass (large intermediates); ns: clips per back-end pass (S and P only)
// clips per front-end pass: the handle's batch, the number of clips, and what ~24 GB of workspace hold
int pass_clips(hpfw_gpu *h, const DevPlan *dp, int64_t n_clips)
{
    const hpfw::HostPlan &p = dp->hp;
    size_t per_clip = (size_t)121 * p.c * 4 + (size_t)64 * std::max(p.n_frames, 1) * 4;
    if (p.bluestein)
        per_clip += 2 * hpfw::bz_plane_bytes(dp->bz, 1) + (size_t)(p.kmax - p.kmin) * 8;
    else
        per_clip += (size_t)hpfw::z_floats_per_clip(p.hq, p.n2) * 4 + (size_t)p.n1 * p.q2w * 8 * (h->pass_pipeline ? 2 : 1); // (X[0], X[1])
    size_t work = 0;
    for (const hpfw::CqClassDev &cd : dp->cls) work = std::max(work, hpfw::cq_big_work_bytes(cd, 1));
    per_clip += work;
    const int64_t fit = std::max<int64_t>(1, (int64_t)(((size_t)24 << 30) / per_clip));
    // passes of equal size (1000 clips at a batch of 256: four passes of 250, not three and a ragged one)
    const int64_t cap = std::min<int64_t>(h->batch, fit), n = std::max<int64_t>(n_clips, 1);
    const int64_t passes = (n + cap - 1) / cap;
    return (int)((n + passes - 1) / passes);
}

int ensure_ws(hpfw_gpu *h, const DevPlan *dp, int nb, int ns, int x_bufs)
{
    const hpfw::HostPlan &p = dp->hp;
    size_t work = 0;
    for (const hpfw::CqClassDev &cd : dp->cls) work = std::max(work, hpfw::cq_big_work_bytes(cd, nb));
    if (work) {
        int rc = ensure(h->d_cqwork, work);
        if (rc) return rc;
    }
    const size_t planar = p.bluestein ? hpfw::bz_plane_bytes(dp->bz, nb) : 0;
    // ws[0]: the column stage's output z [hq][n2] (chirp-z path: a planar buffer); ws[1]: the forward bins (XsView layout),
    // x_bufs buffers of nb clips one behind the other (two where the passes of a group are pipelined)
    const size_t need[7] = {p.bluestein ? planar : (size_t)nb * hpfw::z_floats_per_clip(p.hq, p.n2) * 4,
                            p.bluestein ? (size_t)nb * (p.kmax - p.kmin) * 8 : (size_t)x_bufs * nb * p.n1 * p.q2w * 8,
                            (size_t)ns * 121 * p.c * 4, (size_t)ns * 64 * (size_t)std::max(p.n_frames, 1) * 4, // (P: the f32-chain projection only)
                            (size_t)ns * 121 * hpfw::kCqMaxWaves * 4,
                            0, planar};
    for (int i = 0; i < 7; ++i) {
        int rc = ensure(h->ws[i], need[i], h);
        if (rc) return rc;
    }
    return ensure(h->d_clipmax, (size_t)ns * 4, h);
}

namespace {
// the side streams and their events (chirp-z classes side by side, chunks of the forward transform in turn).  The last
// join event is made last: a set left incomplete by a failure is made anew by the next call.
int ensure_side_streams(hpfw_gpu *h)
{
    if (h->cq_join[hpfw_gpu::kCqSide - 1]) return HPFW_OK;
    bool ok = h->cq_fork.create() == hipSuccess;
    for (int b = 0; b < 2 && ok; ++b)
        for (int k = 0; k <= hpfw_gpu::kCqSide && ok; ++k) ok = h->pp_fwd[b][k].create() == hipSuccess && h->pp_cq[b][k].create() == hipSuccess;
    for (int k = 0; k < hpfw_gpu::kCqSide && ok; ++k) ok = h->cq_side[k].create() == hipSuccess && h->cq_join[k].create() == hipSuccess;
    return ok ? HPFW_OK : fail(HPFW_E_HIP, "side streams");
}

// One stage's work spread over lanes: lane 0 is the caller's stream s, lane k > 0 the side stream cq_side[k - 1].  fork(n)
// makes lanes 1..n wait for what s holds; the destructor makes s wait for every side lane that lane() handed out, on
// every exit, so that the next call never reuses the workspaces under work still queued on a side stream.  A failed
// join is reported to the call (ordered_call) and waited for on the host.
class Fanout {
public:
    Fanout(hpfw_gpu *h, hipStream_t s) : h_(h), s_(s) {}
    Fanout(const Fanout &) = delete;
    Fanout &operator=(const Fanout &) = delete;
    ~Fanout()
    {
        for (int k = 0; k < hpfw_gpu::kCqSide; ++k) {
            if (!(used_ >> k & 1u)) continue;
            hipStream_t side = h_->cq_side[k].get();
            hipEvent_t join = h_->cq_join[k].get();
            if (report(h_, hipEventRecord(join, side), "side stream join") || report(h_, hipStreamWaitEvent(s_, join, 0), "side stream join"))
                (void)hipStreamSynchronize(side);
        }
    }
    int fork(int n)
    {
        int rc = ensure_side_streams(h_);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(h_->cq_fork.get(), s_));
        for (int k = 0; k < n; ++k) HIP_TRY(hipStreamWaitEvent(h_->cq_side[k].get(), h_->cq_fork.get(), 0));
        return 0;
    }
    hipStream_t lane(int k)
    {
        if (k == 0) return s_;
        used_ |= 1u << (k - 1);
        return h_->cq_side[k - 1].get();
    }

private:
    hpfw_gpu *h_;
    hipStream_t s_;
    unsigned used_ = 0;
};

#if defined(HPFW_ROWS_SNAP) || defined(HPFW_ROWS_STAMPS)
hpfw::cf *g_rows_snap = nullptr; // diagnosis builds: fft_rows.h HPFW_SNAP / HPFW_STAMP
#endif

// the forward transform of nb clips (7-smooth lengths) queued in chunks that the first fwd_streams lanes of `fan` take in
// turn (or the lanes `turns` lists, over and over): PCM -> bins in x.  A lane's chunks follow each other in order, so
// every lane has one region of z of its own
void queue_fwd_chunks(hpfw_gpu *h, DevPlan *dp, const int16_t *d_pcm, int nb, hpfw::cf *x, Fanout &fan,
                      const std::vector<int> *turns = nullptr)
{
    const hpfw::HostPlan &p = dp->hp;
    hpfw::ColsQArgs cols = dp->cols;
    cols.variant = h->cols_variant;
    float *yp = h->ws[0].as<float>();
    const int lanes = h->fwd_streams;
    const int64_t region = (int64_t)h->fwd_chunk * dp->rows_out.zclip;
    int i = 0;
    for (int c0 = 0; c0 < nb; c0 += h->fwd_chunk, ++i) {
        const int nc = std::min(nb - c0, h->fwd_chunk);
        const int lane = turns ? (*turns)[i % turns->size()] : i % lanes;
        hipStream_t st = fan.lane(lane);
        float *zr = yp + lane * region;
        {
            Timed t(h, K_COLS, st);
            hpfw::launch_fwd_cols_q(cols, d_pcm + (int64_t)c0 * p.n, p.n, nc, zr, st);
        }
        {
            Timed t(h, K_ROWS, st);
            hpfw::launch_fwd_rows2(dp->rows, dp->rows_out, zr, nc, x + (int64_t)c0 * dp->rows_out.n1 * dp->rows_out.q2w, st);
        }
    }
}

// a1 + the forward transform for nb clips: PCM -> bins [kmin, kmax) in x
int run_forward(hpfw_gpu *h, DevPlan *dp, const int16_t *d_pcm, int nb, hpfw::cf *x, hipStream_t s)
{
    const hpfw::HostPlan &p = dp->hp;
    float *yp = h->ws[0].as<float>();
    int rc;
    if (p.bluestein) { // S15: the clip length has a prime factor above 7
        float *other = h->ws[6].as<float>();
        if (h->bz_chunk > 0 && nb >= 6 * h->bz_chunk) {
            // in chunks taken in turn by the streams, as below: 24 MB per clip between the three kernels
            const int lanes = h->fwd_streams;
            Fanout fan(h, s);
            if (lanes > 1 && (rc = fan.fork(lanes - 1))) return rc;
            const int64_t region = (int64_t)(hpfw::bz_plane_bytes(dp->bz, h->bz_chunk) / sizeof(float));
            int i = 0;
            for (int c0 = 0; c0 < nb; c0 += h->bz_chunk, ++i) {
                const int nc = std::min(nb - c0, h->bz_chunk);
                const int lane = i % lanes;
                hipStream_t st = fan.lane(lane);
                float *ya = yp + lane * region, *yb = other + lane * region;
                {
                    Timed t(h, K_COLS, st);
                    hpfw::launch_bz_cols_first(dp->bz, d_pcm + (int64_t)c0 * p.n, p.n, nc, ya, st);
                }
                {
                    Timed t(h, K_ROWS, st);
                    hpfw::launch_bz_rows_both(dp->rows, dp->bz, ya, nc, yb, st);
                }
                {
                    Timed t(h, K_COLS, st);
                    hpfw::launch_bz_cols_last(dp->bz, yb, nc, x + (int64_t)c0 * dp->cq.xclip, st);
                }
            }
            return check_launch("bz_chunks");
        }
        {
            Timed t(h, K_COLS, s);
            hpfw::launch_bz_cols_first(dp->bz, d_pcm, p.n, nb, yp, s); // pcm as it lies -> G' [q1][k2']
        }
        if ((rc = check_launch("bz_cols"))) return rc;
        {
            Timed t(h, K_ROWS, s);
            hpfw::launch_bz_rows_both(dp->rows, dp->bz, yp, nb, other, s); // G' -> A -> C -> H' [q1][m2]
        }
        if ((rc = check_launch("bz_rows"))) return rc;
        {
            Timed t(h, K_COLS, s);
            hpfw::launch_bz_cols_last(dp->bz, other, nb, x, s);
        }
        return check_launch("bz_cols");
    }
    Timed span(h, K_FWD, s);                     // the whole forward transform as one span (its chunks overlap)
    hpfw::ColsQArgs cols = dp->cols;
    cols.variant = h->cols_variant;
    if (h->fwd_chunk > 0 && nb >= 6 * h->fwd_chunk) {
        const int lanes = h->fwd_streams;
        Fanout fan(h, s);
        if (lanes > 1 && (rc = fan.fork(lanes - 1))) return rc;
        queue_fwd_chunks(h, dp, d_pcm, nb, x, fan);
        return check_launch("fwd_chunks");
    }
    {
        Timed t(h, K_COLS, s);
        hpfw::launch_fwd_cols_q(cols, d_pcm, p.n, nb, yp, s); // pcm as it lies -> z [hq][Re, Im][n2]
    }
    if ((rc = check_launch("fwd_cols"))) return rc;
    {
        Timed t(h, K_ROWS, s);
#if defined(HPFW_ROWS_SNAP)
        dp->rows.snap = g_rows_snap;
#endif
#if defined(HPFW_ROWS_STAMPS)
        dp->rows.stamps = reinterpret_cast<long long *>(g_rows_snap);
#endif
        hpfw::launch_fwd_rows2(dp->rows, dp->rows_out, yp, nb, x, s); // -> x [n1][q2w]
    }
    return check_launch("fwd_rows");
}
} // namespace

// front end for nb clips: PCM -> dB terms t (and their per-clip maximum in d_clipmax) at clip slot
// `slot` of the S workspace; finish_db: also turn them into the dB spectrogram S = max(t - t_max, -80)
// in place (the projection does that itself while staging, the covariance wants S)
int run_front(hpfw_gpu *h, DevPlan *dp, const int16_t *d_pcm, int nb, int slot, bool finish_db, hipStream_t s)
{
    using hpfw::cf;
    const hpfw::HostPlan &p = dp->hp;
    cf *x = h->ws[1].as<cf>();
    float *mag = h->ws[2].as<float>() + (size_t)slot * 121 * p.c;
    float *mm = h->ws[4].as<float>() + (size_t)slot * 121 * hpfw::kCqMaxWaves; // this pass's wave maxima
    float *clipmax = h->d_clipmax.as<float>() + slot;
    int rc;
    if ((rc = run_forward(h, dp, d_pcm, nb, x, s))) return rc;
    {
        // fork: classes that run in LDS alone go to the side streams in turn (the caller's stream takes one too), largest
        // first -- dp->cls is in ascending order of size; classes with passes through the shared global workspace stay
        // on the caller's stream.  join: the caller's stream waits for every side stream used.
        Timed t(h, K_CQ, s);
        int n_lds = 0;
        for (const hpfw::CqClassDev &cd : dp->cls) n_lds += cd.outer ? 0 : 1;
        // (a handful of clips: the five launches are tens of microseconds each, and forking costs the host a dozen calls)
        const bool fork = h->cq_concurrent && n_lds > 1 && nb >= 4;
        Fanout fan(h, s);
        if (fork && (rc = fan.fork(hpfw_gpu::kCqSide))) return rc;
        int turn = 0;
        for (size_t ci = dp->cls.size(); ci-- > 0;) {
            const hpfw::CqClassDev &cd = dp->cls[ci];
            if (cd.outer) {
                hpfw::launch_cq_big_class(dp->cq, cd, x, nb, h->d_cqwork.as<cf>(), mag, mm, h->db_fast ? hpfw::kDbFast : hpfw::kDbSpec, s);
                continue;
            }
            const int lane = fork ? turn++ % (hpfw_gpu::kCqSide + 1) : 0; // 0: the caller's stream
            hpfw::launch_cq_class(dp->cq, cd, x, nb, mag, mm, h->db_fast ? hpfw::kDbFast : hpfw::kDbSpec, fan.lane(lane));
        }
        if ((rc = check_launch("cq_chirpz"))) return rc;
    }
    {
        Timed t(h, K_DB, s);
        hpfw::launch_clipmax(mm, clipmax, nb, s);
        if (finish_db) hpfw::launch_db_finish(mag, clipmax, nb, (int64_t)121 * p.c, s);
    }
    return check_launch("db");
}

int q_split(hpfw_gpu *h, int n_shifts, int64_t n_clips, int64_t c, hpfw::QSplit *qs, const hpfw::QSplit **use)
{
    *use = nullptr;
    if (n_shifts || h->q_products != 6 || !h->projection) return 0;
    const int64_t tiles = hpfw::project_q_tiles(n_clips, c);
    if (tiles <= 0) return 0;
    if (int rc = ensure(h->d_q_split, hpfw::project_q_split_bytes(tiles), h)) return rc;
    *qs = {h->d_q_thr.as<int32_t>(), h->d_q_split.get()};
    *use = qs;
    return 0;
}

namespace {
// back end for ns clips: dB spectrograms of the S workspace -> hashprints [ns][max(n_shifts, 1)][n_hp] of the filter
// images at `images` as launch_hashprints_q takes them (the f32 chain: the handle's filters, n_shifts = 0)
int run_back(hpfw_gpu *h, DevPlan *dp, const void *images, int n_shifts, int ns, uint64_t *d_hp, hipStream_t s)
{
    const hpfw::HostPlan &p = dp->hp;
    const float *sdb = h->ws[2].as<float>();
    int rc;
    if (h->projection) { // S9q: reference level, clip, exact integer sums on the int8 matrix pipe, sign and pack in ONE kernel
        hpfw::QSplit qs;
        const hpfw::QSplit *split;
        if ((rc = q_split(h, n_shifts, ns, p.c, &qs, &split))) return rc;
        {
            Timed t(h, K_PROJECT, s);
            hpfw::launch_hashprints_q(images, n_shifts, sdb, h->d_clipmax.as<float>(), ns, p.c, d_hp, nullptr, s, split);
        }
        if (split) h->q_last_tiles = hpfw::project_q_tiles(ns, p.c);
        return check_launch("project");
    }
    float *proj = h->ws[3].as<float>();
    {
        Timed t(h, K_PROJECT, s);
        hpfw::launch_project(h->d_fpack.as<float>(), sdb, h->d_clipmax.as<float>(), ns, p.c, proj, s);
    }
    if ((rc = check_launch("project"))) return rc;
    {
        Timed t(h, K_PACK, s);
        hpfw::launch_pack(proj, ns, p.n_frames, d_hp, s);
    }
    return check_launch("delta_pack");
}

constexpr int kBackBatch = 1024; // clips per projection launch: ~10^4 workgroups, a small launch tail

// whether the passes of a group of ns clips, nbmax to a pass, run pipelined (run_group_pipelined) instead of joined one
// after the other (run_front): 7-smooth length, every class in LDS alone and side by side, two passes or more, each with
// chunks enough for the forward lanes; and no timing but the hashprint kernel's and the forward span, so that every
// other kind keeps the launches and the meaning it has in the joined loop
bool group_pipelines(const hpfw_gpu *h, const DevPlan *dp, int ns, int nbmax)
{
    constexpr unsigned kept = 1u << K_PROJECT | 1u << K_FWD;
    if (!h->pass_pipeline || dp->hp.bluestein || !h->cq_concurrent || h->fwd_chunk <= 0 || (h->timing_mask & ~kept)) return false;
    for (const hpfw::CqClassDev &cd : dp->cls)
        if (cd.outer) return false;
    const int passes = (ns + nbmax - 1) / nbmax, last = ns - (passes - 1) * nbmax; // (the last pass is the smallest)
    return passes >= 2 && last >= 6 * h->fwd_chunk;
}

// The front ends of a group of ns clips, nbmax to a pass, with the passes pipelined: PCM -> dB terms in slots 0 .. ns of the S
// workspace and their per-clip maxima.  Units: F(p), the forward chunks of pass p on the forward lanes (lanes 0 ..
// fwd_streams - 1; lane 0 is the caller's stream), into X[p & 1]; Q(p), its chirp-z classes; M, one clipmax launch over the
// group (the wave maxima lie by slot).  Queued as F(0), then Q(p), F(p + 1) for every p, ordered by events alone:
// Q(p) waits for every lane of F(p); F(p + 2) waits for every class of Q(p) (X[p & 1]); F(p + 1) waits for nothing of Q(p)
// but what was queued before it on its own lane; M follows the join of every lane into s.  The largest class goes to the
// first lane without forward chunks, so that what ends last holds up no chunk of the next pass; the second largest goes
// ahead of the chunks of the last forward lane, the others ahead of those of lane 0 (streams that share a hardware queue
// run one after the other, and three of a process's four queues are to be had: handle.h).  HPFW_PASS_PLAN names another
// plan.  S and the wave maxima are written by slot, z by lane.
// fwd_span (K_FWD): per pass, on s, from before its first chunk there to after s has waited for its last; from the second
// pass on the span begins under the largest class of the pass before.
int run_group_pipelined(hpfw_gpu *h, DevPlan *dp, const int16_t *d_pcm, int ns, int nbmax, hipStream_t s)
{
    using hpfw::cf;
    const hpfw::HostPlan &p = dp->hp;
    constexpr int kLanes = hpfw_gpu::kCqSide + 1;
    const int passes = (ns + nbmax - 1) / nbmax;
    const int64_t xbuf = (int64_t)nbmax * p.n1 * p.q2w;
    const int db = h->db_fast ? hpfw::kDbFast : hpfw::kDbSpec;
    // the plan: the lane of every chunk in turn, the lane of every class (dp->cls is in ascending order of size)
    std::vector<int> turns = h->pp_turns, lane_of(dp->cls.size());
    if (turns.empty())
        for (int k = 0; k < h->fwd_streams; ++k) turns.push_back(k);
    unsigned fwd_lanes = 0, cq_lanes = 0;
    for (int k : turns) fwd_lanes |= 1u << k;
    const int fl = h->fwd_streams;
    for (size_t ci = dp->cls.size(), i = 0; ci-- > 0; ++i) {
        if (!h->pp_class_lane.empty()) lane_of[ci] = h->pp_class_lane[std::min(i, h->pp_class_lane.size() - 1)];
        else lane_of[ci] = i == 0 ? std::min(fl, kLanes - 1) : i == 1 ? fl - 1 : 0;
        cq_lanes |= 1u << lane_of[ci];
    }
    int rc;
    {
        Fanout fan(h, s);
        if ((rc = fan.fork(hpfw_gpu::kCqSide))) return rc;
        std::optional<Timed> span;
        auto forward = [&](int pass) -> int {
            const int c0 = pass * nbmax, nb = std::min(nbmax, ns - c0), b = pass & 1;
            span.emplace(h, K_FWD, s);
            if (pass >= 2) // X[b] is read by the classes of pass - 2
                for (int k = 0; k < kLanes; ++k)
                    for (int j = 0; j < kLanes; ++j)
                        if ((fwd_lanes >> k & 1u) && (cq_lanes >> j & 1u) && j != k) HIP_TRY(hipStreamWaitEvent(fan.lane(k), h->pp_cq[b][j].get(), 0));
            queue_fwd_chunks(h, dp, d_pcm + (int64_t)c0 * p.n, nb, h->ws[1].as<cf>() + b * xbuf, fan, &turns);
            for (int k = 0; k < kLanes; ++k)
                if (fwd_lanes >> k & 1u) HIP_TRY(hipEventRecord(h->pp_fwd[b][k].get(), fan.lane(k)));
            return check_launch("fwd_chunks");
        };
        auto classes = [&](int pass) -> int {
            const int c0 = pass * nbmax, nb = std::min(nbmax, ns - c0), b = pass & 1;
            const bool timed = span && span->on;
            for (int j = 0; j < kLanes; ++j)
                if ((cq_lanes >> j & 1u) || (j == 0 && timed))
                    for (int k = 0; k < kLanes; ++k)
                        if ((fwd_lanes >> k & 1u) && k != j) HIP_TRY(hipStreamWaitEvent(fan.lane(j), h->pp_fwd[b][k].get(), 0));
            span.reset();
            for (size_t ci = dp->cls.size(); ci-- > 0;)
                hpfw::launch_cq_class(dp->cq, dp->cls[ci], h->ws[1].as<cf>() + b * xbuf, nb, h->ws[2].as<float>() + (size_t)c0 * 121 * p.c,
                                      h->ws[4].as<float>() + (size_t)c0 * 121 * hpfw::kCqMaxWaves, db, fan.lane(lane_of[ci]));
            if (pass + 2 < passes)
                for (int j = 0; j < kLanes; ++j)
                    if (cq_lanes >> j & 1u) HIP_TRY(hipEventRecord(h->pp_cq[b][j].get(), fan.lane(j)));
            return check_launch("cq_chirpz");
        };
        if ((rc = forward(0))) return rc;
        for (int pass = 0; pass < passes; ++pass) {
            if ((rc = classes(pass))) return rc;
            if (pass + 1 < passes && (rc = forward(pass + 1))) return rc;
        }
    } // (every lane used joins s)
    hpfw::launch_clipmax(h->ws[4].as<float>(), h->d_clipmax.as<float>(), ns, s);
    return check_launch("db");
}

// the one report of a handle without filters
int check_filters(const hpfw_gpu *h) { return h->has_filters ? 0 : fail(HPFW_E_NOFILTERS, "no filters: call hpfw_gpu_set_filters or hpfw_gpu_learn_filters first"); }

// shifts of the transposed entry points: 1..64 distinct values, |s| <= 120 (checked before anything else)
int check_shifts(const int32_t *shifts, int n_shifts)
{
    if (!shifts || n_shifts < 1 || n_shifts > hpfw::kMaxShifts) return fail(HPFW_E_INVALID, "shifts: 1 to 64 values");
    for (int i = 0; i < n_shifts; ++i) {
        if (shifts[i] < -(hpfw::kBins - 1) || shifts[i] > hpfw::kBins - 1) return fail(HPFW_E_INVALID, "shifts: |s| <= 120");
        for (int j = 0; j < i; ++j)
            if (shifts[j] == shifts[i]) return fail(HPFW_E_INVALID, "shifts: values must be distinct");
    }
    return 0;
}

// the shifted filter images of `shifts` on stream s (kept while the list and the filters stay the same)
int shift_images(hpfw_gpu *h, const int32_t *shifts, int n_shifts, hipStream_t s)
{
    std::vector<int32_t> want(shifts, shifts + n_shifts);
    if (want == h->shift_images_of) return 0;
    h->shift_images_of.clear();
    int rc;
    if ((rc = ensure(h->d_shift_images, (size_t)n_shifts * hpfw::project_q_image_bytes()))) return rc;
    hpfw::ShiftList sl{n_shifts, {}};
    for (int i = 0; i < n_shifts; ++i) sl.s[i] = shifts[i];
    hpfw::launch_shift_filter_images(h->d_fq_image.get(), sl, h->d_shift_images.get(), s);
    if ((rc = check_launch("shift_filter_images"))) return rc;
    h->shift_images_of = std::move(want);
    return 0;
}

// the common checks of the transposed extraction entry points
int check_transposed(hpfw_gpu *h, const int32_t *shifts, int n_shifts)
{
    int rc;
    if ((rc = check_shifts(shifts, n_shifts))) return rc;
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (!h->projection) return fail(HPFW_E_INVALID, "transposed extraction needs projection mode 1 (fixed point)");
    if ((rc = check_filters(h))) return rc;
    return 0;
}

// dB spectrograms [n_clips][121][c] (device) -> hashprints [n_clips][max(n_shifts, 1)][c - 99], 256 clips per launch, of
// the handle's filters (n_shifts = 0) or of their images moved by each of shifts[0 .. n_shifts)
int hashprints_from_db(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, const int32_t *shifts, int n_shifts, uint64_t *d_hp,
                       hipStream_t s)
{
    const int64_t nf = c - (hpfw::kCtx - 1), nhp = nf - hpfw::kLag;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        int rc;
        if (n_shifts && (rc = shift_images(h, shifts, n_shifts, s))) return rc;
        const void *images = n_shifts ? h->d_shift_images.get() : h->d_fq_image.get();
        const int nbmax = 256;
        if (!h->projection && (rc = ensure(h->ws[3], (size_t)nbmax * 64 * (size_t)nf * 4))) return rc;
        hpfw::QSplit qs;
        const hpfw::QSplit *split;
        if ((rc = q_split(h, n_shifts, std::min<int64_t>(nbmax, n_clips), c, &qs, &split))) return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            if (h->projection) {
                Timed t(h, K_PROJECT, s);
                hpfw::launch_hashprints_q(images, n_shifts, d_db + c0 * 121 * c, nullptr, nb, (int)c, d_hp + c0 * std::max(n_shifts, 1) * nhp,
                                          nullptr, s, split);
                if (split) h->q_last_tiles = hpfw::project_q_tiles(nb, c);
            } else {
                hpfw::launch_project(h->d_fpack.as<float>(), d_db + c0 * 121 * c, nullptr, nb, (int)c, h->ws[3].as<float>(), s);
                hpfw::launch_pack(h->ws[3].as<float>(), nb, (int)nf, d_hp + c0 * nhp, s);
            }
            if ((rc = check_launch("project"))) return rc;
        }
        return 0;
    });
}

// ---- queries at another tempo ----
// The time-scaled dB spectrograms of the (clip, tempo) pairs of one sub-batch live in h->d_tempo: at most this many bytes,
// unless a single pair is larger (an 18-minute clip at tempo 2: 84 MB)
constexpr size_t kTempoBudget = (size_t)256 << 20;

// tempos of the tempo entry points: 1..64 finite values in [0.5, 2], distinct steps, n_tempos max(n_shifts, 1) <= 64
int check_tempos(const float *tempos, int n_tempos, int n_shifts)
{
    if (!tempos || n_tempos < 1 || n_tempos > hpfw::kMaxTempos) return fail(HPFW_E_INVALID, "tempos: 1 to 64 values");
    for (int i = 0; i < n_tempos; ++i) {
        if (!(tempos[i] >= 0.5f && tempos[i] <= 2.0f)) return fail(HPFW_E_INVALID, "tempos: finite values in [0.5, 2]");
        for (int j = 0; j < i; ++j)
            if (hpfw::tempo_step(tempos[j]) == hpfw::tempo_step(tempos[i]))
                return fail(HPFW_E_INVALID, "tempos: values must have distinct steps rint(65536 / tempo)");
    }
    if ((int64_t)n_tempos * std::max(n_shifts, 1) > hpfw::kMaxShifts) return fail(HPFW_E_INVALID, "tempos x shifts: at most 64 variants");
    return 0;
}

// the common checks of the tempo entry points (all before the handle is used); *tl: the steps
int check_tempo_call(hpfw_gpu *h, const float *tempos, int n_tempos, const int32_t *shifts, int n_shifts, hpfw::TempoList *tl)
{
    int rc;
    if ((rc = check_tempos(tempos, n_tempos, n_shifts))) return rc;
    if ((shifts || n_shifts) && (rc = check_shifts(shifts, n_shifts))) return rc;
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (!h->projection) return fail(HPFW_E_INVALID, "tempo extraction needs projection mode 1 (fixed point)");
    if ((rc = check_filters(h))) return rc;
    tl->n = n_tempos;
    for (int i = 0; i < n_tempos; ++i) tl->step[i] = hpfw::tempo_step(tempos[i]);
    return 0;
}

// the common length of the tempo variants of a clip of c columns: the fewest columns any of the steps gives
int64_t tempo_common_columns(int64_t c, const hpfw::TempoList &tl)
{
    int64_t ct = INT64_MAX;
    for (int i = 0; i < tl.n; ++i) ct = std::min(ct, hpfw::tempo_columns(c, tl.step[i]));
    return ct;
}

// dB spectrograms [nb][121][c] (device) -> hashprints [nb][tl.n][max(n_shifts, 1)][ct - 99]: the (clip, tempo) pairs in
// sub-batches that fit h->d_tempo -- whole clips with all their tempos while one clip's fit, else runs of one clip's tempos
// -- each scaled to ct columns and projected as launch_hashprints_q's clips; pair p's hashprints start at p max(n_shifts, 1)
// (ct - 99)
int tempo_back(hpfw_gpu *h, const void *images, int n_shifts, const float *d_db, int64_t nb, int64_t c, const hpfw::TempoList &tl,
               int64_t ct, uint64_t *d_hp, hipStream_t s)
{
    const int64_t per_pair = (int64_t)std::max(n_shifts, 1) * (ct - (hpfw::kCtx - 1) - hpfw::kLag);
    const size_t pair_bytes = (size_t)hpfw::kBins * ct * 4;
    const int64_t pairs = std::max<int64_t>(1, (int64_t)(kTempoBudget / pair_bytes));
    const int64_t cb = pairs >= tl.n ? std::min<int64_t>(pairs / tl.n, nb) : 1; // clips per sub-batch
    const int tb = pairs >= tl.n ? tl.n : (int)pairs;                           // tempos per sub-batch
    int rc;
    if ((rc = ensure(h->d_tempo, (size_t)cb * tb * pair_bytes, h))) return rc;
    float *scaled = h->d_tempo.as<float>();
    for (int64_t c0 = 0; c0 < nb; c0 += cb) {
        const int nc = (int)std::min(cb, nb - c0);
        for (int j0 = 0; j0 < tl.n; j0 += tb) {
            hpfw::TempoList sub{std::min(tb, tl.n - j0), {}};
            for (int j = 0; j < sub.n; ++j) sub.step[j] = tl.step[j0 + j];
            hpfw::launch_tempo_scale(d_db + c0 * hpfw::kBins * c, nc, c, sub, ct, scaled, s);
            if ((rc = check_launch("tempo_scale"))) return rc;
            {
                Timed t(h, K_PROJECT, s);
                hpfw::launch_hashprints_q(images, n_shifts, scaled, nullptr, nc * sub.n, (int)ct, d_hp + (c0 * tl.n + j0) * per_pair, nullptr, s);
            }
            if ((rc = check_launch("project"))) return rc;
        }
    }
    return 0;
}

// PCM (device) -> hashprints [n_clips][n_tempos][max(n_shifts, 1)][ct - 99]: front ends as hpfw_gpu_stage_spectrogram runs them
// (the dB spectrogram finished in the S workspace), then tempo_back on each pass
int extract_tempo_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, const float *tempos, int n_tempos,
                        const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream)
{
    hpfw::TempoList tl;
    int rc = check_tempo_call(h, tempos, n_tempos, shifts, n_shifts, &tl);
    if (rc) return rc;
    if (!d_pcm || !d_hp || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    if ((rc = get_plan(h, n_samples, &dp))) return rc;
    const int64_t c = dp->hp.c, ct = tempo_common_columns(c, tl);
    if (ct - (hpfw::kCtx - 1) - hpfw::kLag < 1) return fail(HPFW_E_UNSUPPORTED, "clip too short to yield a hashprint at the slowest tempo");
    if (n_clips == 0) return 0;
    const int64_t per_clip = (int64_t)tl.n * std::max(n_shifts, 1) * (ct - (hpfw::kCtx - 1) - hpfw::kLag);
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_shifts && (rc = shift_images(h, shifts, n_shifts, s))) return rc;
        const void *images = n_shifts ? h->d_shift_images.get() : h->d_fq_image.get();
        const int nbmax = pass_clips(h, dp, n_clips);
        if ((rc = ensure_ws(h, dp, nbmax, nbmax))) return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            if ((rc = run_front(h, dp, d_pcm + c0 * n_samples, nb, 0, true, s))) return rc;
            if ((rc = tempo_back(h, images, n_shifts, h->ws[2].as<float>(), nb, c, tl, ct, d_hp + c0 * per_clip, s))) return rc;
        }
        return 0;
    });
}

// PCM (device) -> hashprints [n_clips][max(n_shifts, 1)][n_hp] as hashprints_from_db: front ends of up to a pass of clips, back
// ends of up to kBackBatch clips
int extract_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, const int32_t *shifts, int n_shifts,
                  uint64_t *d_hp, void *stream)
{
    if (!h || !d_pcm || !d_hp || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (int rc = check_filters(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, n_samples, &dp);
    if (rc) return rc;
    if (dp->hp.n_hp <= 0) return fail(HPFW_E_UNSUPPORTED, "clip too short to yield a hashprint");
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_shifts && (rc = shift_images(h, shifts, n_shifts, s))) return rc;
        const void *images = n_shifts ? h->d_shift_images.get() : h->d_fq_image.get();
        const int nbmax = pass_clips(h, dp, n_clips);
        const int nsmax = (int)std::min<int64_t>(std::max(kBackBatch, nbmax), std::max<int64_t>(n_clips, 1));
        const bool pipelined = group_pipelines(h, dp, (int)std::min<int64_t>(nsmax, n_clips), nbmax); // (the first group is the largest)
        if ((rc = ensure_ws(h, dp, nbmax, nsmax, pipelined ? 2 : 1))) return rc;
        for (int64_t s0 = 0; s0 < n_clips; s0 += nsmax) {
            const int ns = (int)std::min<int64_t>(nsmax, n_clips - s0);
            if (pipelined && group_pipelines(h, dp, ns, nbmax)) {
                if ((rc = run_group_pipelined(h, dp, d_pcm + s0 * n_samples, ns, nbmax, s))) return rc;
            } else {
                for (int c0 = 0; c0 < ns; c0 += nbmax) {
                    const int nb = std::min(nbmax, ns - c0);
                    if ((rc = run_front(h, dp, d_pcm + (s0 + c0) * n_samples, nb, c0, false, s))) return rc;
                }
            }
            if ((rc = run_back(h, dp, images, n_shifts, ns, d_hp + s0 * std::max(n_shifts, 1) * dp->hp.n_hp, s))) return rc;
        }
        return 0;
    });
}

// the host-buffer round trip of an extraction whose output is per_clip hashprints per clip: device(d_pcm, cnt, d_hp, stream)
// extracts cnt clips
template <class Device>
int staged_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, int64_t per_clip, uint64_t *hp,
                      Device device)
{
    int rc;
    // uploads in chunks on a copy stream, two device buffers deep, so that the PCIe transfer of chunk
    // i + 1 runs under the kernels of chunk i (from pinned host memory; a pageable source is staged
    // by the runtime and overlaps only partly)
    const int64_t chunk = std::min<int64_t>(n_clips, std::max<int64_t>(1, (192ll << 20) / (n_samples * 2)));
    if ((rc = ensure(h->stage_hp, (size_t)n_clips * std::max<int64_t>(per_clip, 1) * 8))) return rc;
    for (int b = 0; b < 2; ++b) {
        if (b == 1 && chunk >= n_clips) break; // one chunk: one buffer
        if ((rc = ensure(h->stage_pcm[b], (size_t)chunk * n_samples * 2))) return rc;
    }
    if (!h->stage_consumed[1]) { // (made last: a set left incomplete by a failure is made anew by the next call)
        HIP_TRY(h->stage_copy.create());
        HIP_TRY(h->stage_comp.create());
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(h->stage_copied[b].create());
            HIP_TRY(h->stage_consumed[b].create());
        }
    }
    hipStream_t s_copy = h->stage_copy.get(), s_comp = h->stage_comp.get();
    uint64_t *d_hp = h->stage_hp.as<uint64_t>();
    int64_t ci = 0;
    for (int64_t c0 = 0; !rc && c0 < n_clips; c0 += chunk, ++ci) {
        const int b = (int)(ci & 1);
        const int64_t cnt = std::min(chunk, n_clips - c0);
        int16_t *d_pcm = h->stage_pcm[b].as<int16_t>();
        hipEvent_t copied = h->stage_copied[b].get(), consumed = h->stage_consumed[b].get();
        if (ci >= 2 && hipStreamWaitEvent(s_copy, consumed, 0) != hipSuccess) rc = fail(HPFW_E_HIP, "event wait failed");
        if (!rc && hipMemcpyAsync(d_pcm, pcm + c0 * n_samples, (size_t)cnt * n_samples * 2, hipMemcpyHostToDevice, s_copy) !=
                       hipSuccess)
            rc = fail(HPFW_E_HIP, "H2D copy failed");
        if (!rc && (hipEventRecord(copied, s_copy) != hipSuccess || hipStreamWaitEvent(s_comp, copied, 0) != hipSuccess))
            rc = fail(HPFW_E_HIP, "event record failed");
        if (!rc) rc = device(d_pcm, cnt, d_hp + c0 * per_clip, s_comp);
        if (!rc && hipEventRecord(consumed, s_comp) != hipSuccess) rc = fail(HPFW_E_HIP, "event record failed");
    }
    if (hipStreamSynchronize(s_copy) != hipSuccess && !rc) rc = fail(HPFW_E_HIP, "H2D copy failed");
    if (!rc && hipMemcpyAsync(hp, d_hp, (size_t)n_clips * per_clip * 8, hipMemcpyDeviceToHost, s_comp) != hipSuccess)
        rc = fail(HPFW_E_HIP, "D2H copy failed");
    if (hipStreamSynchronize(s_comp) != hipSuccess && !rc) rc = fail(HPFW_E_HIP, "kernel execution failed");
    return rc;
}
} // namespace

extern "C" {

// dB spectrograms [n_clips][121][c] (device) -> hashprints [n_clips][c - 99] with the handle's projection
int hpfw_gpu_hashprints_from_db(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, uint64_t *d_hp, void *stream)
{
    if (!h || !d_db || !d_hp) return fail(HPFW_E_INVALID, "null argument");
    if (int rc = check_filters(h)) return rc;
    if (c - (hpfw::kCtx - 1) - hpfw::kLag <= 0) return 0;
    return hashprints_from_db(h, d_db, n_clips, c, nullptr, 0, d_hp, (hipStream_t)stream);
}

// the six-product split's last launch on this handle (tests, profiles): its tiles, the open values listed in them and the
// tiles redone with nine products.  Waits for the device.  All zero after a launch of the nine-product kernel
int hpfw_gpu_debug_q_products(hpfw_gpu *h, int64_t *tiles, int64_t *listed, int64_t *redone)
{
    if (!h || !tiles || !listed || !redone) return fail(HPFW_E_INVALID, "null argument");
    *tiles = *listed = *redone = 0;
    if (h->q_products != 6 || h->q_last_tiles <= 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> counts((size_t)h->q_last_tiles);
    HIP_TRY(hipMemcpy(counts.data(), h->d_q_split.get(), counts.size() * 4, hipMemcpyDeviceToHost));
    *tiles = h->q_last_tiles;
    for (uint32_t v : counts) {
        if (v == 0xffffffffu) *redone += 1;
        else *listed += v;
    }
    return 0;
}

int hpfw_gpu_stage_delta_q(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, int64_t *d_delta, uint64_t *d_hp, void *stream)
{
    if (!h || !d_db || !d_delta) return fail(HPFW_E_INVALID, "null argument");
    if (int rc = check_filters(h)) return rc;
    const int64_t nhp = c - (hpfw::kCtx - 1) - hpfw::kLag;
    if (nhp <= 0 || n_clips <= 0) return 0;
    if (n_clips > 65535) return fail(HPFW_E_INVALID, "at most 65535 clips per call");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        uint64_t *hp = d_hp;
        if (!hp) { // the kernel always writes its hashprints
            if (int rc = ensure(h->ws[3], (size_t)n_clips * (size_t)nhp * 8)) return rc;
            hp = h->ws[3].as<uint64_t>();
        }
        hpfw::launch_hashprints_q(h->d_fq_image.get(), 0, d_db, nullptr, (int)n_clips, (int)c, hp, (long long *)d_delta, s);
        return check_launch("project");
    });
}

int hpfw_gpu_hashprints_from_db_transposed(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, const int32_t *shifts,
                                           int n_shifts, uint64_t *d_hp, void *stream)
{
    int rc = check_transposed(h, shifts, n_shifts);
    if (rc) return rc;
    if (!d_db || !d_hp || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (c - (hpfw::kCtx - 1) - hpfw::kLag <= 0 || n_clips == 0) return 0;
    return hashprints_from_db(h, d_db, n_clips, c, shifts, n_shifts, d_hp, (hipStream_t)stream);
}

int hpfw_gpu_extract_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                           uint64_t *d_hp, void *stream)
{
    return extract_pcm16(h, d_pcm, n_samples, n_clips, nullptr, 0, d_hp, stream);
}

int hpfw_gpu_extract_transposed_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, const int32_t *shifts,
                                      int n_shifts, uint64_t *d_hp, void *stream)
{
    if (int rc = check_transposed(h, shifts, n_shifts)) return rc;
    return extract_pcm16(h, d_pcm, n_samples, n_clips, shifts, n_shifts, d_hp, stream);
}

// host PCM -> host hashprints [n_clips][max(n_shifts, 1)][n_hp], through extract_pcm16 (shifts as there)
static int extract_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, const int32_t *shifts, int n_shifts,
                              uint64_t *hp)
{
    if (!h || !pcm || !hp || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hpfw_geometry g;
    int rc = hpfw_gpu_geometry(h, n_samples, &g);
    if (rc) return rc;
    if (n_clips == 0) return 0;
    return staged_pcm16_host(h, pcm, n_samples, n_clips, std::max(n_shifts, 1) * g.n_hp, hp,
                             [&](const int16_t *d_pcm, int64_t cnt, uint64_t *d_hp, hipStream_t st) {
                                 return extract_pcm16(h, d_pcm, n_samples, cnt, shifts, n_shifts, d_hp, st);
                             });
}

int hpfw_gpu_extract_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, uint64_t *hp)
{
    return extract_pcm16_host(h, pcm, n_samples, n_clips, nullptr, 0, hp);
}

int hpfw_gpu_extract_transposed_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, const int32_t *shifts,
                                           int n_shifts, uint64_t *hp)
{
    if (int rc = check_transposed(h, shifts, n_shifts)) return rc;
    return extract_pcm16_host(h, pcm, n_samples, n_clips, shifts, n_shifts, hp);
}

int hpfw_gpu_tempo_columns(int64_t c, const float *tempos, int n_tempos, int64_t *c_out)
{
    if (int rc = check_tempos(tempos, n_tempos, 0)) return rc;
    if (c < 1 || !c_out) return fail(HPFW_E_INVALID, "bad argument");
    hpfw::TempoList tl{n_tempos, {}};
    for (int i = 0; i < n_tempos; ++i) tl.step[i] = hpfw::tempo_step(tempos[i]);
    *c_out = tempo_common_columns(c, tl);
    return 0;
}

int hpfw_gpu_hashprints_from_db_tempo(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, const float *tempos, int n_tempos,
                                      const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream)
{
    hpfw::TempoList tl;
    int rc = check_tempo_call(h, tempos, n_tempos, shifts, n_shifts, &tl);
    if (rc) return rc;
    if (!d_db || !d_hp || n_clips < 0 || c < 1) return fail(HPFW_E_INVALID, "bad argument");
    const int64_t ct = tempo_common_columns(c, tl);
    if (ct - (hpfw::kCtx - 1) - hpfw::kLag < 1) return fail(HPFW_E_UNSUPPORTED, "clip too short to yield a hashprint at the slowest tempo");
    if (n_clips == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_shifts && (rc = shift_images(h, shifts, n_shifts, s))) return rc;
        const void *images = n_shifts ? h->d_shift_images.get() : h->d_fq_image.get();
        return tempo_back(h, images, n_shifts, d_db, n_clips, c, tl, ct, d_hp, s);
    });
}

int hpfw_gpu_extract_tempo_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, const float *tempos,
                                 int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream)
{
    return extract_tempo_pcm16(h, d_pcm, n_samples, n_clips, tempos, n_tempos, shifts, n_shifts, d_hp, stream);
}

int hpfw_gpu_extract_tempo_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, const float *tempos,
                                      int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *hp)
{
    hpfw::TempoList tl;
    int rc = check_tempo_call(h, tempos, n_tempos, shifts, n_shifts, &tl);
    if (rc) return rc;
    if (!pcm || !hp || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hpfw_geometry g;
    if ((rc = hpfw_gpu_geometry(h, n_samples, &g))) return rc;
    const int64_t nhp = tempo_common_columns(g.c, tl) - (hpfw::kCtx - 1) - hpfw::kLag;
    if (nhp < 1) return fail(HPFW_E_UNSUPPORTED, "clip too short to yield a hashprint at the slowest tempo");
    if (n_clips == 0) return 0;
    return staged_pcm16_host(h, pcm, n_samples, n_clips, (int64_t)tl.n * std::max(n_shifts, 1) * nhp, hp,
                             [&](const int16_t *d_pcm, int64_t cnt, uint64_t *d_hp, hipStream_t st) {
                                 return extract_tempo_pcm16(h, d_pcm, n_samples, cnt, tempos, n_tempos, shifts, n_shifts, d_hp, st);
                             });
}

// ---- windows of one recording ----
// the checks of the variant the arguments select (none, shifts, tempos with or without shifts), as that variant's own entry
// points make them, then the windows; *per_window: hashprints per window
static int check_windows_call(hpfw_gpu *h, int64_t n_total, int64_t win, int64_t hop, const float *tempos, int n_tempos,
                              const int32_t *shifts, int n_shifts, int64_t *n_w, int64_t *per_window)
{
    int rc;
    hpfw::TempoList tl;
    if (tempos || n_tempos) {
        if ((rc = check_tempo_call(h, tempos, n_tempos, shifts, n_shifts, &tl))) return rc;
    } else if (shifts || n_shifts) {
        if ((rc = check_transposed(h, shifts, n_shifts))) return rc;
    } else {
        if (!h) return fail(HPFW_E_INVALID, "null handle");
        if ((rc = check_filters(h))) return rc;
    }
    if ((rc = hpfw_gpu_window_count(n_total, win, hop, n_w))) return rc;
    hpfw_geometry g;
    if ((rc = hpfw_gpu_geometry(h, win, &g))) return rc;
    int64_t nhp = g.n_hp;
    if (tempos) {
        nhp = tempo_common_columns(g.c, tl) - (hpfw::kCtx - 1) - hpfw::kLag;
        if (nhp < 1) return fail(HPFW_E_UNSUPPORTED, "clip too short to yield a hashprint at the slowest tempo");
    }
    *per_window = (int64_t)(tempos ? n_tempos : 1) * std::max(n_shifts, 1) * nhp;
    return 0;
}

int hpfw_gpu_extract_windows_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_total, int64_t win, int64_t hop, const float *tempos,
                                   int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream)
{
    int64_t n_w, per_window;
    int rc = check_windows_call(h, n_total, win, hop, tempos, n_tempos, shifts, n_shifts, &n_w, &per_window);
    if (rc) return rc;
    if (n_w == 0) return 0;
    if (!d_pcm || !d_hp) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    if ((rc = get_plan(h, win, &dp))) return rc;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        // a pass of windows gathered into clips back to back, then the pass through the extraction of clips
        const int nbmax = pass_clips(h, dp, n_w);
        if ((rc = ensure(h->d_windows, (size_t)nbmax * win * 2, h))) return rc;
        int16_t *clips = h->d_windows.as<int16_t>();
        for (int64_t w0 = 0; w0 < n_w; w0 += nbmax) {
            const int64_t nb = std::min<int64_t>(nbmax, n_w - w0);
            hpfw::launch_gather_windows(d_pcm + w0 * hop, hop, win, nb, clips, s);
            if ((rc = check_launch("gather_windows"))) return rc;
            uint64_t *dst = d_hp + w0 * per_window;
            rc = tempos ? extract_tempo_pcm16(h, clips, win, nb, tempos, n_tempos, shifts, n_shifts, dst, s)
                        : extract_pcm16(h, clips, win, nb, shifts, n_shifts, dst, s);
            if (rc) return rc;
        }
        return 0;
    });
}

// host buffers: the recording uploaded once, the hashprints of all windows downloaded, synchronises
int hpfw_gpu_extract_windows_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_total, int64_t win, int64_t hop, const float *tempos,
                                        int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *hp)
{
    int64_t n_w, per_window;
    int rc = check_windows_call(h, n_total, win, hop, tempos, n_tempos, shifts, n_shifts, &n_w, &per_window);
    if (rc) return rc;
    if (n_w == 0) return 0;
    if (!pcm || !hp) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t used = (n_w - 1) * hop + win; // (the samples behind the last window are not needed)
    if ((rc = ensure(h->stage_pcm[0], (size_t)used * 2))) return rc;
    if ((rc = ensure(h->stage_hp, (size_t)n_w * per_window * 8))) return rc;
    HIP_TRY(hipMemcpy(h->stage_pcm[0].get(), pcm, (size_t)used * 2, hipMemcpyHostToDevice));
    if ((rc = hpfw_gpu_extract_windows_pcm16(h, h->stage_pcm[0].as<int16_t>(), used, win, hop, tempos, n_tempos, shifts, n_shifts,
                                             h->stage_hp.as<uint64_t>(), nullptr)))
        return rc;
    HIP_TRY(hipMemcpy(hp, h->stage_hp.get(), (size_t)n_w * per_window * 8, hipMemcpyDeviceToHost)); // (waits for the null stream)
    return 0;
}

#if defined(HPFW_ROWS_SNAP) || defined(HPFW_ROWS_STAMPS)
int hpfw_gpu_debug_set_rows_snap(void *d_snap)
{
    g_rows_snap = static_cast<hpfw::cf *>(d_snap);
    return 0;
}
#endif

int hpfw_gpu_debug_workspace(hpfw_gpu *h, int which, void **d_ptr, size_t *bytes)
{
    if (!h || which < 0 || which >= 7 || !d_ptr || !bytes) return fail(HPFW_E_INVALID, "bad argument");
    *d_ptr = h->ws[which].get();
    *bytes = h->ws[which].capacity();
    return 0;
}

int hpfw_gpu_debug_db_term_sweep(uint32_t first, uint64_t count, uint64_t *out)
{
    if (!out || count > (1ull << 32) - first) return fail(HPFW_E_INVALID, "bad argument");
    DevBuf d;
    HIP_TRY(d.alloc(3 * sizeof(uint64_t)));
    const uint64_t init[3] = {0, 0, ~0ull};
    HIP_TRY(hipMemcpy(d.get(), init, sizeof(init), hipMemcpyHostToDevice));
    hpfw::launch_db_term_sweep(first, count, d.as<unsigned long long>(), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d.get(), sizeof(init), hipMemcpyDeviceToHost)); // (waits for the null stream)
    return 0;
}

// ---- stages ----------------------------------------------------------------------------------
int hpfw_gpu_stage_spectrum(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                            float *d_x, void *stream)
{
    if (!h || !d_pcm || !d_x) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, n_samples, &dp);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int nbmax = pass_clips(h, dp, n_clips);
        if ((rc = ensure_ws(h, dp, nbmax, nbmax))) return rc;
        const int64_t nk = dp->hp.kmax - dp->hp.kmin;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            if ((rc = run_forward(h, dp, d_pcm + c0 * n_samples, nb, h->ws[1].as<hpfw::cf>(), s))) return rc;
            hpfw::launch_gather_bins(dp->cq, h->ws[1].as<hpfw::cf>(), nb, (hpfw::cf *)d_x + c0 * nk, s); // natural order [kmin, kmax)
            if ((rc = check_launch("gather_bins"))) return rc;
        }
        return 0;
    });
}

int hpfw_gpu_stage_cqmag(hpfw_gpu *h, const float *d_x, int64_t n_samples, int64_t n_clips, float *d_mag,
                         void *stream)
{
    if (!h || !d_x || !d_mag) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, n_samples, &dp);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int nbmax = pass_clips(h, dp, n_clips);
        if ((rc = ensure_ws(h, dp, nbmax, nbmax))) return rc;
        const int64_t nk = dp->hp.kmax - dp->hp.kmin;
        hpfw::CqPlanDev cq = dp->cq; // the caller's bins lie in natural order
        cq.xn1 = 1;
        cq.xw = 0;
        cq.xq0 = dp->hp.kmin;
        cq.xclip = nk;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            for (const hpfw::CqClassDev &cd : dp->cls) {
                if (cd.outer)
                    hpfw::launch_cq_big_class(cq, cd, (const hpfw::cf *)d_x + c0 * nk, nb, h->d_cqwork.as<hpfw::cf>(),
                                              d_mag + c0 * 121 * dp->hp.c, h->ws[4].as<float>(), hpfw::kDbNone, s);
                else
                    hpfw::launch_cq_class(cq, cd, (const hpfw::cf *)d_x + c0 * nk, nb,
                                          d_mag + c0 * 121 * dp->hp.c, h->ws[4].as<float>(), hpfw::kDbNone, s);
            }
            if ((rc = check_launch("cq_chirpz"))) return rc;
        }
        return 0;
    });
}

int hpfw_gpu_stage_db(hpfw_gpu *h, const float *d_mag, int64_t n_clips, int64_t c, float *d_db, void *stream)
{
    if (!h || !d_mag || !d_db || c <= 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        int rc;
        const int64_t per = 121 * c;
        const int nbmax = 1024;
        if ((rc = ensure(h->ws[4], (size_t)nbmax * 121 * hpfw::kCqMaxWaves * 4))) return rc;
        if ((rc = ensure(h->d_clipmax, (size_t)nbmax * 4))) return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            hpfw::launch_magmax(d_mag + c0 * per, nb, (int)c, h->ws[4].as<float>(), s);
            hpfw::launch_db(d_mag + c0 * per, h->ws[4].as<float>(), h->d_clipmax.as<float>(), nb, per, d_db + c0 * per, h->db_fast, s);
            if ((rc = check_launch("db"))) return rc;
        }
        return 0;
    });
}

int hpfw_gpu_stage_project(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, float *d_proj,
                           void *stream)
{
    if (!h || !d_db || !d_proj || c < hpfw::kCtx) return fail(HPFW_E_INVALID, "bad argument");
    if (int rc = check_filters(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int64_t nf = c - (hpfw::kCtx - 1);
        for (int64_t c0 = 0; c0 < n_clips; c0 += 16384) {
            const int nb = (int)std::min<int64_t>(16384, n_clips - c0);
            Timed t(h, K_PROJECT, s);
            hpfw::launch_project(h->d_fpack.as<float>(), d_db + c0 * 121 * c, nullptr, nb, (int)c, d_proj + c0 * 64 * nf, s);
        }
        return check_launch("project");
    });
}

int hpfw_gpu_stage_pack(hpfw_gpu *h, const float *d_proj, int64_t n_clips, int64_t n_frames, uint64_t *d_hp,
                        void *stream)
{
    if (!h || !d_proj || !d_hp || n_frames <= hpfw::kLag) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        for (int64_t c0 = 0; c0 < n_clips; c0 += 16384) {
            const int nb = (int)std::min<int64_t>(16384, n_clips - c0);
            hpfw::launch_pack(d_proj + c0 * 64 * n_frames, nb, (int)n_frames, d_hp + c0 * (n_frames - hpfw::kLag), s);
        }
        return check_launch("delta_pack");
    });
}

// Hashprints of one cached dB spectrogram (collect_fingerprints over cache.get_spectros(),
// parallel_collector.h:114-137; file layout utils.h:77-106: Eigen column-major [rows = 121][cols]).
// The caller passes the matrix as stored; it is transposed to the bin-major device layout here.
int hpfw_gpu_extract_db_host(hpfw_gpu *h, const float *s_colmajor, int32_t rows, int32_t cols, uint64_t *hp,
                             int64_t hp_cap, int64_t *n_hp)
{
    if (!h || !s_colmajor || !n_hp) return fail(HPFW_E_INVALID, "null argument");
    if (rows != hpfw::kBins) return fail(HPFW_E_INVALID, "a spectrogram has 121 rows");
    if (int rc = check_filters(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const int64_t nf = (int64_t)cols - (hpfw::kCtx - 1), nh = nf - hpfw::kLag;
    *n_hp = nh > 0 ? nh : 0;
    if (nh <= 0) return 0; // too short: no hashprints (hashprint_handle.h:118: empty fingerprint)
    if (!hp || hp_cap < nh) return fail(HPFW_E_INVALID, "hashprint buffer too small");
    std::vector<float> binmajor((size_t)rows * cols);
    for (int32_t c = 0; c < cols; ++c)
        for (int32_t b = 0; b < rows; ++b) binmajor[(size_t)b * cols + c] = s_colmajor[(size_t)c * rows + b];
    HostTrip t;
    const float *d_s = t.take<float>(binmajor.size() * 4, binmajor.data());
    uint64_t *d_h = t.take<uint64_t>((size_t)nh * 8, nullptr, -1, hp);
    return t.run(false, [&] { return hpfw_gpu_hashprints_from_db(h, d_s, 1, cols, d_h, nullptr); }); // (the blocking copy waits)
}

// ---- sample-rate conversion to 44.1 kHz (k_resample.hip) ------------------------
static int rs_check_rate(int rate)
{
    if (rate < hpfw::kRsRateMin || rate > hpfw::kRsRateMax)
        return fail(HPFW_E_INVALID, "sample rate " + std::to_string(rate) + " Hz outside [8000, 192000]");
    return 0;
}

int hpfw_gpu_resample_length(int64_t n_in, int rate, int64_t *n_out)
{
    if (!n_out || n_in < 0) return fail(HPFW_E_INVALID, "bad argument");
    int rc = rs_check_rate(rate);
    if (rc) return rc;
    int32_t L, M, H;
    (void)hpfw::resample_ratio(rate, &L, &M, &H);
    *n_out = hpfw::resample_out_length(n_in, L, M);
    return 0;
}

int hpfw_gpu_resample_table(int rate, int16_t *taps, int64_t cap, int32_t *L, int32_t *M, int32_t *T)
{
    if (!L || !M || !T) return fail(HPFW_E_INVALID, "bad argument");
    int rc = rs_check_rate(rate);
    if (rc) return rc;
    if (rate == hpfw::kRsRateOut) { // the identity: no filter
        *L = *M = 1;
        *T = 0;
        return 0;
    }
    std::vector<int16_t> t;
    if (!hpfw::resample_design(rate, t, L, M, T)) return fail(HPFW_E_INVALID, "resampling table out of range");
    if (!taps) return 0;
    if (cap < (int64_t)t.size()) return fail(HPFW_E_INVALID, "buffer smaller than the table");
    std::copy(t.begin(), t.end(), taps);
    return 0;
}

} // extern "C"

int rs_table(hpfw_gpu *h, int rate, hpfw_gpu::Resample::Table **out)
{
    hpfw_gpu::Resample::Table &t = h->rs.tables[rate];
    if (!t.d_taps) { // once per rate (published only when complete)
        std::vector<int16_t> taps;
        int32_t L, M, T;
        if (!hpfw::resample_design(rate, taps, &L, &M, &T)) return fail(HPFW_E_INVALID, "resampling table out of range");
        const std::vector<int32_t> img = hpfw::resample_device_table(taps, L, T);
        DevBuf d;
        HIP_TRY(d.alloc(img.size() * 4));
        HIP_TRY(hipMemcpy(d.get(), img.data(), img.size() * 4, hipMemcpyHostToDevice));
        t.L = L;
        t.M = M;
        t.T = T;
        t.d_taps = std::move(d);
    }
    *out = &t;
    return 0;
}

extern "C" {

int hpfw_gpu_resample_pcm16(hpfw_gpu *h, const int16_t *d_in, int64_t n_in, int64_t n_clips, int rate, int16_t *d_out, void *stream)
{
    if (!h || n_in < 0 || n_clips < 0 || ((!d_in || !d_out) && n_in > 0 && n_clips > 0)) return fail(HPFW_E_INVALID, "bad argument");
    int rc = rs_check_rate(rate);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hpfw_gpu::Resample::Table *tab = nullptr;
    if (rate != hpfw::kRsRateOut && (rc = rs_table(h, rate, &tab))) return rc;
    if (n_in == 0 || n_clips == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (!tab) { // 44.1 kHz: a plain copy
            HIP_TRY(hipMemcpyAsync(d_out, d_in, (size_t)n_clips * n_in * 2, hipMemcpyDeviceToDevice, s));
            return 0;
        }
        if (!hpfw::launch_resample(d_in, n_in, n_clips, tab->L, tab->M, tab->T, tab->d_taps.as<int32_t>(), d_out, s))
            return fail(HPFW_E_INVALID, "resampling: the table and its input span exceed the LDS");
        return check_launch("resample");
    });
}

int hpfw_gpu_resample_pcm16_host(hpfw_gpu *h, const int16_t *in, int64_t n_in, int64_t n_clips, int rate, int16_t *out)
{
    if (!h || n_in < 0 || n_clips < 0 || ((!in || !out) && n_in > 0 && n_clips > 0)) return fail(HPFW_E_INVALID, "bad argument");
    int64_t n_out = 0;
    int rc = hpfw_gpu_resample_length(n_in, rate, &n_out);
    if (rc) return rc;
    if (n_in == 0 || n_clips == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = ensure(h->rs.in, (size_t)n_clips * n_in * 2, h)) || (rc = ensure(h->rs.out, (size_t)n_clips * n_out * 2, h))) return rc;
    HIP_TRY(hipMemcpy(h->rs.in.get(), in, (size_t)n_clips * n_in * 2, hipMemcpyHostToDevice));
    if ((rc = hpfw_gpu_resample_pcm16(h, h->rs.in.as<int16_t>(), n_in, n_clips, rate, h->rs.out.as<int16_t>(), nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out, h->rs.out.get(), (size_t)n_clips * n_out * 2, hipMemcpyDeviceToHost));
    return 0;
}

int hpfw_gpu_stage_spectrogram(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, float *d_db,
                               void *stream)
{
    if (!h || !d_pcm || !d_db || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, n_samples, &dp);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int nbmax = pass_clips(h, dp, n_clips);
        if ((rc = ensure_ws(h, dp, nbmax, nbmax))) return rc;
        const size_t per = (size_t)121 * dp->hp.c;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            if ((rc = run_front(h, dp, d_pcm + c0 * n_samples, nb, 0, true, s))) return rc;
            HIP_TRY(hipMemcpyAsync(d_db + c0 * per, h->ws[2].get(), (size_t)nb * per * 4, hipMemcpyDeviceToDevice, s));
        }
        return 0;
    });
}

} // extern "C"
