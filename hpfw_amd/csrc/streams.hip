// streams.hip -- live feeds (include/hpfw_gpu.h): the rings' bookkeeping on the host, the push of chunks
// into them and the extraction of the windows that have become complete.  The samples move in k_streams.hip, those of feeds at
// another rate than 44.1 kHz through k_streams_resample.hip (the planning of a push: streams_plan.cpp); the gathered windows of
// a pass go through the extraction of clips as the windows of a recording do (extract.hip).
#include "handle.h"

struct hpfw_gpu_streams {
    hpfw_gpu *h = nullptr;
    int n_streams = 0;
    int64_t win = 0, hop = 0, capacity = 0, per_window = 0;
    std::vector<float> tempos;
    std::vector<int32_t> shifts;
    std::vector<hpfw::RingFeed> feeds; // per feed its rate, n_i, e_i and which of its two histories is current
    DevBuf slab;                       // [n_streams][capacity] int16
    // feeds at another rate than 44.1 kHz: per feed two buffers of T - 1 input samples, the current one holding the samples in
    // front of the next chunk; a push reads it and writes the other (k_streams_resample.hip).  The tables live on the handle
    DevBuf hist;
    std::map<int, hpfw_gpu::Resample::Table *> tables;
    // One table per call goes to the device from pinned memory behind the call's other work: the runs of a push (with the
    // chunks behind them in the host form: one upload), the windows of an extraction.  table_ev marks the end of the copy
    // that last read the pinned buffer; the next call waits for it before it writes there.
    HostBuf pin;
    DevBuf d_stage;
    Event table_ev;
    bool table_pending = false;
    DevBuf host_clips; // the clips of the host form of the extraction
};

namespace {

int64_t windows_of(int64_t n, int64_t win, int64_t hop) { return n < win ? 0 : (n - win) / hop + 1; }

int64_t emitted(const hpfw::RingFeed &f) { return hpfw::ring_emitted(f.n, f.L, f.M, f.H); }

int64_t ready_windows(const hpfw_gpu_streams *s)
{
    int64_t n = 0;
    for (const hpfw::RingFeed &f : s->feeds) n += windows_of(emitted(f), s->win, s->hop) - f.e;
    return n;
}

// pinned and device staging of at least `bytes`, free to be written: the copy that last read the pinned buffer has ended
int stage(hpfw_gpu_streams *s, size_t bytes)
{
    if (s->table_pending) {
        HIP_TRY(hipEventSynchronize(s->table_ev.get()));
        s->table_pending = false;
    }
    if (s->pin.capacity() < bytes && s->pin.alloc(bytes + bytes / 2) != hipSuccess) return fail(HPFW_E_NOMEM, "hipHostMalloc failed");
    return ensure(s->d_stage, bytes + bytes / 2);
}

// the first `bytes` of the pinned buffer to the device staging on stream st
int upload(hpfw_gpu_streams *s, size_t bytes, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(s->d_stage.get(), s->pin.get(), bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->table_ev.get(), st));
    s->table_pending = true;
    return 0;
}

// pcm: the chunks concatenated, in host memory (host = true: they travel behind the table) or on the device
int push(hpfw_gpu_streams *s, const int16_t *pcm, bool host, const int64_t *counts, int64_t *n_ready, hipStream_t st)
{
    if (!s || !counts) return fail(HPFW_E_INVALID, "null argument");
    for (int i = 0; i < s->n_streams; ++i)
        if (counts[i] < 0) return fail(HPFW_E_INVALID, "streams: counts must not be negative");
    // the plan of the push (streams_plan.cpp): the runs of the 44.1 kHz feeds, and per other rate the runs of its feeds
    hpfw::RingPushPlan plan;
    const int bad = hpfw::ring_plan_push(s->feeds, counts, s->hop, s->capacity, &plan);
    if (bad >= 0)
        return fail(HPFW_E_INVALID, "streams: the chunk of feed " + std::to_string(bad) + " does not fit its ring (" + std::to_string(counts[bad]) +
                                        " samples, room for " + std::to_string(hpfw::ring_room(s->feeds[(size_t)bad], s->hop, s->capacity)) + ")");
    const int64_t total = plan.total;
    if (total && !pcm) return fail(HPFW_E_INVALID, "null argument");
    if (total) {
        hpfw_gpu *h = s->h;
        HIP_TRY(hipSetDevice(h->device));
        // the tables of both kinds of run, then the chunks (16-byte aligned) in the host form
        const size_t copy_bytes = (plan.copy.size() * sizeof(hpfw::RingRun) + 15) & ~(size_t)15;
        const size_t tab = copy_bytes + ((plan.rs.size() * sizeof(hpfw::RingRsRun) + 15) & ~(size_t)15), bytes = tab + (host ? (size_t)total * 2 : 0);
        if (int rc = stage(s, bytes)) return rc;
        std::memcpy(s->pin.get(), plan.copy.data(), plan.copy.size() * sizeof(hpfw::RingRun));
        std::memcpy(s->pin.as<char>() + copy_bytes, plan.rs.data(), plan.rs.size() * sizeof(hpfw::RingRsRun));
        if (host) std::memcpy(s->pin.as<char>() + tab, pcm, (size_t)total * 2);
        const int16_t *d_src = host ? reinterpret_cast<const int16_t *>(s->d_stage.as<char>() + tab) : pcm;
        const hpfw::RingRsRun *d_rs = reinterpret_cast<const hpfw::RingRsRun *>(s->d_stage.as<char>() + copy_bytes);
        int rc = ordered_call(h, st, [&] {
            if (int e = upload(s, bytes, st)) return e;
            hpfw::launch_ring_append(s->d_stage.as<hpfw::RingRun>(), (int)plan.copy.size(), plan.copy_longest, d_src, s->slab.as<int16_t>(), st);
            if (int e = check_launch("ring_append")) return e;
            for (const hpfw::RingPushPlan::Group &g : plan.groups) {
                const hpfw_gpu::Resample::Table *t = s->tables.at(g.rate);
                if (!hpfw::launch_ring_resample_append(d_rs + g.first, g.n, g.most, d_src, s->slab.as<int16_t>(), s->hist.as<int16_t>(), t->L, t->M,
                                                       t->T, t->d_taps.as<int32_t>(), st))
                    return fail(HPFW_E_INVALID, "resampling: the table and its input span exceed the LDS");
                if (int e = check_launch("ring_resample_append")) return e;
            }
            return 0;
        });
        if (rc) return rc; // (no feed has advanced: what the launches wrote lies behind the rings' ends and in the histories not in use)
        for (int i = 0; i < s->n_streams; ++i) {
            hpfw::RingFeed &f = s->feeds[(size_t)i];
            if (counts[i] && f.H) f.cur ^= 1;
            f.n += counts[i];
        }
    }
    if (n_ready) *n_ready = ready_windows(s);
    return 0;
}

} // namespace

extern "C" {

int hpfw_gpu_streams_create(hpfw_gpu *h, const hpfw_streams_params *p, hpfw_gpu_streams **out)
{
    return hpfw_gpu_streams_create_rates(h, p, nullptr, out);
}

int hpfw_gpu_streams_create_rates(hpfw_gpu *h, const hpfw_streams_params *p, const int32_t *rates, hpfw_gpu_streams **out)
{
    if (!p || !out) return fail(HPFW_E_INVALID, "null argument");
    if (p->n_streams < 1 || p->n_streams > 4096) return fail(HPFW_E_INVALID, "streams: n_streams must be 1 to 4096");
    for (int i = 0; rates && i < p->n_streams; ++i)
        if (rates[i] < hpfw::kRsRateMin || rates[i] > hpfw::kRsRateMax)
            return fail(HPFW_E_UNSUPPORTED, "streams: the sample rate of feed " + std::to_string(i) + ", " + std::to_string(rates[i]) +
                                                " Hz, is outside [8000, 192000]");
    int64_t none;
    int rc = hpfw_gpu_window_count(0, p->win, p->hop, &none);
    if (rc) return rc;
    const int64_t capacity = p->capacity ? p->capacity : 2 * p->win;
    if (capacity < p->win) return fail(HPFW_E_INVALID, "streams: capacity must be at least win (0: 2 win)");
    // the checks of the windows of a recording, with their messages: the lists, the handle, projection mode 1 for variants,
    // the filters, a window too short for the slowest tempo (a recording of no sample has no window: nothing runs)
    if ((rc = hpfw_gpu_extract_windows_pcm16_host(h, nullptr, 0, p->win, p->hop, p->tempos, p->n_tempos, p->shifts, p->n_shifts, nullptr)))
        return rc;
    hpfw_geometry g;
    if ((rc = hpfw_gpu_geometry(h, p->win, &g))) return rc;
    int64_t nhp = g.n_hp;
    if (p->tempos) {
        int64_t ct;
        if ((rc = hpfw_gpu_tempo_columns(g.c, p->tempos, p->n_tempos, &ct))) return rc;
        nhp = ct - (hpfw::kCtx - 1) - hpfw::kLag;
    }
    if (nhp < 1) return fail(HPFW_E_UNSUPPORTED, "clip too short to yield a hashprint");
    auto s = std::make_unique<hpfw_gpu_streams>();
    s->h = h;
    s->n_streams = p->n_streams;
    s->win = p->win;
    s->hop = p->hop;
    s->capacity = capacity;
    if (p->tempos) s->tempos.assign(p->tempos, p->tempos + p->n_tempos);
    if (p->shifts) s->shifts.assign(p->shifts, p->shifts + p->n_shifts);
    s->per_window = (int64_t)std::max<size_t>(s->tempos.size(), 1) * (int64_t)std::max<size_t>(s->shifts.size(), 1) * nhp;
    s->feeds.assign((size_t)p->n_streams, hpfw::RingFeed());
    int64_t hist_total = 0;
    for (int i = 0; rates && i < p->n_streams; ++i) {
        hpfw::RingFeed &f = s->feeds[(size_t)i];
        if (rates[i] == hpfw::kRsRateOut) continue;
        f.rate = rates[i];
        (void)hpfw::resample_ratio(f.rate, &f.L, &f.M, &f.H);
        f.hist = hist_total;
        f.hist_len = (2 * (int64_t)f.H - 1 + 7) & ~(int64_t)7;
        hist_total += 2 * f.hist_len;
    }
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    if ((rc = get_plan(h, p->win, &dp))) return rc; // (the tables of win now: the first push is not the slow one)
    for (const hpfw::RingFeed &f : s->feeds) // ... and those of every other rate
        if (f.H && !s->tables.count(f.rate) && (rc = rs_table(h, f.rate, &s->tables[f.rate]))) return rc;
    if (hist_total && s->hist.alloc((size_t)hist_total * 2) != hipSuccess) return fail(HPFW_E_NOMEM, "hipMalloc failed");
    if (s->slab.alloc((size_t)p->n_streams * (size_t)capacity * 2) != hipSuccess) return fail(HPFW_E_NOMEM, "hipMalloc failed");
    HIP_TRY(s->table_ev.create());
    *out = s.release();
    return 0;
}

void hpfw_gpu_streams_destroy(hpfw_gpu_streams *s)
{
    if (!s) return;
    if (s->table_pending) (void)hipEventSynchronize(s->table_ev.get());
    // the rings may still be read by work in flight: wait for the handle's last call before they are freed
    if (s->h->order == hpfw_gpu::kOrderEvent) (void)hipEventSynchronize(s->h->order_ev.get());
    else if (s->h->order == hpfw_gpu::kOrderSync) (void)hipStreamSynchronize(s->h->order_stream);
    delete s;
}

int hpfw_gpu_streams_push(hpfw_gpu_streams *s, const int16_t *pcm, const int64_t *counts, int64_t *n_ready)
{
    return push(s, pcm, true, counts, n_ready, nullptr);
}

int hpfw_gpu_streams_push_device(hpfw_gpu_streams *s, const int16_t *d_pcm, const int64_t *counts, int64_t *n_ready, void *stream)
{
    return push(s, d_pcm, false, counts, n_ready, (hipStream_t)stream);
}

int hpfw_gpu_streams_room(hpfw_gpu_streams *s, int64_t *room)
{
    if (!s || !room) return fail(HPFW_E_INVALID, "null argument");
    for (int i = 0; i < s->n_streams; ++i) room[i] = hpfw::ring_room(s->feeds[(size_t)i], s->hop, s->capacity);
    return 0;
}

int hpfw_gpu_streams_extract(hpfw_gpu_streams *s, int64_t cap, uint64_t *d_hp, int16_t *d_clips, hpfw_stream_window *which, int64_t *n,
                             void *stream)
{
    if (!s || !n || cap < 0) return fail(HPFW_E_INVALID, "bad argument");
    *n = 0;
    // the windows of this call, in order of (feed, window)
    std::vector<hpfw_stream_window> take;
    for (int i = 0; i < s->n_streams && (int64_t)take.size() < cap; ++i) {
        const int64_t have = windows_of(emitted(s->feeds[(size_t)i]), s->win, s->hop);
        for (int64_t w = s->feeds[(size_t)i].e; w < have && (int64_t)take.size() < cap; ++w) take.push_back({i, 0, w});
    }
    const int64_t n_w = (int64_t)take.size();
    if (n_w == 0) return 0;
    if (!d_hp || !which) return fail(HPFW_E_INVALID, "bad argument");
    hpfw_gpu *h = s->h;
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, s->win, &dp);
    if (rc) return rc;
    const size_t bytes = (size_t)n_w * sizeof(hpfw::RingWindow);
    if ((rc = stage(s, bytes))) return rc;
    hpfw::RingWindow *tab = s->pin.as<hpfw::RingWindow>();
    for (int64_t j = 0; j < n_w; ++j)
        tab[j] = {(int64_t)take[(size_t)j].feed * s->capacity, (int64_t)((__int128)take[(size_t)j].window * s->hop % s->capacity)};
    hipStream_t st = (hipStream_t)stream;
    const float *tempos = s->tempos.empty() ? nullptr : s->tempos.data();
    const int32_t *shifts = s->shifts.empty() ? nullptr : s->shifts.data();
    const int n_tempos = (int)s->tempos.size(), n_shifts = (int)s->shifts.size();
    rc = ordered_call(h, st, [&] {
        int e;
        if ((e = upload(s, bytes, st))) return e;
        // a pass of windows gathered into clips back to back, then the pass through the extraction of clips
        const int nbmax = pass_clips(h, dp, n_w);
        if ((e = ensure(h->d_windows, (size_t)nbmax * s->win * 2, h))) return e;
        int16_t *clips = h->d_windows.as<int16_t>();
        for (int64_t w0 = 0; w0 < n_w; w0 += nbmax) {
            const int64_t nb = std::min<int64_t>(nbmax, n_w - w0);
            hpfw::launch_ring_gather_windows(s->slab.as<int16_t>(), s->d_stage.as<hpfw::RingWindow>() + w0, s->capacity, s->win, nb, clips, st);
            if ((e = check_launch("ring_gather_windows"))) return e;
            if (d_clips) HIP_TRY(hipMemcpyAsync(d_clips + w0 * s->win, clips, (size_t)nb * s->win * 2, hipMemcpyDeviceToDevice, st));
            uint64_t *dst = d_hp + w0 * s->per_window;
            e = tempos   ? hpfw_gpu_extract_tempo_pcm16(h, clips, s->win, nb, tempos, n_tempos, shifts, n_shifts, dst, st)
                : shifts ? hpfw_gpu_extract_transposed_pcm16(h, clips, s->win, nb, shifts, n_shifts, dst, st)
                         : hpfw_gpu_extract_pcm16(h, clips, s->win, nb, dst, st);
            if (e) return e;
        }
        return 0;
    });
    if (rc) return rc; // (nothing was handed out: the windows stay ready)
    for (const hpfw_stream_window &w : take) s->feeds[(size_t)w.feed].e = w.window + 1;
    std::copy(take.begin(), take.end(), which);
    *n = n_w;
    return 0;
}

int hpfw_gpu_streams_extract_host(hpfw_gpu_streams *s, int64_t cap, uint64_t *hp, int16_t *clips, hpfw_stream_window *which, int64_t *n)
{
    if (!s || !n || cap < 0) return fail(HPFW_E_INVALID, "bad argument");
    const int64_t n_w = std::min(cap, ready_windows(s));
    *n = 0;
    if (n_w == 0) return 0;
    if (!hp || !which) return fail(HPFW_E_INVALID, "bad argument");
    hpfw_gpu *h = s->h;
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h->stage_hp, (size_t)n_w * s->per_window * 8))) return rc;
    if (clips && (rc = ensure(s->host_clips, (size_t)n_w * s->win * 2))) return rc;
    if ((rc = hpfw_gpu_streams_extract(s, n_w, h->stage_hp.as<uint64_t>(), clips ? s->host_clips.as<int16_t>() : nullptr, which, n, nullptr)))
        return rc;
    HIP_TRY(hipMemcpy(hp, h->stage_hp.get(), (size_t)n_w * s->per_window * 8, hipMemcpyDeviceToHost)); // (waits for the null stream)
    if (clips) HIP_TRY(hipMemcpy(clips, s->host_clips.get(), (size_t)n_w * s->win * 2, hipMemcpyDeviceToHost));
    return 0;
}

int hpfw_gpu_streams_reset(hpfw_gpu_streams *s, int stream)
{
    if (!s) return fail(HPFW_E_INVALID, "null argument");
    if (stream < 0 || stream >= s->n_streams) return fail(HPFW_E_INVALID, "streams: no such feed");
    // (host bookkeeping only: what the ring holds is never read before it has been written again, and of the history of a feed
    // at another rate only inputs at or behind the feed's first are read: none)
    s->feeds[(size_t)stream].n = s->feeds[(size_t)stream].e = 0;
    return 0;
}

int hpfw_gpu_streams_info(hpfw_gpu_streams *s, hpfw_streams_info *info, int64_t *received, int64_t *extracted)
{
    if (!s) return fail(HPFW_E_INVALID, "null argument");
    if (info)
        *info = {s->per_window, s->win, s->hop, s->capacity, s->n_streams,
                 (int32_t)(std::max<size_t>(s->tempos.size(), 1) * std::max<size_t>(s->shifts.size(), 1))};
    for (int i = 0; i < s->n_streams; ++i) {
        if (received) received[i] = s->feeds[(size_t)i].n;
        if (extracted) extracted[i] = s->feeds[(size_t)i].e;
    }
    return 0;
}

int hpfw_gpu_streams_rates(hpfw_gpu_streams *s, int32_t *rates, int64_t *n_emitted)
{
    if (!s) return fail(HPFW_E_INVALID, "null argument");
    for (int i = 0; i < s->n_streams; ++i) {
        if (rates) rates[i] = s->feeds[(size_t)i].rate;
        if (n_emitted) n_emitted[i] = emitted(s->feeds[(size_t)i]);
    }
    return 0;
}

int hpfw_gpu_streams_emitted(int64_t n_in, int rate, int64_t *n_out)
{
    if (!n_out || n_in < 0) return fail(HPFW_E_INVALID, "bad argument");
    int32_t L = 1, M = 1, H = 0;
    if (!hpfw::resample_ratio(rate, &L, &M, &H)) return fail(HPFW_E_INVALID, "sample rate " + std::to_string(rate) + " Hz outside [8000, 192000]");
    *n_out = rate == hpfw::kRsRateOut ? n_in : hpfw::ring_emitted(n_in, L, M, H);
    return 0;
}

} // extern "C"
