// combiner.hip -- AudioCombiner on the C-ABI: the exact-hash index and its offset votes (k_combiner.hip), the exact
// cross-correlation of PCM16 (k_xcorr.hip) and the Mel front end's kept frames.
#include "handle.h"

extern "C" {

// ---- AudioCombiner: exact-hash index + offset votes (k_combiner.hip) --------------------------------
static hpfw::Combiner *combiner_of(hpfw_gpu *h)
{
    if (!h->combiner) h->combiner.reset(new hpfw::Combiner());
    return h->combiner.get();
}

int hpfw_gpu_combiner_clear(hpfw_gpu *h)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    combiner_of(h)->clear();
    return 0;
}

static int combiner_add_impl(hpfw_gpu *h, const uint16_t *hp, const int64_t *offsets, int64_t n_rec, bool dev, hipStream_t s)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        std::string why;
        const int rc = combiner_of(h)->add(hp, dev, offsets, n_rec, s, why);
        return rc ? fail(rc, why) : 0;
    });
}

int hpfw_gpu_combiner_add(hpfw_gpu *h, const uint16_t *hp, const int64_t *offsets, int64_t n_rec)
{
    return combiner_add_impl(h, hp, offsets, n_rec, false, nullptr);
}

int hpfw_gpu_combiner_add_device(hpfw_gpu *h, const uint16_t *d_hp, const int64_t *offsets, int64_t n_rec, void *stream)
{
    return combiner_add_impl(h, d_hp, offsets, n_rec, true, (hipStream_t)stream);
}

int64_t hpfw_gpu_combiner_size(hpfw_gpu *h) { return h && h->combiner ? h->combiner->size() : 0; }

int hpfw_gpu_combiner_get(hpfw_gpu *h, int64_t *val_start, uint32_t *rec, uint32_t *off, int64_t cap)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    std::string why;
    const int rc = combiner_of(h)->get(val_start, rec, off, cap, why);
    return rc ? fail(rc, why) : 0;
}

static int combiner_search_device(hpfw_gpu *h, const uint16_t *d_q, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                  hpfw_combine_result *d_find, int k, hpfw_align_hit *d_align, hipStream_t s)
{
    if (!h || !q_off || n_q < 0 || (!d_find && !d_align)) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        std::string why;
        const int rc = combiner_of(h)->search(d_q, q_off, exclude, n_q, d_find, k, d_align, s, why);
        return rc ? fail(rc, why) : 0;
    });
}

// host buffers: queries in, results out, synchronises
static int combiner_search_host(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                hpfw_combine_result *find_out, int k, hpfw_align_hit *align_out)
{
    if (!h || !q_off || n_q < 0 || (!find_out && !align_out)) return fail(HPFW_E_INVALID, "bad argument");
    if (align_out && (k < 1 || k > 64)) return fail(HPFW_E_INVALID, "k must be in 1..64");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    if (find_out)
        return search_round_trip(q_hp, q_off, n_q, n_q, find_out, [&](const uint16_t *d_q, const int64_t *rel, hpfw_combine_result *d_out) {
            return combiner_search_device(h, d_q, rel, exclude, n_q, d_out, k, nullptr, nullptr);
        });
    return search_round_trip(q_hp, q_off, n_q, n_q * k, align_out, [&](const uint16_t *d_q, const int64_t *rel, hpfw_align_hit *d_out) {
        return combiner_search_device(h, d_q, rel, exclude, n_q, nullptr, k, d_out, nullptr);
    });
}

int hpfw_gpu_combiner_find_device(hpfw_gpu *h, const uint16_t *d_q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                  hpfw_combine_result *d_out, void *stream)
{
    if (!d_out) return fail(HPFW_E_INVALID, "null output");
    return combiner_search_device(h, d_q_hp, q_off, exclude, n_q, d_out, 0, nullptr, (hipStream_t)stream);
}

int hpfw_gpu_combiner_find(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                           hpfw_combine_result *out)
{
    if (!out) return fail(HPFW_E_INVALID, "null output");
    return combiner_search_host(h, q_hp, q_off, exclude, n_q, out, 0, nullptr);
}

int hpfw_gpu_combiner_align_device(hpfw_gpu *h, const uint16_t *d_q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                   int k, hpfw_align_hit *d_out, void *stream)
{
    if (!d_out || k < 1 || k > 64) return fail(HPFW_E_INVALID, "null output or k outside 1..64");
    return combiner_search_device(h, d_q_hp, q_off, exclude, n_q, nullptr, k, d_out, (hipStream_t)stream);
}

int hpfw_gpu_combiner_align(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q, int k,
                            hpfw_align_hit *out)
{
    if (!out) return fail(HPFW_E_INVALID, "null output");
    return combiner_search_host(h, q_hp, q_off, exclude, n_q, nullptr, k, out);
}

// ---- sample-accurate offsets: exact cross-correlation of PCM16 (k_xcorr.hip), the Mel front end's kept frames ----
// n_pcm < 0: the buffer's size is not known (the device entry point)
static int xcorr_device(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *d_r,
                        hpfw_xcorr_peak *d_peaks, hipStream_t s)
{
    if (!h || n_jobs < 0 || (n_jobs > 0 && (!d_pcm || !jobs || !d_peaks))) return fail(HPFW_E_INVALID, "xcorr: null argument");
    for (int64_t i = 0; i < n_jobs; ++i)
        if (const char *why = hpfw::xcorr_check(jobs[i], n_pcm)) return fail(HPFW_E_INVALID, std::string(why) + " (job " + std::to_string(i) + ")");
    HIP_TRY(hipSetDevice(h->device));
    if (n_jobs == 0) return 0;
    const char *mode = std::getenv("HPFW_XCORR");
    const bool valu_only = mode && !std::strcmp(mode, "valu");
    return ordered_call(h, s, [&] {
        // passes of jobs: the parts and (when the caller keeps no r) the lags of a pass are bounded
        constexpr int64_t kMaxItems = (int64_t)1 << 20, kMaxLags = (int64_t)1 << 24;
        std::vector<hpfw::XcJob> tab;
        std::vector<hpfw::XcItem> mfma, valu;
        int64_t r_done = 0; // lags of the passes before this one
        for (int64_t j0 = 0; j0 < n_jobs;) {
            tab.clear();
            mfma.clear();
            valu.clear();
            int64_t j1 = j0, lags = 0;
            for (; j1 < n_jobs && (j1 == j0 || ((int64_t)(mfma.size() + valu.size()) < kMaxItems && lags < kMaxLags)); ++j1) {
                tab.push_back(hpfw::xcorr_plan_job(jobs[j1], (int32_t)(j1 - j0), (d_r ? r_done : 0) + lags, valu_only, mfma, valu));
                lags += hpfw::xcorr_lags(jobs[j1]);
            }
            const size_t jb = tab.size() * sizeof(hpfw::XcJob), mb = mfma.size() * sizeof(hpfw::XcItem), vb = valu.size() * sizeof(hpfw::XcItem);
            if (j0 > 0) HIP_TRY(hipStreamSynchronize(s)); // the pass before this one still reads the tables
            if (int rc = ensure(h->xcorr.d_tab, jb + mb + vb)) return rc;
            if (!d_r)
                if (int rc = ensure(h->xcorr.d_r, (size_t)lags * 8)) return rc;
            char *d_tab = h->xcorr.d_tab.as<char>();
            HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), jb, hipMemcpyHostToDevice, s));
            if (mb) HIP_TRY(hipMemcpyAsync(d_tab + jb, mfma.data(), mb, hipMemcpyHostToDevice, s));
            if (vb) HIP_TRY(hipMemcpyAsync(d_tab + jb + mb, valu.data(), vb, hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s)); // (the host vectors are reused or die)
            hpfw::launch_xcorr(d_pcm, (const hpfw::XcJob *)d_tab, j1 - j0, (const hpfw::XcItem *)(d_tab + jb), (int64_t)mfma.size(),
                               (const hpfw::XcItem *)(d_tab + jb + mb), (int64_t)valu.size(), d_r ? d_r : h->xcorr.d_r.as<int64_t>(),
                               d_peaks + j0, s);
            if (int rc = check_launch("xcorr")) return rc;
            r_done += lags;
            j0 = j1;
        }
        return 0;
    });
}

int hpfw_gpu_xcorr_pcm16(hpfw_gpu *h, const int16_t *d_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *d_r,
                         hpfw_xcorr_peak *d_peaks, void *stream)
{
    return xcorr_device(h, d_pcm, -1, jobs, n_jobs, d_r, d_peaks, (hipStream_t)stream);
}

int hpfw_gpu_xcorr_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *r,
                              hpfw_xcorr_peak *peaks)
{
    if (!h || n_jobs < 0 || n_pcm < 0 || (n_jobs > 0 && (!pcm || !jobs || !peaks))) return fail(HPFW_E_INVALID, "xcorr: null argument");
    int64_t lags = 0;
    for (int64_t i = 0; i < n_jobs; ++i) { // (before anything is allocated; the device entry point checks again)
        if (const char *why = hpfw::xcorr_check(jobs[i], n_pcm)) return fail(HPFW_E_INVALID, std::string(why) + " (job " + std::to_string(i) + ")");
        lags += hpfw::xcorr_lags(jobs[i]);
    }
    HIP_TRY(hipSetDevice(h->device));
    if (n_jobs == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)std::max<int64_t>(n_pcm, 1) * 2, n_pcm ? pcm : nullptr);
    int64_t *d_r = r ? t.take<int64_t>((size_t)lags * 8, nullptr, -1, r) : nullptr;
    hpfw_xcorr_peak *d_peaks = t.take<hpfw_xcorr_peak>((size_t)n_jobs * sizeof(hpfw_xcorr_peak), nullptr, -1, peaks);
    return t.run(true, [&] { return xcorr_device(h, d_pcm, n_pcm, jobs, n_jobs, d_r, d_peaks, nullptr); });
}

int hpfw_gpu_mel_kept_frames_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, int32_t *frames,
                                        int64_t stride, int32_t *n_kept)
{
    if (!h || !pcm || !frames || !n_kept || n_clips < 0 || n_samples < 1) return fail(HPFW_E_INVALID, "bad argument");
    const int64_t nf = hpfw::mel_frames(n_samples), n_blk = (n_samples + hpfw::kMelHop - 1) / hpfw::kMelHop;
    if (stride < nf) return fail(HPFW_E_INVALID, "stride smaller than hpfw_gpu_mel_frames(n_samples)");
    if (n_clips > 65535) return fail(HPFW_E_INVALID, "more than 65535 clips in one call");
    HIP_TRY(hipSetDevice(h->device));
    if (n_clips == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)n_clips * n_samples * 2, pcm);
    int64_t *d_blk = t.take<int64_t>((size_t)n_clips * n_blk * 8);
    int *d_pos = t.take<int>((size_t)n_clips * nf * 4);
    int32_t *d_frames = t.take<int32_t>((size_t)n_clips * stride * 4, nullptr, -1, frames);
    int32_t *d_count = t.take<int32_t>((size_t)n_clips * 4, nullptr, -1, n_kept);
    return t.run(true, [&] {
        return ordered_call(h, nullptr, [&] {
            hpfw::launch_mel_kept_frames(d_pcm, n_samples, (int)n_clips, d_blk, d_pos, d_count, d_frames, stride, nullptr);
            return check_launch("mel kept frames");
        });
    });
}

} // extern "C"
