// warp.hip -- the entry points of clock drift and rendering: the time warp and the fused mix
// (k_warp.hip), and the host-only logic Python and C++ share (drift_plan.h: anchors, the Theil-Sen line, the time map).
#include "drift_plan.h"
#include "handle.h"

namespace {

// the device image of the table, made and cached on first use; the device is set
int warp_table(hpfw_gpu *h)
{
    if (h->warp.d_taps) return 0;
    std::vector<int16_t> taps;
    if (!hpfw::warp_design(taps)) return fail(HPFW_E_INVALID, "warp table out of range");
    const std::vector<int32_t> img = hpfw::resample_device_table(taps, hpfw::kWarpP, hpfw::kWarpT);
    DevBuf d;
    HIP_TRY(d.alloc(img.size() * 4));
    HIP_TRY(hipMemcpy(d.get(), img.data(), img.size() * 4, hipMemcpyHostToDevice));
    h->warp.d_taps = std::move(d); // (published only when complete)
    return 0;
}

int warp_check_call(hpfw_gpu *h, const void *pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0, int64_t n_out,
                    const void *out, bool mix)
{
    if (!h || n_pcm < 0 || n_tracks < 0 || (n_tracks > 0 && !tracks)) return fail(HPFW_E_INVALID, "warp: null or negative argument");
    if (m0 < 0 || n_out < 0 || m0 > hpfw::kWarpMEnd || n_out > hpfw::kWarpMEnd - m0) return fail(HPFW_E_INVALID, "warp: outputs outside 0 .. 2^31");
    if (n_tracks > INT32_MAX) return fail(HPFW_E_INVALID, "warp: more than 2^31 - 1 tracks");
    for (int64_t i = 0; i < n_tracks; ++i)
        if (const char *why = hpfw::warp_check(tracks[i], n_pcm)) return fail(HPFW_E_INVALID, std::string(why) + " (track " + std::to_string(i) + ")");
    if (n_out > 0 && (mix || n_tracks > 0) && !out) return fail(HPFW_E_INVALID, "warp: null output");
    if (n_pcm > 0 && !pcm) return fail(HPFW_E_INVALID, "warp: null pcm");
    return 0;
}

int warp_device(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0, int64_t n_out,
                bool mix, int16_t *d_out, hipStream_t s)
{
    if (int rc = warp_check_call(h, d_pcm, n_pcm, tracks, n_tracks, m0, n_out, d_out, mix)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = warp_table(h)) return rc;
    if (n_out == 0 || (!mix && n_tracks == 0)) return 0;
    std::vector<hpfw::WarpTrack> tab((size_t)n_tracks);
    for (int64_t i = 0; i < n_tracks; ++i) {
        const hpfw_warp_track &t = tracks[i];
        hpfw::WarpTrack &w = tab[(size_t)i];
        w = hpfw::WarpTrack{t.src_off, t.src_len, t.i0, t.f0, t.d, t.gain, 0, 0, 0};
        hpfw::warp_reach(t, &w.m_lo, &w.m_hi);
    }
    return ordered_call(h, s, [&] {
        if (int rc = ensure(h->warp.d_tracks, std::max<size_t>(tab.size(), 1) * sizeof(hpfw::WarpTrack))) return rc;
        if (!tab.empty()) {
            HIP_TRY(hipMemcpyAsync(h->warp.d_tracks.get(), tab.data(), tab.size() * sizeof(hpfw::WarpTrack), hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s)); // (the host vector dies)
        }
        hpfw::launch_warp(d_pcm, h->warp.d_tracks.as<hpfw::WarpTrack>(), n_tracks, h->warp.d_taps.as<int32_t>(), m0, n_out, mix, d_out, s);
        return check_launch(mix ? "mix" : "warp");
    });
}

int warp_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0, int64_t n_out, bool mix,
              int16_t *out)
{
    if (int rc = warp_check_call(h, pcm, n_pcm, tracks, n_tracks, m0, n_out, out, mix)) return rc; // (before anything is allocated)
    HIP_TRY(hipSetDevice(h->device));
    const int64_t rows = mix ? 1 : n_tracks;
    if (n_out == 0 || rows == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)std::max<int64_t>(n_pcm, 1) * 2, n_pcm ? pcm : nullptr);
    int16_t *d_out = t.take<int16_t>((size_t)rows * (size_t)n_out * 2, nullptr, -1, out);
    return t.run(true, [&] { return warp_device(h, d_pcm, n_pcm, tracks, n_tracks, m0, n_out, mix, d_out, nullptr); });
}

} // namespace

extern "C" {

int hpfw_gpu_warp_table(int16_t *taps, int64_t cap, int32_t *P, int32_t *T)
{
    if (!P || !T) return fail(HPFW_E_INVALID, "bad argument");
    *P = hpfw::kWarpP;
    *T = hpfw::kWarpT;
    if (!taps) return 0;
    if (cap < (int64_t)hpfw::kWarpP * hpfw::kWarpT) return fail(HPFW_E_INVALID, "buffer smaller than the table");
    std::vector<int16_t> t;
    if (!hpfw::warp_design(t)) return fail(HPFW_E_INVALID, "warp table out of range");
    std::copy(t.begin(), t.end(), taps);
    return 0;
}

int hpfw_gpu_warp_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0,
                        int64_t n_out, int16_t *d_out, void *stream)
{
    return warp_device(h, d_pcm, n_pcm, tracks, n_tracks, m0, n_out, false, d_out, (hipStream_t)stream);
}

int hpfw_gpu_warp_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0,
                             int64_t n_out, int16_t *out)
{
    return warp_host(h, pcm, n_pcm, tracks, n_tracks, m0, n_out, false, out);
}

int hpfw_gpu_mix_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0,
                       int64_t n_out, int16_t *d_mix, void *stream)
{
    return warp_device(h, d_pcm, n_pcm, tracks, n_tracks, m0, n_out, true, d_mix, (hipStream_t)stream);
}

int hpfw_gpu_mix_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks, int64_t m0,
                            int64_t n_out, int16_t *mix)
{
    return warp_host(h, pcm, n_pcm, tracks, n_tracks, m0, n_out, true, mix);
}

int hpfw_gpu_drift_anchors(int64_t s_lo, int64_t s_hi, int64_t q, int64_t len, int64_t anchor_len, int64_t anchor_hop, int64_t *starts,
                           int64_t cap, int32_t *n_left, int32_t *n_right, int64_t *n)
{
    if (!n) return fail(HPFW_E_INVALID, "drift anchors: null argument");
    const int64_t got = hpfw::drift_anchors(s_lo, s_hi, q, len, anchor_len, anchor_hop, starts, cap, n_left, n_right);
    if (got < 0) return fail(HPFW_E_INVALID, "drift anchors: the centre segment outside the overlap, a length below 1, or a buffer too small");
    *n = got;
    return 0;
}

int hpfw_gpu_drift_fit(const int64_t *n, const int64_t *lag, int count, double *a, double *b, double *rms)
{
    if (!a || !b || !rms || count < 0 || (count > 0 && (!n || !lag))) return fail(HPFW_E_INVALID, "drift fit: null or negative argument");
    if (count > 1 << 14) return fail(HPFW_E_INVALID, "drift fit: more than 2^14 points");
    hpfw::drift_fit(n, lag, count, a, b, rms);
    return 0;
}

int hpfw_gpu_time_map_q40(double A, double B, int64_t *i0, int64_t *f0, int64_t *d)
{
    if (!i0 || !f0 || !d) return fail(HPFW_E_INVALID, "time map: null argument");
    if (!hpfw::time_map_q40(A, B, i0, f0, d)) return fail(HPFW_E_INVALID, "time map: |1 / (1 + B) - 1| above 2^-10 or |A| above 2^30");
    return 0;
}

} // extern "C"
