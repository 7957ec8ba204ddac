// learn.hip -- filter learning (covariance, eigen-solve), HashprintHandle configurations other than the default, and
// the Mel front end.
#include "handle.h"

namespace {
template <class T>
int upload(const std::vector<T> &v, const T **out, std::vector<DevBuf> &owned)
{
    if (v.empty()) {
        *out = nullptr;
        return 0;
    }
    owned.emplace_back();
    HIP_TRY(owned.back().alloc(v.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(owned.back().get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = owned.back().as<const T>();
    return 0;
}

// the eigen-solve's top `bits` eigenvectors of the kt x kt covariance as column-major filters (element (r, k) at
// r + bits k): installed by install(filters), copied to filters_out when given
template <class Install>
int learn_filters(const float *cov, int kt, int bits, float *filters_out, Install install)
{
    std::vector<float> rows((size_t)bits * kt);
    if (hpfw::top_eigenvectors(cov, kt, bits, rows.data(), nullptr) != 0) return fail(HPFW_E_INVALID, "eigen-solve failed");
    std::vector<float> colmajor((size_t)bits * kt);
    for (int r = 0; r < bits; ++r)
        for (int k = 0; k < kt; ++k) colmajor[(size_t)r + (size_t)bits * k] = rows[(size_t)r * kt + k];
    if (int rc = install(colmajor.data())) return rc;
    if (filters_out) std::memcpy(filters_out, colmajor.data(), colmajor.size() * 4);
    return 0;
}

// n floats of an accumulated covariance d (null: none yet, zeros) to the host, after the device-wide wait
int read_cov(const void *d, float *cov, size_t n)
{
    if (!d) {
        std::memset(cov, 0, n * 4);
        return 0;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cov, d, n * 4, hipMemcpyDeviceToHost));
    return 0;
}
} // namespace

extern "C" {

// ---- Mel front-end (f3): MelSpectrogram<>::spectrogram (mel.h:34-104) ---------------------------
int64_t hpfw_gpu_mel_frames(int64_t n_samples) { return hpfw::mel_frames(n_samples); }

static int mel_prepare(hpfw_gpu *h)
{
    if (h->mel.ready) return 0;
    h->mel.owned.clear(); // (what an attempt that failed part-way uploaded)
    std::string why;
    if (!hpfw::build_frame_transform(hpfw::kMelFrame, h->mel.plan, why)) return fail(HPFW_E_UNSUPPORTED, why.c_str());
    const hpfw::HostPlan &p = h->mel.plan;
    hpfw::RowsArgs &ra = h->mel.rows;
    std::memset(&ra, 0, sizeof(ra));
    ra.n1 = 2;
    ra.n2 = p.n2;
    ra.h = p.h;
    ra.hpad = 2208;
    ra.pair_stride = 1;
    ra.groups.n = (int)p.groups.size();
    for (size_t g = 0; g < p.groups.size(); ++g) {
        ra.groups.r1[g] = p.groups[g].first;
        ra.groups.r2[g] = p.groups[g].second;
        ra.groups.tw_off[g] = p.rows_gtw_off[g];
    }
    int rc;
    if ((rc = upload(p.rows_gtw, reinterpret_cast<const hpfw::HostCf **>(&ra.gtw), h->mel.owned))) return rc;
    if ((rc = upload(p.tw_big, reinterpret_cast<const hpfw::HostCf **>(&ra.tw_big), h->mel.owned))) return rc;
    if ((rc = upload(p.pos_n2, &ra.pos_n2, h->mel.owned))) return rc;
    if ((rc = upload(p.kb_last, &ra.kb_last, h->mel.owned))) return rc;
    std::vector<float> win, cpack;
    hpfw::mel_tables(win, cpack);
    if ((rc = upload(win, &h->mel.d_win, h->mel.owned))) return rc;
    if ((rc = upload(cpack, &h->mel.d_cpack, h->mel.owned))) return rc;
    h->mel.ready = true;
    return 0;
}

int hpfw_gpu_mel_spectrogram_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, float *d_out,
                                   int32_t *d_cols, void *stream)
{
    if (!h || !d_pcm || !d_out || !d_cols || n_clips < 0 || n_samples < 1) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = mel_prepare(h);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int nf = hpfw::mel_frames(n_samples), n_blk = (int)((n_samples + hpfw::kMelHop - 1) / hpfw::kMelHop);
        // clips per pass: the split spectra take 2 * 2208 floats per frame
        const int64_t per_clip = (int64_t)hpfw::mel_work_bytes(n_samples, 1);
        const int nbmax = (int)std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(n_clips, 1), ((int64_t)8 << 30) / per_clip));
        if ((rc = ensure(h->mel.d_work, hpfw::mel_work_bytes(n_samples, nbmax)))) return rc;
        if ((rc = ensure(h->mel.d_small, (size_t)nbmax * ((size_t)n_blk * 8 + (size_t)nf * 4 + 8)))) return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            int64_t *blk = h->mel.d_small.as<int64_t>();
            int *pos = (int *)(blk + (size_t)nbmax * n_blk);
            float *pmax = (float *)(pos + (size_t)nbmax * nf);
            hpfw::launch_mel(h->mel.rows, h->mel.d_win, h->mel.d_cpack, d_pcm + c0 * n_samples, n_samples, nb, blk, pos,
                             d_cols + c0, pmax, h->mel.d_work.as<float>(), d_out + c0 * hpfw::kMelBands * nf, h->db_fast, s);
            if ((rc = check_launch("mel"))) return rc;
        }
        return 0;
    });
}

int hpfw_gpu_mel_spectrogram_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, float *out,
                                        int32_t *cols)
{
    if (!h || !pcm || !out || !cols || n_clips < 0 || n_samples < 1) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_clips == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)n_clips * n_samples * 2, pcm);
    float *d_out = t.take<float>((size_t)n_clips * hpfw::kMelBands * hpfw::mel_frames(n_samples) * 4, nullptr, 0, out);
    int32_t *d_cols = t.take<int32_t>((size_t)n_clips * 4, nullptr, -1, cols);
    return t.run(true, [&] { return hpfw_gpu_mel_spectrogram_pcm16(h, d_pcm, n_samples, n_clips, d_out, d_cols, nullptr); });
}

// ---- HashprintHandle with other template arguments (hashprint_handle.h:50-64) -------------------------
static int cfg_check(const hpfw_handle_config *c)
{
    if (!c) return fail(HPFW_E_INVALID, "null config");
    if (c->rows < 1 || c->rows > 512 || c->context < 1 || c->context > 256 || c->lag < 1 ||
        (c->bits != 16 && c->bits != 32 && c->bits != 64))
        return fail(HPFW_E_INVALID, "config: rows 1..512, context 1..256, lag >= 1, bits 16, 32 or 64");
    hpfw::CfgArgs a{c->rows, c->context, c->lag, c->bits, nullptr};
    if (hpfw::project_cfg_lds_bytes(a) > 160 * 1024) return fail(HPFW_E_UNSUPPORTED, "config: rows x context exceeds the LDS slab");
    return 0;
}

int hpfw_gpu_cfg_set_filters(hpfw_gpu *h, const hpfw_handle_config *c, const float *f)
{
    if (!h || !f) return fail(HPFW_E_INVALID, "null argument");
    int rc = cfg_check(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::vector<float> packed(hpfw::cfg_fpack_floats(c->rows, c->context, c->bits));
    hpfw::pack_cfg_filters(c->rows, c->context, c->bits, f, packed.data());
    const std::vector<int> key{c->rows, c->context, c->bits};
    auto it = h->learn.cfg_fpack.find(key);
    if (it == h->learn.cfg_fpack.end()) { // (the configuration is known once its buffer exists)
        DevBuf d;
        HIP_TRY(d.alloc(packed.size() * 4));
        it = h->learn.cfg_fpack.emplace(key, std::move(d)).first;
    }
    return ordered_call(h, nullptr, [&] {
        HIP_TRY(hipMemcpy(it->second.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        return 0;
    });
}

int hpfw_gpu_cfg_hashprints(hpfw_gpu *h, const hpfw_handle_config *c, const float *d_s, const int32_t *d_cols, int64_t n_clips,
                            int64_t stride, void *d_hp, int64_t hp_stride, float *d_proj, void *stream)
{
    if (!h || !d_s || !d_hp || n_clips < 0 || stride < 1) return fail(HPFW_E_INVALID, "bad argument");
    int rc = cfg_check(c);
    if (rc) return rc;
    auto it = h->learn.cfg_fpack.find({c->rows, c->context, c->bits});
    if (it == h->learn.cfg_fpack.end()) return fail(HPFW_E_NOFILTERS, "no filters for this configuration: call hpfw_gpu_cfg_set_filters first");
    const int64_t nf = stride - c->context + 1, nhp = nf - c->lag;
    if (nhp > hp_stride) return fail(HPFW_E_INVALID, "hp_stride smaller than stride - context + 1 - lag");
    if (n_clips == 0 || nhp <= 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const hpfw::CfgArgs a{c->rows, c->context, c->lag, c->bits, it->second.as<float>()};
        // clips per pass: the projection scratch stays below 1 GiB
        const int64_t per = (int64_t)c->bits * nf * 4;
        const int64_t chunk = d_proj ? n_clips : std::max<int64_t>(1, std::min<int64_t>(n_clips, ((int64_t)1 << 30) / per));
        if (!d_proj && (rc = ensure(h->learn.d_cfg_proj, (size_t)chunk * per))) return rc;
        const size_t word = (size_t)c->bits / 8;
        for (int64_t c0 = 0; c0 < n_clips; c0 += chunk) {
            const int nb = (int)std::min<int64_t>(chunk, n_clips - c0);
            float *pj = d_proj ? d_proj + c0 * c->bits * nf : h->learn.d_cfg_proj.as<float>();
            const int *cols = d_cols ? d_cols + c0 : nullptr;
            {
                Timed t(h, K_PROJECT, s);
                hpfw::launch_project_cfg(a, d_s + c0 * c->rows * stride, cols, nb, stride, pj, nf, s);
            }
            if ((rc = check_launch("project_cfg"))) return rc;
            {
                Timed t(h, K_PACK, s);
                hpfw::launch_pack_cfg(a, pj, cols, nb, stride, nf, (char *)d_hp + (size_t)c0 * hp_stride * word, hp_stride, s);
            }
            if ((rc = check_launch("pack_cfg"))) return rc;
        }
        return 0;
    });
}

static int cfg_cov_slot(hpfw_gpu *h, const hpfw_handle_config *c, hpfw_gpu::Learn::CfgCov **out)
{
    const std::vector<int> key{c->rows, c->context};
    auto it = h->learn.cfg_cov.find(key);
    if (it == h->learn.cfg_cov.end()) { // (entered once complete)
        const int kt = c->rows * c->context;
        hpfw_gpu::Learn::CfgCov cc;
        HIP_TRY(cc.d_accum.alloc((size_t)kt * kt * 4));
        HIP_TRY(hipMemset(cc.d_accum.get(), 0, (size_t)kt * kt * 4));
        std::vector<int> xy((size_t)2 * hpfw::cov_cfg_tile_count(kt));
        hpfw::cov_cfg_tile_list(kt, xy.data());
        HIP_TRY(cc.d_tiles.alloc(xy.size() * 4));
        HIP_TRY(hipMemcpy(cc.d_tiles.get(), xy.data(), xy.size() * 4, hipMemcpyHostToDevice));
        it = h->learn.cfg_cov.emplace(key, std::move(cc)).first;
    }
    *out = &it->second;
    return 0;
}

int hpfw_gpu_cfg_cov_reset(hpfw_gpu *h, const hpfw_handle_config *c)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    int rc = cfg_check(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    auto it = h->learn.cfg_cov.find({c->rows, c->context});
    if (it == h->learn.cfg_cov.end()) return 0;
    return ordered_call(h, nullptr, [&] {
        const int kt = c->rows * c->context;
        HIP_TRY(hipMemset(it->second.d_accum.get(), 0, (size_t)kt * kt * 4));
        it->second.clips = 0;
        return 0;
    });
}

int hpfw_gpu_cfg_cov_accumulate(hpfw_gpu *h, const hpfw_handle_config *c, const float *d_s, const int32_t *d_cols, int64_t n_clips,
                                int64_t stride, void *stream)
{
    if (!h || !d_s || n_clips < 0 || stride < 1) return fail(HPFW_E_INVALID, "bad argument");
    int rc = cfg_check(c);
    if (rc) return rc;
    const hpfw::CfgArgs a{c->rows, c->context, c->lag, c->bits, nullptr};
    if (!hpfw::cov_cfg_supported(a)) return fail(HPFW_E_UNSUPPORTED, "covariance: context below 9 is not supported");
    HIP_TRY(hipSetDevice(h->device));
    hpfw_gpu::Learn::CfgCov *cc;
    if ((rc = cfg_cov_slot(h, c, &cc))) return rc;
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int64_t chunk = 512; // clips per pass: bounds the partial tiles and the per-clip sums
        if ((rc = ensure(h->learn.d_cfg_cov_ws,
                         hpfw::cov_cfg_workspace_bytes(a, (int)std::min(chunk, std::max<int64_t>(n_clips, 1))))))
            return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += chunk) {
            const int nb = (int)std::min(chunk, n_clips - c0);
            hpfw::launch_cov_cfg(a, d_s + c0 * c->rows * stride, d_cols ? d_cols + c0 : nullptr, nb, stride, cc->d_tiles.as<int>(),
                                 h->learn.d_cfg_cov_ws.as<float>(), cc->d_accum.as<float>(), s);
            if ((rc = check_launch("cov_cfg"))) return rc;
        }
        cc->clips += n_clips;
        return 0;
    });
}

int hpfw_gpu_cfg_cov_get(hpfw_gpu *h, const hpfw_handle_config *c, float *cov, int64_t *n_clips)
{
    if (!h || !cov) return fail(HPFW_E_INVALID, "null argument");
    int rc = cfg_check(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    auto it = h->learn.cfg_cov.find({c->rows, c->context});
    const bool have = it != h->learn.cfg_cov.end();
    if ((rc = read_cov(have ? it->second.d_accum.get() : nullptr, cov, (size_t)c->rows * c->context * c->rows * c->context))) return rc;
    if (n_clips) *n_clips = have ? it->second.clips : 0;
    return 0;
}

int hpfw_gpu_cfg_learn_filters(hpfw_gpu *h, const hpfw_handle_config *c, float *filters_out)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    int rc = cfg_check(c);
    if (rc) return rc;
    const int kt = c->rows * c->context;
    std::vector<float> cov((size_t)kt * kt);
    int64_t clips = 0;
    if ((rc = hpfw_gpu_cfg_cov_get(h, c, cov.data(), &clips))) return rc;
    if (clips == 0) return fail(HPFW_E_INVALID, "no covariance accumulated for this configuration");
    return learn_filters(cov.data(), kt, c->bits, filters_out, [&](const float *f) { return hpfw_gpu_cfg_set_filters(h, c, f); });
}

int hpfw_gpu_mel_hashprints_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, uint16_t *hp,
                                       int64_t hp_stride, int32_t *n_hp)
{
    if (!h || !pcm || !hp || !n_hp || n_clips < 0 || n_samples < 1) return fail(HPFW_E_INVALID, "bad argument");
    const hpfw_handle_config cfg = HPFW_CONFIG_COMBINER;
    const int64_t frames = hpfw::mel_frames(n_samples), nhp_max = frames - cfg.context + 1 - cfg.lag;
    if (nhp_max > hp_stride) return fail(HPFW_E_INVALID, "hp_stride smaller than hpfw_gpu_mel_frames(n_samples) - 81");
    HIP_TRY(hipSetDevice(h->device));
    if (n_clips == 0) return 0;
    if (h->learn.cfg_fpack.find({cfg.rows, cfg.context, cfg.bits}) == h->learn.cfg_fpack.end())
        return fail(HPFW_E_NOFILTERS, "no filters for the combiner configuration: call hpfw_gpu_cfg_set_filters first");
    std::vector<int32_t> cols((size_t)n_clips);
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)n_clips * n_samples * 2, pcm);
    float *d_s = t.take<float>((size_t)n_clips * hpfw::kMelBands * frames * 4, nullptr, 0);
    void *d_hp = t.take<void>((size_t)n_clips * std::max<int64_t>(hp_stride, 1) * 2, nullptr, 0, hp);
    int32_t *d_cols = t.take<int32_t>((size_t)n_clips * 4, nullptr, -1, cols.data());
    const int rc = t.run(true, [&] {
        const int rc = hpfw_gpu_mel_spectrogram_pcm16(h, d_pcm, n_samples, n_clips, d_s, d_cols, nullptr);
        return rc ? rc : hpfw_gpu_cfg_hashprints(h, &cfg, d_s, d_cols, n_clips, frames, d_hp, hp_stride, nullptr, nullptr);
    });
    for (int64_t i = 0; !rc && i < n_clips; ++i) n_hp[i] = std::max<int32_t>(cols[(size_t)i] - cfg.context + 1 - cfg.lag, 0);
    return rc;
}

int hpfw_gpu_mel_cov_accumulate_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips)
{
    if (!h || !pcm || n_clips < 0 || n_samples < 1) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_clips == 0) return 0;
    const hpfw_handle_config cfg = HPFW_CONFIG_COMBINER;
    const int64_t frames = hpfw::mel_frames(n_samples);
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)n_clips * n_samples * 2, pcm);
    float *d_s = t.take<float>((size_t)n_clips * hpfw::kMelBands * frames * 4, nullptr, 0);
    int32_t *d_cols = t.take<int32_t>((size_t)n_clips * 4);
    return t.run(true, [&] {
        const int rc = hpfw_gpu_mel_spectrogram_pcm16(h, d_pcm, n_samples, n_clips, d_s, d_cols, nullptr);
        return rc ? rc : hpfw_gpu_cfg_cov_accumulate(h, &cfg, d_s, d_cols, n_clips, frames, nullptr);
    });
}

// ---- filter learning: preprocess() of the reference (parallel_collector.h:82-112) ---------------
static int cov_prepare(hpfw_gpu *h, hipStream_t s)
{
    // (each buffer is the handle's once it is filled)
    if (!h->learn.d_cov) {
        DevBuf cov;
        HIP_TRY(cov.alloc((size_t)hpfw::kFrame * hpfw::kFrame * 4));
        HIP_TRY(hipMemsetAsync(cov.get(), 0, (size_t)hpfw::kFrame * hpfw::kFrame * 4, s));
        h->learn.d_cov = std::move(cov);
        h->learn.cov_files = 0;
    }
    if (!h->learn.d_cov_tiles) {
        std::vector<int> xy((size_t)2 * hpfw::cov_tile_count());
        hpfw::cov_tile_list(xy.data());
        DevBuf tiles;
        HIP_TRY(tiles.alloc(xy.size() * 4));
        HIP_TRY(hipMemcpy(tiles.get(), xy.data(), xy.size() * 4, hipMemcpyHostToDevice));
        h->learn.d_cov_tiles = std::move(tiles);
    }
    return 0;
}

int hpfw_gpu_cov_reset(hpfw_gpu *h)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (h->learn.d_cov) HIP_TRY(hipMemset(h->learn.d_cov.get(), 0, (size_t)hpfw::kFrame * hpfw::kFrame * 4));
    h->learn.cov_files = 0;
    return 0;
}

int hpfw_gpu_cov_accumulate_db(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, void *stream)
{
    if (!h || !d_db || n_clips < 0 || c < hpfw::kCtx + 1) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        int rc = cov_prepare(h, s);
        if (rc) return rc;
        const int64_t chunk = 128; // clips per pass: bounds the workspace (Z, correction vectors, partial sums)
        if ((rc = ensure(h->learn.d_cov_ws,
                         hpfw::cov_workspace_bytes((int)std::min(chunk, std::max<int64_t>(n_clips, 1)), (int)c))))
            return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += chunk) {
            const int nb = (int)std::min(chunk, n_clips - c0);
            hpfw::launch_cov(d_db + c0 * 121 * c, nb, (int)c, h->learn.d_cov_tiles.as<int>(), h->learn.d_cov_ws.as<float>(), h->learn.d_cov.as<float>(), s);
            if ((rc = check_launch("covariance"))) return rc;
        }
        h->learn.cov_files += n_clips;
        return 0;
    });
}

int hpfw_gpu_cov_accumulate_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                                  void *stream)
{
    if (!h || !d_pcm || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    DevPlan *dp;
    int rc = get_plan(h, n_samples, &dp);
    if (rc) return rc;
    if (dp->hp.n_frames < 2) return fail(HPFW_E_UNSUPPORTED, "clip too short for a covariance");
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        const int nbmax = pass_clips(h, dp, n_clips);
        if ((rc = ensure_ws(h, dp, nbmax, nbmax))) return rc;
        for (int64_t c0 = 0; c0 < n_clips; c0 += nbmax) {
            const int nb = (int)std::min<int64_t>(nbmax, n_clips - c0);
            if ((rc = run_front(h, dp, d_pcm + c0 * n_samples, nb, 0, true, s))) return rc;
            if ((rc = hpfw_gpu_cov_accumulate_db(h, h->ws[2].as<float>(), nb, dp->hp.c, stream))) return rc;
        }
        return 0;
    });
}

int hpfw_gpu_cov_accumulate_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips)
{
    if (!h || !pcm || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_clips == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)n_clips * n_samples * 2, pcm);
    return t.run(true, [&] { return hpfw_gpu_cov_accumulate_pcm16(h, d_pcm, n_samples, n_clips, nullptr); });
}

// full symmetric matrix, row-major 2420 x 2420 (= the column-major Eigen matrix of accum_cov.cereal)
int hpfw_gpu_cov_get(hpfw_gpu *h, float *cov, int64_t *n_files)
{
    if (!h || !cov) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = read_cov(h->learn.d_cov.get(), cov, (size_t)hpfw::kFrame * hpfw::kFrame)) return rc;
    if (h->learn.d_cov) { // the device holds tiles on or above the diagonal (128-wide); mirror them
        for (int r = 0; r < hpfw::kFrame; ++r)
            for (int c2 = 0; c2 < r; ++c2)
                if (c2 / 128 < r / 128) cov[(size_t)r * hpfw::kFrame + c2] = cov[(size_t)c2 * hpfw::kFrame + r];
    }
    if (n_files) *n_files = h->learn.cov_files;
    return 0;
}

int hpfw_gpu_cov_set(hpfw_gpu *h, const float *cov, int64_t n_files)
{
    if (!h || !cov || n_files < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = cov_prepare(h, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(h->learn.d_cov.get(), cov, (size_t)hpfw::kFrame * hpfw::kFrame * 4, hipMemcpyHostToDevice));
    h->learn.cov_files = n_files;
    return 0;
}

int hpfw_gpu_cov_device(hpfw_gpu *h, float **d_cov)
{
    if (!h || !d_cov) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = cov_prepare(h, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    *d_cov = h->learn.d_cov.as<float>();
    return 0;
}

int64_t hpfw_gpu_cov_files(hpfw_gpu *h) { return h ? h->learn.cov_files : 0; }

int hpfw_gpu_cov_set_files(hpfw_gpu *h, int64_t n_files)
{
    if (!h || n_files < 0) return fail(HPFW_E_INVALID, "bad argument");
    h->learn.cov_files = n_files;
    return 0;
}

// calc_filters (hashprint_handle.h:105-112): eigenvectors of the accumulated covariance by descending
// eigenvalue, the first 64 as rows; they become the handle's filters.  filters_out (optional) receives
// them in the reference's column-major layout.
int hpfw_gpu_learn_filters(hpfw_gpu *h, float *filters_out)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (!h->learn.d_cov || h->learn.cov_files == 0) return fail(HPFW_E_INVALID, "no covariance accumulated");
    std::vector<float> cov((size_t)hpfw::kFrame * hpfw::kFrame);
    int rc = hpfw_gpu_cov_get(h, cov.data(), nullptr);
    if (rc) return rc;
    return learn_filters(cov.data(), hpfw::kFrame, hpfw::kFilters, filters_out, [&](const float *f) { return hpfw_gpu_set_filters(h, f); });
}

} // extern "C"
