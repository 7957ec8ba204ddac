// handle.hip -- the handle of the C-ABI (include/hpfw_gpu.h): creation, filters, projection, conventions, batch,
// error messages and timing.
#include "handle.h"

namespace {
thread_local std::string g_err;

const char *const kKernelNames[K_COUNT] = {"fwd_rows", "fwd_cols", "cq_chirpz", "db",
                                           "project_mfma", "delta_pack", "hamming_scan", "topk", "pcm_pairs", "fwd_span"};
} // namespace

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

extern "C" {

const char *hpfw_gpu_last_error(void) { return g_err.c_str(); }
// used by legacy.cpp so that the file entry points report through the same thread-local message
void hpfw_internal_set_error(const char *msg) { g_err = msg ? msg : ""; }
const char *hpfw_gpu_version(void) { return "hpfw-gpu 0.1 (gfx950)"; }

int hpfw_gpu_create(int device, hpfw_gpu **out)
{
    if (!out) return fail(HPFW_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(HPFW_E_INVALID, "no such device");
    HIP_TRY(hipSetDevice(device));
    auto h = std::make_unique<hpfw_gpu>();
    h->device = device;
    if (std::getenv("HPFW_CQ_SERIAL")) h->cq_concurrent = 0;
    if (const char *e = std::getenv("HPFW_FWD_CHUNK")) h->fwd_chunk = std::max(0, atoi(e));
    if (const char *e = std::getenv("HPFW_PASS_PIPELINE")) h->pass_pipeline = atoi(e) != 0;
    if (const char *e = std::getenv("HPFW_PASS_PLAN")) {
        std::vector<int> *to = &h->pp_class_lane;
        for (; *e; ++e) {
            if (*e == ':') to = &h->pp_turns;
            else if (*e >= '0' && *e <= '0' + hpfw_gpu::kCqSide) to->push_back(*e - '0');
        }
    }
    if (const char *e = std::getenv("HPFW_BZ_CHUNK")) h->bz_chunk = std::max(0, atoi(e));
    if (const char *e = std::getenv("HPFW_COLS_VARIANT")) h->cols_variant = atoi(e);
    if (const char *e = std::getenv("HPFW_PRUNE")) h->prune = (unsigned)std::strtoul(e, nullptr, 0);
    if (const char *e = std::getenv("HPFW_Q_PRODUCTS")) h->q_products = atoi(e) == 9 ? 9 : 6;
    if (const char *e = std::getenv("HPFW_DB_TERM")) h->db_fast = std::strcmp(e, "spec") != 0;
    if (const char *e = std::getenv("HPFW_FWD_STREAMS")) h->fwd_streams = std::min(hpfw_gpu::kCqSide + 1, std::max(1, atoi(e)));
    if (const char *e = std::getenv("HPFW_PROJECTION")) // "f32": handles start with the f32 fma chain (hpfw_gpu_set_projection(h, 0))
        h->projection = std::strcmp(e, "f32") == 0 ? 0 : 1;
    if (h->ev0.create(hipEventDefault) != hipSuccess || h->ev1.create(hipEventDefault) != hipSuccess || h->order_ev.create() != hipSuccess ||
        init_plans(h.get()) != hipSuccess)
        return fail(HPFW_E_HIP, "hipEventCreate failed");
    *out = h.release();
    return 0;
}

int hpfw_gpu_device(const hpfw_gpu *h) { return h ? h->device : -1; }

void hpfw_gpu_destroy(hpfw_gpu *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
}

int hpfw_gpu_set_filters(hpfw_gpu *h, const float *f)
{
    if (!h || !f) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    std::vector<float> packed((size_t)hpfw::kFilters * hpfw::kFrame);
    hpfw::pack_filters_for_mfma(f, packed.data());
    if (!h->d_fpack) HIP_TRY(h->d_fpack.alloc(packed.size() * 4));
    HIP_TRY(hipMemcpy(h->d_fpack.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    std::vector<int8_t> image;
    std::vector<int32_t> thr;
    hpfw::pack_filters_q(f, image, &thr);
    if (!h->d_fq_image) HIP_TRY(h->d_fq_image.alloc(image.size()));
    HIP_TRY(hipMemcpy(h->d_fq_image.get(), image.data(), image.size(), hipMemcpyHostToDevice));
    if (!h->d_q_thr) HIP_TRY(h->d_q_thr.alloc(thr.size() * 4));
    HIP_TRY(hipMemcpy(h->d_q_thr.get(), thr.data(), thr.size() * 4, hipMemcpyHostToDevice));
    h->shift_images_of.clear();
    h->filters.assign(f, f + (size_t)hpfw::kFilters * hpfw::kFrame);
    h->has_filters = true;
    return 0;
}

int hpfw_gpu_get_filters(hpfw_gpu *h, float *out)
{
    if (!h || !out) return fail(HPFW_E_INVALID, "null argument");
    if (!h->has_filters) return fail(HPFW_E_NOFILTERS, "no filters: call hpfw_gpu_set_filters or hpfw_gpu_learn_filters first");
    std::memcpy(out, h->filters.data(), h->filters.size() * sizeof(float));
    return 0;
}

int hpfw_gpu_set_projection(hpfw_gpu *h, int mode)
{
    if (!h || (mode != 0 && mode != 1)) return fail(HPFW_E_INVALID, "projection mode must be 0 (f32 chain) or 1 (fixed point)");
    h->projection = mode;
    return 0;
}

int hpfw_gpu_get_projection(hpfw_gpu *h) { return h ? h->projection : -1; }

int hpfw_gpu_set_conventions(hpfw_gpu *h, unsigned flags)
{
    if (!h || flags > hpfw::kConvAll) return fail(HPFW_E_INVALID, "unknown convention flag");
    HIP_TRY(hipSetDevice(h->device));
    if (flags != h->conventions) { // the tables of every cached length were built under the old conventions
        HIP_TRY(hipDeviceSynchronize());
        clear_plans(h);
    }
    h->conventions = flags;
    return 0;
}

int hpfw_gpu_set_batch(hpfw_gpu *h, int clips)
{
    if (!h || clips < 0 || clips > 4096) return fail(HPFW_E_INVALID, "batch out of range");
    h->batch = clips == 0 ? 256 : clips;
    return 0;
}

// ---- timing ------------------------------------------------------------------------------------
int hpfw_gpu_timer_start(hpfw_gpu *h, void *stream)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    HIP_TRY(hipEventRecord(h->ev0.get(), (hipStream_t)stream));
    return 0;
}

int hpfw_gpu_timer_stop(hpfw_gpu *h, void *stream, float *ms)
{
    if (!h || !ms) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipEventRecord(h->ev1.get(), (hipStream_t)stream));
    HIP_TRY(hipEventSynchronize(h->ev1.get()));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0.get(), h->ev1.get()));
    return 0;
}

int hpfw_gpu_set_kernel_timing(hpfw_gpu *h, int mask)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    h->timing_mask = (unsigned)mask;
    for (TimedLaunch &t : h->timed) h->ev_pool.emplace_back(std::move(t.a), std::move(t.b));
    h->timed.clear();
    std::memset(h->k_ms, 0, sizeof(h->k_ms));
    std::memset(h->k_launches, 0, sizeof(h->k_launches));
    return 0;
}

int hpfw_gpu_get_kernel_timing(hpfw_gpu *h, const char **names, float *ms, int *launches, int *n)
{
    if (!h || !names || !ms || !launches || !n) return fail(HPFW_E_INVALID, "null argument");
    for (const TimedLaunch &t : h->timed) {
        HIP_TRY(hipEventSynchronize(t.b.get()));
        float e = 0.0f;
        HIP_TRY(hipEventElapsedTime(&e, t.a.get(), t.b.get()));
        h->k_ms[t.kind] += e;
        h->k_launches[t.kind] += 1;
    }
    for (TimedLaunch &t : h->timed) h->ev_pool.emplace_back(std::move(t.a), std::move(t.b));
    h->timed.clear();
    const int cap = *n;
    int w = 0;
    for (int i = 0; i < K_COUNT && w < cap; ++i, ++w) {
        names[w] = kKernelNames[i];
        ms[w] = h->k_ms[i];
        launches[w] = h->k_launches[i];
    }
    *n = w;
    return 0;
}

} // extern "C"
