// legacy.cpp -- the eight extern "C" symbols of the reference's only FFI boundary
// (modules/python/parallel_collector_wrapper.hpp:21-38, implementation wrapper.cpp:5-62), kept
// source-compatible and routed to the GPU path.  Ownership as in the reference: results are
// allocated with new[] and released by the paired *_free function.  Unlike the reference
// (wrapper.cpp has no exception barrier) nothing throws through the C boundary: failures return
// NULL / *got = 0 and leave a message in hpfw_gpu_last_error().
//
// Audio input: essentia MonoLoader (reference include/hpfw/spectrum/cqt.h:45-52) is replaced by a
// RIFF/WAVE reader for PCM16 at 44.1 kHz (wav_file.h: mono, or stereo averaged as MonoLoader's "mix" downmix);
// other containers are rejected, and so are other rates unless the collector's resampling switch is on
// (hpfw_gpu_collector_set_resample: any rate in [8 000, 192 000] Hz, converted to 44.1 kHz on the GPU).
// Filters, accum_cov and the cached spectrograms: cereal's binary layout of an Eigen matrix (cache_files.h).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/hpfw_gpu.h"
#include "cache_files.h"
#include "hip_owned.h"
#include "legacy_internal.h" // the extern "C" signatures multi.cpp sees, checked against the definitions below
#include "wav_file.h"

namespace {

using hpfw::WavProbe;
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// fn(i) for i in [0, n) on a small team of host threads; returns the team's size
template <class F>
unsigned host_team(int n, F fn)
{
    unsigned team = std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    team = std::min<unsigned>(team, (unsigned)std::max(n, 1));
    std::atomic<int> next{0};
    auto work = [&] {
        for (int i; (i = next.fetch_add(1)) < n;) fn(i);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < team; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    return team;
}

// the hashprints of one file on their way to the caller (empty: the file yielded none)
struct Hp {
    std::unique_ptr<uint64_t[]> bits;
    int size = 0;
};

Hp copy_hp(const uint64_t *src, int64_t n_hp)
{
    Hp h;
    h.bits.reset(new uint64_t[(size_t)n_hp]);
    std::memcpy(h.bits.get(), src, (size_t)n_hp * 8);
    h.size = (int)n_hp;
    return h;
}

// the name a track is returned and cached under (parallel_collector.h:123,129)
std::string stem_of(const char *path) { return std::filesystem::path(path).stem().string(); }

// the one place where results leave their owners: released by prepare_result_free
FilenameHashprintPair *make_result(const std::vector<std::string> &stems, std::vector<Hp> &hps)
{
    std::vector<std::unique_ptr<char[]>> names(stems.size());
    for (size_t w = 0; w < stems.size(); ++w) {
        names[w].reset(new char[stems[w].size() + 1]);
        std::memcpy(names[w].get(), stems[w].c_str(), stems[w].size() + 1);
    }
    auto *res = new FilenameHashprintPair[std::max<size_t>(stems.size(), 1)];
    for (size_t w = 0; w < stems.size(); ++w) {
        res[w].filename = names[w].release();
        res[w].hp_size = hps[w].size;
        res[w].hashprint = hps[w].bits.release();
    }
    return res;
}

} // namespace

struct hpfw_legacy_collector {
    hpfw_gpu *gpu = nullptr;
    std::string cache_dir = "cache/"; // parallel_collector.h:38
    std::vector<float> filters;
    // prepare() / calc_hashprints(): one window of files is read straight into pinned host memory (clips of equal length
    // side by side) and goes to the device in one copy; both buffers are kept between windows and calls
    // two pinned host arenas in turn: the files of the next window are read while this one is copied and extracted
    // (spare_db: the spectrogram buffer of the last group that was not kept, for the next one -- freeing and allocating
    // hundreds of MB of device memory per window stalls the reader threads, who share the address space)
    hpfw::DevBuf spare_db;
    // hashprints of a whole window when nothing is learned or cached (calc_hashprints): device buffer and pinned host copy
    hpfw::DevBuf d_hp_win;
    hpfw::HostBuf h_hp_win;
    // ... on a stream of the collector's own (non-blocking): the tables of the next file's length are generated and
    // uploaded through the default stream while the kernels of the previous file run
    hpfw::Stream win_stream;
    // pinned host copy of a group's spectrograms on their way to cache/spectros/ (grow-only)
    hpfw::HostBuf h_spec;
    hpfw::HostBuf arena[2];
    // ... and two device copies in turn: window w + 1 is uploaded while the kernels of window w read theirs
    hpfw::DevBuf d_arena_buf[2];
    void *d_arena = nullptr; // the copy of the window in hand
    // hpfw_gpu_collector_set_resample: files at other rates than 44.1 kHz are converted on the device (grow-only staging
    // of a group's 44.1 kHz clips, read by the extraction in place of the arena)
    bool resample = false;
    hpfw::DevBuf rs_stage;
};

// the exported entry points: no exception leaves the C boundary (the reference's wrapper.cpp has no such
// barrier); a failure that surfaces as one -- out of host memory, in practice -- becomes NULL + a message
template <class F>
static auto guarded(F f) -> decltype(f())
{
    try {
        return f();
    } catch (const std::exception &e) {
        hpfw_internal_set_error((std::string("host failure: ") + e.what()).c_str());
    } catch (...) {
        hpfw_internal_set_error("host failure");
    }
    return nullptr;
}

// NULL or "" keeps the directory in use (the default is "cache/"), as the reference wrapper's optional argument
static void set_cache_dir(hpfw_legacy_collector *c, const char *cache)
{
    if (!cache || !*cache) return;
    c->cache_dir = cache;
    if (c->cache_dir.back() != '/') c->cache_dir += '/';
}

extern "C" {

hpfw_legacy_collector *par_collector_new(void)
{
    auto *c = new hpfw_legacy_collector();
    int dev = 0;
    if (const char *e = std::getenv("HPFW_GPU_DEVICE")) dev = std::atoi(e);
    if (hpfw_gpu_create(dev, &c->gpu) != 0) {
        delete c;
        return nullptr;
    }
    return c;
}

void par_collector_del(hpfw_legacy_collector *c)
{
    if (!c) return;
    hpfw_gpu_destroy(c->gpu);
    delete c;
}

// ParallelCollector::load (parallel_collector.h:68-73)
void par_collector_load(hpfw_legacy_collector *c, const char *cache)
{
    if (!c) return;
    set_cache_dir(c, cache);
    std::vector<float> f;
    if (hpfw::load_filters_cereal(c->cache_dir + "filters.cereal", f)) { // missing file: silent no-op, cache.h:77-79
        c->filters.swap(f);
        (void)hpfw_gpu_set_filters(c->gpu, c->filters.data());
    }
    std::vector<float> cov; // cache.h:34-36: the reference keeps accumulating across runs
    if (hpfw::load_cov_cereal(c->cache_dir + "accum_cov.cereal", cov)) (void)hpfw_gpu_cov_set(c->gpu, cov.data(), 1);
}

void par_collector_save(hpfw_legacy_collector *c, const char *cache)
{
    if (!c || c->filters.empty()) return;
    set_cache_dir(c, cache);
    std::error_code ec;
    std::filesystem::create_directories(c->cache_dir, ec);
    (void)hpfw::save_filters_cereal(c->cache_dir + "filters.cereal", c->filters);
    std::vector<float> cov((size_t)HPFW_FRAME_SIZE * HPFW_FRAME_SIZE);
    int64_t n_files = 0;
    if (hpfw_gpu_cov_get(c->gpu, cov.data(), &n_files) == 0 && n_files > 0) // cache.h:34-36
        (void)hpfw::save_cov_cereal(c->cache_dir + "accum_cov.cereal", cov);
}

// A file of any length: the reference hands the exact sample count to NSGConstantQ (cqt.h:54-55) and so does
// this -- lengths with a prime factor above 7 take the chirp-z forward transform (k_bluestein.hip); nothing is padded.
static bool read_clip(const std::string &path, std::vector<int16_t> &pcm, std::string &why, uint32_t *rate_any = nullptr)
{
    try { // nothing may throw through the C boundary: e.g. bad_alloc on a huge file
        return hpfw::read_wav_pcm16_mono(path, pcm, why, rate_any);
    } catch (const std::exception &e) {
        why = path + ": " + e.what();
        return false;
    }
}

// rate: NULL = 44.1 kHz only
static int wav_read(const char *path, int16_t *out, int64_t cap, int64_t *n, int32_t *rate)
{
    *n = 0;
    if (rate) *rate = 0;
    std::vector<int16_t> pcm;
    std::string why;
    uint32_t r = 0;
    if (!read_clip(path, pcm, why, rate ? &r : nullptr)) {
        hpfw_internal_set_error(why.c_str());
        return HPFW_E_IO;
    }
    *n = (int64_t)pcm.size();
    if (rate) *rate = (int32_t)r;
    if (!out) return 0;
    if (cap < *n) {
        hpfw_internal_set_error("buffer smaller than the file's samples");
        return HPFW_E_INVALID;
    }
    std::copy(pcm.begin(), pcm.end(), out);
    return 0;
}

extern "C" int hpfw_gpu_wav_read_pcm16(const char *path, int16_t *out, int64_t cap, int64_t *n)
{
    if (!path || !n) {
        hpfw_internal_set_error("null argument");
        return HPFW_E_INVALID;
    }
    return wav_read(path, out, cap, n, nullptr);
}

extern "C" int hpfw_gpu_wav_read_pcm16_any(const char *path, int16_t *out, int64_t cap, int64_t *n, int32_t *rate)
{
    if (!path || !n || !rate) {
        hpfw_internal_set_error("null argument");
        return HPFW_E_INVALID;
    }
    return wav_read(path, out, cap, n, rate);
}

extern "C" int hpfw_gpu_wav_write_pcm16(const char *path, const int16_t *pcm, int64_t n, int channels)
{
    if (!path) {
        hpfw_internal_set_error("null argument");
        return HPFW_E_INVALID;
    }
    std::string why;
    if (hpfw::write_wav_pcm16(path, pcm, n, channels, why)) return 0;
    hpfw_internal_set_error(why.c_str());
    return why.rfind("wav write:", 0) == 0 ? HPFW_E_INVALID : HPFW_E_IO;
}

extern "C" int hpfw_gpu_collector_set_resample(hpfw_legacy_collector *c, int on)
{
    if (!c) {
        hpfw_internal_set_error("null collector");
        return HPFW_E_INVALID;
    }
    c->resample = on != 0;
    return 0;
}

static uint64_t *calc_hashprint_impl(hpfw_legacy_collector *c, const char *filename, int *size)
{
    if (size) *size = 0;
    if (!c || !filename || !size) return nullptr;
    std::vector<int16_t> pcm;
    std::string why;
    uint32_t rate = 44100;
    if (!read_clip(filename, pcm, why, c->resample ? &rate : nullptr)) {
        hpfw_internal_set_error(why.c_str());
        return nullptr;
    }
    if (rate != 44100) { // converted on the device first
        int64_t n_out = 0;
        if (hpfw_gpu_resample_length((int64_t)pcm.size(), (int)rate, &n_out) != 0) return nullptr;
        std::vector<int16_t> y((size_t)n_out);
        if (hpfw_gpu_resample_pcm16_host(c->gpu, pcm.data(), (int64_t)pcm.size(), 1, (int)rate, y.data()) != 0) return nullptr;
        pcm.swap(y);
    }
    hpfw_geometry g;
    if (hpfw_gpu_geometry(c->gpu, (int64_t)pcm.size(), &g) != 0) return nullptr;
    if (g.n_hp <= 0) {
        hpfw_internal_set_error((std::string(filename) + ": clip too short to yield a hashprint").c_str());
        return nullptr;
    }
    std::unique_ptr<uint64_t[]> hp(new uint64_t[(size_t)g.n_hp]);
    if (hpfw_gpu_extract_pcm16_host(c->gpu, pcm.data(), (int64_t)pcm.size(), 1, hp.get()) != 0) return nullptr;
    *size = (int)g.n_hp;
    return hp.release();
}

void calc_hashprint_result_free(uint64_t *hp) { delete[] hp; }

} // extern "C"

// ---- prepare(): files in windows, equally long clips batched through the device stages ----------
namespace {

struct Loaded {
    const int16_t *pcm = nullptr; // in the collector's pinned arena
    int64_t n = 0;                // samples (mono) as read
    uint32_t rate = 44100;        // their rate: other than 44.1 kHz only with the resampling switch on
    int64_t n_out = 0;            // samples at 44.1 kHz
    size_t arena_off = 0;         // byte offset of the clip in the arena (the device copy has the same layout)
    bool ok = false;
};

// One window of files into the collector's pinned arena, clips of equal length side by side (so that a group goes
// through the device stages as one batch, straight from the window's single host-to-device copy).  The reference
// reads its files on a taskflow pool (parallel_collector.h:95-108); here a team of host threads walks the headers, then
// reads the payloads into their slots.  The reader threads also prepare the host half of the tables of every length
// they meet (hpfw_gpu_prepare_length: a corpus of full-length tracks brings a new length with almost every file).
// Returns the bytes of the arena in use (0: nothing readable).
size_t read_window(hpfw_legacy_collector *c, int slot, const char **filenames, const std::vector<int> &files, size_t first, size_t last,
                   std::vector<Loaded> &out, std::string &first_why)
{
    const auto t_begin = Clock::now();
    std::mutex why_mtx;
    first_why.clear(); // error messages are thread-local and this runs on a thread of its own: the first failure goes back to the caller
    const int count = (int)(last - first);
    out.assign((size_t)count, Loaded());
    std::vector<WavProbe> probes((size_t)count);
    auto name = [&](int i) { return std::string(filenames[files[first + (size_t)i]]); };
    auto fail = [&](const std::string &why) {
        std::scoped_lock lock(why_mtx);
        if (first_why.empty()) first_why = why;
    };
    host_team(count, [&](int i) {
        WavProbe &w = probes[(size_t)i];
        std::string why;
        try {
            if (!hpfw::probe_wav(name(i), w, why, c->resample)) {
                fail(why);
            } else if (c->gpu) { // the tables of the length the extraction will see (too short: skipped later)
                int64_t n_out = w.frames;
                if (w.rate != 44100) (void)hpfw_gpu_resample_length(n_out, (int)w.rate, &n_out);
                (void)hpfw_gpu_prepare_length(c->gpu, n_out);
            }
        } catch (const std::exception &e) {
            fail(name(i) + ": " + e.what());
        }
    });
    const auto t_probe = Clock::now();
    // slots: by (rate, length), then input order; every group starts 16-byte aligned
    std::map<std::pair<uint32_t, int64_t>, std::vector<int>> by_len;
    for (int i = 0; i < count; ++i)
        if (probes[(size_t)i].ok() && probes[(size_t)i].frames > 0) by_len[{probes[(size_t)i].rate, probes[(size_t)i].frames}].push_back(i);
    size_t bytes = 0;
    for (auto &kv : by_len) {
        bytes = (bytes + 15) / 16 * 16;
        int64_t n_out = kv.first.second;
        if (kv.first.first != 44100) (void)hpfw_gpu_resample_length(n_out, (int)kv.first.first, &n_out);
        for (int i : kv.second) {
            out[(size_t)i].arena_off = bytes;
            out[(size_t)i].n = kv.first.second;
            out[(size_t)i].rate = kv.first.first;
            out[(size_t)i].n_out = n_out;
            bytes += (size_t)kv.first.second * 2;
        }
    }
    if (bytes > c->arena[slot].capacity() && c->arena[slot].alloc(std::max(bytes + bytes / 4, (size_t)64 << 20)) != hipSuccess) {
        first_why = "prepare: out of pinned host memory";
        return 0;
    }
    const unsigned team = host_team(count, [&](int i) {
        WavProbe &w = probes[(size_t)i];
        if (!w.ok() || w.frames <= 0) return;
        int16_t *dst = reinterpret_cast<int16_t *>(c->arena[slot].as<char>() + out[(size_t)i].arena_off);
        bool ok = false;
        try {
            ok = hpfw::read_mono(w, dst);
        } catch (const std::exception &) { // e.g. bad_alloc on a huge stereo file
        }
        w.close();
        if (!ok) fail(name(i) + ": short read");
        out[(size_t)i].pcm = dst;
        out[(size_t)i].ok = ok;
    });
    if (std::getenv("HPFW_FFI_TIMING"))
        std::fprintf(stderr, "[hpfw ffi]   reader: headers + tables of new lengths %.1f ms, payloads %.1f ms (%u threads)\n",
                     ms_between(t_begin, t_probe), ms_between(t_probe, Clock::now()), team);
    return bytes; // (skipped files, parallel_collector.h:101-103: first_why holds the message)
}

// the window's clips on the device: one copy of the arena (its layout is kept)
bool upload_window(hpfw_legacy_collector *c, int slot, size_t bytes)
{
    if (bytes > c->d_arena_buf[slot].capacity() && c->d_arena_buf[slot].alloc(std::max(bytes + bytes / 4, (size_t)64 << 20)) != hipSuccess) {
        hpfw_internal_set_error("prepare: out of device memory");
        return false;
    }
    c->d_arena = c->d_arena_buf[slot].get();
    return bytes == 0 || hipMemcpy(c->d_arena, c->arena[slot].get(), bytes, hipMemcpyHostToDevice) == hipSuccess;
}

// the n clips of a group at 44.1 kHz on the device, side by side from `first`: the device copy of the arena itself, or, for
// another rate, the collector's staging buffer after the conversion on stream s (NULL on failure)
const int16_t *group_pcm(hpfw_legacy_collector *c, const Loaded &first, size_t n, hipStream_t s)
{
    const int16_t *d_in = reinterpret_cast<const int16_t *>(static_cast<const char *>(c->d_arena) + first.arena_off);
    if (first.rate == 44100) return d_in;
    if (c->rs_stage.ensure(n * (size_t)first.n_out * 2) != hipSuccess) {
        hpfw_internal_set_error("prepare: out of device memory for the resampled clips");
        return nullptr;
    }
    if (hpfw_gpu_resample_pcm16(c->gpu, d_in, first.n, (int64_t)n, (int)first.rate, c->rs_stage.as<int16_t>(), s) != 0) return nullptr;
    return c->rs_stage.as<const int16_t>();
}

// dB spectrograms [n][121][C] of n equally long clips (side by side from d_pcm, on the device) into d_db (empty on entry),
// which is release_spectrograms' spare when that is large enough
bool group_spectrograms(hpfw_legacy_collector *c, const int16_t *d_pcm, size_t n, int64_t len, const hpfw_geometry &g, hpfw::DevBuf &d_db)
{
    const size_t need = n * (size_t)121 * g.c * 4;
    if (c->spare_db.capacity() >= need) {
        d_db = std::move(c->spare_db);
    } else if (d_db.alloc(need) != hipSuccess) {
        hpfw_internal_set_error("prepare: out of device memory");
        return false;
    }
    // (no synchronisation: what follows runs on the default stream too, and the copies to the host wait for it)
    return hpfw_gpu_stage_spectrogram(c->gpu, d_pcm, len, (int64_t)n, d_db.as<float>(), nullptr) == 0;
}

// a group's spectrogram buffer is done with: the larger of it and the spare stays for the next group
void release_spectrograms(hpfw_legacy_collector *c, hpfw::DevBuf d_db)
{
    if (d_db.capacity() > c->spare_db.capacity()) c->spare_db = std::move(d_db);
}

// the collector's hashprint buffers (device, and pinned on the host) hold at least `bytes`
bool ensure_hp_buffers(hpfw_legacy_collector *c, size_t bytes)
{
    if (bytes <= c->d_hp_win.capacity() && bytes <= c->h_hp_win.capacity()) return true;
    c->h_hp_win.reset(); // (both go before either is made again)
    const size_t want = std::max(bytes + bytes / 4, (size_t)8 << 20);
    if (c->d_hp_win.alloc(want) != hipSuccess || c->h_hp_win.alloc(want) != hipSuccess) {
        hpfw_internal_set_error("prepare: out of memory for the hashprints");
        return false;
    }
    return true;
}

// hashprints of a group of clips from their dB spectrograms (default stream): clip k's into hp[ids[k]]
bool group_hashprints(hpfw_legacy_collector *c, const float *d_db, const hpfw_geometry &g, const std::vector<int> &ids, std::vector<Hp> &hp)
{
    const size_t bytes = ids.size() * (size_t)g.n_hp * 8;
    if (!ensure_hp_buffers(c, bytes)) return false;
    if (hpfw_gpu_hashprints_from_db(c->gpu, d_db, (int64_t)ids.size(), g.c, c->d_hp_win.as<uint64_t>(), nullptr) != 0) return false;
    if (hipMemcpy(c->h_hp_win.get(), c->d_hp_win.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        hpfw_internal_set_error("prepare: D2H copy failed");
        return false;
    }
    for (size_t k = 0; k < ids.size(); ++k) hp[(size_t)ids[k]] = copy_hp(c->h_hp_win.as<const uint64_t>() + k * (size_t)g.n_hp, g.n_hp);
    return true;
}

struct KeptGroup {
    std::vector<int> files; // indices into the caller's list
    hpfw_geometry g;
    hpfw::DevBuf d_db;
};

// what a pass over files does with each spectrogram; neither: the direct path, PCM to hashprints on the collector's stream
struct PassMode {
    bool learn = false; // its covariance is added to accum_cov, and it is kept on the device for the hashprints
    bool cache = false; // it is written to <cache>/spectros/
    bool direct() const { return !learn && !cache; }
};

} // namespace

// ParallelCollector::prepare (parallel_collector.h:48-52): preprocess (:82-112) adds every file's
// frame covariance to accum_cov, takes the 64 leading eigenvectors as the new filters and saves them;
// collect_fingerprints (:114-137) then turns the cached spectrograms into hashprints.  Here the
// spectrograms stay in device memory between the two steps (up to HPFW_PREPARE_KEEP_GB, default 32;
// files beyond that are read and transformed again), the files are read in windows by a team of
// host threads, and clips of equal length go through the device stages together.  Per-file errors are
// skipped as the reference does (:101-103), so *got may be < n; results keep the input order; the name
// is the stem of the path (:123,129).  HPFW_PREPARE_KEEP_FILTERS=1 skips the learning step and keeps
// the filters that load() / a previous prepare() installed.
// The two halves of prepare() around the point where the filters are learned: accumulate() is preprocess()'s
// parallel_for (parallel_collector.h:85-105: spectrogram, covariance into accum_cov, spectrogram cached),
// finish() is collect_fingerprints (:115-137) for the files of this call.  Between the two the caller learns the
// filters -- from this collector's accum_cov alone (collect_files) or from the sum over the collectors of a
// multi-GPU group (hpfw_gpu_group_prepare, multi.cpp).
struct hpfw_prepare_job {
    std::vector<Hp> hp; // one per file of the call
    std::vector<KeptGroup> kept;
    std::vector<int> again; // files whose spectrogram could not be kept
    size_t kept_bytes = 0;
    int64_t used = 0;
    PassMode mode; // of the first pass
};

namespace {

// the windows [first, second) of a pass: at most 256 files and about 1 GiB of audio each
std::vector<std::pair<size_t, size_t>> plan_windows(const char **filenames, const std::vector<int> &files)
{
    std::vector<std::pair<size_t, size_t>> windows;
    for (size_t at = 0; at < files.size();) {
        size_t end = at;
        uintmax_t bytes = 0;
        while (end < files.size() && end - at < 256 && (end == at || bytes < ((uintmax_t)1 << 30))) {
            std::error_code ec;
            const uintmax_t sz = std::filesystem::file_size(filenames[files[end]], ec);
            if (!ec) bytes += sz;
            ++end;
        }
        windows.emplace_back(at, end);
        at = end;
    }
    return windows;
}

// The groups of a window: positions of clips of one (rate, length), by (rate, length), in input order.  A group whose
// files were all read lies side by side in the arena; one with a failed read in its middle is cut into its contiguous runs
std::vector<std::vector<int>> contiguous_runs(const std::vector<Loaded> &clips)
{
    std::map<std::pair<uint32_t, int64_t>, std::vector<int>> all;
    for (size_t i = 0; i < clips.size(); ++i)
        if (clips[i].n > 0) all[{clips[i].rate, clips[i].n}].push_back((int)i);
    std::vector<std::vector<int>> runs;
    for (auto &kv : all) {
        std::vector<int> run;
        for (int i : kv.second) {
            if (clips[(size_t)i].ok) {
                run.push_back(i);
            } else if (!run.empty()) {
                runs.push_back(run);
                run.clear();
            }
        }
        if (!run.empty()) runs.push_back(run);
    }
    return runs;
}

// The direct path (nothing learned, nothing cached: calc_hashprints, and the second pass of prepare()): every group of
// window w goes straight from its PCM to hashprints in one buffer for the window, enqueued on the collector's stream
// with one copy to the host behind them; the hashprints are fetched only after window w + 1 has been uploaded -- the
// upload runs under the kernels
struct Pending {
    struct Part {
        std::vector<int> pos; // positions of the group's clips in the window
        hpfw_geometry g;
        size_t off;           // hashprints before this group in the window's buffer
        bool done;
    };
    bool active = false, ok = true;
    std::vector<Part> parts;
    size_t total = 0, at = 0; // hashprints of the window; its first file in the pass
};

void enqueue_direct(hpfw_legacy_collector *c, const std::vector<Loaded> &clips, const std::vector<std::vector<int>> &runs, size_t at,
                    Pending &pend)
{
    pend.parts.clear();
    pend.total = 0;
    pend.at = at;
    size_t stage = 0; // the resampled clips of the largest group at another rate (one buffer, reused in stream order)
    for (const std::vector<int> &pos : runs) {
        hpfw_geometry g;
        const Loaded &l0 = clips[(size_t)pos[0]];
        if (hpfw_gpu_geometry(c->gpu, l0.n_out, &g) != 0 || g.n_frames < 2 || g.n_hp <= 0) continue; // skipped
        pend.parts.push_back(Pending::Part{pos, g, pend.total, false});
        pend.total += pos.size() * (size_t)g.n_hp;
        if (l0.rate != 44100) stage = std::max(stage, pos.size() * (size_t)l0.n_out * 2);
    }
    bool ok = ensure_hp_buffers(c, pend.total * 8);
    if (ok && stage && c->rs_stage.ensure(stage) != hipSuccess) {
        hpfw_internal_set_error("prepare: out of device memory for the resampled clips");
        ok = false;
    }
    if (ok && !c->win_stream && c->win_stream.create() != hipSuccess) {
        hpfw_internal_set_error("prepare: no stream");
        ok = false;
    }
    const auto t_enq = Clock::now();
    for (size_t k = 0; ok && k < pend.parts.size(); ++k) {
        Pending::Part &pt = pend.parts[k];
        const Loaded &l0 = clips[(size_t)pt.pos[0]];
        const int16_t *d_pcm = group_pcm(c, l0, pt.pos.size(), c->win_stream.get());
        pt.done = d_pcm && hpfw_gpu_extract_pcm16(c->gpu, d_pcm, l0.n_out, (int64_t)pt.pos.size(), c->d_hp_win.as<uint64_t>() + pt.off,
                                                  c->win_stream.get()) == 0; // a failed group is skipped
    }
    if (ok && pend.total > 0 &&
        hipMemcpyAsync(c->h_hp_win.get(), c->d_hp_win.get(), pend.total * 8, hipMemcpyDeviceToHost, c->win_stream.get()) != hipSuccess) {
        hpfw_internal_set_error("prepare: D2H copy failed");
        ok = false;
    }
    if (std::getenv("HPFW_FFI_TIMING"))
        std::fprintf(stderr, "[hpfw ffi]   %zu groups enqueued in %.1f ms (tables of new lengths included)\n", pend.parts.size(),
                     ms_between(t_enq, Clock::now()));
    pend.ok = ok;
    pend.active = true; // fetched by fetch_direct: after the next window's upload, or after the last window
}

// the results of the window whose kernels are in flight (if any), into hp[files[...]]
void fetch_direct(hpfw_legacy_collector *c, Pending &pend, const std::vector<int> &files, std::vector<Hp> &hp)
{
    if (!pend.active) return;
    pend.active = false;
    if (c->win_stream && hipStreamSynchronize(c->win_stream.get()) != hipSuccess) {
        hpfw_internal_set_error("prepare: the window's kernels failed");
        pend.ok = false;
    } else if (c->win_stream) {
        // everything this collector has queued on its handle ran on that stream (the tables' stream and the side streams
        // are joined into it), and the next window's groups are queued only after this point
        hpfw_internal_note_idle(c->gpu);
    }
    for (size_t k = 0; pend.ok && k < pend.parts.size(); ++k) {
        const Pending::Part &pt = pend.parts[k];
        if (!pt.done) continue;
        for (size_t q = 0; q < pt.pos.size(); ++q)
            hp[(size_t)files[pend.at + (size_t)pt.pos[q]]] = copy_hp(c->h_hp_win.as<const uint64_t>() + pt.off + q * (size_t)pt.g.n_hp, pt.g.n_hp);
    }
}

// the window's spectrograms on their way to cache/spectros/: one pinned buffer (the collector's h_spec) for all of them,
// written to the cache by the team of host threads when the window's groups are through (a window of files of different
// lengths is as many groups of one file: written group by group, one thread would do all the writing)
struct SpecWrites {
    struct Item {
        std::string path;
        size_t off; // floats into the pinned buffer
        int32_t c;
    };
    std::vector<Item> items;
    size_t used = 0; // bytes of the pinned buffer
};

// the pinned buffer holds the spectrograms of all the window's groups (left as it is when it cannot grow: run_staged
// then caches what fits)
void reserve_spectrograms(hpfw_legacy_collector *c, const std::vector<Loaded> &clips, const std::vector<std::vector<int>> &runs)
{
    size_t total = 0;
    for (const std::vector<int> &pos : runs) {
        hpfw_geometry g;
        if (hpfw_gpu_geometry(c->gpu, clips[(size_t)pos[0]].n_out, &g) == 0 && g.n_frames >= 2) total += pos.size() * (size_t)121 * g.c * 4;
    }
    if (total > c->h_spec.capacity()) // (pinned: the copies run at the link's rate, not through the driver's staging)
        (void)c->h_spec.alloc(total + total / 8);
}

void write_spectrograms(hpfw_legacy_collector *c, const SpecWrites &sw)
{
    const float *host = c->h_spec.as<const float>();
    host_team((int)sw.items.size(), [&](int k) {
        const SpecWrites::Item &it = sw.items[(size_t)k];
        (void)hpfw::save_spectro_cereal(it.path, host + it.off, it.c);
    });
}

// The staged path, on the default stream: one group (the clips `first` and the n - 1 behind it in the arena, files `ids`
// of the call) through its spectrograms, then as the mode says: a copy for the cache, the covariance, and the
// spectrograms kept for prepare_finish (or the files noted to be read again) -- or, nothing being learned, the hashprints
void run_staged(hpfw_legacy_collector *c, const char **filenames, const Loaded &first, const std::vector<int> &ids, PassMode mode,
                size_t keep_budget, SpecWrites &sw, hpfw_prepare_job &job)
{
    const size_t n = ids.size();
    const int64_t len = first.n_out; // (at 44.1 kHz)
    hpfw_geometry g;
    if (hpfw_gpu_geometry(c->gpu, len, &g) != 0 || g.n_frames < 2) return; // skipped
    hpfw::DevBuf d_db;
    const int16_t *d_pcm = group_pcm(c, first, n, nullptr);
    if (!d_pcm || !group_spectrograms(c, d_pcm, n, len, g, d_db)) return;
    const size_t sz = n * (size_t)121 * g.c * 4;
    // cache.set_spectro(filename, spectro) (parallel_collector.h:98-100): "it will also be needed
    // when adding new tracks" -- a later prepare() recomputes every cached track's hashprints
    if (mode.cache && c->h_spec && sw.used + sz <= c->h_spec.capacity() &&
        hipMemcpy(c->h_spec.as<char>() + sw.used, d_db.get(), sz, hipMemcpyDeviceToHost) == hipSuccess) {
        for (size_t k = 0; k < n; ++k)
            sw.items.push_back(SpecWrites::Item{c->cache_dir + "spectros/" + stem_of(filenames[ids[k]]), sw.used / 4 + k * (size_t)121 * g.c, (int32_t)g.c});
        sw.used += sz;
    }
    if (mode.learn) {
        if (hpfw_gpu_cov_accumulate_db(c->gpu, d_db.as<float>(), (int64_t)n, g.c, nullptr) == 0) job.used += (int64_t)n;
        if (g.n_hp > 0 && job.kept_bytes + sz <= keep_budget) {
            job.kept.push_back(KeptGroup{ids, g, std::move(d_db)});
            job.kept_bytes += sz;
            return;
        }
        if (g.n_hp > 0) job.again.insert(job.again.end(), ids.begin(), ids.end());
    } else if (g.n_hp > 0) {
        (void)group_hashprints(c, d_db.as<float>(), g, ids, job.hp);
    }
    release_spectrograms(c, std::move(d_db)); // (its next user is ordered after this group on the default stream; hipFree waits)
}

// one pass over `files` (indices into filenames, results into job.hp at the same indices)
void prepare_pass(hpfw_legacy_collector *c, const char **filenames, hpfw_prepare_job &job, const std::vector<int> &files, PassMode mode)
{
    size_t keep_budget = (size_t)32 << 30;
    if (const char *e = std::getenv("HPFW_PREPARE_KEEP_GB")) keep_budget = (size_t)std::max(0.0, std::atof(e) * 1073741824.0);
    const int device = hpfw_gpu_device(c->gpu);
    (void)hipSetDevice(device);
    const std::vector<std::pair<size_t, size_t>> windows = plan_windows(filenames, files);
    // window w + 1 is read (into the other arena) by a task of its own while window w is copied and extracted
    struct Read {
        std::vector<Loaded> clips;
        size_t used = 0;
        double ms = 0.0;
        std::string why;
    };
    auto start_read = [&](size_t w) {
        return std::async(std::launch::async, [&, w] {
            Read r;
            const auto t_a = Clock::now();
            (void)hipSetDevice(device);
            r.used = read_window(c, (int)(w & 1), filenames, files, windows[w].first, windows[w].second, r.clips, r.why);
            r.ms = ms_between(t_a, Clock::now());
            return r;
        });
    };
    const bool timing = std::getenv("HPFW_FFI_TIMING") != nullptr; // where a window's time goes, on stderr
    Pending pend;
    std::future<Read> ahead;
    if (!windows.empty()) ahead = start_read(0);
    for (size_t w = 0; w < windows.size(); ++w) {
        const size_t at = windows[w].first, end = windows[w].second;
        const auto t_0 = Clock::now();
        Read got = ahead.get();
        if (!got.why.empty()) hpfw_internal_set_error(got.why.c_str()); // the message survives the skipped files
        if (w + 1 < windows.size()) ahead = start_read(w + 1);
        const auto t_1 = Clock::now();
        if (!upload_window(c, (int)(w & 1), got.used)) {
            if (ahead.valid()) (void)ahead.get(); // the task works on this function's state: it ends before we return
            break;
        }
        fetch_direct(c, pend, files, job.hp); // (the previous window's kernels ran under this upload)
        const auto t_2 = Clock::now();
        const std::vector<std::vector<int>> runs = contiguous_runs(got.clips);
        if (mode.direct()) {
            enqueue_direct(c, got.clips, runs, at, pend);
        } else {
            SpecWrites sw;
            if (mode.cache) reserve_spectrograms(c, got.clips, runs);
            for (const std::vector<int> &pos : runs) {
                std::vector<int> ids;
                for (int q : pos) ids.push_back(files[at + (size_t)q]);
                run_staged(c, filenames, got.clips[(size_t)pos[0]], ids, mode, keep_budget, sw, job);
            }
            write_spectrograms(c, sw);
        }
        if (timing)
            std::fprintf(stderr, "[hpfw ffi] window of %zu files, %.1f MB: read %.1f ms (waited %.1f ms), upload %.1f ms, device + results %.1f ms\n",
                         end - at, got.used / 1e6, got.ms, ms_between(t_0, t_1), ms_between(t_1, t_2), ms_between(t_2, Clock::now()));
    }
    fetch_direct(c, pend, files, job.hp);
}

void prepare_accumulate(hpfw_legacy_collector *c, const char **filenames, int n, hpfw_prepare_job &job)
{
    if (job.mode.cache) {
        std::error_code ec;
        std::filesystem::create_directories(c->cache_dir + "spectros/", ec);
    }
    job.hp.clear();
    job.hp.resize((size_t)n);
    std::vector<int> all((size_t)n);
    for (int i = 0; i < n; ++i) all[(size_t)i] = i;
    prepare_pass(c, filenames, job, all, job.mode);
}

// hashprints of the spectrograms kept on the device, then of the files that have to be read again (the direct path);
// ok = false: the filters could not be learned -- release what was kept and produce nothing
void prepare_finish(hpfw_legacy_collector *c, const char **filenames, hpfw_prepare_job &job, bool ok)
{
    (void)hipSetDevice(hpfw_gpu_device(c->gpu));
    for (KeptGroup &k : job.kept)
        if (ok) (void)group_hashprints(c, k.d_db.as<float>(), k.g, k.files, job.hp);
    job.kept.clear();
    if (ok && !job.again.empty()) {
        std::sort(job.again.begin(), job.again.end());
        prepare_pass(c, filenames, job, job.again, PassMode{});
    }
}

// both halves on this collector alone; false: the filters could not be learned
bool collect_files(hpfw_legacy_collector *c, const char **filenames, int n, PassMode mode, std::vector<Hp> &hp)
{
    hpfw_prepare_job job;
    job.mode = mode;
    prepare_accumulate(c, filenames, n, job);
    bool failed = false;
    if (mode.learn) {
        if (job.used > 0) {
            c->filters.assign((size_t)HPFW_FILTERS * HPFW_FRAME_SIZE, 0.0f);
            if (hpfw_gpu_learn_filters(c->gpu, c->filters.data()) != 0) {
                c->filters.clear();
                failed = true;
            } else {
                par_collector_save(c, nullptr);
            }
        }
        prepare_finish(c, filenames, job, !failed);
    }
    hp.swap(job.hp);
    return !failed;
}

// collect_fingerprints (parallel_collector.h:114-137) walks EVERY spectrogram under cache/spectros/, not only
// the files of this call: tracks indexed by an earlier run come back with hashprints under the filters just
// learned.  The files of this call are already done (their spectrograms never left the device); this adds the
// others: read by a team of host threads, grouped by width, projected and packed on the GPU.
void collect_cached(hpfw_legacy_collector *c, const std::vector<std::string> &done_stems, std::vector<std::string> &stems, std::vector<Hp> &hp)
{
    std::error_code ec;
    std::vector<std::string> paths;
    const std::unordered_set<std::string> done(done_stems.begin(), done_stems.end()); // a 100 k-track cache: no quadratic scan
    for (const auto &e : std::filesystem::directory_iterator(c->cache_dir + "spectros/", ec)) {
        if (!e.is_regular_file(ec)) continue;
        // the cache names its files by the track's stem (cache.h:30-33); the name returned is that file name as it is.
        // (The reference returns path(cache file).stem() -- parallel_collector.h:123 -- i.e. a second stem: "a.b.wav" is
        // cached as "a.b" and comes back as "a" there, as "a.b" here; INTEGRATION.md notes the deviation.)
        if (!done.count(e.path().filename().string())) paths.push_back(e.path().string());
    }
    std::sort(paths.begin(), paths.end()); // the reference's order is the directory's (and racy, :129): sorted here
    for (size_t at = 0; at < paths.size();) {
        const size_t end = std::min(paths.size(), at + 256);
        struct Item {
            std::vector<float> cm;
            int32_t cols = 0;
            bool ok = false;
        };
        std::vector<Item> items(end - at);
        host_team((int)items.size(), [&](int i) { items[(size_t)i].ok = hpfw::load_spectro_cereal(paths[at + (size_t)i], items[(size_t)i].cm, items[(size_t)i].cols); });
        std::vector<Hp> win_hp(items.size());
        std::map<int32_t, std::vector<int>> by_cols;
        for (size_t i = 0; i < items.size(); ++i)
            if (items[i].ok && items[i].cols >= HPFW_CONTEXT + HPFW_LAG) by_cols[items[i].cols].push_back((int)i);
        for (auto &kv : by_cols) {
            const int32_t cols = kv.first;
            const std::vector<int> &pos = kv.second;
            hpfw_geometry g{};
            g.c = cols;
            g.n_frames = cols - (HPFW_CONTEXT - 1);
            g.n_hp = g.n_frames - HPFW_LAG;
            std::vector<float> bm(pos.size() * (size_t)HPFW_BINS * cols);
            host_team((int)pos.size(), [&](int k) {
                const float *cm = items[(size_t)pos[(size_t)k]].cm.data();
                float *out = bm.data() + (size_t)k * HPFW_BINS * cols;
                for (int32_t col = 0; col < cols; ++col)
                    for (int32_t b = 0; b < HPFW_BINS; ++b) out[(size_t)b * cols + col] = cm[(size_t)col * HPFW_BINS + b];
            });
            hpfw::DevBuf d_db;
            if (d_db.alloc(bm.size() * 4) == hipSuccess && hipMemcpy(d_db.get(), bm.data(), bm.size() * 4, hipMemcpyHostToDevice) == hipSuccess)
                (void)group_hashprints(c, d_db.as<float>(), g, pos, win_hp);
        }
        for (size_t i = 0; i < items.size(); ++i) { // groups ran by width; the results keep the sorted order
            if (!win_hp[i].bits) continue;
            stems.push_back(std::filesystem::path(paths[at + i]).filename().string());
            hp.push_back(std::move(win_hp[i]));
        }
        at = end;
    }
}

// What prepare() returns: the files of the call that yielded hashprints, in input order; then, with_cached, every other
// track of the cache, sorted -- other than those returned (the single collector), or, skip_all_named, other than all
// the n named files (a group: the names are all the shards' files, whose hashprints the shards produce)
FilenameHashprintPair *prepare_result(hpfw_legacy_collector *c, const char **filenames, int n, std::vector<Hp> &hp, bool with_cached,
                                      bool skip_all_named, int *got)
{
    std::vector<std::string> stems, done;
    std::vector<Hp> out;
    for (int i = 0; i < n; ++i) {
        const bool has = (size_t)i < hp.size() && hp[(size_t)i].bits;
        if (has || skip_all_named) done.push_back(stem_of(filenames[i]));
        if (!has) continue;
        stems.push_back(done.back());
        out.push_back(std::move(hp[(size_t)i]));
    }
    if (with_cached) collect_cached(c, done, stems, out);
    FilenameHashprintPair *res = make_result(stems, out);
    *got = (int)stems.size();
    return res;
}

} // namespace

static FilenameHashprintPair *prepare_impl(hpfw_legacy_collector *c, const char **filenames, int n, int *got)
{
    if (got) *got = 0;
    if (!c || !filenames || n < 0 || !got) return nullptr;
    PassMode mode;
    mode.learn = !(std::getenv("HPFW_PREPARE_KEEP_FILTERS") && !c->filters.empty());
    mode.cache = !std::getenv("HPFW_NO_SPECTRO_CACHE");
    std::vector<Hp> hp;
    if (!collect_files(c, filenames, n, mode, hp)) return nullptr;
    return prepare_result(c, filenames, n, hp, mode.cache, false, got);
}

// calc_hashprint (parallel_collector.h:54-59) for a list of files in one call, as LiveSongIdentification::search
// needs it for its queries (live_song_id.h:37-41): the files are read and transformed in batches as in
// prepare(), nothing is learned.  Returns n entries in input order, released with prepare_result_free(res, n);
// an entry whose file failed has hashprint == NULL and hp_size == 0.  NULL when no filters are loaded.
static FilenameHashprintPair *calc_hashprints_impl(hpfw_legacy_collector *c, const char **filenames, int n)
{
    if (!c || !filenames || n < 0) return nullptr;
    if (c->filters.empty()) {
        hpfw_internal_set_error("no filters loaded: call par_collector_load or par_collector_prepare first");
        return nullptr;
    }
    std::vector<Hp> hp;
    if (!collect_files(c, filenames, n, PassMode{}, hp)) return nullptr;
    std::vector<std::string> stems;
    for (int i = 0; i < n; ++i) stems.push_back(stem_of(filenames[i]));
    return make_result(stems, hp);
}

extern "C" {

uint64_t *par_collector_calc_hashprint(hpfw_legacy_collector *c, const char *filename, int *size)
{
    return guarded([&] { return calc_hashprint_impl(c, filename, size); });
}

FilenameHashprintPair *par_collector_prepare(hpfw_legacy_collector *c, const char **filenames, int n, int *got)
{
    FilenameHashprintPair *res = guarded([&] { return prepare_impl(c, filenames, n, got); });
    if (!res && got) *got = 0;
    return res;
}

FilenameHashprintPair *par_collector_calc_hashprints(hpfw_legacy_collector *c, const char **filenames, int n)
{
    return guarded([&] { return calc_hashprints_impl(c, filenames, n); });
}

// ---- the halves of prepare() for a multi-GPU host (libhpfw_gpu_multi.so; declared in legacy_internal.h) ----
hpfw_legacy_collector *hpfw_internal_collector_on_device(int device, const char *cache)
{
    auto *c = new hpfw_legacy_collector();
    if (hpfw_gpu_create(device, &c->gpu) != 0) {
        delete c;
        return nullptr;
    }
    par_collector_load(c, cache);
    return c;
}

hpfw_gpu *hpfw_internal_collector_gpu(hpfw_legacy_collector *c) { return c ? c->gpu : nullptr; }

int hpfw_internal_collector_set_filters(hpfw_legacy_collector *c, const float *f)
{
    if (!c || !f) return HPFW_E_INVALID;
    c->filters.assign(f, f + (size_t)HPFW_FILTERS * HPFW_FRAME_SIZE);
    return hpfw_gpu_set_filters(c->gpu, f);
}

hpfw_prepare_job *hpfw_internal_prepare_accumulate(hpfw_legacy_collector *c, const char **filenames, int n, int learn)
{
    return guarded([&]() -> hpfw_prepare_job * {
        if (!c || !filenames || n < 0) return nullptr;
        auto job = std::make_unique<hpfw_prepare_job>();
        job->mode.learn = learn != 0;
        job->mode.cache = !std::getenv("HPFW_NO_SPECTRO_CACHE");
        prepare_accumulate(c, filenames, n, *job);
        return job.release();
    });
}

int64_t hpfw_internal_prepare_used(const hpfw_prepare_job *job) { return job ? job->used : 0; }

// hashprints of the job's files (input order, failed files dropped) [+ with_cached: every other spectrogram of
// the cache, sorted by name]; consumes the job.  ok = 0: learning failed, release and return NULL.
FilenameHashprintPair *hpfw_internal_prepare_finish(hpfw_legacy_collector *c, hpfw_prepare_job *job_in, const char **filenames, int n,
                                                    int ok, int with_cached, int *got)
{
    if (got) *got = 0;
    const std::unique_ptr<hpfw_prepare_job> job(job_in);
    return guarded([&]() -> FilenameHashprintPair * {
        if (!c || !job || !got) return nullptr;
        if (job->mode.learn || !ok) prepare_finish(c, filenames, *job, ok != 0);
        if (!ok) return nullptr;
        return prepare_result(c, filenames, n, job->hp, with_cached && job->mode.cache, true, got);
    });
}

// the tracks of the cache other than the n named files (whose hashprints the shards have just produced), sorted
FilenameHashprintPair *hpfw_internal_prepare_finish_cached(hpfw_legacy_collector *c, const char **filenames, int n, int *got)
{
    if (got) *got = 0;
    return guarded([&]() -> FilenameHashprintPair * {
        if (!c || !got) return nullptr;
        (void)hipSetDevice(hpfw_gpu_device(c->gpu));
        std::vector<Hp> none;
        return prepare_result(c, filenames, n, none, true, true, got);
    });
}

void prepare_result_free(FilenameHashprintPair *res, int got)
{
    if (!res) return;
    for (int i = 0; i < got; ++i) {
        delete[] res[i].filename;
        delete[] res[i].hashprint;
    }
    delete[] res;
}

} // extern "C"
