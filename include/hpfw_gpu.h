/*
 * hpfw_gpu.h -- C-ABI of the MI355X (gfx950) hashprint hot path: the drop-in boundary.
 *
 * What it replaces (paths relative to the hpfw reference tree):
 *   extraction  ParallelCollector::calc_hashprint / collect_fingerprints
 *               include/hpfw/core/parallel_collector.h:54-59, 115-137, i.e.
 *               CQT<>::spectrogram            include/hpfw/spectrum/cqt.h:36-84
 *               amplitude_to_db/power_to_db   include/hpfw/spectrum/convert.h:7-25
 *               calc_frames, filters*frames, calc_fingerprint, fingerprint_to_hashprint
 *                                             include/hpfw/core/hashprint_handle.h:79-142
 *   search      MemoryStorage::build / find   include/hpfw/audioproblems/live-song-id/storage.h:21-64
 *               and the notebook's top-10 rule examples/python/liveid.ipynb cell 9
 *   legacy FFI  the eight extern "C" symbols of modules/python/parallel_collector_wrapper.hpp:21-38
 *               (declared at the end of this file with the same shapes)
 *
 * Conventions
 *   - plain C, no C++ or torch types; every function returns 0 on success and a negative
 *     hpfw_status otherwise and never throws; hpfw_gpu_last_error() returns a thread-local
 *     message for the last failure on the calling thread.
 *   - pointers named d_* are DEVICE pointers (HBM) on the handle's device; all others are host
 *     pointers.  `stream` is a hipStream_t passed as void* (NULL = the default stream); device
 *     entry points only enqueue work on it and return without synchronising.
 *   - a handle may be used by one host thread at a time.
 *   - layouts: PCM is int16 mono 44.1 kHz, clips of equal length back to back;
 *     spectrograms are bin-major [121][C] (the reference's Eigen matrix is column-major 121 x C:
 *     element (b, c) at b + 121 c; ours is at b * C + c); filters are the reference's
 *     Matrix<float,64,Dynamic> column-major: element (r, k) at r + 64 k, k = bin * 20 + t;
 *     hashprints are uint64, bit (63 - r) <-> filter row r (hashprint_handle.h:137-142).
 */
#ifndef HPFW_GPU_H
#define HPFW_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPFW_BINS 121     /* cqt.h:21 NumberBins                      */
#define HPFW_CONTEXT 20   /* live_song_id.h:16 FramesContext          */
#define HPFW_LAG 80       /* live_song_id.h:16 T                      */
#define HPFW_FILTERS 64   /* hashprint_handle.h:64 sizeof(uint64_t)*8 */
#define HPFW_FRAME_SIZE (HPFW_BINS * HPFW_CONTEXT)

typedef enum {
    HPFW_OK = 0,
    HPFW_E_INVALID = -1,     /* bad argument                                       */
    HPFW_E_UNSUPPORTED = -2, /* clip too short (below ~1.3 s) or too long (~18 min) */
    HPFW_E_NOFILTERS = -3,   /* extraction before hpfw_gpu_set_filters             */
    HPFW_E_HIP = -4,         /* a HIP runtime call failed (message has the detail) */
    HPFW_E_NOMEM = -5,
    HPFW_E_IO = -6           /* legacy file entry points: unreadable / unsupported WAV */
} hpfw_status;

typedef struct hpfw_gpu hpfw_gpu; /* opaque */

/* geometry of clips of n_samples samples: essentia NSGConstantQ as configured at cqt.h:54-61 */
typedef struct {
    int64_t n_samples;
    int64_t n1, n2;   /* forward transform split N = n1 * n2                       */
    int64_t kmin, kmax; /* forward DFT bins [kmin, kmax) consumed by the 121 bands  */
    int64_t m;        /* M: inverse transform length of every band                 */
    int64_t c;        /* spectrogram columns ceil(M / 3)                           */
    int64_t n_frames; /* c - 19    hashprint_handle.h:84                           */
    int64_t n_hp;     /* c - 99    hashprint_handle.h:118                          */
} hpfw_geometry;

/* one search result; SearchResult{filename, cnt, offset} of storage.h:11-15 with the filename
 * replaced by the clip's index in hpfw_gpu_index_add order */
typedef struct {
    uint32_t dist;   /* sum of popcounts over the query                  */
    uint32_t clip;   /* clip_base + index in add order; 0xffffffff = none */
    int32_t offset;  /* first offset reaching dist (storage.h:50-53)      */
    uint32_t pad;
} hpfw_hit;

const char *hpfw_gpu_last_error(void);
const char *hpfw_gpu_version(void);

/* Environment read when a handle is created (tests and timing; results are the same bits either way): HPFW_DB_TERM=spec --
 * dB terms by the specified sequence alone; HPFW_PRUNE=<mask>, default 1 -- bit 0: the forward transform's row stage leaves
 * out the outputs of its last pass that hold no consumed bin where the clip length allows it, 0: every output is formed. */
int hpfw_gpu_create(int device, hpfw_gpu **out);
void hpfw_gpu_destroy(hpfw_gpu *h);
int hpfw_gpu_device(const hpfw_gpu *h); /* the device ordinal the handle was created on */

/* filters = ParallelCollector::filters (parallel_collector.h:77), host pointer, 64 x 2420 floats */
int hpfw_gpu_set_filters(hpfw_gpu *h, const float *filters_colmajor);
/* the filters the handle holds (set, learned, or read from a cache by its collector), same layout; HPFW_E_NOFILTERS when none */
int hpfw_gpu_get_filters(hpfw_gpu *h, float *filters_colmajor_out);
/* the sizes of a clip length (columns, frames, hashprints: cqt.h:66-73, hashprint_handle.h:79-93).  Host arithmetic only:
 * no table of the length is built or uploaded for the question; a length the extraction would refuse (a factor n2 beyond
 * the LDS) is refused here with the same status.  Like every entry point but hpfw_gpu_prepare_length it belongs to the one
 * host thread that drives the handle. */
int hpfw_gpu_geometry(hpfw_gpu *h, int64_t n_samples, hpfw_geometry *out);

/* essentia's NSGConstantQ is not vendored with hpfw and its version is not pinned (CMakeLists.txt:36), so four of
 * its conventions are restated from the published algorithm and cannot be checked offline (DESIGN.md appendix
 * A).  They are switchable per handle: a maintainer holding one real essentia output can pin them without
 * touching a kernel (the tables of every clip length are rebuilt).  0 = the defaults. */
#define HPFW_CONV_HANN_PERIODIC 1u  /* window 0.5 - 0.5 cos(2 pi i / L) instead of 2 pi i / (L - 1)                 */
#define HPFW_CONV_LG_HALF_EVEN 2u   /* Lg = round-half-to-even(bw / fftres) instead of round-half-away-from-zero   */
#define HPFW_CONV_FLOAT_GEOMETRY 4u /* fftres, f_j, posit_j, Lg_j evaluated in float (essentia's Real), not double */
#define HPFW_CONV_NO_IFFT_SCALE 8u  /* band transforms without the inverse FFT's 1/M (seen only by the 1e-10 floor) */
int hpfw_gpu_set_conventions(hpfw_gpu *h, unsigned flags);

/* ---- extraction: calc_hashprint for n_clips clips of n_samples samples each ------------- */
/* d_hp receives [n_clips][n_hp] */
int hpfw_gpu_extract_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                           uint64_t *d_hp, void *stream);
/* host buffers; copies in, runs, copies out, synchronises */
int hpfw_gpu_extract_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips,
                                uint64_t *hp);
/* clips processed per internal pass at most (workspace = ~9.5 MB per clip at 30 s; a call splits into passes of equal size); 0 = default (256) */
int hpfw_gpu_set_batch(hpfw_gpu *h, int clips_per_pass);

/* The smallest supported clip length >= n_samples, or -1 beyond the longest supported clip.  Host-only.
 * Any length between the shortest clip that yields a hashprint (54 254 samples, 1.23 s) and the longest the
 * tables allow is supported as it is -- the reference hands the file's exact sample count to NSGConstantQ
 * (cqt.h:54-55): 7-smooth lengths (every multiple of 1/7 s at 44.1 kHz among them) take the mixed-radix forward
 * transform, all others the chirp-z (Bluestein) one, about three times slower.  Nothing is padded. */
int64_t hpfw_gpu_supported_length(int64_t n_samples);

/* ---- per-stage entry points (parity checkpoints; same kernels the full chain runs) ------- */
/* PCM -> forward DFT bins [kmin,kmax): d_x [n_clips][kmax-kmin][2]           cqt.h:45-52,66 */
int hpfw_gpu_stage_spectrum(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                            float *d_x, void *stream);
/* bins -> |c_j[3c]|: d_mag [n_clips][121][C]                                  cqt.h:66-81 */
int hpfw_gpu_stage_cqmag(hpfw_gpu *h, const float *d_x, int64_t n_samples, int64_t n_clips,
                         float *d_mag, void *stream);
/* amplitude_to_db, per clip: d_mag, d_db [n_clips][121][C] (may alias)        convert.h:7-25 */
int hpfw_gpu_stage_db(hpfw_gpu *h, const float *d_mag, int64_t n_clips, int64_t c, float *d_db,
                      void *stream);
/* filters * calc_frames(S): d_proj [n_clips][64][C-19]       hashprint_handle.h:79-93 + :57 */
int hpfw_gpu_stage_project(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c,
                           float *d_proj, void *stream);
/* calc_fingerprint + fingerprint_to_hashprint: d_hp [n_clips][n_frames-80]   :115-142 */
int hpfw_gpu_stage_pack(hpfw_gpu *h, const float *d_proj, int64_t n_clips, int64_t n_frames,
                        uint64_t *d_hp, void *stream);

/* PCM -> dB spectrogram through the front end exactly as extraction runs it (the chirp-z kernel
 * writes dB terms, the reference level is applied afterwards): d_db [n_clips][121][C]
 *                                                              cqt.h:45-81 + convert.h:7-25 */
int hpfw_gpu_stage_spectrogram(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples,
                               int64_t n_clips, float *d_db, void *stream);

/* ---- Mel front-end: spectrum::MelSpectrogram<44100, 33, 4410, 441>::spectrogram (mel.h:34-104) ----
 * essentia FrameCutter(4410, 441) -> Windowing(hann) -> Spectrum -> MelBands(33) per frame, silent frames
 * dropped (mel.h:94-96), power_to_db over the kept columns (mel.h:103).  Any clip length.
 * hpfw_gpu_mel_frames: frames cut from n_samples (silent ones included) = the row stride of the output.
 * d_out [n_clips][33][frames]: the kept columns at the front of every row; d_cols [n_clips] their number. */
int64_t hpfw_gpu_mel_frames(int64_t n_samples);
int hpfw_gpu_mel_spectrogram_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples,
                                   int64_t n_clips, float *d_out, int32_t *d_cols, void *stream);
int hpfw_gpu_mel_spectrogram_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples,
                                        int64_t n_clips, float *out, int32_t *cols);

/* ---- HashprintHandle<N, SpectrogramHandler, FramesContext, T> with other template arguments -------------
 * (hashprint_handle.h:50-64).  Everything above is the live-id default <uint64_t, CQT<>, 20, 80>
 * (live_song_id.h:16); this is the same calc_frames / filters * frames / calc_fingerprint /
 * fingerprint_to_hashprint (hashprint_handle.h:79-142) for any spectrogram height, context, lag and word
 * size -- the combiner's HashPrint<uint16_t, MelSpectrogram<>, 32, 50> (combiner.h:12) first of all. */
typedef struct {
    int32_t rows;    /* Spectrogram::RowsAtCompileTime: 33 for MelSpectrogram<> (mel.h:17-21), 121 for CQT<> */
    int32_t context; /* FramesContext                                                                          */
    int32_t lag;     /* T                                                                                      */
    int32_t bits;    /* 8 * sizeof(N) = NumOfFilters (hashprint_handle.h:64): 16, 32 or 64                     */
} hpfw_handle_config;
#define HPFW_CONFIG_COMBINER {33, 32, 50, 16} /* combiner.h:12 */
/* filters: Matrix<float, NumOfFilters, Dynamic> column-major, element (r, k) at r + bits * k, k = row * context + t */
int hpfw_gpu_cfg_set_filters(hpfw_gpu *h, const hpfw_handle_config *cfg, const float *filters_colmajor);
/* d_s [n_clips][rows][stride] (row-major: element (row, col) of clip i at (i * rows + row) * stride + col);
 * d_cols [n_clips]: valid columns of each clip, or NULL = stride (the Mel front end drops silent frames, so its
 * clips differ).  d_hp: uintN [n_clips][hp_stride]; clip i receives max(cols_i - context + 1 - lag, 0) words.
 * d_proj (optional, NULL to skip): the projection filters * frames [n_clips][bits][stride - context + 1]. */
int hpfw_gpu_cfg_hashprints(hpfw_gpu *h, const hpfw_handle_config *cfg, const float *d_s, const int32_t *d_cols,
                            int64_t n_clips, int64_t stride, void *d_hp, int64_t hp_stride, float *d_proj, void *stream);
/* filter learning for such a configuration: calc_cov of every clip's frames (hashprint_handle.h:96-102: centred on the
 * clip's own frame means, / (n_frames - 1); clips with fewer than two frames add nothing) accumulated on the GPU as
 * ParallelCollector::preprocess does (parallel_collector.h:93-97), then calc_filters (hashprint_handle.h:105-112) on the
 * host: the `bits` leading eigenvectors become the configuration's filters.  d_s / d_cols / stride as above.
 * cov: host, [rows * context][rows * context].  context >= 9. */
int hpfw_gpu_cfg_cov_reset(hpfw_gpu *h, const hpfw_handle_config *cfg);
int hpfw_gpu_cfg_cov_accumulate(hpfw_gpu *h, const hpfw_handle_config *cfg, const float *d_s, const int32_t *d_cols,
                                int64_t n_clips, int64_t stride, void *stream);
int hpfw_gpu_cfg_cov_get(hpfw_gpu *h, const hpfw_handle_config *cfg, float *cov, int64_t *n_clips);
int hpfw_gpu_cfg_learn_filters(hpfw_gpu *h, const hpfw_handle_config *cfg, float *filters_colmajor_out);
/* the combiner's Algo end to end on host buffers: MelSpectrogram<44100, 33, 4410, 441>::spectrogram (mel.h:34-104)
 * + HashprintHandle<uint16_t, Mel, 32, 50>: hp [n_clips][hp_stride] (hp_stride >= hpfw_gpu_mel_frames(n) - 81),
 * n_hp [n_clips] the number of hashprints of each clip (0 when too few frames are left after the silent ones) */
int hpfw_gpu_mel_hashprints_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips,
                                       uint16_t *hp, int64_t hp_stride, int32_t *n_hp);

/* the combiner's filter learning from host PCM: the Mel front end above, then hpfw_gpu_cfg_cov_accumulate for
 * HPFW_CONFIG_COMBINER (what hpfw_gpu_cov_accumulate_pcm16_host is for live-id).  Finish with
 * hpfw_gpu_cfg_learn_filters(h, &combiner_config, ...). */
int hpfw_gpu_mel_cov_accumulate_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips);

/* ---- AudioCombiner: exact-hash inverted index + offset votes (combiner.h:90-132) ----------------------------
 * Recordings are uint16 hashprints of HPFW_CONFIG_COMBINER, numbered 0, 1, ... in the order they are added.  The
 * index is a CSR over the 65 536 values: val_start [65537] and postings (rec, off) in ascending global position
 * (recording, offset) inside every value -- build_db (:90-97) with the recordings in add order.  An append rebuilds it.
 *
 * find (:100-132) walks the events of a query in stream order: frame c ascending, then the postings of Q[c] in index
 * order, the query's own recording (`exclude`, -1 = none) skipped.  Event (j, d = c - o) has count = ++cnt[j][d]; it
 * changes the result iff count > confidence: to {j, count, 1, d} when j differs from the result's recording, else to
 * {j, count, confidence + 1, d}.  The result starts as {0xffffffff, 0, 0, 0}.  Computed on the device, bit-exact.
 *
 * align: for every recording j but the excluded one, peak = the most events on one offset d and offset = the smallest
 * such d; the k best recordings per query by (peak desc, rec asc), recordings with peak 0 not listed (rec = 0xffffffff).
 *
 * Workspace: the per-query bin arrays (sum over j of C_q + L_j - 1 uint32) and the event chunks are bounded by
 * HPFW_COMBINER_WORKSPACE_MB in the environment (default 1024, read at every call); a query whose bin array alone
 * exceeds it fails with HPFW_E_INVALID.  Unlike the other device entry points, the combiner's wait for their stream
 * once per pass of queries (the host sizes the event chunks from the pass's event total) and once per add (the CSR is
 * rebuilt at once). */
typedef struct {
    uint32_t rec;        /* recording id, 0xffffffff = none */
    uint32_t pad;
    int64_t cnt;
    int64_t confidence;
    int64_t offset;      /* d = c - o */
} hpfw_combine_result;
typedef struct {
    uint32_t rec;        /* 0xffffffff = padding */
    uint32_t peak;
    int64_t offset;
} hpfw_align_hit;
int hpfw_gpu_combiner_clear(hpfw_gpu *h);
/* appends n_rec recordings: recording i is hp[offsets[i] .. offsets[i+1]) (host or device source) */
int hpfw_gpu_combiner_add(hpfw_gpu *h, const uint16_t *hp, const int64_t *offsets, int64_t n_rec);
int hpfw_gpu_combiner_add_device(hpfw_gpu *h, const uint16_t *d_hp, const int64_t *offsets, int64_t n_rec, void *stream);
int64_t hpfw_gpu_combiner_size(hpfw_gpu *h); /* number of recordings */
/* the index on the host: val_start [65537] always; rec / off [postings] when not NULL (cap = their capacity; the number
 * of postings is val_start[65536]).  Synchronises. */
int hpfw_gpu_combiner_get(hpfw_gpu *h, int64_t *val_start, uint32_t *rec, uint32_t *off, int64_t cap);
/* query q is q_hp[q_off[q] .. q_off[q+1]); exclude [n_q] or NULL (= -1 for all).  Device variants: d_q_hp and d_out on
 * the device, q_off and exclude on the host. */
int hpfw_gpu_combiner_find(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                           hpfw_combine_result *out);
int hpfw_gpu_combiner_find_device(hpfw_gpu *h, const uint16_t *d_q_hp, const int64_t *q_off, const int32_t *exclude,
                                  int64_t n_q, hpfw_combine_result *d_out, void *stream);
/* out [n_q][k], k <= 64 */
int hpfw_gpu_combiner_align(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                            int k, hpfw_align_hit *out);
int hpfw_gpu_combiner_align_device(hpfw_gpu *h, const uint16_t *d_q_hp, const int64_t *q_off, const int32_t *exclude,
                                   int64_t n_q, int k, hpfw_align_hit *d_out, void *stream);

/* ---- sample-accurate offsets: exact windowed cross-correlation of PCM16 (k_xcorr.hip) ----
 * Operands a and b of a job are ranges [a_off, a_off + a_len) and [b_off, b_off + b_len) of ONE int16 buffer.  For
 * every lag l in [-radius, radius]
 *     r[l] = sum over n in [0, len) of a[p + l + n] * b[q + n]
 * with a read as 0 outside [0, a_len) and b[q .. q + len) inside b: exact int64 sums (|r| <= 2^52), no floating point
 * and no summation order -- int8 digit products on the matrix cores (HPFW_XCORR=valu in the environment, read at every
 * call: the plain integer kernel for every lag), 64-bit integer atomics between the parts of a job.
 * peak: the lag with the largest |r| (ties: the smaller |lag|, then the negative lag), r there,
 * energy_a = sum a[p + lag + n]^2 and energy_b = sum b[q + n]^2.
 * HPFW_E_INVALID: len < 1 or > 2^22, radius < 0 or > 4096, q < 0 or q + len > b_len, a range outside the buffer (the
 * device variant is not told the buffer's size: negative offsets and lengths only), |p| > 2^40, null pointers. */
#define HPFW_XCORR_MAX_LEN (1 << 22)
#define HPFW_XCORR_MAX_RADIUS 4096
typedef struct {
    int64_t a_off, a_len, b_off, b_len; /* operands: ranges of the pcm buffer */
    int64_t p, q, len;                  /* as in the formula above */
    int32_t radius, pad;
} hpfw_xcorr_job;
typedef struct {
    int64_t r, energy_a, energy_b;
    int32_t lag, pad;
} hpfw_xcorr_peak;
/* d_pcm, d_r (NULL, or [sum of 2 radius + 1], job after job, lag -radius first) and d_peaks [n_jobs] on the device,
 * jobs on the host (read before the call returns).  The host variant takes n_pcm, uploads and synchronises. */
int hpfw_gpu_xcorr_pcm16(hpfw_gpu *h, const int16_t *d_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *d_r,
                         hpfw_xcorr_peak *d_peaks, void *stream);
int hpfw_gpu_xcorr_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs,
                              int64_t *r, hpfw_xcorr_peak *peaks);
/* the frames the Mel front end keeps (it drops the frames essentia calls silent before anything is hashed): column c of
 * clip i came from frame frames[i * stride + c], centred on sample 441 * frame; n_kept [n_clips] columns per clip, the
 * rest of a row is -1.  stride >= hpfw_gpu_mel_frames(n_samples). */
int hpfw_gpu_mel_kept_frames_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips,
                                        int32_t *frames, int64_t stride, int32_t *n_kept);

/* a WAV file as the live-id file entry points read it: PCM16 mono, or stereo averaged (truncating) to mono, 44.1 kHz
 * only (HPFW_E_IO otherwise).  *n = samples in the file; out receives them when cap >= *n (out may be NULL). */
int hpfw_gpu_wav_read_pcm16(const char *path, int16_t *out, int64_t cap, int64_t *n);

/* a WAV file at its own rate (8 000 .. 192 000 Hz): PCM16 mono, or stereo averaged (truncating) to mono, not resampled.
 * *rate = the file's sample rate; other bit depths, more than two channels, non-PCM files and rates outside the range
 * are HPFW_E_IO.  *n and out as hpfw_gpu_wav_read_pcm16. */
int hpfw_gpu_wav_read_pcm16_any(const char *path, int16_t *out, int64_t cap, int64_t *n, int32_t *rate);

/* ---- sample-rate conversion to 44.1 kHz (essentia MonoLoader's resampling, cqt.h:45-47, mel.h:42-44) -------------
 * Polyphase windowed sinc in exact integer arithmetic: g = gcd(44100, rate), L = 44100 / g,
 * M = rate / g; output m sits at input time m M / L and is clamp((sum_j x[floor(m M / L) - H + 1 + j] h[(m M) mod L][j]
 * + 2^13) >> 14) over T = 2 H int16 taps per phase, x = 0 outside the clip.  n_out = ceil(n_in L / M).  44 100 Hz is
 * a plain copy.  Rates outside [8 000, 192 000] are HPFW_E_INVALID. */
int hpfw_gpu_resample_length(int64_t n_in, int rate, int64_t *n_out); /* host only */
/* the [L][T] int16 table (host only; taps may be NULL to ask for L, M, T; cap = its capacity).  44 100 Hz: L = M = 1,
 * T = 0. */
int hpfw_gpu_resample_table(int rate, int16_t *taps, int64_t cap, int32_t *L, int32_t *M, int32_t *T);
/* n_clips clips of n_in samples back to back -> d_out [n_clips][n_out] (device entry point) */
int hpfw_gpu_resample_pcm16(hpfw_gpu *h, const int16_t *d_in, int64_t n_in, int64_t n_clips, int rate, int16_t *d_out,
                            void *stream);
int hpfw_gpu_resample_pcm16_host(hpfw_gpu *h, const int16_t *in, int64_t n_in, int64_t n_clips, int rate, int16_t *out);

/* ---- time warp and mix of PCM16: clock drift between recorders, and the event rendered (k_warp.hip, DESIGN.md
 * section 16) ----
 * A track is a range [src_off, src_off + src_len) of ONE int16 buffer, read at the affine position
 * i0 + m + (f0 + m d) 2^-40 of output m.  For 0 <= m < 2^31, in exact integers:
 *     u     = f0 + m d                          (int64)
 *     ip    = i0 + m + (u >> 40)                (arithmetic shift: floor)
 *     phase = (u & (2^40 - 1)) >> 28            (P = 4096 rows, truncated)
 *     acc   = sum over j < T of x[ip - H + 1 + j] h[phase][j]        x = 0 outside [0, src_len); T = 2 H = 32; int32
 *     y[m]  = clamp((acc + 2^13) >> 14, -32768, 32767)
 * h is hpfw_gpu_warp_table's [P][T] int16 table in Q14: row p the windowed sinc of the fractional delay p / P, every row
 * summing to 2^14 and row 0 the unit impulse, so that d = 0, f0 = 0 copies the source shifted by i0 bit for bit.
 * HPFW_E_INVALID: a source range outside the buffer, |d| > 2^30 (977 ppm), f0 outside [0, 2^40), |i0| > 2^62,
 * |gain| > 2^17, m0 < 0, n_out < 0, m0 + n_out > 2^31, null pointers. */
typedef struct {
    int64_t src_off, src_len; /* the source: a range of the pcm buffer */
    int64_t i0, f0, d;        /* the time map */
    int32_t gain, pad;        /* signed, Q15 */
} hpfw_warp_track;
/* the [P][T] int16 table (host only; taps may be NULL to ask for P and T; cap = its capacity) */
int hpfw_gpu_warp_table(int16_t *taps, int64_t cap, int32_t *P, int32_t *T);
/* outputs m0 .. m0 + n_out - 1 of every track -> d_out [n_tracks][n_out].  A negative gain negates the value before the
 * clamp (+32768 becomes 32767); the size of the gain is not used.  d_pcm and d_out on the device, tracks on the host (read
 * before the call returns).  The host variant uploads, synchronises and downloads. */
int hpfw_gpu_warp_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks,
                        int64_t m0, int64_t n_out, int16_t *d_out, void *stream);
int hpfw_gpu_warp_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks,
                             int64_t m0, int64_t n_out, int16_t *out);
/* mix[m] = clamp((sum over the tracks of gain_k y_k[m] + 2^14) >> 15) -> d_mix [n_out], with y_k the clamped, un-negated
 * value above and the sum in int64: no track is materialised, and the result equals the mix of materialised tracks bit for
 * bit (integer sums have no order). */
int hpfw_gpu_mix_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks,
                       int64_t m0, int64_t n_out, int16_t *d_mix, void *stream);
int hpfw_gpu_mix_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_warp_track *tracks, int64_t n_tracks,
                            int64_t m0, int64_t n_out, int16_t *mix);
/* Host only: the anchors of a pair.  [s_lo, s_hi) is the pair's overlap in the recording's samples, [q, q + len) the
 * centre segment (len = min(anchor_len, overlap), as the refinement places it).  Further anchors of anchor_len samples start
 * at q - t anchor_hop and q + t anchor_hop, t = 1, 2, ..., for as long as a whole anchor lies in the overlap; an overlap
 * shorter than one anchor has the centre alone.  starts (NULL to count; cap = its capacity):
 * [centre, left 1 .. *n_left, right 1 .. *n_right], *n = 1 + *n_left + *n_right. */
int hpfw_gpu_drift_anchors(int64_t s_lo, int64_t s_hi, int64_t q, int64_t len, int64_t anchor_len, int64_t anchor_hop,
                           int64_t *starts, int64_t cap, int32_t *n_left, int32_t *n_right, int64_t *n);
/* Host only: the Theil-Sen line lag ~ a + b n.  b = the median of (lag_j - lag_i) / (n_j - n_i) over the pairs i < j in
 * index order (pairs with equal n left out; the median of an even count is the mean of the two middle values), a = the
 * median of lag_i - b n_i, rms = the root mean square of lag_i - (a + b n_i): float64 in exactly this order.  Fewer than 3
 * points: b = 0 and a = lag[0] (callers put the centre anchor first); count = 0: all 0. */
int hpfw_gpu_drift_fit(const int64_t *n, const int64_t *lag, int count, double *a, double *b, double *rms);
/* Host only: the time map of a source whose sample n sits at t = A + (1 + B) n of the output's timeline: output m reads
 * the source at (m - A) / (1 + B), and |i0 + m + (f0 + m d) 2^-40 - (m - A) / (1 + B)| <= 2^-40 + m 2^-41 samples.
 * HPFW_E_INVALID: |1 / (1 + B) - 1| > 2^-10, |A| > 2^30. */
int hpfw_gpu_time_map_q40(double A, double B, int64_t *i0, int64_t *f0, int64_t *d);
/* pcm [n] int16 (n = frames x channels, interleaved) as a RIFF/WAVE file: a 44-byte header, PCM16, 44.1 kHz.  HPFW_E_IO
 * when the file cannot be written; channels 1 or 2, n a multiple of channels and below 2^31 bytes. */
int hpfw_gpu_wav_write_pcm16(const char *path, const int16_t *pcm, int64_t n, int channels);

/* ---- filter learning: ParallelCollector::preprocess + calc_filters ------------------------
 * (parallel_collector.h:82-112, hashprint_handle.h:96-112).  The handle owns accum_cov
 * (2420 x 2420, parallel_collector.h:76): per clip, the covariance of its context frames (centred
 * on the clip's own mean, / (n_frames - 1)) is added on the GPU (f32 MFMA); learn_filters takes the
 * eigenvectors of the 64 largest eigenvalues on the host and installs them as the filters.
 * Eigenvector signs are arbitrary in the reference; here the largest component is positive. */
int hpfw_gpu_cov_reset(hpfw_gpu *h);
int hpfw_gpu_cov_accumulate_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                                  void *stream);
int hpfw_gpu_cov_accumulate_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips);
/* stage entry point: from dB spectrograms d_db [n_clips][121][C] */
int hpfw_gpu_cov_accumulate_db(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, void *stream);
/* host copies of accum_cov (full symmetric 2420 x 2420 floats; synchronises) and the file count */
int hpfw_gpu_cov_get(hpfw_gpu *h, float *cov, int64_t *n_files);
int hpfw_gpu_cov_set(hpfw_gpu *h, const float *cov, int64_t n_files);
/* filters_colmajor_out may be NULL; layout as hpfw_gpu_set_filters */
int hpfw_gpu_learn_filters(hpfw_gpu *h, float *filters_colmajor_out);
/* accum_cov where it lives: DEVICE pointer to 2420 x 2420 floats (allocated and zeroed on first use; the tiles
 * of 128 x 128 on or above the diagonal are maintained, the rest stays zero) and the number of files added --
 * what a multi-GPU host sums with one ncclAllReduce (include/hpfw_gpu_multi.h) */
int hpfw_gpu_cov_device(hpfw_gpu *h, float **d_cov);
int64_t hpfw_gpu_cov_files(hpfw_gpu *h);
int hpfw_gpu_cov_set_files(hpfw_gpu *h, int64_t n_files);
/* host-only: unit eigenvectors of the m largest eigenvalues of a symmetric n x n float matrix */
int hpfw_gpu_host_top_eigenvectors(const float *cov, int n, int m, float *out, double *evals);

/* Hashprints of one cached dB spectrogram, as collect_fingerprints computes them from
 * cache/spectros/<stem> (parallel_collector.h:114-137).  s_colmajor is the matrix as the cereal file
 * holds it (utils.h:77-106: int32 rows = 121, int32 cols, column-major floats).  *n_hp = cols - 99
 * (0 when the spectrogram is too short); hp receives them when hp_cap >= *n_hp. */
int hpfw_gpu_extract_db_host(hpfw_gpu *h, const float *s_colmajor, int32_t rows, int32_t cols,
                             uint64_t *hp, int64_t hp_cap, int64_t *n_hp);

/* ---- index + search: MemoryStorage::build / find ----------------------------------------- */
int hpfw_gpu_index_clear(hpfw_gpu *h);
/* appends n_clips hashprints; clip i is hp[offsets[i] .. offsets[i+1]); host or device source */
int hpfw_gpu_index_add(hpfw_gpu *h, const uint64_t *hp, const int64_t *offsets, int64_t n_clips);
int hpfw_gpu_index_add_device(hpfw_gpu *h, const uint64_t *d_hp, const int64_t *offsets,
                              int64_t n_clips, void *stream);
int64_t hpfw_gpu_index_size(hpfw_gpu *h); /* number of clips */
/* The index back on the host -- what MemoryStorage::save dumps (storage.h:67-75).  offsets
 * [n_clips + 1] is always written; hp [offsets[n_clips]] when hp != NULL (hp_cap = its capacity). */
int hpfw_gpu_index_get(hpfw_gpu *h, int64_t *offsets, uint64_t *hp, int64_t hp_cap);
/* added to every reported clip id (rank's first global clip id when the index is sharded) */
int hpfw_gpu_index_set_clip_base(hpfw_gpu *h, uint32_t clip_base);
/* Index maintenance.  Removal keeps every id: the clips named become empty, the hashprints of the
 * others close up in place, in order, and hpfw_gpu_index_get returns byte for byte what index_clear + index_add of the same
 * clips with the removed ones empty would have built -- so every search answers as on that index.  hpfw_gpu_index_size,
 * the clip base and the buffer's capacity do not change; a later index_add appends behind the last hashprint with ids
 * size, size + 1, ... and uses the freed room before anything is allocated.
 * clips [n]: ids in add order without the clip base, host, read before the call returns, in any order; a repeated id and an
 * id of an empty clip are no-ops.  Refused before anything changes (HPFW_E_INVALID): an id outside [0, size), n < 0, a null
 * list with n > 0, and a staging buffer that cannot be allocated (HPFW_INDEX_STAGE_MB, read at the call; default 128).
 * Enqueues on stream, ordered with every other entry point of the handle: a search enqueued before the call, on any stream,
 * sees the old index, one enqueued after it the new one, without the caller synchronising; no device-wide synchronisation.
 * The device memory it needs beyond the index is the staging buffer and the list of moves. */
int hpfw_gpu_index_remove(hpfw_gpu *h, const int64_t *clips, int64_t n, void *stream);
/* room for n_hashprints without a later reallocation; never shrinks */
int hpfw_gpu_index_reserve(hpfw_gpu *h, int64_t n_hashprints);
int64_t hpfw_gpu_index_capacity(hpfw_gpu *h); /* in hashprints */
/* host-only: the plan of a removal (hpfw_amd/csrc/index_plan.h).  A move piece copies len hashprints from src to dst
 * (dst < src); pieces are listed chunk after chunk with adjacent ascending destinations; a chunk whose sources meet its own
 * destinations is staged (read whole into the staging buffer, then written), every other is direct. */
typedef struct {
    int64_t dst, src, len;
    int64_t chunk;  /* the chunk's number, from 0 */
    int32_t staged; /* 1: the chunk goes through the staging buffer */
    int32_t pad;
} hpfw_index_move;
/* offsets [n_clips + 1]; removed [n_removed] strictly ascending ids; chunk >= 1 hashprints; new_offsets [n_clips + 1];
 * moves [moves_cap] (NULL to count); *n_moves the number of pieces.  HPFW_E_INVALID for arguments outside these conditions
 * and for a moves_cap below *n_moves. */
int hpfw_gpu_index_remove_plan(const int64_t *offsets, int64_t n_clips, const int64_t *removed, int64_t n_removed, int64_t chunk,
                               int64_t *new_offsets, hpfw_index_move *moves, int64_t moves_cap, int64_t *n_moves);
/* host-only: the hashprints of the destination one workgroup takes, and the default chunk in hashprints */
int hpfw_gpu_index_remove_geometry(int64_t *tile, int64_t *chunk);

/* top-k clips per query, ascending (dist, clip): query q is q_hp[q_off[q] .. q_off[q+1]).
 * d_q_hp device; q_off host; d_out device [n_q][k].  k <= 64.
 * Environment (tests, timing; the results are the same bytes), read per call: HPFW_SEARCH_POPC -- the xor/popcount scan for
 * every query (it otherwise serves queries whose window does not fit the LDS); HPFW_SEARCH_MFMA / HPFW_SEARCH_SHIFT -- the
 * grouped / the shifted-rows matrix-core scan for any number of queries (the default: shifted rows below 8 queries);
 * HPFW_SEARCH_TABLE_KB=<KiB> -- the size of the (query, clip) table of one pass over the queries (default and most 1 GiB,
 * at least 32 queries' rows), for tests of more than one pass.  They act on the scored, transposed and within-sets forms
 * too. */
int hpfw_gpu_search_topk_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off,
                                int64_t n_q, int k, hpfw_hit *d_out, void *stream);
/* host convenience: copies queries in and hits out, synchronises */
int hpfw_gpu_search_topk(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                         int k, hpfw_hit *out);
/* AnnStorage::find (annoy_storage.h:41-63) with the approximate Annoy forest replaced by exact nearest
 * neighbours.  Items are windows of 64 consecutive hashprints (the reference indexes 64 uint64 words per
 * item, annoy_storage.h:23,32; its items whose window runs past the end of a hashprint -- an
 * out-of-bounds read -- are not created).  For every position i of a query, the 5 windows of the index
 * nearest in Hamming distance over the 4096 bits, by (distance, position in the database), vote
 * cnt[clip][i - p] += 1 / (d + 1) (float accumulator, :53); the first bucket to exceed the running
 * maximum wins (:55-59).  Host arrays; out[n_q]; clip = 0xffffffff when the query has no window or the
 * index no item.
 * The two host functions are round trips over hpfw_gpu_search_votes_device and hpfw_gpu_knn_windows_device below on the
 * null stream: the queries are uploaded from q_off[0] on, the offsets rebased, the result downloaded.  Null h, q_hp, q_off,
 * out / keys, n_q < 0, a decreasing q_off and too small a keys_cap are refused (HPFW_E_INVALID) before any device work.
 * Their limits are the device calls': windows are processed in groups of about 256 MiB of workspace, so a call may hold any
 * number of windows, and ONE QUERY may hold at most 2 097 120 (HPFW_E_UNSUPPORTED).  (Earlier versions refused more than
 * 2 097 120 windows in one call; every call they accepted is accepted, with the same answer.) */
typedef struct {
    uint32_t clip;
    uint32_t pad;
    int64_t offset; /* i - p of the winning bucket */
    float cnt;      /* its votes */
    float pad2;
} hpfw_vote;
int hpfw_gpu_search_votes(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                          hpfw_vote *out);
/* the neighbours themselves (for tests): keys [n_windows][5], dist << 40 | global hashprint position,
 * ascending, ~0 where fewer exist; windows of all queries in order, n_windows = sum max(k - 63, 0) */
int hpfw_gpu_knn_windows(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                         uint64_t *keys, int64_t keys_cap);
/* ---- the voting search with device buffers on a stream.  The tally runs on the device: events are
 * grouped by bucket with a stable sort, every bucket's count is accumulated in the arithmetic above in window order, and the
 * winner is the event earliest in stream order whose post-event count is the query's largest -- the result of the reference's
 * sequential loop (annoy_storage.h:47-60), bit for bit, whatever the scheduling.  Windows are processed in groups of whole queries whose
 * workspaces stay within 256 MiB (HPFW_VOTES_GROUP_WINDOWS in the environment: fewer windows per group), so these calls
 * have no limit on the windows of one call; the 256 MiB are an estimate, and one query with more windows than a group is
 * processed alone, above it.  Bad arguments are refused before any device work.
 * q_off indexes d_q_hp by ABSOLUTE offset: query q is d_q_hp[q_off[q] .. q_off[q+1]), as hpfw_gpu_search_topk_device takes it
 * (the host functions above upload from q_off[0] on instead).
 * Not fully asynchronous: every call uploads its small host tables (q_off, w_first) and WAITS for the caller's stream before
 * it queues its kernels, so it returns with its work queued but cannot be captured into a graph. */
/* keys [n_windows][5] on the device, ascending per window, positions in THIS handle's index; keys_cap in keys */
int hpfw_gpu_knn_windows_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                uint64_t *d_keys, int64_t keys_cap, void *stream);
/* the tally alone: window w of the call is d_keys[w][5]; w_first [n_q + 1] host, query q owns the windows
 * [w_first[q], w_first[q + 1]); d_db_off [n_clips + 1] device; clip_base is added to the reported clip; d_out [n_q] */
int hpfw_gpu_vote_windows_device(hpfw_gpu *h, const uint64_t *d_keys, const int64_t *w_first, int64_t n_q,
                                 const int64_t *d_db_off, int64_t n_clips, uint32_t clip_base,
                                 hpfw_vote *d_out, void *stream);
/* knn + tally against the handle's index; d_q_hp and d_out [n_q] device, q_off host */
int hpfw_gpu_search_votes_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                 hpfw_vote *d_out, void *stream);
/* the per-shard neighbour lists of a sharded index merged: d_in [n_shards][n_win][5], pos_base [n_shards] host (the
 * hashprints in earlier shards: non-negative, non-decreasing) is added to the position of every real key; d_out [n_win][5]
 * the 5 smallest, ascending, ~0 behind them.  n_shards <= 64. */
int hpfw_gpu_merge_knn_device(hpfw_gpu *h, const uint64_t *d_in, const int64_t *pos_base, int n_shards,
                              int64_t n_win, uint64_t *d_out, void *stream);

/* deterministic merge of per-shard top-k lists (e.g. after an all-gather): in [n_shards][n_q][k]
 * -> out [n_q][k], ascending (dist, clip).  Host arrays. */
int hpfw_gpu_merge_topk(const hpfw_hit *in, int n_shards, int64_t n_q, int k, hpfw_hit *out);

/* ---- overlap search: the query may overhang either end of a clip, and alignments are rated per
 * overlapping hashprint.  hpfw_gpu_search_topk slides the query inside the clip (offsets 0 .. n - k) and compares a clip
 * shorter than the query over its own n hashprints at offset 0 (storage.h:37-39), which puts short clips on another scale
 * and finds no window that begins before a clip does.  This search is a rule of its own beside it.
 *
 * Query q[0..k), 1 <= k <= 16000; clip r[0..n).  A lag d (signed) puts query position j on clip position d + j.
 *   J(d) = { j : 0 <= j < k, 0 <= d + j < n },  L(d) = |J(d)| = min(k, n - d) - max(0, -d),
 *   dist(d) = sum over j in J(d) of popcount(q[j] ^ r[d + j]).
 * A lag is ADMISSIBLE when L(d) >= min_overlap.  min_overlap is the caller's, 1 <= min_overlap <= 16000, and has no
 * default.  A clip with n < min_overlap or a query with k < min_overlap has no candidate.
 * Candidates are ordered by (1) smaller dist / L as an exact rational -- dist1 L2 < dist2 L1, products below 2^34 --,
 * (2) larger L, (3) smaller d.  A clip's candidate is its minimum in that order; the k <= 64 clips of a query are ordered
 * by (1), (2), then the smaller clip id.  The order is computed in integers: no floating point takes part, and the result
 * does not depend on how the work is scheduled.
 * exclude: NULL, or [n_q] (host): per query the index, in add order (without clip_base), of a clip to leave out; -1 = none.
 * With min_overlap = k and no clip shorter than the query the hits are hpfw_gpu_search_topk's (dist, clip, offset), with
 * overlap = k.
 * Refused before anything runs: null pointers, k outside 1..64, min_overlap outside 1..16000, decreasing q_off, an exclude
 * entry below -1 or at or above the number of clips (HPFW_E_INVALID); a query above 16000 hashprints (HPFW_E_UNSUPPORTED).
 * An empty index, a query without candidates and the slots past the last candidate give padding records.
 * Environment (tests; the results are the same bytes): HPFW_OVERLAP_POPC -- the xor/popcount kernel for every query (it
 * otherwise serves queries whose window does not fit the LDS); HPFW_OVERLAP_SPLITS=<1..64> -- workgroups per clip;
 * HPFW_OVERLAP_TABLE_KB=<KiB> -- the size of the (query, clip, split) table of one pass over the queries (default and most
 * 1 GiB, at least 32 queries' rows), for tests of more than one pass. */
typedef struct {
    uint32_t dist;    /* mismatching bits over the overlap                 */
    uint32_t clip;    /* as hpfw_hit; 0xffffffff = none                    */
    int32_t lag;      /* clip position of query position 0                 */
    uint32_t overlap; /* L(lag)                                            */
} hpfw_overlap_hit;
/* padding: dist = clip = 0xffffffff, lag = overlap = 0 */
/* d_q_hp, d_out [n_q][k] device; q_off, exclude host */
int hpfw_gpu_search_overlap_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                   const int32_t *exclude, int min_overlap, int k, hpfw_overlap_hit *d_out, void *stream);
/* host convenience: copies queries in and hits out, synchronises */
int hpfw_gpu_search_overlap(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                            const int32_t *exclude, int min_overlap, int k, hpfw_overlap_hit *out);

/* ---- catalogue self-join: the recordings of the index that duplicate or contain each other.
 * The index is joined with itself where it lies; recordings may have any indexed length up to 2^18 - 1 hashprints, every
 * unordered pair is computed once, and every pair under a threshold is reported.
 * Take clips a < b of the index in add order, both non-empty and both with at least min_overlap hashprints.  Clip a takes
 * the part of the query of the overlap search above and b the part of the clip:
 *   lag d puts position j of a on position d + j of b;
 *   L(d) = min(n_a, n_b - d) - max(0, -d);    dist(d) = sum of popcount(a[j] ^ b[d + j]) over the positions both have.
 * A lag is ADMISSIBLE when L(d) >= min_overlap, so d runs from min_overlap - n_a to n_b - min_overlap.  Candidates are
 * ordered by dist / L as an exact rational, then by larger L, then by smaller d (the overlap search's order); the pair's
 * candidate is its minimum.  The pair is REPORTED when dist * rate_den <= rate_num * L: rate_num / rate_den is the caller's
 * threshold in mismatching bits per hashprint, 1 <= rate_den <= 1024, 0 <= rate_num <= 64 rate_den.  Neither min_overlap,
 * 1 <= min_overlap <= 2^18 - 1, nor the threshold has a default.
 * Pairs come in ascending (a, b); no floating point takes part, nothing depends on the order in which workgroups run, and
 * no atomics are used.  Removed recordings (empty clips) and recordings below min_overlap never appear.  The clip base is
 * added to both ids.
 * d_out receives the first cap reported pairs, *d_count (int64) their total number, which may exceed cap: the caller
 * enlarges the buffer and calls again.  An empty index and an index of one clip give count 0.
 * Refused before a device is touched (HPFW_E_INVALID): a null handle, rate_den outside 1..1024, rate_num outside
 * 0..64 rate_den, min_overlap outside 1..2^18 - 1, cap < 0, a null out with cap > 0, a null count.  An index that holds a
 * recording above 2^18 - 1 hashprints is refused before a kernel runs (HPFW_E_UNSUPPORTED): below that bound 64 L < 2^24
 * and the fp32 accumulators of the fp4 contraction are exact.
 * HPFW_SELFJOIN_POPC in the environment selects the xor/popcount kernel, HPFW_SELFJOIN_SPLITS (1..64) the workgroups that
 * share a pair's lags, HPFW_SELFJOIN_TABLE_KB the size of the table of one pass over the rows (default and most 1 GiB);
 * they are read at every call and change no result. */
typedef struct {
    uint32_t a, b;    /* a < b, ids in add order + the clip base      */
    uint32_t dist;    /* mismatching bits over the overlap            */
    uint32_t overlap; /* L(lag)                                       */
    int32_t lag;      /* position 0 of a lies on position lag of b    */
    uint32_t pad;
} hpfw_dup_pair;
int hpfw_gpu_index_selfjoin_device(hpfw_gpu *h, int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *d_out,
                                   int64_t cap, int64_t *d_count, void *stream);
/* host buffers (the null stream): out [cap], *count */
int hpfw_gpu_index_selfjoin(hpfw_gpu *h, int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *out, int64_t cap,
                            int64_t *count);
/* host-only: *slice = the positions of a staged per pass over the LDS, *chunk = the lags of b one workgroup pass takes (a
 * pair's chunks begin at min_overlap - the longest of the 32 rows a that share the workgroup).  NULL is HPFW_E_INVALID. */
int hpfw_gpu_selfjoin_geometry(int32_t *slice, int32_t *chunk);

/* ---- ingest check: recordings that are not in the index joined against it, before they are added.
 * The index has n slots.  The call brings m EXTERNAL recordings x_0 .. x_(m-1): their hashprints in device memory, x_i at
 * d_x_hp[x_off[i] .. x_off[i + 1]), and the offsets x_off [m + 1] on the host.  x_i is given the id n + i, the id
 * hpfw_gpu_index_add would give it.  The join reports every pair (a, b) with
 *   n <= b < n + m,    a < b,    and which the self-join above would report of the index with the m recordings appended,
 * with that pair's dist, overlap and lag under the same order of candidates (dist / L exact, then larger L, then smaller
 * lag): a takes the query's part and b the clip's.  among_new = 0 reports only pairs with a < n (an indexed recording
 * against an external one), among_new = 1 the pairs between two externals as well.  In other words: what index_add followed
 * by index_selfjoin would add to the self-join's answer, byte for byte -- without the index changing.
 * Pairs come in ascending (a, b) as hpfw_dup_pair; the clip base is added to both ids; empty slots, removed recordings and
 * recordings below min_overlap (indexed or external) never appear; the index is not modified; no floating point takes part
 * in the order, no atomics are used and nothing depends on the order in which workgroups run.  Work is about (n / 32) m
 * workgroup pairs (among_new = 1: (n + m / 2) / 32 m), not the self-join's n^2 / 64.
 * cap, *d_count and the call's ordering are the self-join's: d_out receives the first cap pairs, *d_count their total,
 * which may exceed cap.  n_x = 0 gives count 0; an empty index with among_new = 1 gives the pairs among the batch.
 * Refused before a device is touched (HPFW_E_INVALID): everything the self-join refuses, a null x_off, n_x < 0, decreasing
 * offsets, null hashprints when the offsets name any, among_new outside 0..1.  Refused before a kernel runs
 * (HPFW_E_UNSUPPORTED): an external or an indexed recording above 2^18 - 1 hashprints, n + m above 2 097 152.
 * HPFW_SELFJOIN_POPC, HPFW_SELFJOIN_SPLITS and HPFW_SELFJOIN_TABLE_KB act as on the self-join; the table of a pass is
 * [rows of the pass][m][splits]. */
int hpfw_gpu_index_join_device(hpfw_gpu *h, const uint64_t *d_x_hp, const int64_t *x_off, int64_t n_x, int among_new,
                               int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *d_out, int64_t cap,
                               int64_t *d_count, void *stream);
/* host buffers (the null stream): x_hp, out [cap], *count */
int hpfw_gpu_index_join(hpfw_gpu *h, const uint64_t *x_hp, const int64_t *x_off, int64_t n_x, int among_new,
                        int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *out, int64_t cap, int64_t *count);
/* host-only: how a pass of the join over the row groups group0 .. group0 + n_groups - 1 numbers its work.  Row group g holds
 * the ids 32 g .. 32 g + 31 of the list "the n_clips slots of the index, then the n_x externals"; its items are the externals
 * b >= max(n_clips, 32 g + 1), one workgroup pair (group, b) each, and none when no row of the group is launched (among_new =
 * 0: groups at or above ceil(n_clips / 32)).  pair_first [n_groups + 1]: item pair_first[i] + j is (group0 + i,
 * b = max(n_clips, 32 (group0 + i) + 1) + j).  Negative counts, among_new outside 0..1 and NULL are HPFW_E_INVALID;
 * n_clips + n_x above 2 097 152 is HPFW_E_UNSUPPORTED. */
int hpfw_gpu_join_plan(int64_t n_clips, int64_t n_x, int among_new, int64_t group0, int64_t n_groups, uint32_t *pair_first);

/* ---- warped search: subsequence DTW over hashprints.  Every other search lines a query up with a
 * clip rigidly (query position j on clip position offset + j); this one lets the query run faster or slower than the clip
 * inside the window, and tells which clip column every query hashprint lies on.  Exact integers throughout.
 *
 * Query q[0..K), 1 <= K <= 16000; clip r[0..n), n >= 1; c(i, j) = popcount(q[i] ^ r[j]).
 * Row 0 starts anywhere for free: D(0, j) = c(0, j), S(0, j) = j.  For i >= 1 a cell takes the smallest of
 *   A: D(i-1, j-1) + c(i, j)                 both advance by one
 *   B: D(i-1, j-2) + c(i, j)                 the clip skips a column (the query runs faster)
 *   C: D(i-2, j-1) + c(i-1, j) + c(i, j)     rows i-1 and i both lie on column j (the query runs slower); i >= 2
 * each valid only where its predecessor exists and is reachable; ties go to the first of A, B, C; S(i, j) is the S of the
 * chosen predecessor; a cell without a valid candidate is unreachable.  Every query hashprint is charged once, at the
 * column it lies on, so distances are on hpfw_gpu_search_topk's scale, and the all-A path is the rigid alignment: for
 * n >= K the warped distance of a clip is never above the plain search's.  The local slope stays within 1/2 .. 2.
 * Per (query, clip): dist = min_j D(K-1, j), end = the smallest j reaching it, start = S(K-1, end).  A clip has a
 * candidate iff n >= K / 2 + 1 (integer division); an empty query has none.  A query's clips are ordered by (dist, clip).
 * The path of a pair is path[0..K), the clip column of every query row, walked back from (K-1, end) along the choices (a C
 * step gives rows i-1 and i the same column): path[0] = start, path[K-1] = end, increments in {0, 1, 2} with a 0 only
 * directly after a 1, and the sum of c(i, path[i]) is dist.
 * Refused before any device work: null pointers, n_q < 0, n_pairs < 0, a decreasing q_off, k outside 1..64, candidates
 * outside {0} and [k, 64], a negative pair or clip index (HPFW_E_INVALID); a query above 16000 hashprints, a path of more
 * than 2^31 cells (K n; its choices take 2 bits each) (HPFW_E_UNSUPPORTED).  A pair or clip index at or above the number of
 * queries or clips is HPFW_E_INVALID.  The sharded index (hpfw_gpu_multi.h) has no warped search. */
typedef struct {
    uint32_t dist;  /* mismatching bits along the path                        */
    uint32_t clip;  /* 0xffffffff = none                                      */
    int32_t start;  /* clip column of query hashprint 0                       */
    int32_t end;    /* clip column of the query's last hashprint              */
} hpfw_dtw_hit;
/* padding: dist = clip = 0xffffffff, start = end = 0 */
/* pairs [n_pairs][2] (host): (query index, clip index in add order, without clip_base); d_out [n_pairs]: one hit per pair, clip
 * as the pair names it, the padding record for a pair without a candidate.  d_q_hp, d_out device; q_off, pairs host */
int hpfw_gpu_dtw_pairs_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *pairs,
                              int64_t n_pairs, hpfw_dtw_hit *d_out, void *stream);
int hpfw_gpu_dtw_pairs(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, const int32_t *pairs,
                       int64_t n_pairs, hpfw_dtw_hit *out);
/* d_out [n_q][k], 1 <= k <= 64: the k best clips of every query by (dist, clip), clip_base added as in hpfw_hit, padding
 * records behind the last candidate.  candidates (no default in any binding: the caller decides) = 0: every clip of the index
 * is a pair of every query; k <= candidates <= 64: the pairs of a query are its hpfw_gpu_search_topk hits for k = candidates,
 * re-ranked by the rule exactly as it stands. */
int hpfw_gpu_search_dtw_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int candidates, int k,
                               hpfw_dtw_hit *d_out, void *stream);
int hpfw_gpu_search_dtw(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int candidates, int k,
                        hpfw_dtw_hit *out);
/* one query of k_q hashprints against clip `clip` (add order, without clip_base): d_path [k_q] and the pair's hit (clip as
 * given); no candidate: the padding record and -1 in every entry of the path */
int hpfw_gpu_dtw_path_device(hpfw_gpu *h, const uint64_t *d_q_hp, int64_t k_q, int32_t clip, int32_t *d_path,
                             hpfw_dtw_hit *d_hit, void *stream);
int hpfw_gpu_dtw_path(hpfw_gpu *h, const uint64_t *q_hp, int64_t k_q, int32_t clip, int32_t *path, hpfw_dtw_hit *hit);
/* Host only (tests): the columns a lane of the pairs kernel holds and the columns of one pass of its wave -- the widths at
 * which a clip crosses into the next lane and the next block */
int hpfw_gpu_dtw_geometry(int32_t *strip, int32_t *block);

/* ---- local search: which part of the query is which part of which clip.  Every search above rates a
 * whole alignment; this one rates the best RUN of consecutive query hashprints on any diagonal, so a query that shares only
 * a passage with a recording (a window of a mix, a sample, an edit with its own intro) is found with the passage's ends.
 *
 * max_rate = T, 1 <= T <= 31, in mismatching bits per hashprint, is the caller's and has no default.
 * Query q[0..k), 1 <= k <= 16000; clip r[0..n).  Lags d = 1 - k .. n - 1; at lag d both have the positions j in [ja, jb),
 * ja = max(0, -d), jb = min(k, n - d).  x_j = T - popcount(q[j] ^ r[d + j]).  A run is a non-empty [j0, j1) inside
 * [ja, jb): score = sum of x_j, dist = sum of popcount, length = j1 - j0, so score = T length - dist.
 * A clip's candidate is its best run over all lags: larger score, then smaller lag, then smaller j1, then smaller j0 (what
 * a forward pass gives with a running prefix minimum updated on strict <, a best updated on strict >, lags in rising
 * order).  A clip is a hit only with a score >= 1; a query's k <= 64 hits are ordered by larger score, then smaller clip
 * id.  Exact integers: no floating point takes part in any order, and the result does not depend on scheduling.
 * Refused before a device is touched: null pointers, k outside 1..64, max_rate outside 1..31, decreasing q_off
 * (HPFW_E_INVALID); a query above 16000 hashprints (HPFW_E_UNSUPPORTED).  An empty index, empty queries, removed (empty)
 * clips, clips without a positive run and the slots past the last hit give padding records.  The ends of every hit come
 * from a walk of its diagonal that computes the score again; a walk that does not give the scan's score fails the call
 * (HPFW_E_HIP); the device form waits for its stream to learn that, unless there was nothing to scan.
 * Environment (tests; the results are the same bytes): HPFW_LOCAL_POPC -- the xor/popcount kernel for every query (it
 * otherwise serves queries whose window does not fit the LDS); HPFW_LOCAL_TABLE_KB=<KiB> -- the size of the (query, clip)
 * table of one pass over the queries (default and most 512 MiB, at least 32 queries' rows), for tests of more than one
 * pass.  The sharded index (hpfw_gpu_multi.h) has no local search. */
typedef struct {
    int32_t score;    /* T length - dist                                   */
    uint32_t clip;    /* as hpfw_hit; 0xffffffff = none                    */
    int32_t lag;      /* clip position of query position 0                 */
    uint32_t q_start; /* first query position of the run                   */
    uint32_t length;  /* hashprints of the run                             */
    uint32_t dist;    /* mismatching bits over the run                     */
} hpfw_local_hit; /* 24 B; padding: clip = 0xffffffff, rest 0 */
/* d_q_hp, d_out [n_q][k] device; q_off host */
int hpfw_gpu_search_local_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int max_rate, int k,
                                 hpfw_local_hit *d_out, void *stream);
/* host convenience: copies queries in and hits out, synchronises */
int hpfw_gpu_search_local(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int max_rate, int k,
                          hpfw_local_hit *out);

/* ---- local self-join: which recordings of the index share a passage, and where -- a sample lifted
 * into another track, one intro under two programmes, a medley, a set recorded twice with different talk around it.  The
 * self-join above rates everything two recordings have in common at a lag, so foreign material around a shared passage
 * hides the pair from it; this join rates the best RUN of consecutive hashprints, as the local search does, for every
 * unordered pair of the index once, where the index lies, at any indexed length up to 2^18 - 1 hashprints.
 *
 * The caller passes max_rate = T, 1 <= T <= 31, in mismatching bits per hashprint, and min_score >= 1; neither has a
 * default in any binding.
 * Take clips a < b of the index in add order, both live and non-empty.  Clip a takes the part of the query of the local
 * search above and b the part of the clip:
 *   lag d puts position j of a on position d + j of b, d = 1 - n_a .. n_b - 1;
 *   x_j = T - popcount(a[j] ^ b[d + j]);    a run [j0, j1) of positions both have scores the sum of its x_j.
 * The pair's candidate is its best run over all lags: larger score, then smaller lag, then smaller j1, then smaller j0
 * (what a forward pass gives with a running prefix minimum updated on strict <, a best updated on strict >, lags in rising
 * order).  The pair is REPORTED when score >= min_score.
 * Pairs come in ascending (a, b) with the clip base added to both ids.  The passage is a[a_start .. a_start + length) on
 * b[lag + a_start .. lag + a_start + length); score = T length - dist.  Exact integers: no floating point takes part in
 * any order, no atomics are used, and nothing depends on the order in which workgroups run.  Empty slots, removed
 * recordings and pairs without a qualifying run never appear.  A run that scores min_score has at least
 * ceil(min_score / T) positions, so only lags that overlap that much are scanned; that changes the work, not the result.
 * d_out receives the first cap reported pairs, *d_count (int64) their total number, which may exceed cap: the caller
 * enlarges the buffer and calls again.  An empty index and an index of one clip give count 0.
 * Refused before a device is touched (HPFW_E_INVALID): a null handle, max_rate outside 1..31, min_score < 1, cap < 0, a
 * null out with cap > 0, a null count.  An index that holds a recording above 2^18 - 1 hashprints is refused before a
 * kernel runs (HPFW_E_UNSUPPORTED): below that bound 2 * 31 * L < 2^24 and the doubled running score is exact in the fp32
 * accumulators.  The ends of every written pair come from a walk of its diagonal that computes the score again; a walk
 * that does not give the scan's score fails the call (HPFW_E_HIP); the device form waits for its stream to learn that,
 * unless there was nothing to scan.
 * HPFW_LOCALJOIN_POPC in the environment selects the xor/popcount kernel, HPFW_LOCALJOIN_SPLITS (1..64) the workgroups
 * that share a pair's lags, HPFW_LOCALJOIN_TABLE_KB the size of the table of one pass over the rows (default and most
 * 512 MiB); they are read at every call and change no result.  The sharded index (hpfw_gpu_multi.h) has no local
 * self-join. */
typedef struct {
    uint32_t a, b;    /* a < b, ids in add order + the clip base       */
    int32_t score;    /* T length - dist                               */
    int32_t lag;      /* position 0 of a lies on position lag of b     */
    uint32_t a_start; /* first position of the run in a                */
    uint32_t length;  /* hashprints of the run                         */
    uint32_t dist;    /* mismatching bits over the run                 */
    uint32_t pad;
} hpfw_passage_pair; /* 32 B */
int hpfw_gpu_index_localjoin_device(hpfw_gpu *h, int max_rate, int min_score, hpfw_passage_pair *d_out, int64_t cap,
                                    int64_t *d_count, void *stream);
/* host buffers (the null stream): out [cap], *count */
int hpfw_gpu_index_localjoin(hpfw_gpu *h, int max_rate, int min_score, hpfw_passage_pair *out, int64_t cap, int64_t *count);
/* host-only: *slice = the positions of a staged per pass over the LDS, *chunk = the lags of b one workgroup pass takes (a
 * pair's chunks begin at ceil(min_score / max_rate) - the longest of the 32 rows a that share the workgroup).  NULL is
 * HPFW_E_INVALID. */
int hpfw_gpu_localjoin_geometry(int32_t *slice, int32_t *chunk);

/* ---- events: time a region on `stream` with HIP events (bench.py uses these so that the
 * timing is taken on the stream the kernels run on) ---------------------------------------- */
int hpfw_gpu_timer_start(hpfw_gpu *h, void *stream);
int hpfw_gpu_timer_stop(hpfw_gpu *h, void *stream, float *ms); /* synchronises on the stop event */
/* per-kernel device time, measured with one HIP event pair per launch on the launch stream.
 * mask bit i enables kernel kind i in the order reported by hpfw_gpu_get_kernel_timing
 * (fwd_rows, fwd_cols, cq_chirpz, db, project_mfma, delta_pack, hamming_scan, topk, pcm_pairs); -1 = all,
 * 0 = off.  Setting the mask resets the accumulated times. */
int hpfw_gpu_set_kernel_timing(hpfw_gpu *h, int mask);
/* names[i] (static strings) and ms[i], launches[i] for i < *n; pass capacity in *n */
int hpfw_gpu_get_kernel_timing(hpfw_gpu *h, const char **names, float *ms, int *launches, int *n);

/* ---- host-only diagnostic: FNV-1a checksums of the eight groups of constant tables built for
 * clips of n_samples samples (twiddles, digit reversal, bands, window*chirp, chirp spectra).
 * No device is touched.  (For a chirp-z length slot 2, T_N, is the hash of nothing: see hpfw_gpu_chirpz_table.) */
int hpfw_gpu_plan_checksum(int64_t n_samples, uint64_t *out8);
/* the same with the chirp-z forward transform forced and under given conventions (HPFW_CONV_*) */
int hpfw_gpu_plan_checksum_ex(int64_t n_samples, int force_bluestein, unsigned conventions, uint64_t *out8);
/* host-only: the column stage's tables for a 7-smooth n_samples, copied out.  dims9 = {n1, n2, hq = n1 / 2 + 1,
 * cols_mt, cols_ks, cols2_mt, cols2_ks, 1 when the parity-split image exists, 0}.  Any other pointer may be NULL; otherwise
 * wq [2 n1] (Re, Im of rint(2^22 T_n1[m])), corr [2 hq], image [cols_mt * cols_ks * 3072] and image2
 * [cols2_mt * 2 * cols2_ks * 3072] bytes, the twiddle digits as the int8 matrix instructions read them. */
int hpfw_gpu_plan_cols_tables(int64_t n_samples, int32_t *dims9, int32_t *wq, double *corr, int8_t *image, int8_t *image2);
/* host-only: the shape of the chirp-z forward transform of n_samples (a length with a prime factor above 7, or
 * any length with force_bluestein).  out15 = {a, n1 = 16 a, L = n1 n2, slack = L - (n_samples + (kmax - kmin) - 1), k1lo, k1n,
 * need, nt2, n_tiles2, step, n_blocks, n2, n_tiles1, kmin, kmax}: the rows k1lo .. k1lo + k1n - 1 of the last stage hold the
 * consumed bins, in `need` row tiles of 32, nt2 per wave, n_tiles2 in the coefficient image; that stage walks the n1 residues
 * in n_blocks register sets of `step`.  -2 when the length takes the mixed-radix transform or is unsupported. */
int hpfw_gpu_plan_bz_shape(int64_t n_samples, int force_bluestein, int *out15);

/* ---- the projection's arithmetic.  The reference multiplies filters and frames in f32 (an Eigen/MKL sgemm,
 * parallel_collector.h:57,127) and keeps only the sign of P[r,i] - P[r,i+80] (hashprint_handle.h:119-122).  mode 1
 * (default): both factors rounded once to fixed point (S to 1/98304 dB, F to 2^-22 of its row's largest entry), the
 * lag-80 difference taken on the quantised spectrogram and its 2420-term sums with the filters exact integers on the
 * int8 matrix pipe (closer to the real-number product than an f32 sgemm in any order; no projection is
 * ever stored).  mode 0: the f32 fma chain in ascending k on the f32 matrix pipe.  The two differ in a
 * hashprint bit only where the difference of the two projections is within rounding of zero. */
int hpfw_gpu_set_projection(hpfw_gpu *h, int mode);
int hpfw_gpu_get_projection(hpfw_gpu *h);
/* dB spectrograms [n_clips][121][c] (device, as hpfw_gpu_stage_spectrogram writes them) -> hashprints
 * [n_clips][c - 99] with the handle's filters and projection mode */
int hpfw_gpu_hashprints_from_db(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, uint64_t *d_hp, void *stream);
/* ---- transposed queries: a performance in another key.  shifts: host array of 1 to 64 distinct
 * bin shifts, |s| <= 120 (24 bins per octave: t semitones up is s = +2t).  Shift s hashes the clip's dB spectrogram with
 * row b replaced by row b + s, -80 dB where b + s is not a bin, in projection mode 1; shifts = {0} gives what extraction
 * gives.  In projection mode 0, and for any other shifts argument, HPFW_E_INVALID.  d_hp [n_clips][n_shifts][n_hp]. */
int hpfw_gpu_extract_transposed_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips,
                                      const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream);
/* host buffers, as hpfw_gpu_extract_pcm16_host: copies in, runs, copies out, synchronises */
int hpfw_gpu_extract_transposed_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips,
                                           const int32_t *shifts, int n_shifts, uint64_t *hp);
/* dB spectrograms [n_clips][121][c] (device) -> d_hp [n_clips][n_shifts][c - 99] */
int hpfw_gpu_hashprints_from_db_transposed(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, const int32_t *shifts,
                                           int n_shifts, uint64_t *d_hp, void *stream);
/* one result of the transposed search: hpfw_hit and the index (in the caller's shift list) of the winning shift */
typedef struct {
    uint32_t dist;       /* smallest distance of the clip over all shifts   */
    uint32_t clip;       /* as hpfw_hit; 0xffffffff = none                  */
    int32_t offset;      /* first offset reaching dist in that shift        */
    int32_t shift_index; /* smallest shift index reaching dist; -1 = none   */
} hpfw_shift_hit;
/* query set q * n_shifts + i (q_off [n_q * n_shifts + 1]) holds shift i of query q.  Per clip the smallest distance over
 * the shifts, ties to the smallest shift index; the k best clips by (dist, clip), padded as hpfw_gpu_search_topk pads.
 * k <= 64, n_shifts <= 64.  out [n_q][k]. */
int hpfw_gpu_search_topk_transposed_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                           int n_shifts, int k, hpfw_shift_hit *d_out, void *stream);
int hpfw_gpu_search_topk_transposed(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts,
                                    int k, hpfw_shift_hit *out);
/* ---- queries at another tempo: a performance faster or slower than the indexed recording.
 * tempos: host array of 1 to 64 finite factors in [0.5, 2] (query tempo / indexed tempo; 1.05 = played 5 % faster) whose
 * steps rint(65536 / tempo) are distinct.  Tempo rho rescales the query's dB spectrogram S [121][C] onto the indexed time
 * axis: column k interpolates S linearly at source column k step / 65536 (64-bit fixed point, exact products in double,
 * one rounding to float).  Every tempo of a call is cut to the common length c_t = min over the tempos of
 * floor((C - 1) 65536 / step) + 1 columns, so every variant has n_hp_t = c_t - 99 hashprints and the distances of
 * different tempos are comparable; offsets are positions in the indexed recording.  shifts: NULL with n_shifts = 0 (no
 * shift), or a list as the transposed entry points take it; variant v = j max(n_shifts, 1) + i is tempo j with shift i,
 * n_tempos max(n_shifts, 1) <= 64.  tempos = {1.0} gives what extraction gives.  Projection mode 1 only; any other argument
 * is HPFW_E_INVALID (checked before the handle is used), n_hp_t < 1 is HPFW_E_UNSUPPORTED.
 * d_hp [n_clips][n_tempos][max(n_shifts, 1)][n_hp_t].  To search, pass the V = n_tempos max(n_shifts, 1) sets of each
 * query to hpfw_gpu_search_topk_transposed(_device) with n_shifts = V: a hit's shift_index is then v. */
/* c_t of a clip of c columns under a tempo list (no handle needed) */
int hpfw_gpu_tempo_columns(int64_t c, const float *tempos, int n_tempos, int64_t *c_out);
/* dB spectrograms [n_clips][121][c] (device, as hpfw_gpu_stage_spectrogram writes them) -> d_hp as above */
int hpfw_gpu_hashprints_from_db_tempo(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, const float *tempos,
                                      int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream);
int hpfw_gpu_extract_tempo_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_samples, int64_t n_clips, const float *tempos,
                                 int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *d_hp, void *stream);
/* host buffers, as hpfw_gpu_extract_pcm16_host: copies in, runs, copies out, synchronises */
int hpfw_gpu_extract_tempo_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, const float *tempos,
                                      int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *hp);
/* parity checkpoint of mode 1: the exact integer sums D[r][i] = sum_k fq[r][k] (u[k][i] - u[k][i + 80]) whose signs are
 * the hashprint bits, d_delta [n_clips][64][c - 99] int64 (device); d_hp may be NULL.  The nine-product kernel, which
 * the extraction runs under HPFW_Q_PRODUCTS=9. */
int hpfw_gpu_stage_delta_q(hpfw_gpu *h, const float *d_db, int64_t n_clips, int64_t c, int64_t *d_delta, uint64_t *d_hp,
                           void *stream);
/* the six-product split (the default of mode 1's unshifted extraction; HPFW_Q_PRODUCTS=9 in the environment when the handle
 * is created switches it off): of the last such launch on this handle, its tiles of 128 hashprints, the values listed
 * for exact recomputation and the tiles redone with nine products.  Waits for the device; zeros without such a launch.
 * The kernel settles the listed values and the redone tiles itself. */
int hpfw_gpu_debug_q_products(hpfw_gpu *h, int64_t *tiles, int64_t *listed, int64_t *redone);

/* ---- timeline of a long recording: scored search, windows of one recording, segments.
 *
 * Scored search.  The scan leaves, per query and clip, the clip's best distance d_c.  The scored entry points return the
 * hits of their unscored counterparts, bit for bit, and per query row the exact integer moments of d_c over the COUNTED
 * clips: those with n_c >= k_q >= 1 hashprints (k_q the query's length).  A shorter clip is compared over n_c < k_q
 * hashprints (storage.h:37-39), so its distance is on another scale and it is left out.  n, sum d_c and sum d_c^2 do not
 * depend on the order of summation: they are bitwise deterministic.  d_c <= 64 * 16000 < 2^20, so sum_sq is exact while
 * n_clips * k_max^2 * 4096 < 2^64 (k_max the longest query of the call); beyond that the call is refused with
 * HPFW_E_UNSUPPORTED before anything runs.  An empty index or an empty query gives n = 0.  The moments are additive over
 * the shards of a sharded index. */
typedef struct {
    uint64_t sum, sum_sq; /* sum of d_c and of d_c^2 over the counted clips */
    uint32_t n, pad;      /* number of counted clips                       */
} hpfw_dist_stats;
/* as hpfw_gpu_search_topk(_device); stats [n_q] (device pointer in the device form) */
int hpfw_gpu_search_topk_scored_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k,
                                       hpfw_hit *d_out, hpfw_dist_stats *d_stats, void *stream);
int hpfw_gpu_search_topk_scored(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *out,
                                hpfw_dist_stats *stats);
/* as hpfw_gpu_search_topk_transposed(_device); stats [n_q][n_shifts], one row per variant set.  A merged hit's distance is its
 * clip's best distance in the winning set, so the hit is scored against stats[q][shift_index]. */
int hpfw_gpu_search_topk_transposed_scored_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                                  int n_shifts, int k, hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats,
                                                  void *stream);
int hpfw_gpu_search_topk_transposed_scored(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts,
                                           int k, hpfw_shift_hit *out, hpfw_dist_stats *stats);

/* ---- search within sets of clips: every query names the set of clips it may be answered with.
 *
 * Arguments.  A call brings n_sets >= 0 sets in CSR form and a set per query, all on the host:
 *   set_off [n_sets + 1], set_off[0] = 0, not decreasing;
 *   set_clips [set_off[n_sets]]: the clips of set s are set_clips[set_off[s] .. set_off[s + 1]), indexes in add order (without
 *     clip_base), STRICTLY ASCENDING inside a set.  A clip may be in many sets, a set may be empty;
 *   q_set [n_q]: the set of each query, or -1 for "the whole index".
 * Equality with the sub-index.  Query q with s = q_set[q] >= 0 is answered exactly as hpfw_gpu_search_topk would answer it on
 * an index that holds only the clips of set s, in that order, with the clip ids mapped back to this index's (clip_base added
 * as in hpfw_hit): the order (dist, clip), the offsets, the padding records past the set's size and the rule for clips
 * shorter than the query (storage.h:37-39) are the sub-index's.  Strict ascent is what makes the sub-index's tie order by
 * clip id this index's.  With stats (may be NULL) the same holds for hpfw_gpu_search_topk_scored: the moments are those of
 * the counted clips of the set (n_c >= k_q >= 1).  A set may name an emptied slot (a removed recording, hpfw_gpu_index_remove):
 * it behaves as an empty clip of the sub-index does.  A query with q_set = -1 gets the bytes of the unrestricted call.
 * Nothing floats on the device and nothing depends on the order workgroups run in.  The work is that of searching the
 * sets: the scans are launched for the listed clips only and the table of a query is as wide as its set.
 * The transposed forms: q_off [n_q n_shifts + 1] and stats [n_q][n_shifts] as hpfw_gpu_search_topk_transposed_scored takes
 * them, q_set [n_q] with one entry per query (for all its variants); shift_index is the sub-index's.
 * Refused with HPFW_E_INVALID before a device is touched: n_sets < 0, null set_off with n_sets > 0, set_off[0] != 0, a
 * decreasing set_off, a set that is not strictly ascending or holds a negative clip, null q_set, a q_set entry below -1 or
 * at or above n_sets, and everything the unrestricted call refuses.  Refused once the index is known, before a kernel runs:
 * a clip at or above the number of slots (HPFW_E_INVALID); with stats, n k_max^2 4096 >= 2^64 (HPFW_E_UNSUPPORTED), n the
 * largest set a query names (the index for a -1 query).  The set arrays have been read when the call returns (the device
 * forms wait for the stream when a query is restricted). */
int hpfw_gpu_search_topk_within_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k,
                                       const int64_t *set_off, int64_t n_sets, const int32_t *set_clips, const int32_t *q_set,
                                       hpfw_hit *d_out, hpfw_dist_stats *d_stats, void *stream);
int hpfw_gpu_search_topk_within(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k,
                                const int64_t *set_off, int64_t n_sets, const int32_t *set_clips, const int32_t *q_set,
                                hpfw_hit *out, hpfw_dist_stats *stats);
int hpfw_gpu_search_topk_transposed_within_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                                  int n_shifts, int k, const int64_t *set_off, int64_t n_sets,
                                                  const int32_t *set_clips, const int32_t *q_set, hpfw_shift_hit *d_out,
                                                  hpfw_dist_stats *d_stats, void *stream);
int hpfw_gpu_search_topk_transposed_within(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts,
                                           int k, const int64_t *set_off, int64_t n_sets, const int32_t *set_clips,
                                           const int32_t *q_set, hpfw_shift_hit *out, hpfw_dist_stats *stats);

/* Host only: how far a hit of distance `dist` stands out from the other counted clips of its row.  counted: whether the
 * hit's clip is counted (the caller knows the query's and the clip's lengths).  With n' = n - 1 the others have mean
 * m = (sum - d) / n' and variance var = (n' (sum_sq - d^2) - (sum - d)^2) / n'^2 (numerators in exact 128-bit integers,
 * converted to double once); *score = (m - d) / sqrt(var).  *score is NaN, with status OK, when counted == 0, n < 3 or
 * var == 0.  Moments no set of distances can have (d > sum, d^2 > sum_sq, a negative variance) are HPFW_E_INVALID. */
int hpfw_gpu_hit_score(uint32_t dist, int counted, const hpfw_dist_stats *s, double *score);
/* What a sharded search does with the gathered per-shard results, on the device that holds them (include/hpfw_gpu_multi_search.h).
 * device twin of hpfw_gpu_merge_topk: records are hpfw_hit or hpfw_shift_hit (same 16-byte layout, key (dist, clip)); d_in
 * [n_shards][n_q][k] -> d_out [n_q][k], bit for bit what hpfw_gpu_merge_topk gives on the same bytes (records of equal key keep
 * their input order, the words after the key travel with their record).  dist < 2^20, as every search returns it, but for
 * the padding record dist = clip = 0xffffffff.  n_shards in 1..64, k in 1..64, 16-byte aligned pointers, d_out apart from d_in. */
int hpfw_gpu_merge_topk_device(hpfw_gpu *h, const void *d_in, int n_shards, int64_t n_q, int k, void *d_out, void *stream);
/* d_out[r] = sum over shards of d_in[shard][r], r < rows: sum and sum_sq modulo 2^64, n modulo 2^32, pad = 0 */
int hpfw_gpu_sum_stats_device(hpfw_gpu *h, const hpfw_dist_stats *d_in, int n_shards, int64_t rows, hpfw_dist_stats *d_out,
                              void *stream);

/* Windows of ONE recording of n_total samples: window w is samples [w hop, w hop + win).  Host only:
 * *n_w = (n_total - win) / hop + 1, 0 when n_total < win.  1 <= hop <= win, win a supported clip length
 * (hpfw_gpu_supported_length(win) == win), n_total >= 0; anything else is HPFW_E_INVALID. */
int hpfw_gpu_window_count(int64_t n_total, int64_t win, int64_t hop, int64_t *n_w);
/* Hashprints of every window.  The recording may be of any length: only win has to be a clip length.  tempos == NULL and
 * shifts == NULL (n_tempos = n_shifts = 0): d_hp [n_w][n_hp], what hpfw_gpu_extract_pcm16 gives for the windows copied out
 * back to back, bit for bit, in either projection mode.  shifts only: d_hp [n_w][n_shifts][n_hp] as
 * hpfw_gpu_extract_transposed_pcm16; tempos (with or without shifts): d_hp [n_w][V][n_hp_t] as
 * hpfw_gpu_extract_tempo_pcm16; the argument checks and the requirement of projection mode 1 are theirs.  The windows are
 * gathered on the device, a pass of clips (hpfw_gpu_set_batch) at a time, and each pass goes through the existing
 * extraction.  The host form uploads the recording once. */
int hpfw_gpu_extract_windows_pcm16(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_total, int64_t win, int64_t hop,
                                   const float *tempos, int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *d_hp,
                                   void *stream);
int hpfw_gpu_extract_windows_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_total, int64_t win, int64_t hop,
                                        const float *tempos, int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *hp);

/* Segments: a pure function of the per-window best hits, no device and no handle.
 * Window w sits at t_w = w * hop_cols index columns, hop_cols = hop * M / (3 * win) in double with M from
 * hpfw_gpu_geometry(win) (one column is 3 win / M samples).
 * Rule.  A window is STRONG when it has a hit (clip != 0xffffffff) and score >= min_score; NaN is never strong.  The windows
 * are scanned left to right.  The first strong window opens a segment.  With l the open segment's last accepted window, a
 * later strong window w CONTINUES it when it names the same clip, w - l - 1 <= max_gap, and
 *     fabs((o_w - o_l) - rho_l * (t_w - t_l)) <= tol_cols * (w - l)
 * (o: offset, rho: tempo; evaluated in double exactly as written).  A strong window that does not continue the open segment
 * closes it and opens a new one; a segment also closes once more than max_gap windows have passed since l without a
 * continuation.  A closed segment is kept when it holds at least min_windows strong windows.  Segments come out in order
 * of their first window. */
typedef struct {
    uint32_t clip;   /* the window's best clip; 0xffffffff = none                            */
    int32_t offset;  /* its offset in index columns                                          */
    int32_t variant; /* the variant (shift_index) that found it; 0 without variants          */
    int32_t pad;
    double tempo;    /* the variant's tempo factor rho; 1 without tempos                     */
    double score;    /* hpfw_gpu_hit_score of the hit                                        */
} hpfw_window_hit;
typedef struct {
    double min_score;    /* REQUIRED: > 0 (<= 0 or NaN is HPFW_E_INVALID); there is no default            */
    double hop_cols;     /* > 0, finite                                                                   */
    double tol_cols;     /* > 0; 0 = the default max(2, 0.08 hop_cols); negative or NaN is invalid        */
    int64_t win, hop;    /* samples, 1 <= hop <= win: a segment's start = first * hop, end = last * hop + win */
    int32_t max_gap;     /* >= 0; -1 = the default 1                                                      */
    int32_t min_windows; /* >= 1; 0 = the default 1                                                       */
} hpfw_timeline_params;
typedef struct {
    uint32_t clip;
    int32_t n_strong;     /* strong windows accepted                                 */
    int64_t first, last;  /* first and last accepted window                          */
    int64_t start, end;   /* samples                                                 */
    int64_t best_window;  /* the best-scoring accepted window, the earliest on ties  */
    double best_score;    /* its score, offset, variant and tempo                    */
    double best_tempo;
    int32_t best_offset, best_variant;
    int32_t first_offset; /* the offset at the first window                          */
    int32_t pad;
} hpfw_segment;
/* *n_seg = the number of segments kept; the first min(*n_seg, cap) are written (out may be NULL when cap = 0) */
int hpfw_gpu_timeline_segments(const hpfw_window_hit *w, int64_t n_w, const hpfw_timeline_params *p, hpfw_segment *out,
                               int64_t cap, int64_t *n_seg);

/* ---- scored overlap search: how far a hit of hpfw_gpu_search_overlap stands out from the rest of
 * the index, so that windows of a timeline can be searched by the overlap rule.
 *
 * A candidate (dist, L, lag) is ordered by the exact rational dist / L; for statistics it is mapped to one integer,
 *     rate(dist, L) = floor(dist * 2^HPFW_OVERLAP_RATE_BITS / L),   L >= 1, dist <= 64 L.
 * L <= 16000, so the numerator is below 2^30 and a 32-bit unsigned division is exact; rate <= 2^16.  The scored entry points
 * return the hits of their unscored counterparts byte for byte and, per query row, the moments {sum, sum_sq, n} of rate_c
 * over the COUNTED clips: those that have a candidate for the query (n_c >= min_overlap and k_q >= min_overlap) and are not
 * the query's exclude entry.  rate^2 <= 2^32 and an index holds fewer than 2^31 clips, so sum_sq stays below 2^63 for every
 * index the overlap search accepts: no call is refused because a sum could wrap.  The sums are integers, so they are bitwise
 * deterministic for any number of splits, slices and query groups and for either scan kernel; no floating point runs on the
 * device.  An empty index, an empty query and a query below min_overlap give n = 0.
 * The score of a hit is hpfw_gpu_hit_score(rate(hit.dist, hit.overlap), 1, &stats[q], &score): a clip that is hit is counted.
 * Refusals as hpfw_gpu_search_overlap's, and a null stats pointer (HPFW_E_INVALID). */
#define HPFW_OVERLAP_RATE_BITS 10
/* d_q_hp, d_out [n_q][k], d_stats [n_q] device; q_off, exclude host */
int hpfw_gpu_search_overlap_scored_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q,
                                          const int32_t *exclude, int min_overlap, int k, hpfw_overlap_hit *d_out,
                                          hpfw_dist_stats *d_stats, void *stream);
int hpfw_gpu_search_overlap_scored(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                                   const int32_t *exclude, int min_overlap, int k, hpfw_overlap_hit *out,
                                   hpfw_dist_stats *stats);
/* Host only: *rate = rate(dist, overlap).  overlap == 0, overlap > 16000 or dist > 64 overlap is HPFW_E_INVALID. */
int hpfw_gpu_overlap_rate(uint32_t dist, uint32_t overlap, uint32_t *rate);
/* Host only: the part of a window that lies on the clip it was found in, in samples of the window.  The window has k_q
 * hashprints and was found at lag `lag` on a clip of n_clip hashprints; a hashprint spans `span` columns (S = c - n_hp + 1 of
 * hpfw_gpu_geometry(win), 100 for the live-id configuration), and one column is col = 3 win / m samples (m of the same
 * geometry).  In columns the window lies on the clip over
 *     a_cols = max(0, -lag),   b_cols = min(k_q + span - 1, n_clip + span - 1 - lag),
 * and *a = floor(a_cols col + 0.5), *b = min(win, floor(b_cols col + 0.5)), evaluated in double exactly as written.  For a
 * hit inside the clip (0 <= lag <= n_clip - k_q) that is the whole window, [0, win).  A segment of windows searched by the
 * overlap rule starts at first * hop + a(first window) and ends at last * hop + b(last window).
 * n_clip, k_q, span, win or m below 1, or a lag at which window and clip share no hashprint, is HPFW_E_INVALID. */
int hpfw_gpu_overlap_extent(int32_t lag, int64_t n_clip, int64_t k_q, int64_t span, int64_t win, int64_t m, int64_t *a,
                            int64_t *b);

/* ---- live feeds: the timeline of feeds that are still running, as their samples arrive.
 *
 * A set of n_streams feeds on one handle, each a ring of `capacity` samples in device memory.  A feed is mono PCM16 at 44.1 kHz
 * or, in a set made by hpfw_gpu_streams_create_rates, at any integer rate fs in [8 000, 192 000] Hz: its chunks are converted to
 * 44.1 kHz on their way into the ring.  n_i: the samples feed i has received (at its own rate), e_i: the windows of it already
 * handed out.  y_i: the feed at 44.1 kHz.  For a 44.1 kHz feed y_i is what was pushed; for a feed at fs, with (L, M, T = 2 H) of
 * hpfw_gpu_resample_table(fs), it is y_i[0 .. emitted(n_i)), the first emitted(n_i) = (n_i <= H ? 0 : ceil((n_i - H) L / M))
 * samples of what hpfw_gpu_resample_pcm16 gives for everything pushed to the feed as one clip: output m reads the inputs up to
 * floor(m M / L) + H and is given once they have arrived.  H zero samples pushed behind a feed that has ended bring out the
 * rest: emitted(n + H) = hpfw_gpu_resample_length(n).  Window w of a feed is y_i[w hop, w hop + win), as hpfw_gpu_window_count
 * cuts a recording; the ring holds y_i[e_i hop, emitted(n_i)).  win, hop and capacity are in 44.1 kHz samples.
 * CONTRACT.  The hashprints of window w of a feed equal, bit for bit, what hpfw_gpu_extract_windows_pcm16 gives for window w
 * of y_i -- everything pushed to that feed since its last reset, converted as one clip -- and the clips equal those samples:
 * whatever the chunking (chunks of 0 samples, of 1 sample, of fewer than T), the other feeds and their rates, cap, and however
 * often the ring has wrapped.
 * A set works in its handle's workspaces: calls on it are ordered with every other call on the handle, it is used by one
 * thread at a time, and it is destroyed before the handle. */
typedef struct hpfw_gpu_streams hpfw_gpu_streams;
typedef struct {
    int32_t n_streams;     /* 1 .. 4096                                                                  */
    int32_t n_tempos;      /* tempos / shifts as hpfw_gpu_extract_windows_pcm16 takes them: NULL and 0 for  */
    int32_t n_shifts;      /* none; the lists are copied                                                 */
    int32_t pad;
    int64_t win, hop;      /* samples, as hpfw_gpu_window_count: 1 <= hop <= win, win a supported length  */
    int64_t capacity;      /* samples per ring, >= win; 0 = 2 win                                        */
    const float *tempos;
    const int32_t *shifts;
} hpfw_streams_params;
typedef struct {
    int32_t feed, pad;
    int64_t window;
} hpfw_stream_window;
typedef struct {
    int64_t per_window;    /* hashprints per window: [V][n_hp_v] flattened, as hpfw_gpu_extract_windows_pcm16 lays them out */
    int64_t win, hop, capacity;
    int32_t n_streams, n_sets; /* n_sets = V: max(n_tempos, 1) max(n_shifts, 1)                           */
} hpfw_streams_info;
/* Every check of hpfw_gpu_extract_windows_pcm16 with its messages (the lists first, then the handle, projection mode 1 for
 * variants, the filters), after n_streams, win / hop and capacity.  Builds the tables of `win` and allocates the rings. */
int hpfw_gpu_streams_create(hpfw_gpu *h, const hpfw_streams_params *p, hpfw_gpu_streams **out);
/* The same with rates [n_streams], the sample rate of every feed; NULL: 44 100 Hz for all, which is hpfw_gpu_streams_create.  A
 * rate outside [8 000, 192 000] is HPFW_E_UNSUPPORTED (after n_streams, before everything else: the handle is not used) and the
 * message names the first such feed.  Also builds the conversion tables of every distinct rate (the cache of
 * hpfw_gpu_resample_pcm16) and allocates per feed at another rate two histories of T - 1 input samples. */
int hpfw_gpu_streams_create_rates(hpfw_gpu *h, const hpfw_streams_params *p, const int32_t *rates, hpfw_gpu_streams **out);
void hpfw_gpu_streams_destroy(hpfw_gpu_streams *s);
/* Appends counts[i] >= 0 samples to feed i, for every feed: pcm holds the chunks concatenated in feed order (host memory; the
 * device form takes a device pointer and enqueues on `stream`), each chunk counted in samples at its feed's rate.  One upload,
 * one launch for the 44.1 kHz feeds that take part and one per other rate among those that do.
 * A chunk that does not fit (counts[i] > room[i] below) makes the whole call HPFW_E_INVALID: nothing is appended to any feed, no
 * history moves, and the message names the first such feed.  *n_ready (may be NULL): complete windows not yet handed out, over
 * all feeds.  pcm may be NULL when every count is 0. */
int hpfw_gpu_streams_push(hpfw_gpu_streams *s, const int16_t *pcm, const int64_t *counts, int64_t *n_ready);
int hpfw_gpu_streams_push_device(hpfw_gpu_streams *s, const int16_t *d_pcm, const int64_t *counts, int64_t *n_ready, void *stream);
/* room[i]: the samples feed i can take now, at its own rate: H + floor((e_i hop + capacity) M / L) - n_i, the most it can hold
 * while emitted <= e_i hop + capacity; at 44.1 kHz (L = M = 1, H = 0) that is capacity - (n_i - e_i hop) */
int hpfw_gpu_streams_room(hpfw_gpu_streams *s, int64_t *room);
/* Hashes up to cap >= 0 ready windows in order of (feed, window) ascending; the others stay ready.  *n: how many; which [*n]
 * (host, room for min(cap, ready) entries) names them; d_hp [*n][per_window]; d_clips NULL or [*n][win], the windows' samples.
 * The windows go through the extraction a pass of clips (hpfw_gpu_set_batch) at a time, one gather launch per pass.  The
 * host form downloads and synchronises. */
int hpfw_gpu_streams_extract(hpfw_gpu_streams *s, int64_t cap, uint64_t *d_hp, int16_t *d_clips, hpfw_stream_window *which, int64_t *n,
                             void *stream);
int hpfw_gpu_streams_extract_host(hpfw_gpu_streams *s, int64_t cap, uint64_t *hp, int16_t *clips, hpfw_stream_window *which, int64_t *n);
/* feed `stream` starts again at sample 0 and window 0 (a feed that reconnects); its windows not yet handed out are dropped */
int hpfw_gpu_streams_reset(hpfw_gpu_streams *s, int stream);
/* info, received [n_streams] = n_i (samples pushed, at the feed's rate) and extracted [n_streams] = e_i; each may be NULL */
int hpfw_gpu_streams_info(hpfw_gpu_streams *s, hpfw_streams_info *info, int64_t *received, int64_t *extracted);
/* rates [n_streams] and emitted [n_streams] = emitted(n_i), the 44.1 kHz samples each ring has received; each may be NULL */
int hpfw_gpu_streams_rates(hpfw_gpu_streams *s, int32_t *rates, int64_t *emitted);
/* *n_out = emitted(n_in) of a feed at `rate` (n_in itself at 44 100 Hz).  Host only, no handle; a rate outside the range or
 * n_in < 0 is HPFW_E_INVALID, as for hpfw_gpu_resample_length. */
int hpfw_gpu_streams_emitted(int64_t n_in, int rate, int64_t *n_out);

/* Segments as the windows arrive: hpfw_gpu_timeline_segments one push at a time.  Host only, no handle.  Windows are numbered
 * from 0 in push order; the parameter checks and messages are those of hpfw_gpu_timeline_segments.
 * CONTRACT.  For any window list and any partition of it into pushes, the popped segments followed by those popped after
 * _finish equal hpfw_gpu_timeline_segments on the whole list, byte for byte.
 * A segment whose last accepted window is l is closed, and can be popped, after the push of the first window that shows that
 * nothing continues it: a strong window that does not continue it, or window l + max_gap + 1 when that one does not. */
typedef struct hpfw_timeline_tracker hpfw_timeline_tracker;
int hpfw_gpu_timeline_tracker_create(const hpfw_timeline_params *p, hpfw_timeline_tracker **out);
void hpfw_gpu_timeline_tracker_destroy(hpfw_timeline_tracker *t);
int hpfw_gpu_timeline_tracker_push(hpfw_timeline_tracker *t, const hpfw_window_hit *w, int64_t n_w);
/* takes up to cap closed and kept segments off the queue, oldest first; *n: how many were written */
int hpfw_gpu_timeline_tracker_pop(hpfw_timeline_tracker *t, hpfw_segment *out, int64_t cap, int64_t *n);
/* the segment in progress as it would close now, whatever min_windows; *has = 0 when none is open */
int hpfw_gpu_timeline_tracker_open(hpfw_timeline_tracker *t, hpfw_segment *cur, int *has);
/* closes the segment in progress (kept when it holds min_windows strong windows); the window numbering goes on */
int hpfw_gpu_timeline_tracker_finish(hpfw_timeline_tracker *t);

/* ---- table preparation ahead of time.  A corpus of real recordings brings a new clip length with almost every file,
 * and the host half of a length's tables (constant-Q windows and chirp spectra, twiddles) costs more than the
 * extraction of the file: 3 ms for 30 s, 15 ms for 3 minutes.  hpfw_gpu_prepare_length builds that half on the
 * CALLING thread and keeps it for the next call that meets the length; it may be called from any number of threads
 * concurrently with any other call on the handle (the collectors' file-reader threads do so for every file they
 * decode).  Returns HPFW_E_UNSUPPORTED for a length outside the supported range. */
int hpfw_gpu_prepare_length(hpfw_gpu *h, int64_t n_samples);

/* ---- diagnostic: the tables of the chirp-z forward transform (clip lengths with a prime factor above 7), which are
 * generated on the device.  which: 0 = chirp w [n1][n2], 1 = T_L [n1][n2], 2 = Bhat [n1][n2],
 * 3 = w[k] / L [kmax - kmin]; complex as (re, im) float pairs.  *count = floats in the table; out may be NULL to
 * ask for the count only.  HPFW_E_INVALID for a 7-smooth length (unless HPFW_FORCE_BLUESTEIN is set).
 * which = 4, for EVERY length: the constant-Q stage's window table (121 bands concatenated, sum of Lg values), which is
 * generated on the device too (reference cqt.h:54-61: essentia builds these windows per file). */
int hpfw_gpu_chirpz_table(hpfw_gpu *h, int64_t n_samples, int which, float *out, int64_t capacity, int64_t *count);

/* ---- diagnostic: the handle's extraction workspaces as the last call left them (device pointers; valid until the next
 * call that grows them).  which: 0 = z, the column stage's output (chunked forward transform: one region per stream),
 * 1 = forward bins in the rows layout, 2 = dB terms / spectrograms, 4 = wave maxima.  Used by tools/ and tests to name
 * the first stage that differs; not part of the reference's interface. */
int hpfw_gpu_debug_workspace(hpfw_gpu *h, int which, void **d_ptr, size_t *bytes);

/* ---- diagnostic: the two evaluations of the dB term (the specified sequence, and the table and short
 * polynomial that stand in for it) on the `count` consecutive float bit patterns from `first`, on the current device.
 * out[0] = patterns whose results differ (0 is the claim), out[1] = patterns in 1e-10f <= p < inf for which the fast
 * evaluation was not certain and ran the specified sequence, out[2] = the first differing pattern (all ones: none). */
int hpfw_gpu_debug_db_term_sweep(uint32_t first, uint64_t count, uint64_t out[3]);

/* ---- legacy FFI: modules/python/parallel_collector_wrapper.hpp:12-38, same shapes --------- */
typedef struct {
    char *filename;
    uint64_t *hashprint;
    int hp_size;
} FilenameHashprintPair; /* wrapper.hpp:12-16 */

typedef struct hpfw_legacy_collector hpfw_legacy_collector; /* stands in for LiveIdCollector */

hpfw_legacy_collector *par_collector_new(void);                         /* wrapper.hpp:21 */
void par_collector_del(hpfw_legacy_collector *collector);               /* wrapper.hpp:23 */
FilenameHashprintPair *par_collector_prepare(hpfw_legacy_collector *collector,
                                             const char **filenames, int n, int *got); /* :25-28 */
uint64_t *par_collector_calc_hashprint(hpfw_legacy_collector *collector, const char *filename,
                                       int *size);                      /* wrapper.hpp:30 */
void par_collector_save(hpfw_legacy_collector *collector, const char *cache); /* wrapper.hpp:32 */
void par_collector_load(hpfw_legacy_collector *collector, const char *cache); /* wrapper.hpp:34 */
/* not in the reference's FFI: calc_hashprint for a list of files in one call (batched like prepare,
 * nothing learned) -- what LiveSongIdentification::search (live_song_id.h:37-41) does query by query.
 * n entries in input order, release with prepare_result_free(res, n); a file that failed has
 * hashprint == NULL and hp_size == 0; NULL when no filters are loaded */
FilenameHashprintPair *par_collector_calc_hashprints(hpfw_legacy_collector *collector,
                                                     const char **filenames, int n);
void prepare_result_free(FilenameHashprintPair *res, int got);          /* wrapper.hpp:36 */
void calc_hashprint_result_free(uint64_t *hp);                          /* wrapper.hpp:38 */
/* not in the reference's FFI: on != 0 makes the collector accept WAV files at any rate in [8 000, 192 000] Hz and
 * resample them to 44.1 kHz on the GPU before the extraction (hpfw_gpu_resample_pcm16).  Off by default: files at
 * other rates are skipped with a message, as before. */
int hpfw_gpu_collector_set_resample(hpfw_legacy_collector *collector, int on);

#ifdef __cplusplus
}
#endif
#endif
