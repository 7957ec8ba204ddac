// kernels.h -- host-callable launchers of the gfx950 kernels (one per hot loop of the reference,
// SURVEY.md section 2.1).  Each launcher only enqueues on `stream`.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hpfw_gpu.h"
#include "device_math.h"
#include "fft_lds.h"
#include "fft_rows.h"
#include "index_plan.h"
#include "join_plan.h"
#include "streams_plan.h"
#include "xcorr_plan.h"

namespace hpfw {

// "once per device" for hipFuncSetAttribute calls: a process may hold handles on several devices (one
// handle = one device), and a launcher may be entered from several host threads
struct PerDeviceOnce {
    std::atomic<uint64_t> done{0};
    static uint64_t bit()
    {
        int dev = 0;
        (void)hipGetDevice(&dev);
        return 1ull << (dev & 63);
    }
    bool need() const { return !(done.load(std::memory_order_acquire) & bit()); }
    void mark() { done.fetch_or(bit(), std::memory_order_release); } // after the calls: a second thread may repeat them, harmlessly
};


constexpr int kBins = 121;
constexpr int kCtx = 20;
constexpr int kLag = 80;
constexpr int kFilters = 64;
constexpr int kFrame = kBins * kCtx;

// S6, the column stage of the forward transform on the int8 matrix cores (k_forward.hip): the clip as it lies is an
// [n1][n2] sample matrix; rows q1 <= n1 / 2 of its length-n1 DFT down the columns, exact integers, rounded once to f32
// (the row stage multiplies them by the twiddles between the stages on its way in).
constexpr int kZBlock = 128;   // columns per block of the column stage's output (= columns per workgroup of both column kernels)
inline long long z_floats_per_clip(int hq, int n2) { return (long long)((n2 + kZBlock - 1) / kZBlock) * 2 * hq * kZBlock; }

struct ColsQArgs {
    int n1, n2, hq;      // hq = n1 / 2 + 1 rows
    int mt, ks;          // 32-row tiles of the (Re, Im) interleaved rows; 32-sample steps of k1
    const void *image;   // digits of the fixed-point twiddles as the A operand [mt][ks][3][64][16 bytes]
    const double *corr;  // [2 hq]: what the samples' +128 digit offset adds to every element of a row
    long long *stamps;   // diagnostic builds (-DHPFW_COLS_STAMPS) only: per workgroup 8 cycle sums
    int n_clips;         // set by the launch of the register-resident kernel: its grid is one-dimensional
    int variant;         // HPFW_COLS_VARIANT at handle creation (tests, diagnosis), bits: 1 = the LDS-staged kernel for every n1;
                         // 2 = the un-split register-resident kernel for even n1 too
    int mt2, ks2;        // even n1 <= 224, split by the parity of k1: 16-row tiles of the rows q1 <= n1 / 4; 64-sample steps per parity
    const void *image2;  // ... and the twiddle digits as the 16x16x64 A operand [mt2][2 ks2][3][64][16 bytes] (null: not split)
    long long zclip;     // floats of z per clip: z is [clip][block of kZBlock columns][row 2 q1 + (Re: 0, Im: 1)][kZBlock] (round 4: a
                         // workgroup's stores of a tile are then ONE contiguous 16 KB instead of 32 pieces 25 KB apart)
};

// Where the forward bins of one clip lie: in natural order from bin q0 on (n1 == 1: the chirp-z forward transform, the
// stage entry points), or as the row stage of S6 leaves them, x[k mod n1][k / n1 - q0] in rows of w elements.
#ifndef HPFW_XS_BATCH
#define HPFW_XS_BATCH 4
#endif
constexpr int kXsBatch = HPFW_XS_BATCH; // elements per thread whose loads are in flight together in the band loaders below
struct XsView {
    const cf *base;
    int n1, w, q0;
    // ceil(2^40 / n1): k / n1 = (k magic) >> 40 for every k < 2^27, n1 <= 2^13.  With e = magic n1 - 2^40 < n1 the product is
    // 2^40 (k / n1 + k e / (2^40 n1)), and the floor is that of k / n1 while k e < 2^40.  (Bins reach 2.7 M at the longest
    // clip; the product stays below 2^64 because k / n1 < n2 / 2 < 2^12.)
    unsigned long long magic;
    HPFW_DEVICE_MEMBER cf operator()(int k) const
    {
        if (n1 == 1) return base[k - q0];
        const int q2 = (int)(((unsigned long long)(unsigned)k * magic) >> 40);
        return base[(int64_t)(k - q2 * n1) * w + (q2 - q0)];
    }
};
// the slice of one band: element i is bin start + i
struct XsBand {
    XsView v;
    int start;
    HPFW_DEVICE_MEMBER cf operator()(int i) const { return v(start + i); }
    // every element of the slice times its window value, in natural order: f(i, x[i] g[i])
    // (kXsBatch elements per thread at a time, all their loads issued before the first product: one element per trip left
    // one memory round trip per element in a row -- tools/cq_stamps.py: a fifth to a third of a band's time)
    template <class F>
    HPFW_DEVICE_MEMBER void for_each(int tid, int nthreads, int lg, const cf *__restrict__ g, F f) const
    {
        for (int i0 = tid; i0 < lg; i0 += kXsBatch * nthreads) {
            cf xv[kXsBatch], gv[kXsBatch];
#pragma unroll
            for (int u = 0; u < kXsBatch; ++u) {
                const int i = i0 + u * nthreads;
                const int ic = i < lg ? i : lg - 1; // (a valid element again: loaded, not used)
                xv[u] = v(start + ic);
                gv[u] = g[ic];
            }
#pragma unroll
            for (int u = 0; u < kXsBatch; ++u) {
                const int i = i0 + u * nthreads;
                if (i < lg) f(i, c_mul(xv[u], gv[u]));
            }
        }
    }
};
// the same slice walked in the order the rows layout stores it (row q1 = k mod n1, then the q2 of the slice, which are
// consecutive in memory), with the window permuted likewise on the host (CqPlanDev::g2): lanes read runs of a row
// instead of 64 different rows.  t = q1 nq2 + tq is bin k = q1 + n1 (q2a + tq), element i = k - start (skipped outside
// [0, lg): there the permuted window holds zeros).
struct XsBandRows {
    const cf *base;  // clip's first element
    int n1, w, q0;   // as XsView
    int start, q2a, nq2;
    unsigned magic;  // ceil(2^32 / nq2) (nq2 >= 2): t / nq2 = umulhi(t, magic) for every t < 2^19
    template <class F>
    HPFW_DEVICE_MEMBER void for_each(int tid, int nthreads, int lg, const cf *__restrict__ g2, F f) const
    {
        // every t < total names an element of the clip's rows (inside or outside the band) and an entry of g2: the loads
        // are unconditional and issued kXsBatch at a time, only the use is guarded (written as `if (inside) f(.., load ..)`
        // every element cost a memory round trip of its own: tools/cq_stamps.py)
        const int total = n1 * nq2;
        for (int t0 = tid; t0 < total; t0 += kXsBatch * nthreads) {
            cf xv[kXsBatch], gv[kXsBatch];
            int ii[kXsBatch];
#pragma unroll
            for (int u = 0; u < kXsBatch; ++u) {
                const int t = t0 + u * nthreads;
                const int tc = t < total ? t : total - 1;
                const int q1 = nq2 == 1 ? tc : (int)(((unsigned long long)(unsigned)tc * magic) >> 32);
                const int tq = tc - q1 * nq2;
                const int i = q1 + n1 * (q2a + tq) - start;
                ii[u] = (t < total && i >= 0 && i < lg) ? i : -1;
                xv[u] = base[(int64_t)q1 * w + (q2a - q0 + tq)];
                gv[u] = g2[tc];
            }
#pragma unroll
            for (int u = 0; u < kXsBatch; ++u)
                if (ii[u] >= 0) f(ii[u], c_mul(xv[u], gv[u]));
        }
    }
};

// Forward transform of a clip length with a prime factor above 7 (k_bluestein.hip): a chirp-z
// convolution of length n1 * n2, n2 = 6300.  Tables are [n1][n2] complex.
struct BzArgs {
    int n1, n2, n2pad;  // n2pad: row stride (floats) of the planar buffers, a multiple of 32
    int kmin, kmax;     // forward bins consumed
    int a;              // n1 = 16 a: the first transform's column stage splits into length-a and length-16 transforms
    int n_tiles1;       // row tiles of 32 (16 outputs k_a each) of the length-a stage
    int k1lo, k1n;      // rows k1lo .. k1lo + k1n - 1 of the second transform hold the consumed bins
    int n_tiles2;       // row tiles of their coefficient image apack2 (a multiple of nt2)
    int nt2;            // row tiles per wave of that stage: what the consumed rows need, at most 3
    const float *wp;    // chirp w[j], planar [2][L] (Re plane, Im plane), 0 from sample N on
    const cf *tl;       // T_L[q1 k2] at [q1 n2 + k2]
    const cf *bhat;     // DFT_L(conj chirp)[q1 + n1 q2] at [q1 n2 + q2]
    const cf *wk;       // w[k] / L  [kmax - kmin]
    const float *apack1; // coefficient image of the length-a DFT          [a][n_tiles1][64]
    const float *apack3; // ... of the length-16 stage with its twiddles, per k_a  [a][16][64]
    const float *apack2; // ... of the rows k1lo .. k1lo + k1n - 1   [n1][n_tiles2][64]
};

// One Bluestein size class (all bands whose chirp-z length is p).
struct CqClassDev {
    int p;              // transform length (power of two)
    int n_bands;        // bands in this class
    RadixList radix;
    const cf *tw;       // T_p   [p]
    CqTwiddles gtw;     // per-butterfly twiddle tables of the fused groups
    const cf *vrev;     // DFT_p(chirp) at digit-reversed positions [p]
    const int *band;    // band index j                 [n_bands]
    int len0, outer;    // p > 16384: `outer` radix-4 passes through global memory around blocks of len0 (k_cq_big.hip)
};

struct CqPlanDev {
    int kmin, nk;       // first forward bin, number of bins per clip
    int xn1, xw, xq0;   // layout of the forward bins (XsView); set per call
    int64_t xclip;      // elements per clip
    unsigned long long xmagic;
    HPFW_DEVICE_MEMBER XsView view(const cf *x, int clip) const { return XsView{x + (int64_t)clip * xclip, xn1, xw, xq0, xmagic}; }
    int c;              // spectrogram columns
    const int *start;   // slice start (absolute bin)   [121]
    const int *lg;      // window length                [121]
    const int64_t *g_off; // offset of band j in g     [121]
    const cf *g;        // window * chirp / (M P)       [sum lg]
    // the same windows in the order of the rows layout (XsBandRows): band j at g2_off[j], n1 * nq2[j] entries
    const cf *g2;
    const int64_t *g2_off; // [121]
    const int *q2a, *nq2;  // [121]
    const unsigned *nq2_magic; // [121]
    int rows_min;          // bands whose slice holds fewer than this many bins per row are walked element by element
};

// per-band constants of the window table (S5; plan.h cq_window_scale / cq_hann_den), by value into cq_window_kernel
struct CqWindowBands {
    double scale[121];
    int hann_den[121];
};
// the window table g [sum lg] and its rows-layout twin g2 (7-smooth lengths) generated on the device; c.lg, c.g_off (and
// c.start, c.q2a, c.nq2, c.g2_off, c.g for the twin) must be in place on the stream
void launch_cq_windows(const CqPlanDev &c, const CqWindowBands &b, int64_t big_m, int lg_max, cf *d_g, hipStream_t s);
void launch_cq_windows_rows(const CqPlanDev &c, int n1, int max_entries, cf *d_g2, hipStream_t s);

// S6 column stage: pcm [n_clips][n1][n2] (clips `clip_samples` apart) -> z [n_clips][hq][Re row, Im row][n2]
void launch_fwd_cols_q(const ColsQArgs &a, const int16_t *d_pcm, int64_t clip_samples, int n_clips, float *d_z, hipStream_t s);
// S6 row stage: z -> x [n_clips][n1][q2w] (XsView layout)
size_t fwd_rows_lds_bytes(const RowsArgs &a);
void launch_fwd_rows2(const RowsArgs &a, const Rows2Out &o, const float *d_z, int n_clips, cf *d_x, hipStream_t s);
// the bins [kmin, kmax) in natural order out of either layout (stage entry point)
void launch_gather_bins(const CqPlanDev &cp, const cf *d_x, int n_clips, cf *d_out, hipStream_t s);
// chirp-z forward transform (k_bluestein.hip): pcm -> G' -> H' -> x; the planar buffers hold bz_plane_bytes(bz, n_clips) each
size_t bz_plane_bytes(const BzArgs &bz, int n_clips);
// coefficient images of the first transform's two column stages (apack1, apack3), from T_n1 on the device
void launch_bz_pack_stages(const BzArgs &bz, const cf *d_tw_n1, float *d_apack1, float *d_apack3, hipStream_t s);
// coefficient image [n1][n_tiles][64] of rows k1_first .. k1_first + k1_count - 1 of the length-n1 DFT, from T_n1 on the device
void launch_bz_pack_coefficients(int n1, int k1_first, int k1_count, const cf *d_tw_n1, int n_tiles, float *d_apack, hipStream_t s);
// the tables bz.wp, bz.tl, bz.wk, bz.bhat of a clip length, generated on the device (d_b: 2 L floats, d_y: one planar buffer)
void launch_bz_make_tables(const RowsArgs &rows, const BzArgs &bz, int64_t n, float *d_b, float *d_y, hipStream_t s);
void launch_bz_cols_first(const BzArgs &bz, const int16_t *d_pcm, int64_t n, int n_clips, float *d_out, hipStream_t s);
void launch_bz_rows_both(const RowsArgs &rows, const BzArgs &bz, const float *d_in, int n_clips, float *d_out, hipStream_t s);
void launch_bz_cols_last(const BzArgs &bz, const float *d_in, int n_clips, cf *d_x, hipStream_t s);
// band chirp-z transforms: x -> mag [n_clips][121][c]; also the maxima each wave saw,
// d_wavemax [n_clips][121][kCqMaxWaves] (slots of absent waves are written as 0)
constexpr int kCqMaxWaves = 16;
// db_mode: store the magnitude m, or t(m^2) = (float)(10 log10(max(m^2, 1e-10))) instead, by the specified sequence of
// DESIGN.md S8 alone or by db_term_fast (db_spec.h), which gives the same floats
enum DbMode { kDbNone = 0, kDbSpec = 1, kDbFast = 2 };
void launch_cq_class(const CqPlanDev &cp, const CqClassDev &cc, const cf *d_x, int n_clips,
                     float *d_mag, float *d_wavemax, int db_mode, hipStream_t s);
// the same for a class whose length exceeds the LDS (cc.outer > 0); d_work: cq_big_work_bytes(cc, n_clips)
size_t cq_big_work_bytes(const CqClassDev &cc, int n_clips);
void launch_cq_big_class(const CqPlanDev &cp, const CqClassDev &cc, const cf *d_x, int n_clips, cf *d_work, float *d_mag,
                         float *d_wavemax, int db_mode, hipStream_t s);
// d_clipmax [n_clips] = the largest of each clip's wave maxima
void launch_clipmax(const float *d_wavemax, float *d_clipmax, int n_clips, hipStream_t s);
// dB terms -> dB spectrogram in place: S = max(t - t_max, -80)
void launch_db_finish(float *d_t, const float *d_clipmax, int n_clips, int64_t per_clip, hipStream_t s);
// the same maxima when the chirp-z stage did not run (stage entry point)
void launch_magmax(const float *d_mag, int n_clips, int c, float *d_wavemax, hipStream_t s);
// amplitude_to_db: d_clipmax [n_clips] receives the per-clip maximum of d_wavemax first
void launch_db(const float *d_mag, const float *d_wavemax, float *d_clipmax, int n_clips, int64_t per_clip,
               float *d_db, bool fast, hipStream_t s);
// (tests) db_term_fast against db_term_spec on the bit patterns first .. first + count - 1: d_out[0] += those that differ,
// d_out[1] += those in 1e-10f <= p < inf that took the fallback, d_out[2] = min(d_out[2], first differing pattern)
void launch_db_term_sweep(uint32_t first, uint64_t count, unsigned long long *d_out, hipStream_t s);
// filters * frames on f32 MFMA: s_db [n_clips][121][c] -> proj [n_clips][64][c-19]
// d_fpack: filters repacked by pack_filters_for_mfma().  d_tmax != NULL: s_db holds dB terms and
// S = max(t - d_tmax[clip], -80) is applied while the slab is staged.
void launch_project(const float *d_fpack, const float *d_db, const float *d_tmax, int n_clips, int c,
                    float *d_proj, hipStream_t s);
// delta over 80 frames, sign, bit pack: proj [n_clips][64][nf] -> hp [n_clips][nf-80]
void launch_pack(const float *d_proj, int n_clips, int nf, uint64_t *d_hp, hipStream_t s);
// a4's reference level + a5..a8 in fixed point (k_project_q.hip): filter digits image; dB terms (d_tmax != NULL)
// or dB spectrograms -> hashprints in one kernel, the lag-80 difference taken on the quantised spectrogram (exact integers).
// d_images: the unshifted filter digit image (n_shifts = 0) or n_shifts shifted ones (project_q_image_bytes() each),
// hashprints [n_clips][max(n_shifts, 1)][c - 99], the slab of each (clip, tile) staged once for all images.  d_dbg: NULL,
// or (tests, unshifted) the integer sums D [n_clips][64][c - 99]
size_t project_q_image_bytes();
// The six-product split of the unshifted extraction (S9q): split != NULL, n_shifts = 0 and no d_dbg run the kernel that
// forms only the digit products of weight >= 2^16 and settles the values whose sign those leave open from its own slab,
// before it stores the hashprints.  d_thr: pack_filters_q's 64 thresholds; d_work: project_q_split_bytes(project_q_tiles(
// n_clips, c)) bytes, the tiles' counts
struct QSplit {
    const int32_t *d_thr;
    void *d_work;
};
size_t project_q_split_bytes(int64_t tiles);
int64_t project_q_tiles(int64_t n_clips, int64_t c);
void pack_filters_q(const float *f_colmajor, std::vector<int8_t> &image, std::vector<int32_t> *thr = nullptr);
void launch_hashprints_q(const void *d_images, int n_shifts, const float *d_db, const float *d_tmax, int n_clips, int c, uint64_t *d_hp,
                         long long *d_dbg, hipStream_t s, const QSplit *split = nullptr);
// transposed extraction: the digit images of the filters moved by each of shifts.s[0 .. n) bins
// (d_images: n * project_q_image_bytes()), for launch_hashprints_q
constexpr int kMaxShifts = 64;
struct ShiftList {
    int n;
    int s[kMaxShifts];
};
void launch_shift_filter_images(const void *d_fq_image, const ShiftList &shifts, void *d_images, hipStream_t s);
// queries at another tempo (k_tempo.hip): tempo rho moves along the source by step = rint(65536 / rho)
// sixteenths of a column per output column; a clip of c columns gives (c - 1) 65536 / step + 1 of them
constexpr int kMaxTempos = 64;
struct TempoList {
    int n;
    int32_t step[kMaxTempos];
};
inline int32_t tempo_step(float rho) { return (int32_t)std::rint(65536.0 / (double)rho); }
inline int64_t tempo_columns(int64_t c, int32_t step) { return (c - 1) * 65536 / step + 1; }
// db [n_clips][121][c] -> out [n_clips][tl.n][121][ct]: column k of tempo r interpolates source position k tl.step[r] / 65536
// (ct <= tempo_columns(c, every step))
void launch_tempo_scale(const float *d_db, int n_clips, int64_t c, const TempoList &tl, int64_t ct, float *d_out, hipStream_t s);

// ---- HashprintHandle with other template arguments (k_hashprint_cfg.hip) ----------------------------
struct CfgArgs {
    int rows, context, lag, filters; // spectrogram rows, FramesContext, T, 8 sizeof(N)
    const float *fpack;              // filters as the MFMA operand image (pack_cfg_filters)
};
size_t cfg_fpack_floats(int rows, int context, int filters);
void pack_cfg_filters(int rows, int context, int filters, const float *f_colmajor, float *fpack);
size_t project_cfg_lds_bytes(const CfgArgs &a);
// d_s [n_clips][rows][stride], d_cols [n_clips] valid columns (NULL: stride) -> d_proj [n_clips][filters][proj_stride]
void launch_project_cfg(const CfgArgs &a, const float *d_s, const int *d_cols, int n_clips, int64_t stride, float *d_proj,
                        int64_t proj_stride, hipStream_t s);
// -> d_hp [n_clips][hp_stride] of uint16 / uint32 / uint64 (by a.filters)
void launch_pack_cfg(const CfgArgs &a, const float *d_proj, const int *d_cols, int n_clips, int64_t stride, int64_t proj_stride,
                     void *d_hp, int64_t hp_stride, hipStream_t s);

// calc_cov + accumulate for such a configuration (k_cov_cfg.hip): accum [kt][kt], kt = rows * context, both triangles
bool cov_cfg_supported(const CfgArgs &a);
int cov_cfg_tile_count(int kt);
void cov_cfg_tile_list(int kt, int *xy /* 2 * cov_cfg_tile_count(kt) */);
size_t cov_cfg_workspace_bytes(const CfgArgs &a, int n_clips);
void launch_cov_cfg(const CfgArgs &a, const float *d_s, const int *d_cols, int n_clips, int64_t stride, const int *d_tiles,
                    float *d_ws, float *d_accum, hipStream_t s);

// ---- filter learning (index() only) -------------------------------------------------------
// accum [2420][2420] (tiles on or above the diagonal) += sum over clips of centred^T centred / (nf - 1),
// by lag correlations (k_cov.hip); d_ws: cov_workspace_bytes(n_clips, c) of scratch
int cov_tile_count();
void cov_tile_list(int *xy /* 2 * cov_tile_count() */);
size_t cov_workspace_bytes(int n_clips, int c);
void launch_cov(const float *d_db, int n_clips, int c, const int *d_tiles, float *d_ws, float *d_accum, hipStream_t s);
// host: unit eigenvectors of the m largest eigenvalues of a symmetric n x n matrix (eigen_host.cpp)
int top_eigenvectors(const float *cov, int n, int m, float *out, double *evals);

// host helper: [kp][lane][2] operand image of the filters for v_mfma_f32_32x32x2_f32
void pack_filters_for_mfma(const float *filters_colmajor, float *fpack /* 64*2420 */);

// ---- Mel front-end (f3, k_mel.hip) ----------------------------------------------------------
constexpr int kMelFrame = 4410, kMelHop = 441, kMelBins = 2206, kMelBands = 33;
int mel_frames(int64_t n_samples);
size_t mel_work_bytes(int64_t n_samples, int n_clips);
// d_out [n_clips][33][frames] (kept columns at the front of every row), d_count [n_clips] their number
void launch_mel(const RowsArgs &rows, const float *d_win, const float *d_cpack, const int16_t *d_pcm, int64_t n, int n_clips,
                int64_t *d_blk, int *d_pos, int *d_count, float *d_pmax, float *d_work, float *d_out, bool db_fast, hipStream_t s);
// the silence test alone: d_frames [n_clips][stride] = the frame of every kept column (-1 behind them), d_count their number;
// d_blk [n_clips][ceil(n / 441)], d_pos [n_clips][mel_frames(n)] scratch; stride >= mel_frames(n)
void launch_mel_kept_frames(const int16_t *d_pcm, int64_t n, int n_clips, int64_t *d_blk, int *d_pos, int *d_count,
                            int32_t *d_frames, int64_t stride, hipStream_t s);

// ---- exact cross-correlation of PCM16 (k_xcorr.hip) ---------------------------------------------
// (jobs and their parts: xcorr_plan.h) r of jobs [0, n_jobs) from the two item lists (either may be empty), then the
// peaks when d_peaks is not null
void launch_xcorr(const int16_t *d_pcm, const XcJob *d_jobs, int64_t n_jobs, const XcItem *d_mfma, int64_t n_mfma,
                  const XcItem *d_valu, int64_t n_valu, int64_t *d_r, hpfw_xcorr_peak *d_peaks, hipStream_t s);

// ---- search ------------------------------------------------------------------------------
struct SearchArgs {
    const uint64_t *db;      // concatenated hashprints
    const int64_t *db_off;   // [n_clips + 1] (device)
    int n_clips;
    const uint64_t *q;       // concatenated queries (device)
    const int64_t *q_off;    // [n_q + 1] (device)
    int n_q;
    int k_max;               // longest query
    uint64_t *best;          // [n_q][n_clips]: (dist << 32) | offset
    // search within a set: NULL, or [n_clips] slots of the index, strictly ascending: "clip" p of
    // the launch is slot set[p] of db_off, and column p of best.  The launches below pick the kernels' SET instantiation.
    const int32_t *set = nullptr;
};
// first hashprint and length n of position p of a launch's clips: slot p of the index, or slot set[p] (SET)
template <bool SET>
__device__ __forceinline__ int64_t clip_span(const int64_t *__restrict__ db_off, const int32_t *__restrict__ set, int p, int &n)
{
    const int slot = SET ? set[p] : p;
    const int64_t r0 = db_off[slot];
    n = (int)(db_off[slot + 1] - r0);
    return r0;
}
void launch_hamming_scan(const SearchArgs &a, hipStream_t s);
// the same scan on the matrix cores (k_search_mfma.hip): queries expanded to fp4 +-1 first
int hamming_mfma_kt_pad(int k_max);            // rows of the expanded-query image per group of 32
size_t hamming_mfma_lds_bytes(int k_max);      // dynamic LDS of the scan; > 160 KB: use launch_hamming_scan
void launch_expand_queries(const uint64_t *d_q, const int64_t *d_q_off, int n_q, int kt_pad, void *d_qa, hipStream_t s);
// one query against the whole index with the tile rows = 32 shifts of the query (few queries: no padded rows)
size_t hamming_shift_lds_bytes(int k);
size_t hamming_shift_image_bytes(int k);       // scratch for the query's expanded image (d_qexp)
void launch_hamming_shift(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int n_off_max, const uint64_t *d_q,
                          int k, void *d_qexp, uint64_t *d_best, hipStream_t s, const int32_t *d_set = nullptr);
// nearest windows (AnnStorage semantics with exact neighbours): rows = windows of `win` hashprints
void launch_expand_windows(const uint64_t *d_q, const int64_t *d_w_start, int n_win, int win, int kt_pad, void *d_qa,
                           hipStream_t s);
void launch_knn_windows(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int n_off_max, const void *d_qa,
                        int kt_pad, int n_win, int win, int nn, void *d_slots /* [n_win][8] u64, preset to ~0 */,
                        hipStream_t s);
// d_gk: per group of 32 queries {longest, shortest non-empty}; n_off_max: most offsets any (query, clip) has
void launch_hamming_mfma(const SearchArgs &a, const void *d_qa, int kt_pad, const int *d_gk, int n_off_max, hipStream_t s);
// d_set (here and in the launches below): NULL, or what SearchArgs::set is -- column c of the table is slot d_set[c]
void launch_topk(const uint64_t *d_best, int n_q, int n_clips, int k, uint32_t clip_base, void *d_out,
                 hipStream_t s, const int32_t *d_set = nullptr);
// the same result in two steps (64 slices of the clips per query, then a merge): large indexes, few queries
size_t topk_scratch_bytes(int n_q, int k);
void launch_topk_two_step(const uint64_t *d_best, int n_q, int n_clips, int k, uint32_t clip_base, void *d_scratch,
                          void *d_out, hipStream_t s, const int32_t *d_set = nullptr);
// overlap search (k_search_overlap.hip): lags min_overlap - k .. n - min_overlap of every (query, clip),
// rated by dist / overlap.  d_tab [n_q][n_clips][splits] of 16-byte entries {dist, overlap, lag, 0}, every byte preset to
// 0xff; a clip's chunks of kOverlapChunk lags are dealt round robin to its `splits` workgroups.
constexpr int kOverlapChunk = 1024;
// the rule on the device (overlap_rule.h: overlap of at most LMAX, "none" at dist NODIST, 24-bit products or full ones)
template <unsigned LMAX, unsigned NODIST, bool MUL24>
struct OverlapRule;
using OverlapSearchRule = OverlapRule<16383, 1u << 21, true>; // L <= 16000 < 2^14, dist <= 64 * 16000 < 2^20
// the matrix-core scan: d_qa the image of launch_expand_queries, d_gk [group] the longest query of each group of 32,
// k_max the longest query of the call (hamming_mfma_lds_bytes(k_max) <= 160 KB)
void launch_overlap_mfma(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const int64_t *d_q_off, int n_q, const void *d_qa,
                         int kt_pad, const int *d_gk, int k_max, int min_overlap, int splits, void *d_tab, hipStream_t s);
// the same entries by xor/popcount, one workgroup per (query, clip, split)
void launch_overlap_popc(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const uint64_t *d_q, const int64_t *d_q_off, int n_q,
                         int min_overlap, int splits, void *d_tab, hipStream_t s);
// folds the splits (in d_tab) and writes the k best clips of each query to d_out [n_q][k] (hpfw_overlap_hit);
// d_exclude: NULL or [n_q] clips to skip (-1: none); n_clips == 0: padding records
void launch_overlap_select(void *d_tab, int n_q, int n_clips, int splits, const int32_t *d_exclude, int k, uint32_t clip_base, void *d_out,
                           hipStream_t s);
// local search (k_search_local.hip): per (query, clip) the best-scoring run of consecutive query positions
// on any diagonal, score = sum of max_rate - popcount over the run.  d_best [n_q][n_clips], every byte preset to 0xff, takes
// (kLocalScoreBias - score) << 32 | (lag + kLocalLagBias) of every pair with a positive run: smaller is better, so launch_topk
// picks a query's clips (its hit's dist = kLocalScoreBias - score, its offset = lag + kLocalLagBias).  A clip's lags
// 1 - k .. n - 1 are cut into `chunks` workgroups of kLocalChunk.
constexpr int kLocalChunk = 1024;
constexpr int kLocalScoreBias = 1 << 20; // above every score: 31 * 16000
constexpr int kLocalLagBias = 1 << 14;   // above every query's length: lag + bias >= 0
// the matrix-core scan: d_qa, d_gk [group], k_max as launch_overlap_mfma's
void launch_local_mfma(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const int64_t *d_q_off, int n_q, const void *d_qa,
                       int kt_pad, const int *d_gk, int k_max, int max_rate, int chunks, uint64_t *d_best, hipStream_t s);
// the same keys by xor/popcount, one workgroup per (query, clip, chunk)
void launch_local_popc(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const uint64_t *d_q, const int64_t *d_q_off, int n_q,
                       int max_rate, int chunks, uint64_t *d_best, hipStream_t s);
// d_top [n_q][k]: launch_topk's hits of d_best (NULL: padding everywhere) -> d_out [n_q][k] (hpfw_local_hit): the winning
// diagonals walked once; *d_disagree += the winners whose walk does not give the scan's score
void launch_local_ends(const void *d_top, const uint64_t *d_db, const int64_t *d_db_off, const uint64_t *d_q, const int64_t *d_q_off,
                       int64_t n_q, int k, int max_rate, uint32_t clip_base, void *d_out, unsigned *d_disagree, hipStream_t s);
// scored overlap search (k_stats.hip), after launch_overlap_select on the same d_tab: d_stats [n_q]
// (hpfw_dist_stats, zeroed by the caller) += per query row the moments of floor(dist 2^kOverlapRateBits / overlap) over the
// clips with a candidate but d_exclude's.  A row is cut into overlap_stats_slices(n_clips) workgroups.
constexpr int kOverlapRateBits = HPFW_OVERLAP_RATE_BITS;
inline int overlap_stats_slices(int n_clips) { return std::max(1, std::min(64, n_clips / 4096)); } // as launch_dist_stats cuts a row
void launch_overlap_stats(const void *d_tab, int n_q, int n_clips, int splits, const int32_t *d_exclude, void *d_stats, hipStream_t s);
// the index joined with itself (k_selfjoin.hip): for clips a < b the best lag of a against b by the
// overlap rule.  The rows a of a pass are row groups g0 .. g0 + n_groups - 1 (32 rows each); the pairs (group, b) with b above
// the group's first row are numbered by d_pair_first [n_groups + 1], n_pairs of them in all (> 0); each has `splits`
// workgroups.  d_tab [32 n_groups][n_clips][splits] of 16-byte entries {dist, overlap, lag, 0}, every byte preset to 0xff.
// A row is walked in slices of kSelfjoinSlice positions, a pair's lags in chunks of kSelfjoinChunk.  The scan's geometry, a
// workgroup's pair, the walk of a chunk and the selection kernels are in join_scan.h, shared by the three joins; the plan
// of the passes is join_plan.h's.
constexpr int kSelfjoinChunk = 1024;
constexpr int kSelfjoinSlice = 32;
constexpr int kSelfjoinMaxLen = (1 << 18) - 1; // hashprints of a recording: 64 L < 2^24 keeps the fp32 accumulators exact
using JoinRule = OverlapRule<(unsigned)kSelfjoinMaxLen, 1u << 25, false>; // dist <= 64 L < 2^24: products below 2^42
void launch_selfjoin_scan(bool popc, const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int g0, int n_groups,
                          const uint32_t *d_pair_first, uint32_t n_pairs, int min_overlap, int splits, void *d_tab, hipStream_t s);
// folds the splits (in d_tab), counts the pairs of rows row0 .. row0 + n_rows - 1 with dist rate_den <= rate_num overlap into
// d_row_count, their positions from *d_count on into d_row_first, writes those below cap to d_out (hpfw_dup_pair, rising
// (a, b)) and adds the pass's pairs to *d_count
// (column c of d_tab [n_rows][n_cols][splits] is clip col0 + c: the self-join's col0 is 0 and its n_cols the index's clips)
void launch_selfjoin_select(void *d_tab, int n_cols, int col0, int splits, int row0, int n_rows, uint32_t rate_num, uint32_t rate_den,
                            int *d_row_count, int64_t *d_row_first, uint32_t clip_base, void *d_out, int64_t cap, int64_t *d_count, hipStream_t s);
// the index joined with n_x recordings that are not in it: launch_selfjoin_scan over the list "the
// n_index slots of the index, then the externals d_x / d_x_off [n_x + 1]" with b an external only.  The pairs (group, b) of a
// pass are numbered by d_pair_first as join_group_pairs (join_plan.h) counts them: pair i of group g is
// b = max(n_index, 32 g + 1) + i.  Rows at or above n_index are masked unless among_new.  d_tab [32 n_groups][n_x][splits]:
// the columns are the externals (launch_selfjoin_select with col0 = n_index).
void launch_join_scan(bool popc, const uint64_t *d_db, const int64_t *d_db_off, int n_index, const uint64_t *d_x, const int64_t *d_x_off, int n_x,
                      int among_new, int g0, int n_groups, const uint32_t *d_pair_first, uint32_t n_pairs, int min_overlap, int splits,
                      void *d_tab, hipStream_t s);
// the local self-join (k_localjoin.hip): for clips a < b the best-scoring run of consecutive hashprints
// of a on any diagonal of b, score = sum of max_rate - popcount over the run.  Passes, row groups, d_pair_first, n_pairs,
// splits, slices and chunks are launch_selfjoin_scan's -- the same code, join_scan.h; min_len = ceil(min_score / max_rate)
// takes min_overlap's part.  The step's pieces and the walk of a diagonal are the local search's (local_rule.h).
// d_tab [32 n_groups][n_clips][splits] of 8-byte keys (kLocaljoinScoreBias - score) << 32 | (lag + kLocaljoinLagBias), every
// byte preset to 0xff: smaller is better, and the fold of a pair's splits is their minimum.
constexpr int kLocaljoinScoreBias = 1 << 24; // above every score: 31 * kSelfjoinMaxLen < 2^23
constexpr int kLocaljoinLagBias = 1 << 19;   // above every recording's length: lag + bias >= 0
// the accumulators hold twice the running score, and one product on top of it, before the step's constant is taken off
static_assert(2 * 31 * (int64_t)kSelfjoinMaxLen + 64 < (1 << 24), "the doubled running score is exact in f32 below 2^24");
void launch_localjoin_scan(bool popc, const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int g0, int n_groups,
                           const uint32_t *d_pair_first, uint32_t n_pairs, int min_len, int max_rate, int splits, void *d_tab, hipStream_t s);
// folds the splits (in d_tab), counts the pairs of rows row0 .. row0 + n_rows - 1 with score >= min_score into d_row_count,
// their positions from *d_count on into d_row_first, writes those below cap to d_out (hpfw_passage_pair, rising (a, b), the
// run's ends still 0) and adds the pass's pairs to *d_count
void launch_localjoin_select(void *d_tab, int n_clips, int splits, int row0, int n_rows, int min_score, int *d_row_count, int64_t *d_row_first,
                             uint32_t clip_base, void *d_out, int64_t cap, int64_t *d_count, hipStream_t s);
// after the last pass: the diagonals of the min(*d_count, cap) pairs in d_out walked once -- a_start, length, dist and the
// score again; *d_disagree += the pairs whose walk does not give the scan's score
void launch_localjoin_ends(const uint64_t *d_db, const int64_t *d_db_off, int max_rate, uint32_t clip_base, void *d_out, int64_t cap,
                           const int64_t *d_count, unsigned *d_disagree, hipStream_t s);
// per-shift top-k lists in [n_q][n_shifts][k] (hpfw_hit) -> out [n_q][k] (hpfw_shift_hit): per clip its smallest
// (dist, shift index), then the k best by (dist, clip)
void launch_topk_merge_shifts(const void *d_in, int n_q, int n_shifts, int k, void *d_out, hipStream_t s);
// scored search (k_stats.hip): d_stats [n_q] (hpfw_dist_stats, zeroed by the caller) += per query row the
// moments n, sum d, sum d^2 of d = best >> 32 over the clips with db_off[c + 1] - db_off[c] >= q_off[q + 1] - q_off[q] >= 1
void launch_dist_stats(const uint64_t *d_best, const int64_t *d_db_off, const int64_t *d_q_off, int n_q, int n_clips, void *d_stats,
                       hipStream_t s, const int32_t *d_set = nullptr);
// search within sets (k_within.hip): the queries regrouped by set and the results put back.
// d_dst[dst_off[i] ..) = d_src[src_off[i] .. src_off[i] + dst_off[i + 1] - dst_off[i]) for i < n (offsets on the device)
void launch_within_gather(const uint64_t *d_src, const int64_t *d_src_off, const int64_t *d_dst_off, int64_t n, uint64_t *d_dst, hipStream_t s);
// rows of `words` 8-byte words: d_out[perm[r]] = d_in[r], r < n (perm on the device, a permutation of 0 .. n - 1)
void launch_within_scatter(const uint64_t *d_in, const int64_t *d_perm, int64_t n, int words, uint64_t *d_out, hipStream_t s);
// a sharded search's gathered results (k_merge.hip): per-shard top-k lists in [n_shards][n_q][k] of 16-byte
// records keyed (dist, clip) (hpfw_hit or hpfw_shift_hit) -> out [n_q][k], as hpfw_gpu_merge_topk orders them; n_shards k <= 4096
void launch_topk_merge_shards(const void *d_in, int n_shards, int64_t n_q, int k, void *d_out, hipStream_t s);
// d_out[r] = sum over the shards of d_in[shard][r] (hpfw_dist_stats), r < rows
void launch_sum_stats(const void *d_in, int n_shards, int64_t rows, void *d_out, hipStream_t s);
// the same for the neighbour lists of the voting search: d_in [n_shards][n_win][5] keys (dist << 40 | position in the shard,
// ascending, ~0 behind them), pos_base[shard] added to the position of every real key -> d_out [n_win][5], the 5 smallest
// ascending; n_shards <= 64
void launch_knn_merge_shards(const uint64_t *d_in, const int64_t *pos_base, int n_shards, int64_t n_win, uint64_t *d_out, hipStream_t s);
// ---- warped search (k_dtw.hip): subsequence DTW of a query over a clip, one wave per pair ----
constexpr int kDtwStrip = 8;               // columns a lane holds in registers
constexpr int kDtwBlock = 64 * kDtwStrip;  // columns of one pass of the wave; a wider clip runs in blocks from left to right
constexpr int64_t kDtwPathCells = (int64_t)1 << 31; // the path call records 2 bits per cell: 512 MiB at this many
struct DtwArgs {
    const uint64_t *db;      // the index
    const int64_t *db_off;   // [n_clips + 1] (device)
    const uint64_t *q;       // concatenated queries (device)
    const int64_t *q_off;    // [n_q + 1] (device)
    int64_t q_first;         // added to a pair's query where the pairs are not the caller's list
    // pair p is (pairs[2 p], pairs[2 p + 1]); else (p / per_q, clip of the hpfw_hit cand[p] less clip_base, or none for a
    // padding record); else (p / per_q, p % per_q)
    const int32_t *pairs;
    const void *cand;
    int64_t per_q;
    uint32_t clip_base;
    int64_t n_pairs;
    int k_max;               // the longest query: rows of a workgroup's part of bnd
    uint4 *bnd;              // [workgroups][k_max]: the last two columns of the block before, for every row
    uint16_t *choices;       // path form (one pair): [k][blocks][64] the choices of a lane's strip, 2 bits per cell
    void *out;               // hpfw_dtw_hit [n_pairs], clip as the pair names it; a pair without a candidate: padding
    uint64_t *table;         // NULL, or [n_pairs]: dist << 32 | start for launch_topk, ~0 without a candidate
};
// `slots` workgroups of one wave take the pairs in turn
void launch_dtw_pairs(const DtwArgs &a, int slots, bool path, hipStream_t s);
// the path [k_q] of the pair whose hit and choices the path form left (no candidate: -1 everywhere)
void launch_dtw_backtrack(const uint16_t *d_choices, int k_q, int n_blocks, const void *d_hit, int32_t *d_path, hipStream_t s);
// d_top [n_q][k]: launch_topk's hits of the table of per_q pairs per query -> d_out [n_q][k] (hpfw_dtw_hit)
void launch_dtw_finish(const void *d_top, const void *d_pairs, int64_t n_q, int k, int64_t per_q, uint32_t clip_base, void *d_out, hipStream_t s);
// the k best by (dist, clip) of each query's per_q <= 64 pairs -> d_out [n_q][k], clip_base added
void launch_dtw_rank(const void *d_pairs, int64_t n_q, int per_q, int k, uint32_t clip_base, void *d_out, hipStream_t s);
// ---- removal from the index in place (k_index.hip; kIndexTile and the plan: index_plan.h) ----
// d_out[e - out_shift] = d_in[src + (e - dst)] of the piece that holds e, for e in [lo, hi): the n_moves pieces cover [lo, hi)
// without a gap, ascending; out_shift even, d_out and d_in 16-byte aligned
void launch_index_gather(uint64_t *d_out, int64_t out_shift, const uint64_t *d_in, const hpfw_index_move *d_moves, int64_t n_moves, int64_t lo,
                         int64_t hi, hipStream_t s);
// d_out[e] = d_in[e - in_shift] for e in [lo, hi); in_shift even
void launch_index_copy(uint64_t *d_out, const uint64_t *d_in, int64_t in_shift, int64_t lo, int64_t hi, hipStream_t s);
// ---- the tally of the voting search (k_votes.hip) ----
// d_w_start[w] = where window w_base + w begins in the query array: d_q_off[q] + (w_base + w - d_w_first[q]) for the query q
// that holds it (d_w_first, d_q_off [n_q + 1], the first window of each query and its first hashprint)
void launch_window_starts(const int64_t *d_w_first, const int64_t *d_q_off, int n_q, int64_t w_base, int64_t n_win, int64_t *d_w_start,
                          hipStream_t s);
// the slots [n_win][8] of launch_knn_windows -> d_keys [n_win][5] ascending
void launch_sort_knn_slots(const void *d_slots, int64_t n_win, uint64_t *d_keys, hipStream_t s);
// a group of n_q whole queries whose n_win windows begin at window w_base of the call
struct VoteTallyArgs {
    const uint64_t *keys;    // [n_win][5], the group's
    const int64_t *w_first;  // [n_q + 1], the group's first entry first; window numbers of the call
    int64_t w_base, n_win;
    int n_q;
    const int64_t *db_off;   // [n_clips + 1] (device)
    int64_t n_clips;
    uint32_t clip_base;
    int64_t stride;          // the most windows any query of the call has (at least 1): more than every window index i
    int ubits, qbits;        // a bucket's number stays below 2^ubits - 1, a query's below 2^qbits; ubits + qbits <= 64
    uint64_t *sort_keys, *sorted_keys; // [n_win * 5] each
    uint32_t *sort_vals, *sorted_vals;
    float *post;             // [n_win * 5]: every event's bucket value after it
    hpfw_vote *out;          // [n_q], the group's
};
size_t vote_sort_temp_bytes(int64_t n_ev, int bits); // of the sort of n_ev events by `bits` bits (0: the query failed)
hipError_t launch_vote_tally(const VoteTallyArgs &a, void *d_temp, size_t temp_bytes, hipStream_t s);
// windows of one recording (k_windows.hip): window i of d_src is samples [i hop, i hop + win) -> d_dst [n_w][win]
void launch_gather_windows(const int16_t *d_src, int64_t hop, int64_t win, int64_t n_w, int16_t *d_dst, hipStream_t s);
// live feeds (k_streams.hip): rings of `capacity` samples in one slab [n_streams][capacity]
// (RingRun, RingWindow, RingRsRun and the planning of a push: streams_plan.h)
// every run of one push in one launch; max_count: the longest run
void launch_ring_append(const RingRun *d_runs, int n_runs, int64_t max_count, const int16_t *d_src, int16_t *d_slab, hipStream_t s);
// window i of the pass: win samples from d_tab[i] on, modulo capacity -> d_dst [n_w][win]
void launch_ring_gather_windows(const int16_t *d_slab, const RingWindow *d_tab, int64_t capacity, int64_t win, int64_t n_w, int16_t *d_dst,
                                hipStream_t s);
// the feeds of one push at one other rate (k_streams_resample.hip): runs [n_runs], most: the most outputs of one run; d_hist: the
// set's history slab; (L, M, T) and d_taps as launch_resample takes them.  false when the launch configuration is impossible
bool launch_ring_resample_append(const RingRsRun *d_runs, int n_runs, int64_t most, const int16_t *d_src, int16_t *d_slab, int16_t *d_hist,
                                 int32_t L, int32_t M, int32_t T, const int32_t *d_taps, hipStream_t s);

// sample-rate conversion to 44.1 kHz (k_resample.hip)
constexpr int kRsRateOut = 44100, kRsRateMin = 8000, kRsRateMax = 192000;
constexpr int kRsShift = 14; // taps in fixed point: every phase sums to 2^14
// (L, M) = (44100, rate) / gcd and H (taps per phase T = 2 H); false outside [kRsRateMin, kRsRateMax]
bool resample_ratio(int rate, int32_t *L, int32_t *M, int32_t *H);
int64_t resample_out_length(int64_t n_in, int32_t L, int32_t M); // ceil(n_in L / M)
// the [L][T] int16 table (host, float64); false for a rate outside the range
bool resample_design(int rate, std::vector<int16_t> &taps, int32_t *L, int32_t *M, int32_t *T);
int resample_row_words(int T);
std::vector<int32_t> resample_device_table(const std::vector<int16_t> &taps, int32_t L, int32_t T);
bool launch_resample(const int16_t *d_in, int64_t n_in, int64_t n_clips, int32_t L, int32_t M, int32_t T, const int32_t *d_taps,
                     int16_t *d_out, hipStream_t s);

// time warp and mix of PCM16 (k_warp.hip; the constants and the host side: drift_plan.h)
// a track as the kernels take it: hpfw_warp_track and the outputs [m_lo, m_hi] whose taps reach its source (warp_reach)
struct WarpTrack {
    int64_t src_off, src_len, i0, f0, d;
    int32_t gain, pad;
    int64_t m_lo, m_hi;
};
// the [4096][32] int16 table (host, float64): row p the fractional delay p / 4096, row 0 the unit impulse
bool warp_design(std::vector<int16_t> &taps);
// d_tab: resample_device_table's image of that table.  mix: d_out [n_out], the fused mix; else [n_tracks][n_out]
void launch_warp(const int16_t *d_pcm, const WarpTrack *d_tracks, int64_t n_tracks, const int32_t *d_tab, int64_t m0, int64_t n_out, bool mix,
                 int16_t *d_out, hipStream_t s);

// fail-loud launch check
const char *last_launch_error();

} // namespace hpfw
