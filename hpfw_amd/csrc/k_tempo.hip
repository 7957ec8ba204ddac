// k_tempo.hip -- dB spectrograms rescaled in time, for queries played at another tempo (tests/tempo_ref.py
// restates it in numpy).
//
// Tempo factor rho (query tempo / indexed tempo), step = rint(65536 / rho): column k of the scaled spectrogram shows source
// position p = k step / 65536, i = p >> 16, w = p & 0xFFFF, and holds
//   S_rho[b][k] = (float)(((double)S[b][i] (65536 - w) + (double)S[b][min(i + 1, C - 1)] w) / 65536)
// Both products are exact in double (24 + 17 bits), the sum is rounded once, the division is exact, the cast rounds once.
//
//   tempo_scale_kernel   one workgroup = one (clip, bin row, tile of kTsTile source columns): the tile and the column after
//                        it are staged once in LDS by coalesced loads; then, tempo by tempo, the workgroup writes every
//                        output column whose left source column i lies in the tile,
//                          k in [ceil(i0 65536 / step), ceil((i0 + kTsTile) 65536 / step)) and k < ct,
//                        consecutive lanes on consecutive k.  S is read from device memory once and every output element is
//                        written once, in contiguous runs.
#include <algorithm>

#include "kernels.h"

namespace hpfw {

namespace {

constexpr int kTsThreads = 256;
constexpr int kTsTile = 512; // source columns per workgroup (+ 1 staged after them)

// db [n_clips][121][c] -> out [n_clips][tl.n][121][ct]; blockIdx.x = clip * n_tiles + tile, blockIdx.y = bin row
__global__ __launch_bounds__(kTsThreads) void tempo_scale_kernel(const float *__restrict__ db, int64_t c, int64_t ct, int n_tiles,
                                                                 TempoList tl, float *__restrict__ out)
{
    __shared__ float src[kTsTile + 1];
    __shared__ int64_t kbeg[kMaxTempos], kend[kMaxTempos];
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / n_tiles, tile = blockIdx.x - clip * n_tiles, row = blockIdx.y;
    const int64_t i0 = (int64_t)tile * kTsTile;
    const float *s = db + ((int64_t)clip * kBins + row) * c;
    // slot j holds S[min(i0 + j, c - 1)]: the clamp of the right neighbour at the last column comes with the staging
    float v[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int64_t j = tid + u * kTsThreads;
        v[u] = j <= kTsTile ? s[std::min<int64_t>(i0 + j, c - 1)] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (tid + u * kTsThreads <= kTsTile) src[tid + u * kTsThreads] = v[u];
    for (int r = tid; r < tl.n; r += kTsThreads) {
        const int64_t st = tl.step[r];
        kbeg[r] = std::min((i0 * 65536 + st - 1) / st, ct);
        kend[r] = std::min(((i0 + kTsTile) * 65536 + st - 1) / st, ct);
    }
    __syncthreads();
    for (int r = 0; r < tl.n; ++r) {
        const int64_t st = tl.step[r];
        float *o = out + (((int64_t)clip * tl.n + r) * kBins + row) * ct;
        for (int64_t k = kbeg[r] + tid; k < kend[r]; k += kTsThreads) {
            const int64_t p = k * st;
            const int i = (int)((p >> 16) - i0); // in [0, kTsTile): k is in this tile's range
            const int w = (int)(p & 0xFFFF);
            o[k] = (float)(((double)src[i] * (double)(65536 - w) + (double)src[i + 1] * (double)w) / 65536.0);
        }
    }
}

} // namespace

void launch_tempo_scale(const float *d_db, int n_clips, int64_t c, const TempoList &tl, int64_t ct, float *d_out, hipStream_t s)
{
    if (n_clips <= 0 || c <= 0 || ct <= 0 || tl.n <= 0) return;
    const int n_tiles = (int)((c + kTsTile - 1) / kTsTile);
    hipLaunchKernelGGL(tempo_scale_kernel, dim3((unsigned)n_tiles * (unsigned)n_clips, kBins), dim3(kTsThreads), 0, s, d_db, c, ct,
                       n_tiles, tl, d_out);
}

} // namespace hpfw
