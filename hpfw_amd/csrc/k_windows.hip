// k_windows.hip -- windows of one long recording, gathered into clips back to back.
//
// Window w of a recording is samples [w hop, w hop + win).  The extraction kernels take clips of equal length back to
// back and none of them knows a clip stride (DESIGN.md section 11 records what an extra argument did to their register
// allocation), so the windows of one pass are copied out first: dst [n_w][win] int16, window w0 + i from src + (w0 + i) hop.
// One extra read and write of 2 bytes per sample against the ~21 MB the extraction moves per 30 s clip.
//
// dst is taken as one flat array of n_w * win samples cut into chunks of 8 (16 bytes, aligned: the workspace comes from
// hipMalloc); a lane writes one chunk with one 16-byte store.  Window starts are only 2-byte aligned in the source (any hop)
// and in the destination (an odd win), so the 8 source samples are read through a 2-byte-aligned copy, which the compiler
// turns into what unaligned global loads the target allows; a chunk that straddles two windows, and the ragged last chunk,
// go sample by sample.
#include "kernels.h"

namespace hpfw {

struct alignas(16) Pcm8 {
    int16_t v[8];
};

__global__ __launch_bounds__(256) void gather_windows_kernel(const int16_t *__restrict__ src, int64_t hop, int64_t win, int64_t total,
                                                             int16_t *__restrict__ dst)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; // first flat destination sample of the chunk
    if (i0 >= total) return;
    const int64_t w = i0 / win, j = i0 - w * win;
    if (j + 8 <= win && i0 + 8 <= total) { // (the chunk lies in window w: source samples w hop + j .. + 7)
        Pcm8 p;
        __builtin_memcpy(p.v, src + w * hop + j, 16);
        *reinterpret_cast<Pcm8 *>(dst + i0) = p;
        return;
    }
    for (int64_t i = i0; i < i0 + 8 && i < total; ++i) {
        const int64_t wi = i / win;
        dst[i] = src[wi * hop + (i - wi * win)];
    }
}

// src: the recording from the first window of the pass on; windows [0, n_w) of it -> d_dst [n_w][win]
void launch_gather_windows(const int16_t *d_src, int64_t hop, int64_t win, int64_t n_w, int16_t *d_dst, hipStream_t s)
{
    const int64_t total = n_w * win, chunks = (total + 7) / 8;
    if (chunks == 0) return;
    hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, d_src, hop, win, total, d_dst);
}

} // namespace hpfw
