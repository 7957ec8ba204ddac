// k_streams.hip -- live feeds: one ring of int16 per feed in one slab [n_streams][capacity]; sample t of
// feed i lives at slab[i capacity + t mod capacity].  Two copies carry every sample of a feed: the chunks of one push go from
// the staging buffer into their rings (ring_append_kernel), and the windows that have become complete go from the rings into
// clips back to back (ring_gather_windows_kernel), exactly what gather_windows_kernel gives for a linear recording, so that the
// extraction of clips runs unchanged behind it.  (The chunks of a feed at another rate than 44.1 kHz take another way into their
// ring: k_streams_resample.hip.)
//
// Both follow k_windows.hip: the destination is cut into chunks of 8 samples (16 bytes, aligned: slab and workspace come from
// hipMalloc), a lane writes one chunk with one 16-byte store, and the 8 source samples are read through a 2-byte-aligned copy
// (ring positions, an odd capacity, an odd win or hop make every alignment occur).  A chunk goes sample by sample when it is
// not whole: at the ends of an appended run, across two windows, across the ring's end, at the ragged tail.
#include "kernels.h"

namespace hpfw {

namespace {
struct alignas(16) RingPcm8 {
    int16_t v[8];
};
} // namespace

// One launch per push.  A feed's chunk is one run of the slab, or two when it passes the ring's end; blockIdx.y is the run,
// blockIdx.x * 256 + threadIdx.x the aligned chunk of the slab counted from the one that holds the run's first sample.  Runs
// of different feeds may share an aligned chunk (a capacity that is no multiple of 8): such a chunk is not whole for either,
// and each writes its own samples only.
__global__ __launch_bounds__(256) void ring_append_kernel(const RingRun *__restrict__ runs, const int16_t *__restrict__ src,
                                                          int16_t *__restrict__ slab)
{
    const RingRun r = runs[blockIdx.y];
    const int64_t c0 = (r.dst & ~(int64_t)7) + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; // first slab sample of the chunk
    const int64_t end = r.dst + r.count;
    if (c0 >= end) return;
    if (c0 >= r.dst && c0 + 8 <= end) {
        RingPcm8 p;
        __builtin_memcpy(p.v, src + r.src + (c0 - r.dst), 16);
        *reinterpret_cast<RingPcm8 *>(slab + c0) = p;
        return;
    }
    for (int64_t i = c0 < r.dst ? r.dst : c0; i < c0 + 8 && i < end; ++i) slab[i] = src[r.src + (i - r.dst)];
}

// One launch per pass.  dst [n_w][win] flat, total = n_w win; window i of the pass is ring samples start .. start + win - 1
// (modulo capacity) of the ring at slab + base, (base, start) = win_tab[i], 0 <= start < capacity.
__global__ __launch_bounds__(256) void ring_gather_windows_kernel(const int16_t *__restrict__ slab, const RingWindow *__restrict__ win_tab,
                                                                  int64_t capacity, int64_t win, int64_t total, int16_t *__restrict__ dst)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; // first flat destination sample of the chunk
    if (i0 >= total) return;
    const int64_t w = i0 / win, j = i0 - w * win;
    if (j + 8 <= win && i0 + 8 <= total) { // (the chunk lies in window w)
        const RingWindow t = win_tab[w];
        int64_t pos = t.start + j; // < 2 capacity: start < capacity, j < win <= capacity
        if (pos >= capacity) pos -= capacity;
        if (pos + 8 <= capacity) { // (and does not pass the ring's end)
            RingPcm8 p;
            __builtin_memcpy(p.v, slab + t.base + pos, 16);
            *reinterpret_cast<RingPcm8 *>(dst + i0) = p;
            return;
        }
    }
    for (int64_t i = i0; i < i0 + 8 && i < total; ++i) {
        const int64_t wi = i / win;
        const RingWindow t = win_tab[wi];
        int64_t pos = t.start + (i - wi * win);
        if (pos >= capacity) pos -= capacity;
        dst[i] = slab[t.base + pos];
    }
}

// runs [n_runs] (device), max_count: the longest run; d_src: the staged chunks the runs' src offsets count from
void launch_ring_append(const RingRun *d_runs, int n_runs, int64_t max_count, const int16_t *d_src, int16_t *d_slab, hipStream_t s)
{
    if (n_runs == 0 || max_count == 0) return;
    const int64_t chunks = (max_count + 7) / 8 + 1; // (a run that starts inside a chunk touches one more)
    hipLaunchKernelGGL(ring_append_kernel, dim3((unsigned)((chunks + 255) / 256), (unsigned)n_runs), dim3(256), 0, s, d_runs, d_src, d_slab);
}

void launch_ring_gather_windows(const int16_t *d_slab, const RingWindow *d_tab, int64_t capacity, int64_t win, int64_t n_w, int16_t *d_dst,
                                hipStream_t s)
{
    const int64_t total = n_w * win, chunks = (total + 7) / 8;
    if (chunks == 0) return;
    hipLaunchKernelGGL(ring_gather_windows_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, d_slab, d_tab, capacity, win, total,
                       d_dst);
}

} // namespace hpfw
