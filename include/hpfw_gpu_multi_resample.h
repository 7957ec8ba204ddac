/*
 * hpfw_gpu_multi_resample.h -- the sample-rate switch of the multi-GPU collector (libhpfw_gpu_multi.so).
 *
 * Kept beside include/hpfw_gpu_multi.h rather than in it: that header's symbol set is fixed (tests/test_library.py
 * checks it against hpfw_amd.multi.EXPORTS), and this is an addition to it.
 */
#ifndef HPFW_GPU_MULTI_RESAMPLE_H
#define HPFW_GPU_MULTI_RESAMPLE_H

#include "hpfw_gpu_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hpfw_gpu_collector_set_resample (include/hpfw_gpu.h) for the collector of every shard, including the collectors the
 * group makes later (off by default).  With it on, hpfw_gpu_group_prepare and hpfw_gpu_group_calc_hashprint accept WAV
 * files at any rate in [8 000, 192 000] Hz and convert them to 44.1 kHz on the GPU. */
int hpfw_gpu_group_set_resample(hpfw_gpu_group *g, int on);

#ifdef __cplusplus
}
#endif
#endif
