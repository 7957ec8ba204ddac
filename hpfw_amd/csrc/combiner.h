// combiner.h -- AudioCombiner's exact-hash inverted index and offset-vote search (reference
// include/hpfw/audioproblems/combiner/combiner.h:90-132) on the device: the index and the orchestration of
// k_combiner.hip's kernels.  combiner.hip wraps it in the C-ABI (include/hpfw_gpu.h, hpfw_gpu_combiner_*).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/hpfw_gpu.h"
#include "hip_owned.h"

namespace hpfw {

class Combiner {
public:
    Combiner() = default;
    Combiner(const Combiner &) = delete;
    Combiner &operator=(const Combiner &) = delete;

    void clear();
    int64_t size() const { return (int64_t)rec_off_.size() - 1; }
    // appends recordings (host or device hashprints) and rebuilds the CSR on stream s.  0 or an HPFW_E_* status (err set)
    int add(const uint16_t *hp, bool device, const int64_t *offsets, int64_t n_rec, hipStream_t s, std::string &err);
    int get(int64_t *val_start, uint32_t *rec, uint32_t *off, int64_t cap, std::string &err);
    // d_find [n_q] and / or d_align [n_q][k] (either may be null), device; q_off, exclude host
    int search(const uint16_t *d_q, const int64_t *q_off, const int32_t *exclude, int64_t n_q, hpfw_combine_result *d_find,
               int k, hpfw_align_hit *d_align, hipStream_t s, std::string &err);

private:
    int rebuild(hipStream_t s, std::string &err);

    std::vector<int64_t> rec_off_{0}; // recording j is positions [rec_off_[j], rec_off_[j+1])
    bool stale_ = false; // the device tables do not describe rec_off_ (a rebuild failed part-way)
    DevBuf hp_;         // uint16 [positions]: every recording's hashprints back to back
    DevBuf rec_off_d_;  // uint32 [n_rec + 1]
    DevBuf val_start_;  // uint32 [65537]
    DevBuf post_;       // uint2 (rec, off) [positions], ascending position inside every value
    DevBuf sort_keys_, sort_vals_, sort_vals_out_, temp_; // build and search scratch
    // search scratch
    DevBuf q_tab_, fr_len_, fr_tab_, ev_keys_, ev_keys_s_, ev_vals_, ev_vals_s_, ev_rec_, ev_cnt_, bins_, peaks_;
};

} // namespace hpfw
