// transposed.h -- the hashprints of a WAV file under several bin shifts of its constant-Q spectrogram (DESIGN.md
// section 11), as GpuStorage::find_topk_transposed takes them: a query t semitones above the indexed recording matches
// at shift 2t.  `h` holds the filters of the index (hpfw_gpu_set_filters); projection mode 1.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hpfw_gpu.h"

namespace hpfw {

/// per shift the file's hashprints (44.1 kHz PCM16 WAV, mono or stereo downmixed as hpfw_gpu_wav_read_pcm16 reads it);
/// throws std::runtime_error with the library's message on failure
inline std::vector<std::vector<uint64_t>> transposed_hashprints(hpfw_gpu *h, const std::string &path, const std::vector<int32_t> &shifts)
{
    auto fail = [](const char *what) { throw std::runtime_error(std::string("hpfw::transposed_hashprints: ") + what + ": " + hpfw_gpu_last_error()); };
    int64_t n = 0;
    if (hpfw_gpu_wav_read_pcm16(path.c_str(), nullptr, 0, &n) != 0) fail(path.c_str());
    std::vector<int16_t> pcm((size_t)n);
    if (hpfw_gpu_wav_read_pcm16(path.c_str(), pcm.data(), n, &n) != 0) fail(path.c_str());
    hpfw_geometry g;
    if (hpfw_gpu_geometry(h, n, &g) != 0) fail("geometry");
    std::vector<uint64_t> all((size_t)(g.n_hp > 0 ? g.n_hp : 0) * shifts.size());
    if (hpfw_gpu_extract_transposed_pcm16_host(h, pcm.data(), n, 1, shifts.data(), (int)shifts.size(), all.data()) != 0) fail("extraction");
    std::vector<std::vector<uint64_t>> out(shifts.size());
    for (size_t i = 0; i < shifts.size(); ++i) out[i].assign(all.begin() + i * g.n_hp, all.begin() + (i + 1) * g.n_hp);
    return out;
}

} // namespace hpfw
