// tempo.h -- the hashprints of a WAV file rescaled to several tempos (and moved by several bin shifts) of its constant-Q
// spectrogram, as GpuStorage::find_topk_transposed takes them: a query played at rho times the
// indexed recording's tempo matches best at tempo rho.  Variant v is tempos[v / max(S, 1)] with shifts[v % max(S, 1)]
// (S = shifts.size(); shift 0 when shifts is empty), so a result's shift_index decodes to (tempo, shift) that way.  `h`
// holds the filters of the index (hpfw_gpu_set_filters); projection mode 1.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hpfw_gpu.h"

namespace hpfw {

/// per variant (tempo-major, then shift) the file's hashprints (44.1 kHz PCM16 WAV, mono or stereo downmixed as
/// hpfw_gpu_wav_read_pcm16 reads it), every variant cut to the common length; throws std::runtime_error with the
/// library's message on failure
inline std::vector<std::vector<uint64_t>> tempo_hashprints(hpfw_gpu *h, const std::string &path, const std::vector<float> &tempos,
                                                           const std::vector<int32_t> &shifts = {})
{
    auto fail = [](const char *what) { throw std::runtime_error(std::string("hpfw::tempo_hashprints: ") + what + ": " + hpfw_gpu_last_error()); };
    int64_t n = 0;
    if (hpfw_gpu_wav_read_pcm16(path.c_str(), nullptr, 0, &n) != 0) fail(path.c_str());
    std::vector<int16_t> pcm((size_t)n);
    if (hpfw_gpu_wav_read_pcm16(path.c_str(), pcm.data(), n, &n) != 0) fail(path.c_str());
    hpfw_geometry g;
    if (hpfw_gpu_geometry(h, n, &g) != 0) fail("geometry");
    int64_t ct = 0;
    if (hpfw_gpu_tempo_columns(g.c, tempos.data(), (int)tempos.size(), &ct) != 0) fail("tempos");
    const int64_t nhp = std::max<int64_t>(ct - 99, 0);
    const size_t v = tempos.size() * std::max<size_t>(shifts.size(), 1);
    std::vector<uint64_t> all((size_t)nhp * v);
    if (hpfw_gpu_extract_tempo_pcm16_host(h, pcm.data(), n, 1, tempos.data(), (int)tempos.size(), shifts.empty() ? nullptr : shifts.data(),
                                          (int)shifts.size(), all.data()) != 0)
        fail("extraction");
    std::vector<std::vector<uint64_t>> out(v);
    for (size_t i = 0; i < v; ++i) out[i].assign(all.begin() + i * nhp, all.begin() + (i + 1) * nhp);
    return out;
}

} // namespace hpfw
