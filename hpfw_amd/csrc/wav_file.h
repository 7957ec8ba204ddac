// wav_file.h -- the RIFF/WAVE reader of the file entry points (legacy.cpp): PCM16, mono or stereo, at 44.1 kHz or, on
// request, at any rate in [8 000, 192 000] Hz.  Host-only: no HIP, no handle; a failure is a message in `why`.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace hpfw {

// where the samples of a file lie; owns the open file descriptor
struct WavProbe {
    int fd = -1;
    int64_t data_off = 0, frames = 0; // payload offset; samples per channel
    int channels = 0;
    uint32_t rate = 44100;

    WavProbe() = default;
    WavProbe(WavProbe &&o) noexcept { *this = std::move(o); }
    WavProbe &operator=(WavProbe &&o) noexcept;
    ~WavProbe() { close(); }
    void close();
    bool ok() const { return fd >= 0; }
};

// the chunk walk, without reading the payload.  any_rate: accept every rate in [8 000, 192 000] Hz (else 44.1 kHz only)
bool probe_wav(const std::string &path, WavProbe &w, std::string &why, bool any_rate);

// the w.frames samples of the file into dst, stereo averaged (truncating toward zero: MonoLoader's "mix" downmix);
// false on a short read
bool read_mono(const WavProbe &w, int16_t *dst);

// probe, resize, read_mono.  rate_any: NULL = 44.1 kHz only; else any rate in the range is accepted and stored there
bool read_wav_pcm16_mono(const std::string &path, std::vector<int16_t> &out, std::string &why, uint32_t *rate_any = nullptr);

// pcm [n] (interleaved when channels = 2) as a file with a 44-byte header: PCM16 at 44.1 kHz
bool write_wav_pcm16(const std::string &path, const int16_t *pcm, int64_t n, int channels, std::string &why);

} // namespace hpfw
