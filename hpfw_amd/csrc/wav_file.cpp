// wav_file.cpp -- see wav_file.h.  Replaces essentia's MonoLoader (reference include/hpfw/spectrum/cqt.h:45-52).
#include "wav_file.h"

#include <algorithm>
#include <cstring>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace hpfw {

void WavProbe::close()
{
    if (fd >= 0) ::close(fd);
    fd = -1;
}

WavProbe &WavProbe::operator=(WavProbe &&o) noexcept
{
    if (this != &o) {
        close();
        fd = std::exchange(o.fd, -1);
        data_off = o.data_off;
        frames = o.frames;
        channels = o.channels;
        rate = o.rate;
    }
    return *this;
}

bool probe_wav(const std::string &path, WavProbe &w, std::string &why, bool any_rate)
{
    w = WavProbe();
    WavProbe p;
    p.fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (p.fd < 0) {
        why = "cannot open " + path;
        return false;
    }
    struct stat stt;
    if (fstat(p.fd, &stt) != 0) {
        why = "cannot stat " + path;
        return false;
    }
    const int64_t fsize = (int64_t)stt.st_size;
    unsigned char hdr[12];
    if (pread(p.fd, hdr, 12, 0) != 12 || std::memcmp(hdr, "RIFF", 4) || std::memcmp(hdr + 8, "WAVE", 4)) {
        why = path + ": not a RIFF/WAVE file";
        return false;
    }
    uint16_t fmt = 0, channels = 0, bits = 0;
    uint32_t rate = 0;
    bool have_fmt = false;
    // (a 64-bit position: a chunk of any 32-bit size is stepped over, never wrapped back into)
    for (int64_t pos = 12; pos + 8 <= fsize;) {
        unsigned char ch[8];
        if (pread(p.fd, ch, 8, pos) != 8) break;
        uint32_t sz;
        std::memcpy(&sz, ch + 4, 4);
        if (!std::memcmp(ch, "fmt ", 4)) {
            if (sz < 16 || sz > 4096) break; // malformed: reported as "no data chunk" below
            unsigned char b[4096];
            if (pread(p.fd, b, sz, pos + 8) != (ssize_t)sz) break;
            std::memcpy(&fmt, b, 2);
            std::memcpy(&channels, b + 2, 2);
            std::memcpy(&rate, b + 4, 4);
            std::memcpy(&bits, b + 14, 2);
            if (fmt == 0xFFFE && sz >= 26) std::memcpy(&fmt, b + 24, 2); // WAVE_FORMAT_EXTENSIBLE: the sub-format's tag
            have_fmt = true;
        } else if (!std::memcmp(ch, "data", 4)) {
            const bool rate_ok = any_rate ? rate >= 8000 && rate <= 192000 : rate == 44100;
            if (!have_fmt || fmt != 1 || bits != 16 || (channels != 1 && channels != 2) || !rate_ok) {
                why = path + (any_rate ? ": only PCM16 mono/stereo at 8000..192000 Hz is supported" : ": only PCM16 mono/stereo at 44100 Hz is supported");
                return false;
            }
            // a streamed file may carry 0 or 0xffffffff as the size: trust the file's length instead
            const int64_t left = fsize - (pos + 8);
            int64_t bytes = sz;
            if (sz == 0 || bytes > left) bytes = std::min<int64_t>(left, 0xfffffffe);
            p.rate = rate;
            p.data_off = pos + 8;
            p.channels = channels;
            p.frames = bytes / 2 / channels;
            w = std::move(p);
            return true;
        }
        pos += 8 + (int64_t)sz + (sz & 1);
    }
    why = path + ": no data chunk";
    return false;
}

bool read_mono(const WavProbe &w, int16_t *dst)
{
    auto read_all = [&](void *to, int64_t want) {
        int64_t done = 0;
        while (done < want) {
            const ssize_t r = pread(w.fd, static_cast<char *>(to) + done, (size_t)(want - done), w.data_off + done);
            if (r <= 0) break;
            done += r;
        }
        return done == want;
    };
    if (w.channels == 1) return read_all(dst, w.frames * 2);
    std::vector<int16_t> raw((size_t)w.frames * 2);
    if (!read_all(raw.data(), w.frames * 4)) return false;
    for (int64_t k = 0; k < w.frames; ++k) dst[k] = (int16_t)(((int)raw[(size_t)(2 * k)] + (int)raw[(size_t)(2 * k + 1)]) / 2);
    return true;
}

bool read_wav_pcm16_mono(const std::string &path, std::vector<int16_t> &out, std::string &why, uint32_t *rate_any)
{
    WavProbe w;
    if (!probe_wav(path, w, why, rate_any != nullptr)) return false;
    out.resize((size_t)w.frames);
    if (!read_mono(w, out.data())) {
        why = path + ": short read";
        return false;
    }
    if (rate_any) *rate_any = w.rate;
    return true;
}

bool write_wav_pcm16(const std::string &path, const int16_t *pcm, int64_t n, int channels, std::string &why)
{
    if ((channels != 1 && channels != 2) || n < 0 || n % channels || n > (INT64_C(0x7fffffff) - 36) / 2 || (n > 0 && !pcm)) {
        why = "wav write: 1 or 2 channels, whole frames, less than 2^31 bytes";
        return false;
    }
    const uint32_t bytes = (uint32_t)(n * 2), rate = 44100, riff = 36 + bytes, fmt_size = 16, byte_rate = rate * (uint32_t)channels * 2;
    const uint16_t pcm_tag = 1, ch = (uint16_t)channels, align = (uint16_t)(channels * 2), bits = 16;
    unsigned char hdr[44];
    std::memcpy(hdr, "RIFF", 4);
    std::memcpy(hdr + 4, &riff, 4);
    std::memcpy(hdr + 8, "WAVEfmt ", 8);
    std::memcpy(hdr + 16, &fmt_size, 4);
    std::memcpy(hdr + 20, &pcm_tag, 2);
    std::memcpy(hdr + 22, &ch, 2);
    std::memcpy(hdr + 24, &rate, 4);
    std::memcpy(hdr + 28, &byte_rate, 4);
    std::memcpy(hdr + 32, &align, 2);
    std::memcpy(hdr + 34, &bits, 2);
    std::memcpy(hdr + 36, "data", 4);
    std::memcpy(hdr + 40, &bytes, 4);
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) {
        why = "cannot create " + path;
        return false;
    }
    auto write_all = [&](const void *from, int64_t want) {
        int64_t done = 0;
        while (done < want) {
            const ssize_t w = ::write(fd, static_cast<const char *>(from) + done, (size_t)(want - done));
            if (w <= 0) break;
            done += w;
        }
        return done == want;
    };
    const bool ok = write_all(hdr, 44) && write_all(pcm, (int64_t)bytes);
    if (::close(fd) != 0 || !ok) {
        why = path + ": short write";
        return false;
    }
    return true;
}

} // namespace hpfw
