// The library's two parsers of user-supplied files (hpfw_amd/csrc/wav_file.cpp, cache_files.cpp) as a stand-alone host
// program, built with the sanitizers by tests/test_wav_host.py:
//   wav_check wav <file.wav> <out.bin> [any]     "ok <rate> <samples>" + the mono samples (int16) in out.bin, or "error: <why>"
//   wav_check save <in.bin> <cols> <file>        in.bin: a bin-major [121][cols] float spectrogram -> the cache's image
//   wav_check load <file> <out.bin>              "ok <cols>" + the matrix as stored (column-major floats), or "rejected"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "cache_files.h"
#include "wav_file.h"

static bool dump(const char *path, const void *p, size_t bytes)
{
    std::ofstream os(path, std::ios::binary);
    os.write(static_cast<const char *>(p), (std::streamsize)bytes);
    return (bool)os;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "wav" && argc >= 4) {
        std::vector<int16_t> pcm;
        std::string why;
        uint32_t rate = 44100;
        if (!hpfw::read_wav_pcm16_mono(argv[2], pcm, why, argc > 4 ? &rate : nullptr)) {
            std::printf("error: %s\n", why.c_str());
            return 0;
        }
        // the window reader's two calls give the same samples
        hpfw::WavProbe w;
        if (!hpfw::probe_wav(argv[2], w, why, argc > 4) || (size_t)w.frames != pcm.size()) return 2;
        std::vector<int16_t> again(pcm.size());
        hpfw::WavProbe moved = std::move(w);
        if (w.ok() || !hpfw::read_mono(moved, again.data()) || again != pcm) return 2;
        std::printf("ok %u %zu\n", rate, pcm.size());
        return dump(argv[3], pcm.data(), pcm.size() * 2) ? 0 : 3;
    }
    if (mode == "save" && argc == 5) {
        const int32_t cols = std::atoi(argv[3]);
        std::vector<float> bm((size_t)121 * cols);
        std::ifstream is(argv[2], std::ios::binary);
        if (!is.read(reinterpret_cast<char *>(bm.data()), (std::streamsize)bm.size() * 4)) return 3;
        return hpfw::save_spectro_cereal(argv[4], bm.data(), cols) ? 0 : 2;
    }
    if (mode == "load" && argc == 4) {
        std::vector<float> cm;
        int32_t cols = 0;
        if (!hpfw::load_spectro_cereal(argv[2], cm, cols)) {
            std::printf("rejected\n");
            return 0;
        }
        std::printf("ok %d\n", cols);
        return dump(argv[3], cm.data(), cm.size() * 4) ? 0 : 3;
    }
    std::fprintf(stderr, "usage: wav_check wav|save|load ...\n");
    return 1;
}
