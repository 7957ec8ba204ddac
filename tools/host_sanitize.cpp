// Host-only code of the library (table building, Mel tables, eigen-solver, supported lengths, file parsers) under the
// sanitizers -- GPU sanitizers are not available on this pool, the device side is covered by parity tests:
//   bash tools/host_sanitize.sh        (AddressSanitizer + UBSan, then ThreadSanitizer)
#include "plan.h"
#include "cache_files.h"
#include "wav_file.h"
#include <cstdio>
#include <fstream>
#include <thread>
#include <string>
#include <vector>
#include <random>
extern "C" int hpfw_gpu_host_top_eigenvectors(const float *a, int n, int m, float *vec, double *val);
extern "C" long long hpfw_gpu_supported_length(long long n);
int main()
{
    const long long lens[] = {1323000, 88200, 220500, 2646000, 7938000, 54432, 1327104};
    for (long long n : lens) {
        hpfw::HostPlan p;
        std::string why;
        bool ok = hpfw::build_plan(n, p, why, false);
        std::printf("%lld %d %s classes=%zu\n", n, (int)ok, why.c_str(), p.classes.size());
    }
    hpfw::HostPlan f; std::string why;
    std::printf("frame %d\n", (int)hpfw::build_frame_transform(4410, f, why));
    std::vector<float> w, c; hpfw::mel_tables(w, c);
    std::printf("mel %zu %zu\n", w.size(), c.size());
    const int n = 200, m = 16;
    std::mt19937 g(1); std::normal_distribution<float> d;
    std::vector<float> x(n * 300), a(n * n, 0.f);
    for (auto &v : x) v = d(g);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = 0; for (int k = 0; k < 300; ++k) s += x[i*300+k]*x[j*300+k]; a[i*n+j] = (float)(s/300); }
    std::vector<float> vec(m * n); std::vector<double> val(m);
    const int rc = hpfw_gpu_host_top_eigenvectors(a.data(), n, m, vec.data(), val.data());
    std::printf("eig rc %d %f\n", rc, val[0]);
    for (long long q : {10LL, 1323001LL, 5000000LL, 158760000LL}) std::printf("supp %lld -> %lld\n", q, hpfw_gpu_supported_length(q));
    // the file parsers, from two threads at once as the window reader's team calls them: a stereo WAV and a cached spectrogram
    char dir[] = "/tmp/hpfw_sanitize_XXXXXX";
    if (!mkdtemp(dir)) return 1;
    const std::string wav = std::string(dir) + "/s.wav", img = std::string(dir) + "/spectro";
    {
        const unsigned char head[44] = {'R', 'I', 'F', 'F', 44, 0, 0, 0, 'W', 'A', 'V', 'E', 'f', 'm', 't', ' ', 16, 0, 0, 0, 1, 0, 2, 0, 0x44, 0xac, 0, 0,
                                        0x10, 0xb1, 2, 0, 4, 0, 16, 0, 'd', 'a', 't', 'a', 8, 0, 0, 0};
        const int16_t lr[4] = {-3, 0, 7, 2};
        std::ofstream os(wav, std::ios::binary);
        os.write(reinterpret_cast<const char *>(head), 44);
        os.write(reinterpret_cast<const char *>(lr), 8);
    }
    std::vector<float> spec(121 * 9, -40.0f);
    bool files_ok = hpfw::save_spectro_cereal(img, spec.data(), 9);
    auto parse = [&](bool *ok) {
        std::vector<int16_t> pcm;
        std::vector<float> cm;
        std::string msg;
        int32_t cols = 0;
        *ok = hpfw::read_wav_pcm16_mono(wav, pcm, msg) && pcm == std::vector<int16_t>{-1, 4} && hpfw::load_spectro_cereal(img, cm, cols) && cols == 9;
    };
    bool ok_a = false, ok_b = false;
    std::thread other(parse, &ok_a);
    parse(&ok_b);
    other.join();
    std::remove(wav.c_str());
    std::remove(img.c_str());
    std::remove(dir);
    std::printf("parsers %d\n", (int)(files_ok && ok_a && ok_b));
    return files_ok && ok_a && ok_b ? 0 : 1;
}
