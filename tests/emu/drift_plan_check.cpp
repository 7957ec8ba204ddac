// drift_plan_check.cpp -- the host side of clock drift and rendering (hpfw_amd/csrc/drift_plan.h) and the WAV writer
// (hpfw_amd/csrc/wav_file.cpp) in a program of its own, for the sanitizers: what a warp track must satisfy, the reach of a
// track against a direct scan, the anchors of a pair, the Theil-Sen line, the time map's bound and limits, and a file written
// and read back.  Built and run by tests/test_drift_host.py; argv[1] is a directory to write into.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../hpfw_amd/csrc/drift_plan.h"
#include "../../hpfw_amd/csrc/wav_file.h"

using namespace hpfw;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);                      \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static hpfw_warp_track track(int64_t off, int64_t len, int64_t i0, int64_t f0, int64_t d, int32_t g) { return hpfw_warp_track{off, len, i0, f0, d, g, 0}; }

static void check_tracks()
{
    const int64_t F = ((int64_t)1 << 40) - 1;
    EXPECT(!warp_check(track(0, 1000, 0, 0, 0, 1), 1000));
    EXPECT(!warp_check(track(1000, 0, -kWarpI0Max, F, kWarpDMax, (int32_t)kWarpGMax), 1000));
    EXPECT(!warp_check(track(0, 0, kWarpI0Max, 0, -kWarpDMax, (int32_t)-kWarpGMax), 0));
    EXPECT(warp_check(track(1, 1000, 0, 0, 0, 1), 1000));
    EXPECT(warp_check(track(1001, 0, 0, 0, 0, 1), 1000));
    EXPECT(warp_check(track(-1, 10, 0, 0, 0, 1), 1000));
    EXPECT(warp_check(track(0, -1, 0, 0, 0, 1), 1000));
    EXPECT(warp_check(track(INT64_MAX, 10, 0, 0, 0, 1), INT64_MAX));
    EXPECT(warp_check(track(0, 10, 0, 0, kWarpDMax + 1, 1), 1000));
    EXPECT(warp_check(track(0, 10, 0, 0, -kWarpDMax - 1, 1), 1000));
    EXPECT(warp_check(track(0, 10, 0, -1, 0, 1), 1000));
    EXPECT(warp_check(track(0, 10, 0, F + 1, 0, 1), 1000));
    EXPECT(warp_check(track(0, 10, kWarpI0Max + 1, 0, 0, 1), 1000));
    EXPECT(warp_check(track(0, 10, INT64_MIN, 0, 0, 1), 1000));
    EXPECT(warp_check(track(0, 10, 0, 0, 0, (int32_t)kWarpGMax + 1), 1000));
    EXPECT(warp_check(track(0, 10, 0, 0, 0, INT32_MIN), 1000));
    // the reach against a scan of every output near it
    const int64_t ds[] = {0, 1, -1, 13194140, -13194140, kWarpDMax, -kWarpDMax};
    const int64_t i0s[] = {0, 5, -5, -3000, 40, -70000, 100};
    for (int64_t d : ds)
        for (int64_t i0 : i0s)
            for (int64_t len : {(int64_t)1, (int64_t)31, (int64_t)4097}) {
                const hpfw_warp_track t = track(0, len, i0, 12345, d, 1);
                int64_t lo, hi, slo = kWarpMEnd, shi = -1;
                warp_reach(t, &lo, &hi);
                for (int64_t m = 0; m < 80000; ++m) {
                    const int64_t ip = warp_ip(t, m);
                    if (ip + kWarpH >= 0 && ip - kWarpH + 1 <= len - 1) {
                        if (slo == kWarpMEnd) slo = m;
                        shi = m;
                    }
                }
                EXPECT(lo == slo && hi == shi);
            }
    // at the far end of the outputs, and a source nothing reaches
    int64_t lo, hi;
    const int64_t far = kWarpMEnd - 3000;
    hpfw_warp_track t = track(0, 70001, -(far + ((far * kWarpDMax) >> 40)) + 30000, 0, kWarpDMax, 1);
    warp_reach(t, &lo, &hi);
    EXPECT(lo > far - 40000 && lo < far && hi == kWarpMEnd - 1 && warp_ip(t, lo) >= -kWarpH && warp_ip(t, lo - 1) < -kWarpH);
    warp_reach(track(0, 100, -kWarpI0Max, 0, -kWarpDMax, 1), &lo, &hi);
    EXPECT(lo == kWarpMEnd && hi == -1);
    warp_reach(track(0, 100, kWarpI0Max, (int64_t)1 << 39, kWarpDMax, 1), &lo, &hi);
    EXPECT(lo == kWarpMEnd && hi == -1);
    warp_reach(track(0, 0, 0, 0, 0, 1), &lo, &hi);
    EXPECT(lo == kWarpMEnd && hi == -1);
}

static void check_anchors()
{
    int64_t s[64];
    int32_t nl = -1, nr = -1;
    // an overlap shorter than one anchor, and of exactly one anchor: the centre alone
    EXPECT(drift_anchors(100, 600, 100, 500, 1000, 300, s, 64, &nl, &nr) == 1 && s[0] == 100 && nl == 0 && nr == 0);
    EXPECT(drift_anchors(100, 1100, 100, 1000, 1000, 300, s, 64, &nl, &nr) == 1 && s[0] == 100 && nl == 0 && nr == 0);
    // ragged ends: 2 whole anchors fit on the left of the centre, 3 on the right (the fourth would end one sample late)
    EXPECT(drift_anchors(7, 3056, 857, 1000, 1000, 300, s, 64, &nl, &nr) == 6);
    EXPECT(nl == 2 && nr == 3 && s[0] == 857 && s[1] == 557 && s[2] == 257 && s[3] == 1157 && s[4] == 1457 && s[5] == 1757);
    EXPECT(s[2] >= 7 && s[2] - 300 < 7 && s[5] + 1000 <= 3056 && s[5] + 300 + 1000 > 3056);
    EXPECT(drift_anchors(7, 3057, 857, 1000, 1000, 300, nullptr, 0, &nl, &nr) == 7 && nl == 2 && nr == 4);
    // counting, a buffer too small, and what is refused
    EXPECT(drift_anchors(0, 10000, 4500, 1000, 1000, 1000, s, 5, &nl, &nr) == -1);
    EXPECT(drift_anchors(0, 10000, 4500, 1000, 1000, 1000, s, 9, nullptr, nullptr) == 9);
    EXPECT(drift_anchors(0, 10000, 4500, 1001, 1000, 1000, s, 64, &nl, &nr) == -1);  // longer than an anchor
    EXPECT(drift_anchors(0, 10000, 9500, 1000, 1000, 1000, s, 64, &nl, &nr) == -1);  // ends outside the overlap
    EXPECT(drift_anchors(50, 10000, 49, 1000, 1000, 1000, s, 64, &nl, &nr) == -1);
    EXPECT(drift_anchors(0, 10000, 4500, 0, 1000, 1000, s, 64, &nl, &nr) == -1);
    EXPECT(drift_anchors(0, 10000, 4500, 1000, 1000, 0, s, 64, &nl, &nr) == -1);
    EXPECT(drift_anchors(-1, 10000, 4500, 1000, 1000, 1000, s, 64, &nl, &nr) == -1);
    EXPECT(drift_anchors(0, INT64_MAX, 4500, 1000, 1000, 1000, s, 64, &nl, &nr) == -1);
}

static void check_fit()
{
    double a = 1, b = 1, rms = 1;
    drift_fit(nullptr, nullptr, 0, &a, &b, &rms);
    EXPECT(a == 0 && b == 0 && rms == 0);
    const int64_t n[] = {5000, 1000, 9000, 13000, 17000, 21000}, lag[] = {105, 101, 109, 113, 5000, 121};
    drift_fit(n, lag, 1, &a, &b, &rms);
    EXPECT(a == 105 && b == 0 && rms == 0);
    drift_fit(n, lag, 2, &a, &b, &rms);
    EXPECT(a == 105 && b == 0 && rms > 0);
    drift_fit(n, lag, 4, &a, &b, &rms);
    EXPECT(a == 100 && b == 0.001 && rms == 0);
    drift_fit(n, lag, 6, &a, &b, &rms); // one wild value of six
    EXPECT(a == 100 && b == 0.001 && rms > 1000);
    const int64_t same[] = {7, 7, 7}, l3[] = {1, 2, 3};
    drift_fit(same, l3, 3, &a, &b, &rms); // no pair with different n
    EXPECT(a == 1 && b == 0);
}

static void check_time_map()
{
    int64_t i0, f0, d;
    const double two40 = 1099511627776.0;
    for (double B : {0.0, 1e-6, -1e-6, 3e-4, -3e-4, 9.7e-4, -9.7e-4})
        for (double A : {0.0, 0.5, -0.25, 1234.5678, -98765.4321, 1.5e8 + 0.3, -1.5e8 - 0.7}) {
            EXPECT(time_map_q40(A, B, &i0, &f0, &d));
            EXPECT(f0 >= 0 && f0 < ((int64_t)1 << 40) && d <= kWarpDMax && d >= -kWarpDMax);
            for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)1 << 20, kWarpMEnd - 1}) {
                const long double got = (long double)(i0 + m) + (long double)(f0 + m * d) / (long double)two40;
                const long double want = ((long double)m - (long double)A) / (1.0L + (long double)B);
                // (the comparison itself is good to 2^-63 of 2^31: the exact one is in tests/test_drift_host.py)
                EXPECT(fabsl(got - want) <= (1.0L + 1e-6L) * (1.0L / two40 + (long double)m / (2.0L * two40)) + 1e-9L);
            }
        }
    EXPECT(time_map_q40(0.0, 0.0, &i0, &f0, &d) && i0 == 0 && f0 == 0 && d == 0);
    EXPECT(time_map_q40(-3.0, 0.0, &i0, &f0, &d) && i0 == 3 && f0 == 0 && d == 0);
    EXPECT(time_map_q40(0.0, 0.000977, &i0, &f0, &d) && d < 0 && d > -kWarpDMax && time_map_q40(0.0, -0.000975, &i0, &f0, &d) && d < kWarpDMax);
    EXPECT(!time_map_q40(0.0, 0.000979, &i0, &f0, &d) && !time_map_q40(0.0, -0.000977, &i0, &f0, &d));
    EXPECT(!time_map_q40(0.0, 0.6, &i0, &f0, &d) && !time_map_q40(0.0, -1.0, &i0, &f0, &d) && !time_map_q40(0.0, NAN, &i0, &f0, &d));
    EXPECT(!time_map_q40(NAN, 0.0, &i0, &f0, &d) && !time_map_q40(1073741825.0, 0.0, &i0, &f0, &d) && !time_map_q40(INFINITY, 0.0, &i0, &f0, &d));
    EXPECT(time_map_q40(1073741824.0, 0.0, &i0, &f0, &d) && i0 == -1073741824);
}

static void check_wav(const std::string &dir)
{
    std::string why;
    std::vector<int16_t> x(1001), back;
    for (size_t i = 0; i < x.size(); ++i) x[i] = (int16_t)(i * 131 - 30000);
    const std::string p = dir + "/mono.wav";
    EXPECT(write_wav_pcm16(p, x.data(), (int64_t)x.size(), 1, why));
    EXPECT(read_wav_pcm16_mono(p, back, why) && back == x);
    EXPECT(write_wav_pcm16(dir + "/stereo.wav", x.data(), 1000, 2, why));
    EXPECT(read_wav_pcm16_mono(dir + "/stereo.wav", back, why) && back.size() == 500 && back[1] == (int16_t)((x[2] + x[3]) / 2));
    EXPECT(write_wav_pcm16(dir + "/empty.wav", nullptr, 0, 1, why) && read_wav_pcm16_mono(dir + "/empty.wav", back, why) && back.empty());
    EXPECT(!write_wav_pcm16(p, x.data(), 1001, 2, why) && why.rfind("wav write:", 0) == 0);  // half a frame
    EXPECT(!write_wav_pcm16(p, x.data(), 10, 3, why) && !write_wav_pcm16(p, x.data(), -1, 1, why) && !write_wav_pcm16(p, nullptr, 10, 1, why));
    EXPECT(!write_wav_pcm16(p, x.data(), ((int64_t)1 << 30), 1, why));                       // 2^31 bytes
    EXPECT(!write_wav_pcm16(dir + "/no/such/dir.wav", x.data(), 10, 1, why) && why.rfind("cannot create", 0) == 0);
    EXPECT(read_wav_pcm16_mono(p, back, why) && back == x);                                   // the refused calls wrote nothing
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    check_tracks();
    check_anchors();
    check_fit();
    check_time_map();
    check_wav(argv[1]);
    if (failures) return 1;
    std::printf("drift_plan_check ok\n");
    return 0;
}
