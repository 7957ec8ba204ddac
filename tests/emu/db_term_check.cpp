// db_term_check.cpp -- db_term_fast against db_term_spec (hpfw_amd/csrc/db_spec.h) on the host: the same
// text the kernels compile, with the hardware's fused multiply-add.
//   g++ -O2 -std=c++17 -DHPFW_SIMT_EMU -ffp-contract=off -mfma -o db_term_check tests/emu/db_term_check.cpp -lpthread
//   db_term_check all                 every bit pattern 0 .. 0x7F800000 (+0 up to +inf)
//   db_term_check quick               every 4099th pattern and +-64 patterns around each place where a path changes
//   db_term_check range FIRST COUNT   COUNT consecutive patterns from FIRST (what the GPU sweep is compared with)
// One result line: patterns (mode quick: of the strided sample; the others are counted as edge patterns), those inside 1e-10f <= p < inf (the others go to the specified sequence as they are), mismatches,
// fallbacks (patterns inside for which db_term_fast was not certain and ran the specified sequence) and their share of
// the patterns inside, the largest |y - 10 log10_spec| in double, and the fallbacks' share of a log-uniform p in [1e-10, 1e6].
// Exit status 1 if any input differs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../hpfw_amd/csrc/db_spec.h"

namespace {

constexpr uint32_t kInf = 0x7f800000u;
const uint32_t kLowest = __builtin_bit_cast(uint32_t, 1e-10f);
const uint32_t kMillion = __builtin_bit_cast(uint32_t, 1e6f);

struct Tally {
    uint64_t patterns = 0, inside = 0, mismatches = 0, fallbacks = 0, first_bad = ~0ull;
    uint64_t lu_patterns = 0; // patterns in [1e-10, 1e6)
    double max_diff = 0.0;
    double lu_fallback = 0.0, lu_all = 0.0; // log-uniform measure: the width ln(next / p) of each pattern
    void add(const Tally &o)
    {
        patterns += o.patterns;
        inside += o.inside;
        mismatches += o.mismatches;
        fallbacks += o.fallbacks;
        first_bad = std::min(first_bad, o.first_bad);
        lu_patterns += o.lu_patterns;
        max_diff = std::max(max_diff, o.max_diff);
        lu_fallback += o.lu_fallback;
        lu_all += o.lu_all;
    }
};

inline void one(uint32_t bits, Tally &t)
{
    const float p = __builtin_bit_cast(float, bits);
    const float a = hpfw::db_term_spec(p), b = hpfw::db_term_fast(p);
    const bool inside = hpfw::db_fast_in_range(p);
    float unused;
    const bool fb = inside && !hpfw::db_fast_certain(p, unused);
    ++t.patterns;
    t.inside += inside;
    t.fallbacks += fb;
    if (__builtin_bit_cast(uint32_t, a) != __builtin_bit_cast(uint32_t, b)) {
        ++t.mismatches;
        t.first_bad = std::min<uint64_t>(t.first_bad, bits);
    }
    if (inside) {
        const double d = hpfw::db_fast_y(p) - 10.0 * hpfw::log10_spec((double)p);
        t.max_diff = std::max(t.max_diff, d < 0 ? -d : d);
        if (bits < kMillion) {
            const double w = ((double)__builtin_bit_cast(float, bits + 1) - (double)p) / (double)p;
            ++t.lu_patterns;
            t.lu_all += w;
            if (fb) t.lu_fallback += w;
        }
    }
}

void around(std::vector<uint32_t> &v, int64_t centre)
{
    for (int64_t b = centre - 64; b <= centre + 64; ++b)
        if (b >= 0 && b <= (int64_t)kInf) v.push_back((uint32_t)b);
}

// the strided sample first (n_strided of them: the shares are taken over these alone), then the places where a path changes
std::vector<uint32_t> quick_list(size_t &n_strided)
{
    std::vector<uint32_t> v;
    for (uint64_t b = 0; b <= kInf; b += 4099) v.push_back((uint32_t)b);
    n_strided = v.size();
    around(v, kLowest);
    around(v, kInf);
    const uint32_t sqrt2 = __builtin_bit_cast(uint32_t, 1.41421356f) & 0x7fffffu;
    for (int64_t e = 0; e < 255; ++e) {
        around(v, e << 23);                 // powers of two (e = 0: zero and the denormals)
        around(v, (e << 23) | sqrt2);       // where the specified sequence halves m
        for (int64_t i = 1; i < (1 << HPFW_DB_CELL_BITS); ++i) around(v, (e << 23) | (i << (23 - HPFW_DB_CELL_BITS)));
    }
    return v;
}

} // namespace

int main(int argc, char **argv)
{
    const char *mode = argc > 1 ? argv[1] : "quick";
    const unsigned hw = std::thread::hardware_concurrency();
    const int nt = (int)std::min(16u, hw ? hw : 1u);
    std::vector<Tally> part(nt), edge(nt);
    size_t n_strided = 0;
    std::vector<std::thread> th;
    std::vector<uint32_t> list;
    uint64_t first = 0, count = 0;
    if (!strcmp(mode, "all")) {
        count = (uint64_t)kInf + 1;
    } else if (!strcmp(mode, "range") && argc > 3) {
        first = strtoull(argv[2], nullptr, 0);
        count = strtoull(argv[3], nullptr, 0);
        if (first > kInf || count > (uint64_t)kInf + 1 - first) {
            fprintf(stderr, "range past +inf\n");
            return 2;
        }
    } else if (!strcmp(mode, "quick")) {
        list = quick_list(n_strided);
    } else {
        fprintf(stderr, "usage: %s all | quick | range FIRST COUNT\n", argv[0]);
        return 2;
    }
    for (int k = 0; k < nt; ++k)
        th.emplace_back([&, k] {
            Tally t;
            if (!list.empty()) {
                for (size_t i = k; i < n_strided; i += nt) one(list[i], t);
                for (size_t i = n_strided + k; i < list.size(); i += nt) one(list[i], edge[k]);
            } else { // blocks of 2^16 patterns in turn, so that the threads finish together
                for (uint64_t b0 = (uint64_t)k << 16; b0 < count; b0 += (uint64_t)nt << 16)
                    for (uint64_t b = b0; b < std::min(count, b0 + 65536); ++b) one((uint32_t)(first + b), t);
            }
            part[k] = t;
        });
    for (auto &t : th) t.join();
    Tally t;
    for (const Tally &p : part) t.add(p);
    Tally e;
    for (const Tally &p : edge) e.add(p);
    t.mismatches += e.mismatches;
    t.first_bad = std::min(t.first_bad, e.first_bad);
    t.max_diff = std::max(t.max_diff, e.max_diff);
    printf("mode=%s cells=%d degree=%d delta=%.3e patterns=%llu inside=%llu mismatches=%llu fallbacks=%llu fallback_share=%.3e "
           "max_abs_diff=%.3e loguniform_patterns=%llu loguniform_fallback_share=%.3e edge_patterns=%llu edge_fallbacks=%llu "
           "first_mismatch=0x%llx\n",
           mode, 1 << HPFW_DB_CELL_BITS, HPFW_DB_DEGREE, (double)HPFW_DB_DELTA, (unsigned long long)t.patterns,
           (unsigned long long)t.inside, (unsigned long long)t.mismatches, (unsigned long long)t.fallbacks,
           t.inside ? (double)t.fallbacks / t.inside : 0.0,
           t.max_diff, (unsigned long long)t.lu_patterns, t.lu_all > 0 ? t.lu_fallback / t.lu_all : 0.0,
           (unsigned long long)e.patterns, (unsigned long long)e.fallbacks, (unsigned long long)(t.mismatches ? t.first_bad : 0));
    return t.mismatches ? 1 : 0;
}
