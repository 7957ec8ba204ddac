// emu_prune.cpp -- host-side SIMT emulation (tests only) of what the row transform leaves out because nothing reads it
// (HPFW_PRUNE of the handle): hpfw_amd/csrc/fft_rows.h compiled with -DHPFW_SIMT_EMU, the pruned body against the full one on
// the same random input, bit for bit.
//   rows : rows2_body<Groups6300, LastEdges> against <Groups6300, LastAll> for the window geometries of the shortest and the
//          longest clip with n2 = 6300 -- every LDS position the epilogue reads, and the stored forward bins
//   rule : plan.h rows_last_needed / rows_last_edges_ok on windows that do and do not fit outputs {0, 1, 18, 19}
// usage: emu_prune quick|full   (quick: two rows of one geometry and the rule -- what the sanitizer build runs)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hpfw_amd/csrc/fft_rows.h"
#include "../../hpfw_amd/csrc/plan.h"

using hpfw::cf;

template <class T>
struct Checked {
    T *p;
    size_t n;
    T &operator[](long i) const
    {
        if (i < 0 || (size_t)i >= n) {
            std::fprintf(stderr, "LDS index %ld out of [0,%zu)\n", i, n);
            std::abort();
        }
        return p[i];
    }
};

static unsigned g_seed = 2463534242u;
static float rnd() // uniform in [-1, 1)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((double)(g_seed >> 8) / 8388608.0 - 1.0);
}
static const cf kNan = {__builtin_nanf(""), __builtin_nanf("")};
static bool same_bits(const cf &a, const cf &b) { return std::memcmp(&a, &b, sizeof(cf)) == 0; }

static long g_bad = 0;
static void fail(const char *what, long a = 0, long b = 0, long c = 0)
{
    if (g_bad < 10) std::fprintf(stderr, "MISMATCH %s (%ld, %ld, %ld)\n", what, a, b, c);
    ++g_bad;
}

// ---- row transform --------------------------------------------------------------------------------------------
static hpfw::RowsArgs rows_args(const hpfw::HostPlan &hp)
{
    hpfw::RowsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n1 = hp.n1;
    a.n2 = hp.n2;
    a.h = hp.h;
    a.hpad = (hp.h + 31) / 32 * 32;
    a.pair_stride = 1;
    a.groups.n = (int)hp.groups.size();
    for (size_t g = 0; g < hp.groups.size(); ++g) {
        a.groups.r1[g] = hp.groups[g].first;
        a.groups.r2[g] = hp.groups[g].second;
        a.groups.tw_off[g] = hp.rows_gtw_off[g];
    }
    a.gtw = reinterpret_cast<const cf *>(hp.rows_gtw.data());
    a.pos_n2 = hp.pos_n2.data();
    a.kb_last = hp.kb_last.data();
    return a;
}

// rows q1 of one clip length through both policies; returns the number of LDS positions compared
static long check_rows(long n, const std::vector<int> &rows_in)
{
    hpfw::HostPlan hp;
    std::string why;
    if (!hpfw::build_plan(n, hp, why)) {
        std::fprintf(stderr, "plan %ld: %s\n", n, why.c_str());
        std::exit(2);
    }
    const hpfw::RowsArgs a = rows_args(hp);
    if (!hpfw::Groups6300::matches_plan(a)) {
        std::fprintf(stderr, "%ld samples: not the compile-time group sequence\n", n);
        std::exit(2);
    }
    if (!hpfw::rows_last_edges_ok(hp.rows_last_mask, hpfw::Groups6300::kLastPoints)) fail("plan does not pick the pruned row kernel", n, hp.rows_last_mask);
    const hpfw::Rows2Out o{hp.n1, hp.hq, hp.q2lo, hp.q2w, reinterpret_cast<const cf *>(hp.ts_seed.data()),
                           reinterpret_cast<const cf *>(hp.ts_step.data()), (hp.n2 + 3) / 4,
                           28 /* one contiguous row: every piece in block 0 */, 0, hp.n2 /* Im row n2 floats behind Re */, 0, 0};
    std::vector<cf> xa((size_t)hp.n1 * hp.q2w, kNan), xb = xa;
    std::vector<float> z((size_t)2 * hp.n2);
    long compared = 0;
    for (int q1 : rows_in) {
        if (q1 < 0 || q1 >= hp.hq) continue;
        for (float &v : z) v = std::ldexp(rnd(), 38); // the column stage's integers: up to n1 2^15 2^22
        std::vector<cf> la((size_t)hp.n2, kNan), lb = la;
        Checked<cf> lds_a{la.data(), la.size()}, lds_b{lb.data(), lb.size()};
        hpfw::rows2_body<hpfw::Groups6300, hpfw::LastAll>(lds_a, a, 512, z.data(), q1, o, xa.data());
        hpfw::rows2_body<hpfw::Groups6300, hpfw::LastEdges>(lds_b, a, 512, z.data(), q1, o, xb.data());
        for (int q2 = hp.q2lo; q2 < hp.q2lo + hp.q2w; ++q2)
            for (int src : {q2, hp.n2 - 1 - q2}) {
                if (!same_bits(la[(size_t)src], lb[(size_t)src])) fail("row LDS", n, q1, src);
                if (la[(size_t)src].r != la[(size_t)src].r) fail("row LDS not written by the full policy", n, q1, src);
                ++compared;
            }
    }
    if (std::memcmp(xa.data(), xb.data(), xa.size() * sizeof(cf)) != 0) fail("forward bins", n);
    std::printf("rows n=%ld n1=%d q2lo=%d q2w=%d mask=0x%x positions=%ld\n", n, hp.n1, hp.q2lo, hp.q2w, hp.rows_last_mask, compared);
    return compared;
}

// the shortest and the longest clip whose row transform is the n2 = 6300 sequence
static void groups6300_lengths(long &shortest, long &longest)
{
    shortest = longest = 0;
    for (long n1 = 2; n1 <= 400; ++n1) {
        hpfw::HostPlan hp;
        std::string why;
        if (!hpfw::build_plan(6300 * n1, hp, why, true) || hp.bluestein || hp.n2 != 6300) continue;
        if (!shortest) shortest = 6300 * n1;
        longest = 6300 * n1;
    }
}

// ---- plan rule -------------------------------------------------------------------------------------------------
static void check_rule()
{
    hpfw::HostPlan hp;
    std::string why;
    if (!hpfw::build_plan(88200, hp, why)) std::exit(2);
    const int n2 = hp.n2, r = hpfw::Groups6300::kLastPoints, nb = n2 / r;
    struct Case {
        int q2lo, q2w;
        bool pruned;
    };
    const Case cases[] = {{18, 598, true},  {hp.q2lo, hp.q2w, true}, {0, 315, true},   {0, 630, true},   {18, 612, true},
                          {18, 640, false}, {18, 613, false},        {650, 100, false}, {0, n2, false}, {3000, 300, false}};
    for (const Case &c : cases) {
        const unsigned mask = hpfw::rows_last_needed(hp.kb_last.data(), nb, r, n2, c.q2lo, c.q2w);
        // kb_last is a permutation of 0 .. nb - 1: output f of some block is every k2 of [nb f, nb (f + 1))
        unsigned expect = 0;
        for (int q2 = c.q2lo; q2 < c.q2lo + c.q2w; ++q2) expect |= (1u << (q2 / nb)) | (1u << ((n2 - 1 - q2) / nb));
        if (mask != expect) fail("needed outputs", c.q2lo, c.q2w, mask);
        const bool pruned = hpfw::rows_last_edges_ok(mask, r);
        if (pruned != c.pruned) fail("selection", c.q2lo, c.q2w, mask);
        if (c.q2w == 640 && !(mask & 4u)) fail("a window of 640 needs output 2", c.q2lo, c.q2w, mask);
        if (pruned) { // what LastEdges stores covers both windows, for every block
            std::vector<char> written((size_t)n2, 0);
            for (int b = 0; b < nb; ++b)
                for (int f = 0; f < r; ++f)
                    if (hpfw::LastEdges::keep(f, r)) written[(size_t)(hp.kb_last[(size_t)b] + nb * f)] = 1;
            for (int q2 = c.q2lo; q2 < c.q2lo + c.q2w; ++q2)
                if (!written[(size_t)q2] || !written[(size_t)(n2 - 1 - q2)]) fail("pruned stores do not cover the window", c.q2lo, c.q2w, q2);
        }
        std::printf("rule q2lo=%d q2w=%d mask=0x%05x %s\n", c.q2lo, c.q2w, mask, pruned ? "pruned" : "full");
    }
}

int main(int argc, char **argv)
{
    const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;
    long shortest = 0, longest = 0;
    groups6300_lengths(shortest, longest);
    std::printf("n2 = 6300 from %ld to %ld samples\n", shortest, longest);
    if (!shortest) return 2;
    {
        hpfw::HostPlan hp;
        std::string why;
        if (!hpfw::build_plan(shortest, hp, why, true)) return 2;
        check_rows(shortest, quick ? std::vector<int>{0, hp.hq - 1} : std::vector<int>{0, 1, hp.hq / 2, hp.hq - 1});
    }
    if (!quick) {
        hpfw::HostPlan hp;
        std::string why;
        if (!hpfw::build_plan(longest, hp, why, true)) return 2;
        check_rows(longest, {0, 1, hp.hq / 2, hp.hq - 1});
        check_rows(1323000, {0, 1, 105});
    }
    check_rule();
    std::printf("mismatches=%ld\n", g_bad);
    return g_bad ? 1 : 0;
}
