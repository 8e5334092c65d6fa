// Stand-alone host check of the inline functions of csrc/vag_nested.h (nested sampling), built by tests/test_nested_host.py with the
// system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer.  For fixed tables of inputs it prints one line per row, every
// number as 16 hex digits (a double as its bits, an integer as its value):
//   "rank <lnl[0..n-1]> | <order[0..n-1]> <lstar>"  the order by counting vag::nested_before, as the rank kernel counts, and L*;
//   "shrink <j> <N> <n_j> <1 / n_j>"                 vag::nested_live_count and vag::nested_shrink;
//   "tick <it> <walk> <m> <tick>"                    vag::nested_tick;
//   "clone <u> <K> <j0>"                             vag::nested_clone_index;
//   "margin <5 inputs> <margin>"                     vag::nested_margin.
// The test forms the same numbers with sampling's numpy functions and compares the bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../vegasafterglow_amd/csrc/vag_nested.h"

static void put(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    std::printf(" %016llx", (unsigned long long)b);
}
static void put_int(long long x) { std::printf(" %016llx", (unsigned long long)x); }

static void rank_row(const std::vector<double>& lnl) {
    const int n = (int)lnl.size();
    std::vector<int> order(n, -1);
    double lstar = 0.0;
    for (int i = 0; i < n; ++i) {
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += vag::nested_before(lnl[j], j, lnl[i], i) ? 1 : 0;
        order[rank] = i;
        if (rank == n / 2 - 1) lstar = lnl[i];
    }
    std::printf("rank");
    for (double x : lnl) put(x);
    std::printf(" |");
    for (int s : order) put_int(s);
    put(lstar);
    std::printf("\n");
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    rank_row({-3.0, -1.0, -2.0, -4.0});                     // all different
    rank_row({-1.0, -1.0, -1.0, -1.0});                     // all equal: the order of the slots
    rank_row({-2.5, -7.0, -2.5, -7.0, -1.0, -2.5});         // equal ln L in two and three slots, ordered by slot
    rank_row({0.0, -0.0, 1e-300, -1e-300, 5.0, 5.0, -1e300, 1e300});  // signed zeros are equal; the tie sits on the K - 1 | K boundary
    rank_row({-10.0, -10.000000000000002, -9.999999999999998, -10.0});  // neighbours in the last bit
    for (int n_live : {4, 6, 130, 16384})
        for (unsigned long long j : {0ull, 1ull, 2ull, 64ull, 65ull, 8191ull, 8192ull, 1000003ull, (1ull << 40) + 7ull}) {
            const long long n = vag::nested_live_count(j, n_live);
            std::printf("shrink");
            put_int((long long)j);
            put_int(n_live);
            put_int(n);
            put(vag::nested_shrink(n));
            std::printf("\n");
        }
    const unsigned long long its[] = {0ull, 1ull, 7ull, (1ull << 32) + 5ull, 1ull << 50};
    for (unsigned long long it : its)
        for (int walk : {1, 20, 80})
            for (int m : {0, 1, walk}) {
                std::printf("tick");
                put_int((long long)it);
                put_int(walk);
                put_int(m);
                put_int((long long)vag::nested_tick(it, walk, m));
                std::printf("\n");
            }
    const double us[] = {0.0, 0x1p-53, 0.25, 0.5, 0.4999999999999999, 0.7499999999999999, 1.0 - 0x1p-53, 0.3333333333333333, 0.9999};
    for (double u : us)
        for (int k : {2, 3, 65, 512, 8192, 8191}) {
            std::printf("clone");
            put(u);
            put_int(k);
            put_int(vag::nested_clone_index(u, k));
            std::printf("\n");
        }
    // lnl_new, lnprior_new, lnprior_old, lstar, log_u
    const double margin[][5] = {
        {-3.0, -2.0794415416798357, -2.0794415416798357, -5.0, -0.6931471805599453},  // above L*, a flat prior: taken, margin -log u
        {-5.0, -2.0794415416798357, -2.0794415416798357, -5.0, -30.0},                // ln L' == L*: rejected whatever the draw
        {-5.0, -1.0, -9.0, -5.0, -inf},                                               // ... u = 0 included
        {-5.000000000000001, -1.0, -2.0, -5.0, -1e-3},                                // one ulp below L*
        {-4.999999999999999, -1.0, -2.0, -5.0, -1e-3},                                // one ulp above: decided by the priors
        {-1.0, -3.5, -1.25, -5.0, -0.1},                                              // the prior falls by more than the draw allows
        {-1.0, -3.5, -1.25, -5.0, -2.25},                                             // ... by exactly what it allows: margin 0, rejected
        {-1.0, -3.5, -1.25, -5.0, -2.2500000000000004},                               // ... by an ulp less: taken
        {-1.0, -1.0, -1.0, -5.0, -inf},                                               // u = 0: margin +inf
        {nan, -1.0, -1.0, -5.0, -inf},                                                // not finite in ln L': rejected whatever the draw
        {inf, -1.0, -1.0, -5.0, -inf},
        {-inf, -1.0, -1.0, -5.0, -inf},
        {-1.0, nan, -1.0, -5.0, -inf},                                                // not finite in ln prior'
        {-1.0, inf, -1.0, -5.0, -inf},
        {-1.0, -inf, -1.0, -5.0, -inf},
        {nan, nan, -1.0, -5.0, -1.0},
        {1e300, -1e300, 1e300, -1e300, -745.0},                                       // huge finite values are decided like any other
        {-42.68221159873594, -3.660178848656387, -3.901722806019508, -44.65546933420461, -1.2039728043259361},
    };
    for (const auto& r : margin) {
        std::printf("margin");
        for (double x : r) put(x);
        put(vag::nested_margin(r[0], r[1], r[2], r[3], r[4]));
        std::printf("\n");
    }
    return 0;
}
