// Stand-alone host check of csrc/vag_predict.h (posterior-predictive quantile bands), built by tests/test_predict_host.py with the
// system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer.  Every array lives on the heap at exactly its advertised
// length, so a read of y[lo + 1] at lo = n - 1 is a sanitizer report.
//
// First it holds the header's pieces to hand-worked literals (a line "FAIL ..." and exit status 1 where one is missed).  Then it prints
// one line per row, every number as the 16 hex digits of a double's bits (counts too):
//   rank   q n lo g                 vag::predict_rank
//   value  n y[n] lo g Q            vag::predict_value on a sorted column
//   column n x[n] q Q               a column quantile: predict_read, std::sort, predict_rank, predict_value
//   tile   S P T                    vag::predict_network_size and vag::predict_tile_columns
// The test forms the same numbers with sampling's numpy statement and compares the bits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../vegasafterglow_amd/csrc/vag_predict.h"

static int failures = 0;

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return b;
}

static void put(double x) { std::printf(" %016llx", (unsigned long long)bits(x)); }

static void expect_rank(double q, long long n, long long lo_want, double g_want) {
    long long lo = -1;
    const double g = vag::predict_rank(q, n, &lo);
    if (lo != lo_want || bits(g) != bits(g_want)) {
        std::printf("FAIL rank q=%.17g n=%lld: lo %lld g %.17g, expected %lld %.17g\n", q, n, lo, g, lo_want, g_want);
        ++failures;
    }
    std::printf("rank");
    put(q), put((double)n), put((double)lo), put(g);
    std::printf("\n");
}

static void expect_value(const std::vector<double>& y, long long lo, double g, double want, long long stride = 1) {
    const double Q = vag::predict_value(y.data(), lo, g, stride);  // (y.data(): a heap block of exactly y.size() doubles)
    if (bits(Q) != bits(want)) {
        std::printf("FAIL value lo=%lld g=%.17g: %.17g, expected %.17g\n", lo, g, Q, want);
        ++failures;
    }
    if (stride != 1) return;
    std::printf("value");
    put((double)y.size());
    for (double v : y) put(v);
    put((double)lo), put(g), put(Q);
    std::printf("\n");
}

static double column_quantile(const std::vector<double>& x, double q) {
    std::vector<double> y(x.size());
    for (size_t i = 0; i < x.size(); ++i) y[i] = vag::predict_read(x[i]);
    std::sort(y.begin(), y.end());
    long long lo;
    const double g = vag::predict_rank(q, (long long)y.size(), &lo);
    return vag::predict_value(y.data(), lo, g);
}

static void column_row(const std::vector<double>& x, double q) {
    std::printf("column");
    put((double)x.size());
    for (double v : x) put(v);
    put(q), put(column_quantile(x, q));
    std::printf("\n");
}

static void expect_column(const std::vector<double>& x, double q, double want) {
    const double Q = column_quantile(x, q);
    if (bits(Q) != bits(want)) {
        std::printf("FAIL column n=%zu q=%.17g: %.17g, expected %.17g\n", x.size(), q, Q, want);
        ++failures;
    }
    column_row(x, q);
}

int main() {
    // ---- the rank: h = q (n - 1) as one multiply, lo = floor(h), g = h - lo ----
    for (double q : {0.0, 1.0, 0.5, 0.16}) expect_rank(q, 1, 0, 0.0);  // n = 1: h = 0 whatever q
    expect_rank(0.0, 2, 0, 0.0);
    expect_rank(1.0, 2, 1, 0.0);
    expect_rank(0.5, 2, 0, 0.5);
    expect_rank(0.16, 2, 0, 0.16);
    expect_rank(0.0, 3, 0, 0.0);
    expect_rank(1.0, 3, 2, 0.0);
    expect_rank(0.5, 3, 1, 0.0);
    expect_rank(0.16, 3, 0, 0.32);   // (doubling is exact: 2 double(0.16) is double(0.32))
    expect_rank(0.75, 3, 1, 0.5);
    expect_rank(0.0, 101, 0, 0.0);
    expect_rank(1.0, 101, 100, 0.0);
    expect_rank(0.5, 101, 50, 0.0);
    expect_rank(0.16, 101, 16, 0.0);   // double(0.16) 100 = 16 + 3.3e-16 rounds to 16: an order statistic, by the one multiply
    expect_rank(0.025, 101, 2, 0.5);   // double(0.025) 100 = 2.5 + 1.4e-16 rounds to 2.5
    expect_rank(0.975, 101, 97, 0.5);  // double(0.975) 100 = 97.5 - 2.2e-15 rounds to 97.5
    expect_rank(0.3, 11, 3, 0.0);      // double(0.3) 10 = 3 - 1.1e-16 rounds to 3: lo = 3, not 2 with g just below 1
    expect_rank(0.625, 4097, 2560, 0.0);
    expect_rank(0.0001220703125, 4096, 0, 0.4998779296875);  // 2^-13 4095 = 0.4998779296875 exactly
    // ---- the value: y[lo] when g == 0 (y[lo + 1] not read), else fma(g, y[lo + 1] - y[lo], y[lo]) ----
    expect_value({1.0, 2.0, 4.0}, 0, 0.5, 1.5);
    expect_value({1.0, 2.0, 4.0}, 1, 0.25, 2.5);
    expect_value({1.0, 2.0, 4.0}, 2, 0.0, 4.0);  // lo = n - 1: y[3] does not exist
    expect_value({7.0}, 0, 0.0, 7.0);            // n = 1
    expect_value({1.0, 9.0, 2.0, 9.0, 4.0}, 1, 0.25, 2.5, 2);  // stride 2: the column {1, 2, 4}, its last element the block's last
    expect_value({1.0, 9.0, 2.0, 9.0, 4.0}, 2, 0.0, 4.0, 2);
    // one rounding: double(1/3) 3 = 1 - 2^-54 exactly, which a rounded product takes to 1 (and the sum to 0)
    expect_value({-1.0, 2.0}, 0, 1.0 / 3.0, -0x1p-54);
    expect_value({1.0, 1.0 + 0x1p-52}, 0, 0.5, 1.0);           // 1 + 2^-53: the tie goes to the even neighbour
    expect_value({-0x1p-1074, 0x1p-1074}, 0, 0.5, 0.0);        // subnormal neighbours: -2^-1074 + 2^-1074 = +0
    expect_value({1e-300, 1e300}, 0, 0.5, 5e299);              // 0.5 (1e300 - 1e-300) + 1e-300 rounds to 0.5 1e300
    // ---- a column through std::sort ----
    expect_column({5.0, 1.0, 4.0, 2.0, 3.0}, 0.5, 3.0);
    expect_column({5.0, 1.0, 4.0, 2.0, 3.0}, 0.25, 2.0);
    expect_column({5.0, 1.0, 4.0, 2.0, 3.0}, 0.125, 1.5);
    expect_column({5.0, 1.0, 4.0, 2.0, 3.0}, 0.875, 4.5);
    expect_column({5.0, 1.0, 4.0, 2.0, 3.0}, 0.0, 1.0);
    expect_column({5.0, 1.0, 4.0, 2.0, 3.0}, 1.0, 5.0);
    expect_column({2.0, 2.0, 2.0, 2.0}, 0.3, 2.0);
    expect_column({0.0, -0.0, 0.0}, 0.5, 0.0);   // a zero of either sign is +0
    expect_column({-0.0}, 1.0, 0.0);
    expect_column({3.0, -0.0, -2.0}, 0.5, 0.0);
    if (bits(vag::predict_read(-0.0)) != 0 || bits(vag::predict_read(-3.5)) != bits(-3.5)) {
        std::printf("FAIL predict_read\n");
        ++failures;
    }
    // columns of a small generator, for the numpy statement: lognormal-like spreads, ties, subnormals, 1e-300 .. 1e300
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto next = [&state]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(state >> 11) * 0x1p-53;  // [0, 1)
    };
    const double qs[] = {0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0, 0.3, 0.999};
    for (int n : {1, 2, 3, 7, 64, 101}) {
        std::vector<double> wide(n), ties(n), tiny(n), range(n);
        for (int i = 0; i < n; ++i) {
            wide[i] = std::exp(6.0 * next() - 3.0) * (next() < 0.3 ? -1.0 : 1.0);
            ties[i] = (double)(int)(3.0 * next());
            tiny[i] = 0x1p-1074 * (double)(int)(40.0 * next());
            range[i] = std::pow(10.0, 600.0 * next() - 300.0);
        }
        for (double q : qs) column_row(wide, q), column_row(ties, q), column_row(tiny, q), column_row(range, q);
    }
    // ---- the network and the tile ----
    const int want_tile[][3] = {{1, 1, 16},      {2, 2, 16},       {3, 4, 16},       {63, 64, 16},     {64, 64, 16},   {65, 128, 16},
                                {255, 256, 16},  {256, 256, 16},   {257, 512, 16},   {1024, 1024, 16}, {1025, 2048, 8}, {2048, 2048, 8},
                                {2049, 4096, 4}, {4096, 4096, 4}};
    for (const auto& w : want_tile) {
        const int P = vag::predict_network_size(w[0]), T = vag::predict_tile_columns(w[0]);
        if (P != w[1] || T != w[2] || 8 * P * T > VAG_PREDICT_LDS_BYTES) {
            std::printf("FAIL tile S=%d: P %d T %d, expected %d %d\n", w[0], P, T, w[1], w[2]);
            ++failures;
        }
        std::printf("tile");
        put((double)w[0]), put((double)P), put((double)T);
        std::printf("\n");
    }
    if (VAG_PREDICT_MAX_DRAWS != 4096 || VAG_PREDICT_MAX_Q != 16 || VAG_PREDICT_MAX_VALUES != (1ll << 27)) {
        std::printf("FAIL limits\n");
        ++failures;
    }
    return failures ? 1 : 0;
}
