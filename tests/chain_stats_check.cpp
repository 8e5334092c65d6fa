// Stand-alone host check of csrc/vag_chain_stats.h (chain autocorrelation), built by tests/test_chain_stats_host.py with the system
// C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer.  For fixed tables it prints one line per row, every number as the 16
// hex digits of a double's bits (counts too):
//   mean   n x[n] m                                          vag::chain_mean of one series
//   lag    n l m x[n] c                                      vag::chain_lag_sum at lag l about the mean m
//   window c L rho[L + 1] tau M                              vag::sokal_window
//   chain  n W D c L x[n W D] tau[D] window[D] rho[(L + 1) D]   the whole estimate of a chain [n][W][D] through the header's pieces:
//                                                            means, lag sums, pooling in ascending w, vag::chain_tau (strided)
// The test forms the same numbers with sampling's numpy functions and compares the bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../vegasafterglow_amd/csrc/vag_chain_stats.h"

static void put(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    std::printf(" %016llx", (unsigned long long)b);
}

static void mean_row(const std::vector<double>& x) {
    std::printf("mean");
    put((double)x.size());
    for (double v : x) put(v);
    put(vag::chain_mean(x.data(), (long long)x.size(), 1));
    std::printf("\n");
}

static void lag_row(const std::vector<double>& x, int l) {
    const double m = vag::chain_mean(x.data(), (long long)x.size(), 1);
    std::printf("lag");
    put((double)x.size());
    put((double)l);
    put(m);
    for (double v : x) put(v);
    put(vag::chain_lag_sum(x.data(), (long long)x.size(), 1, m, l));
    std::printf("\n");
}

static void window_row(double c, const std::vector<double>& rho) {
    const int L = (int)rho.size() - 1;
    double tau = -7.0;
    const int M = vag::sokal_window(rho.data(), L, c, &tau);
    std::printf("window");
    put(c);
    put((double)L);
    for (double v : rho) put(v);
    put(tau);
    put((double)M);
    std::printf("\n");
}

static void chain_row(int n, int W, int D, double c, int L, const std::vector<double>& x) {
    const int S = W * D;
    std::vector<double> lag((size_t)(L + 1) * S), pooled((size_t)(L + 1) * D), rho((size_t)(L + 1) * D), tau(D);
    std::vector<int> window(D);
    for (int s = 0; s < S; ++s) {
        const double m = vag::chain_mean(x.data() + s, n, S);
        for (int l = 0; l <= L; ++l) lag[(size_t)l * S + s] = vag::chain_lag_sum(x.data() + s, n, S, m, l);
    }
    for (int l = 0; l <= L; ++l)
        for (int d = 0; d < D; ++d) {
            double sum = 0.0;
            for (int w = 0; w < W; ++w) sum += lag[(size_t)l * S + w * D + d];
            pooled[(size_t)l * D + d] = sum;
        }
    for (int d = 0; d < D; ++d) window[d] = vag::chain_tau(pooled.data() + d, L, c, rho.data() + d, &tau[d], D);
    std::printf("chain");
    put(n), put(W), put(D), put(c), put(L);
    for (double v : x) put(v);
    for (double v : tau) put(v);
    for (int v : window) put((double)v);
    for (double v : rho) put(v);
    std::printf("\n");
}

int main() {
    mean_row({1.0, 3.0});                                        // n = 2
    mean_row({52.4});                                            // n = 1: the series itself
    mean_row({52.4, 52.4, 52.4, 52.4, 52.4, 52.4, 52.4});        // a constant that is no dyadic number: the second pass returns it
    mean_row({52.31, 52.47, 52.52, 52.38, 52.4, 52.29, 52.61, 52.44, 52.5});
    mean_row({500.000001, 500.0000004, 499.9999991, 500.0000013, 499.9999997, 500.0000002});  // what the second pass is for
    mean_row({0.07, 0.081, 0.064, 0.0725, 0.069, 0.077, 0.0701});
    mean_row({-1e300, 1e300, 3.0, 4.0});
    mean_row({1e16, 1.0, -1e16, 1.0, 1.0});                      // the first pass loses the ones, the second recovers part
    const std::vector<double> series = {52.31, 52.47, 52.52, 52.38, 52.4, 52.29, 52.61, 52.44, 52.5, 52.36, 52.41, 52.55};
    for (int l : {0, 1, 5, 11}) lag_row(series, l);
    lag_row({1.0, 3.0}, 1);
    window_row(5.0, {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});  // on its threshold: tau = 1, M = 5 = c tau
    window_row(1.0, {1.0, 0.0});                                 // on its threshold at M = 1 = L
    window_row(5.0, {1.0, 0.9, 0.9, 0.9});                       // no window: tau(L) = 6.4
    window_row(5.0, {1.0, -0.5});                                // tau(1) = 0: M = 1
    window_row(5.0, {1.0});                                      // L = 0: tau = 1, 0 >= 5 fails
    window_row(0.25, {1.0, 0.7, 0.49, 0.343, 0.2401, 0.16807, 0.117649, 0.0823543, 0.05764801, 0.040353607, 0.0282475249,
                      0.01977326743, 0.013841287201, 0.0096889010407, 0.00678223072849, 0.004747561509943});
    window_row(5.0, {1.0, 0.31, 0.12, -0.04, 0.07, 0.013, -0.021, 0.0033, 0.0101, -0.0046, 0.0007, 0.002});
    window_row(5.0, {1.0, 0.8, 0.64, 0.512, 0.4096, 0.32768, 0.262144, 0.2097152, 0.16777216, 0.134217728});  // none within L
    const double nan = std::nan("");
    window_row(5.0, {nan, nan, nan});                            // what C(0) = 0 leaves: -1 and a tau that is not a number
    window_row(5.0, {1.0, 0.2, nan, 0.1});
    // whole chains; dyadic values and sums that stay exact, so the lag sums have one value however they are formed
    chain_row(2, 1, 1, 5.0, 1, {1.0, 3.0});                      // n = 2
    chain_row(4, 2, 2, 5.0, 3,                                   // parameter 0 never moves in either walker: C(0) = 0
              {2.5, 1.0, -1.0, 4.0, 2.5, 3.0, -1.0, 0.0, 2.5, -2.0, -1.0, 2.0, 2.5, 2.0, -1.0, 6.0});
    chain_row(4, 2, 1, 5.0, 2, {2.5, 1.0, 2.5, 3.0, 2.5, -2.0, 2.5, 2.0});  // one walker never moves: pooling keeps the estimate
    chain_row(8, 2, 2, 5.0, 7, {3.0,  1.0, -2.0, 5.0,  4.0, 2.0, -1.0, 3.0,  2.0, 0.0, -3.0, 6.0,  5.0,  3.0, 0.0,  2.0,
                                1.0, -1.0, -2.0, 4.0,  6.0, 2.0, 1.0,  7.0,  3.0, 1.0, -1.0, 1.0,  0.0, 0.0, 0.0,  4.0});
    chain_row(8, 1, 3, 1.0, 4, {1.0, 8.0, 0.5,  2.0, 6.0, 0.25,  1.0, 9.0, 0.5,  2.0, 7.0, 0.25,
                                1.0, 8.0, 0.5,  2.0, 5.0, 0.25,  1.0, 9.0, 0.5,  2.0, 4.0, 0.25});
    return 0;
}
