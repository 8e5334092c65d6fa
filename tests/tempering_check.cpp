// Stand-alone host check of the two margins of csrc/vag_tempering.h (parallel tempering), built by tests/test_tempering_host.py with
// the system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer.  For a fixed table of inputs it prints one line per row,
// "ratio <5 inputs> <result>" for vag::tempered_log_ratio and "swap <4 inputs> <result>" for vag::swap_log_ratio, every number as
// the 16 hex digits of its bits; the test forms the same numbers with sampling's numpy functions and compares the bits.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../vegasafterglow_amd/csrc/vag_tempering.h"

static void put(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    std::printf(" %016llx", (unsigned long long)b);
}

int main() {
    // beta, lnl_new, lnl_old, lnprior_new, lnprior_old
    const double ratio[][5] = {
        {0.0, -12.5, -3.25, -4.969813299576001, -4.969813299576001},  // beta = 0: the prior rung, equal priors
        {0.0, -1e30, 7.0, -1.5, -2.75},                               // beta = 0 against a huge difference
        {1.0, -42.68221159873594, -44.65546933420461, 0.0, 0.0},      // beta = 1, no prior: the plain stretch move's difference
        {1.0, -3.0, -3.0, -2.0, -2.5},                                // equal ln L
        {0.3, 1e300, -1e300, -1.0, -2.0},                             // huge differences
        {1e-3, -1e30, 1e25, 3.0, -3.0},
        {0.02619708281795851, -42.68221159873594, -44.65546933420461, -3.660178848656387, -3.901722806019508},  // fma != unfused
        {0.7249066297643184, -49.28611564742037, -46.389133148891275, -2.441020866195495, -4.655068199670413},  // fma != unfused
        {0.46415888336127786, -2.6060174, -5.09316776, -4.969813299576001, -4.969813299576001},
    };
    for (const auto& r : ratio) {
        std::printf("ratio");
        for (double x : r) put(x);
        put(vag::tempered_log_ratio(r[0], r[1], r[2], r[3], r[4]));
        std::printf("\n");
    }
    // beta_lo, beta_hi, lnl_lo, lnl_hi
    const double swap[][4] = {
        {1.0, 0.0, -3.5, -48.45158271},                  // against the prior rung
        {1.0, 0.46415888336127786, -1.45158271, -2.6060174},
        {0.01, 0.0, -39.9151043, -39.9151043},           // equal ln L: always exchanged
        {0.1, 0.04641588833612779, -1e300, 1e300},       // huge differences
        {1.0, 0.25118864315095796, 1e30, -1e30},
        {0.02619708281795851, 0.001, -44.65546933420461, -42.68221159873594},
    };
    for (const auto& r : swap) {
        std::printf("swap");
        for (double x : r) put(x);
        put(vag::swap_log_ratio(r[0], r[1], r[2], r[3]));
        std::printf("\n");
    }
    return 0;
}
