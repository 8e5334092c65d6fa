// vag_poisson_const.h -- the walker-independent constant of the Poisson terms, on the host: plain C++, no device header, so that the
// scans of vag_fit_request.h and a host-only program reach it (vag_poisson.h includes it next to the device-side deviance).
#pragma once
#include <cmath>

namespace vag {

// S(N) = N ln N - N - ln N! for an integer N >= 0 (0 for N = 0), on the host.  N >= 16: Stirling's remainder series
//   ln N! = N ln N - N + ln(2 pi N) / 2 + 1/(12 N) - 1/(360 N^3) + 1/(1260 N^5) - 1/(1680 N^7) + 1/(1188 N^9) - 691/(360360 N^11) + ..,
// whose first omitted term is below 2e-18 there: no difference of large numbers is ever formed (N ln N - N - lgamma(N + 1) loses
// ~1e-6 absolute at N = 1e9).  N < 16: the three-term difference in long double, which is exact enough for such small terms.
inline double poisson_const(double N) {
    if (!(N > 0)) return 0.0;
    if (N < 16) {
        const long double n = (long double)N;
        return (double)(n * logl(n) - n - lgammal(n + 1.0L));
    }
    const double i = 1.0 / N, i2 = i * i;
    const double series = i * (1.0 / 12 + i2 * (-1.0 / 360 + i2 * (1.0 / 1260 + i2 * (-1.0 / 1680 + i2 * (1.0 / 1188 + i2 * (-691.0 / 360360))))));
    return -(0.5 * std::log(6.283185307179586476925 * N) + series);
}

}  // namespace vag
