// vag_poisson.h -- the Poisson deviance D(N, mu) = mu - N - N ln(mu / N) >= 0 in FP64: the counts term of the walker likelihood
// (vag_loglike_counts_batch; 2 w D per row, formed by vag_fit_back_counts_kernel of vag_fit_kernels.h), and the walker-independent
// constant S(N) = N ln N - N - ln N! the host adds once per spec, so that ln P(N | mu) = -D + S.
#pragma once
#include <cmath>

#include "vag_device.h"

namespace vag {

// N = 0: D = mu (the limit of the form below).  N > 0, with d = mu - N and x = d / N, D = N (x - log1p(x)):
//   |d| <= N / 2: d is exact (Sterbenz: mu lies in [N / 2, 2 N]).  x - log1p(x) loses everything near x = 0 when formed directly; with
//         r = x / (2 + x), log1p(x) = 2 atanh(r) = 2 (r + r^3 / 3 + r^5 / 5 + ..) and x = 2 r / (1 - r) give
//         x - log1p(x) = r (x - 2 r^2 sum_k r^(2k) / (2k + 3)),
//         where 2 r^2 sum <= 0.16 |x| (no cancellation).  |r| <= 1/3 here, so 18 terms leave (1/9)^18 / 39 < 2e-19 of the sum.
//   else: x itself is ill-conditioned near -1, so D = d - N ln(mu / N): the two terms have opposite signs and D is at least
//         0.09 N, a tenth of the larger one.  mu = 0 gives +inf (log(0) = -inf), the walker then scores -inf.
// NaN in either argument stays NaN.  Error: a few 1e-16 relative in the series branch, up to ~1e-15 just outside the switch
// (tests/test_counts.py measures it against 40 digits).
VAG_DEV double poisson_deviance(double N, double mu) {
    if (N != N) return N;
    if (!(N > 0)) return mu;
    const double d = mu - N;
    if (fabs(d) <= 0.5 * N) {
        const double x = d / N, r = x / (2.0 + x), r2 = r * r;
        double s = 1.0 / 37.0;
#pragma unroll
        for (int k = 16; k >= 0; --k) s = fma(s, r2, 1.0 / (double)(2 * k + 3));
        return N * (r * (x - 2.0 * r2 * s));
    }
    return fma(-N, log(mu / N), d);
}

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
