// vag_poisson.h -- the Poisson deviance D(N, mu) = mu - N - N ln(mu / N) >= 0 in FP64: the counts term of the walker likelihood
// (vag_loglike_counts_batch; 2 w D per row, formed by vag_fit_back_counts_kernel of vag_fit_kernels.h), and the walker-independent
// constant S(N) = N ln N - N - ln N! the host adds once per spec, so that ln P(N | mu) = -D + S.
#pragma once
#include <cmath>

#include "vag_device.h"
#include "vag_poisson_const.h"  // S(N), the host half

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

}  // namespace vag
