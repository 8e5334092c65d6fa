// vag_log_ndtr.h -- ln Phi(z), the log of the standard normal CDF, in FP64: the upper-limit term of the walker likelihood
// (vag_loglike_lim_batch; -2 w ln Phi((L - M) / sigma) per limit row, formed by the back kernels of vag_fit_kernels.h).
#pragma once
#include "vag_device.h"

namespace vag {

// z < 0:  Phi(z) = 1/2 erfc(-z / sqrt 2) = 1/2 erfcx(-z / sqrt 2) exp(-z^2 / 2), so ln Phi = ln(1/2 erfcx(-z / sqrt 2)) - z^2 / 2:
//         erfcx does not underflow (it falls like 1 / (x sqrt pi)), both terms are negative (no cancellation), and the result is finite
//         down to the z whose z^2 / 2 overflows, where a plain log(0.5 * erfc(..)) is -inf from z = -38.5.
// z >= 0: ln Phi = log1p(-1/2 erfc(z / sqrt 2)), which keeps the relative accuracy of erfc as Phi -> 1 (the result goes to -0).
// NaN stays NaN (it takes the second branch); -inf gives -inf, +inf gives -0.  Error: the library's erfcx / erfc / log / log1p (a few
// ulp each) and, for z > 0, the rounding of z / sqrt 2 amplified by 2 x^2 = z^2 in erfc: about z^2 x 1.6e-16 relative
// (tests/test_limits.py measures it against 40 digits).
VAG_DEV double log_ndtr(double z) {
    const double x = z * 0.70710678118654752440;
    if (z < 0) return log(0.5 * erfcx(-x)) - 0.5 * (z * z);
    return log1p(-0.5 * erfc(x));
}

}  // namespace vag
