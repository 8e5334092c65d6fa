// vag_robust.h -- the row term of an outlier group (INTEGRATION.md "Outlier groups"): the two-component mixture of Hogg, Bovy & Lang
// (2010, section 3) on a detection row of a robust noise group.  A plain inline function for host and device, as in
// vag_chain_stats.h: vag_fit_back_robust_kernel and a host program compiled with the system C++ compiler (tests/robust_check.cpp)
// include the same text.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define VAG_ROBUST_HD __host__ __device__
#else
#define VAG_ROBUST_HD
#endif

namespace vag {

// l = ln((1 - P) N(r; 0, v_in) + P N(r; mu, v_out)) + ln(sqrt(2 pi) sigma) of one row, with r the row's residual in ln F, sig2 its
// ln_err^2, s2 = s_g^2, b2 = b_g^2, ln_good = log1p(-P_g) and ln_bad = ln P_g (formed once per group by the caller):
//   v_in = sig2 + s2,  v_out = v_in + b2,
//   g = ln_good - r^2 / (2 v_in)         - log1p(s2 / sig2) / 2
//   o = ln_bad  - (r - mu)^2 / (2 v_out) - log1p((s2 + b2) / sig2) / 2
//   l = max(g, o) + log1p(exp(-|g - o|)).
// P = 0: ln_bad = -inf, o = -inf and l = g to the bit (exp(-inf) = 0, log1p(0) = 0).  A NaN r gives NaN (the selects keep it: g and o
// are both NaN then); so does r = +-inf (g = o = -inf, g - o = NaN).  Every term of g and of o is <= 0, so neither sum cancels.
VAG_ROBUST_HD inline double robust_row_lnl(double r, double sig2, double s2, double b2, double mu, double ln_good, double ln_bad) {
    const double v_in = sig2 + s2, v_out = v_in + b2;
    const double d = r - mu;
    const double g = ln_good - 0.5 * (r * r) / v_in - 0.5 * log1p(s2 / sig2);
    const double o = ln_bad - 0.5 * (d * d) / v_out - 0.5 * log1p((s2 + b2) / sig2);
    const double hi = g > o ? g : o;
    return hi + log1p(exp(-fabs(g - o)));
}

}  // namespace vag
