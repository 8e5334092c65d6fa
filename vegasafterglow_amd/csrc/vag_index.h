// vag_index.h -- the log-slope S = sum_{k >= 1} c_k ln(F_k / F_0) of a spectral-index row in FP64: the spectral-index term of the
// walker likelihood (vag_loglike_index_batch; w ((S - A_V ext_slope - s) / sigma)^2 per row, formed by vag_fit_back_index_kernel of
// vag_fit_kernels.h).
#pragma once
#include <cmath>

#include "vag_device.h"

namespace vag {

constexpr int INDEX_MAX_NODES = 8;  // VAG_INDEX_MAX_NODES

// F_k = F[k * stride], k = 0 .. K-1, the model's flux density at the group's K frequencies; c_0 is never read.  The pivot form is
// the definition: every log is taken of a ratio to F_0, a correctly rounded quotient of order (nu_k / nu_0)^slope, so a log's error is
// relative to |ln(F_k / F_0)| and the sum stays within a few 2^-52 sum_k |c_k| (1 + |ln(F_k / F_0)|).  A plain sum_k c_k ln F_k would
// carry the error of ln F_k ~ 60 .. 600 times larger than the term (fluxes are 1e-26 erg cm^-2 s^-1 Hz^-1 and below), and, sum_k c_k
// being zero only to rounding, it would depend on the flux unit.  The quotient of two powers of two times F is that of F, so the value
// does not change when a row's fluxes are scaled by a power of two (no subnormals).  Summed in k order, one fma per term.
// The slope is undefined unless every F_k is finite and > 0: NaN then (the walker scores -inf, as the centroid and polarization
// groups treat F <= 0; not the 1e-300 clamp of the point rows, which would turn a vanished flux into a slope of the clamp's making).
VAG_DEV double log_slope(const double* F, int stride, const double* coef, int K) {
    const double f0 = F[0];
    bool ok = f0 > 0 && f0 < INFINITY;  // (false for NaN)
    double s = 0;
    for (int k = 1; k < K; ++k) {
        const double fk = F[(size_t)k * stride];
        ok = ok && fk > 0 && fk < INFINITY;
        s = fma(coef[k], log(fk / f0), s);
    }
    return ok ? s : NAN;
}

}  // namespace vag
