// vag_fold.h -- the expected counts of one channel of a count spectrum folded through the instrument response, in FP64: the inner
// sum of the fold term of the walker likelihood (vag_loglike_fold_batch; 2 w D(N, mu) per row and channel, formed by
// vag_fit_back_fold_kernel of vag_fit_kernels.h).
#pragma once
#include <cmath>

#include "vag_device.h"

namespace vag {

constexpr int FOLD_MAX_BINS = 64;       // VAG_FOLD_MAX_BINS
constexpr int FOLD_MAX_CHANNELS = 256;  // VAG_FOLD_MAX_CHANNELS

// mu = B + sum_j A[j][c] G[j]: A_c = &A[0][c] with the row stride C of the [J][C] layout, G the row's J folded bin fluences
// (erg cm^-2 Hz^-1).  The summation order is part of the definition: the sum starts at 0, runs over j = 0 .. J-1 ascending with one
// fma per term, and B is added last, so a channel's value does not depend on which lane forms it.  Every term is >= 0 for a model
// that is: no cancellation, the sum is within J 2^-53 of the exact one.  A NaN or negative-zero G stays what the arithmetic makes of it.
VAG_DEV double fold_mu(double B, const double* A_c, int C, const double* G, int J) {
    double acc = 0;
    for (int j = 0; j < J; ++j) acc = fma(A_c[(size_t)j * C], G[j], acc);
    return B + acc;
}

}  // namespace vag
