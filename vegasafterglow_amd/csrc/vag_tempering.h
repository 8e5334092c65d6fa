// vag_tempering.h -- parallel tempering around the stretch move (INTEGRATION.md "Parallel tempering"): a ladder of T inverse
// temperatures, temperature t sampling ln p_t = beta_t ln L + ln prior with an ensemble of its own, and exchanges between neighbouring
// temperatures.  The two margins are plain inline functions for host and device, as in vag_philox.h: the kernels below and a host
// program compiled with the system C++ compiler (tests/tempering_check.cpp) include the same text.  The kernels follow vag_sampler.h:
// one lane per item, 256-lane groups, plain vector loads and stores, no LDS, no atomics; the ladder travels by value as a kernel
// argument.  The draws are the stretch move's with the replica's index r = t n_walkers + w in the whole ladder as the counter's first
// word; stream 2 is the exchange.
#pragma once
#include "vag_philox.h"

#define VAG_TEMPER_MAX_RUNGS 64  // (VAG_TEMPER_MAX of the public header)

namespace vag {

struct TemperLadder {  // the inverse temperatures, by value in the kernel arguments; filled by tempered_spec_check (vag_sampler_plan.h)
    double beta[VAG_TEMPER_MAX_RUNGS];
};

// ln of the acceptance ratio of a move within temperature beta, without the (ndim - 1) log z of the stretch: one fma
VAG_PHILOX_HD inline double tempered_log_ratio(double beta, double lnl_new, double lnl_old, double lnprior_new, double lnprior_old) {
    return std::fma(beta, lnl_new - lnl_old, lnprior_new - lnprior_old);
}

// ln of the acceptance ratio of the exchange between beta_lo's state (ln L = lnl_lo) and beta_hi's (lnl_hi): the priors cancel
VAG_PHILOX_HD inline double swap_log_ratio(double beta_lo, double beta_hi, double lnl_lo, double lnl_hi) {
    return (beta_lo - beta_hi) * (lnl_hi - lnl_lo);
}

}  // namespace vag

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "vag_sampler.h"

namespace vag {

// prop[t][i][d] = fma(z, pos[t][w][d] - pos[t][partner][d], pos[t][partner][d]) for walker w = which * half + i of temperature t:
// every temperature's active half against its own complementary half.  One lane per (t, i).
__global__ void __launch_bounds__(STRETCH_LANES)
vag_tempered_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int which, int half, int ndim,
                            int n_temps, const double* __restrict__ pos /* [T][2 half][ndim] */,
                            double* __restrict__ prop /* [T][half][ndim] */) {
    const int item = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (item >= n_temps * half) return;
    const int t = item / half, i = item - t * half;
    stretch_proposal(seed_lo, seed_hi, a, step, t * 2 * half + which * half + i, which, half, i, ndim, pos + (size_t)t * 2 * half * ndim,
                     prop + (size_t)item * ndim);
}

// The decision of walker w = which * half + i of temperature t: reject a proposal whose ln L or ln prior is not finite (at every
// temperature, beta = 0 included), otherwise accept iff log(u_a) < (ndim - 1) log z + tempered_log_ratio(beta_t, ...), u_a from
// stream 1 and z again from stream 0.  An accepted walker takes the proposal, its ln L and its ln prior, and counts one.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_tempered_accept_kernel(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int which, int half, int ndim,
                           int n_temps, TemperLadder ladder, const double* __restrict__ prop /* [T][half][ndim] */,
                           const double* __restrict__ lnl_new /* [T][half] */, const double* __restrict__ lnprior_new /* [T][half] */,
                           double* __restrict__ pos /* [T][2 half][ndim] */, double* __restrict__ lnl /* [T][2 half] */,
                           double* __restrict__ lnprior /* [T][2 half] */, long long* __restrict__ accepted /* [T][2 half] */) {
    const int item = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (item >= n_temps * half) return;
    const int t = item / half, i = item - t * half;
    const int r = t * 2 * half + which * half + i;  // the replica's index in the whole ladder
    const StretchDraw dr = stretch_draw(seed_lo, seed_hi, step, r, half, a);
    const double u_a = stream_uniform(seed_lo, seed_hi, step, r, STREAM_ACCEPT);
    const double l_new = lnl_new[item], p_new = lnprior_new[item];
    const double ratio = tempered_log_ratio(ladder.beta[t], l_new, lnl[r], p_new, lnprior[r]);
    const bool take = isfinite(l_new) && isfinite(p_new) && log(u_a) < (double)(ndim - 1) * log(dr.z) + ratio;  // (log(0) = -inf accepts)
    if (take) {
        take_proposal(pos + (size_t)r * ndim, prop + (size_t)item * ndim, ndim, lnl + r, l_new, accepted + r);
        lnprior[r] = p_new;
    }
}

// The exchanges of step `step`: the pairs (t, t + 1) with t + step even, walker w of t with walker w of t + 1; one lane per
// (pair, w).  With u_s from stream 2 at r = t n_walkers + w the pair exchanges iff log(u_s) < swap_log_ratio(beta_t, beta_t+1,
// lnl[t][w], lnl[t + 1][w]); an accepted pair swaps positions, ln L and ln prior, and swapped[t][w] counts one.  The pairs of a step
// are disjoint, so no lane touches another's walkers.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_tempered_swap_kernel(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int n_walkers, int ndim, int n_pairs,
                         TemperLadder ladder, double* __restrict__ pos /* [T][nw][ndim] */, double* __restrict__ lnl /* [T][nw] */,
                         double* __restrict__ lnprior /* [T][nw] */, long long* __restrict__ swapped /* [T - 1][nw] */) {
    const int item = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (item >= n_pairs * n_walkers) return;
    const int pair = item / n_walkers, w = item - pair * n_walkers;
    const int t = 2 * pair + (int)(step & 1ull);
    const int lo = t * n_walkers + w, hi = lo + n_walkers;
    const double u_s = stream_uniform(seed_lo, seed_hi, step, lo, STREAM_EXCHANGE);
    const double l_lo = lnl[lo], l_hi = lnl[hi];
    if (!(log(u_s) < swap_log_ratio(ladder.beta[t], ladder.beta[t + 1], l_lo, l_hi))) return;
    double* a_pos = pos + (size_t)lo * ndim;
    double* b_pos = pos + (size_t)hi * ndim;
    for (int d = 0; d < ndim; ++d) {
        const double x = a_pos[d];
        a_pos[d] = b_pos[d];
        b_pos[d] = x;
    }
    lnl[lo] = l_hi;
    lnl[hi] = l_lo;
    const double p_lo = lnprior[lo];
    lnprior[lo] = lnprior[hi];
    lnprior[hi] = p_lo;
    swapped[lo] += 1;
}

// Behind a likelihood call: ln L and ln prior of its walkers apart, from what the call leaves by evaluation slot m -- chi2[m] the
// chi^2 over all passes, valid[m], ln_prior[m] -- and the order it evaluated in.  -chi2 / 2 is exact, so lnl + lnprior is the call's
// own output to the bit wherever that is finite.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_fit_split_kernel(const double* __restrict__ chi2, const int* __restrict__ valid, const double* __restrict__ ln_prior, int nb,
                     const int* __restrict__ order /* evaluation slot -> walker, or null */, double* __restrict__ lnl /* [nb] */,
                     double* __restrict__ lnprior /* [nb] */) {
    const int m = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (m >= nb) return;
    const int walker = order ? order[m] : m;
    const double x = chi2[m];
    lnl[walker] = (valid[m] && isfinite(x)) ? -0.5 * x : -INFINITY;
    lnprior[walker] = ln_prior[m];
}

}  // namespace vag
#endif
