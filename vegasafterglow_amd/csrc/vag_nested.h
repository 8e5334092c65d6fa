// vag_nested.h -- nested sampling on the device (INTEGRATION.md "Nested sampling"): N live points, every iteration retires the K = N / 2
// of lowest ln L and replaces each by a clone of a survivor that then walks `walk` constrained differential-evolution steps against the
// survivors, which do not move during the iteration.  The rank comparison, the live count and the shrinkage of a dead point, the tick of
// a draw, the clone's index and the constrained decision with its margin are plain inline functions for host and device, as in
// vag_philox.h: the kernels below and a host program compiled with the system C++ compiler (tests/nested_check.cpp) include the same
// text.  The kernels follow vag_sampler.h: one lane per item, 256-lane groups, plain vector loads and stores, no atomics; the rank kernel
// alone reads through LDS.  The scale of a step is vag_moves.h's (de_gamma0, de_normal, de_quantise, de_gamma) and so are its partners
// (move_pair); every fused operation is an explicit fma(), so that a proposal reproduces on the host to the bit
// (sampling.nested_proposals).
//
// The draws: Philox4x32-10 under the key of the seed with counter (r, tick lo, tick hi, stream): r the rank of the retired point,
// 0 .. K - 1, whose slot the clone takes; tick = it (walk + 1) + m with m = 0 the clone draw and m = 1 .. walk the walk steps.  Streams:
// 0 the proposal (u1 of the normal from words 0, 1; the two survivors from words 2, 3) and 4 its second block (u2 of the normal from
// words 0, 1), 1 the acceptance -- all three as in the move mix -- and 5 the clone choice (its uniform from words 0, 1), read at m = 0.
#pragma once
#include "vag_moves.h"

#define VAG_NESTED_MAX_LIVE_POINTS 16384  // (VAG_NESTED_MAX_LIVE of the public header)

namespace vag {

constexpr uint32_t NESTED_STREAM_CLONE = 5u;

// live slot i ranks before slot j: (lnl_i, i) < (lnl_j, j) lexicographically, ties to the lower slot
VAG_PHILOX_HD inline bool nested_before(double lnl_i, int i, double lnl_j, int j) { return lnl_i < lnl_j || (lnl_i == lnl_j && i < j); }

// the live count when dead point j (flattened index over the whole run) leaves: N - (j mod K), K = N / 2
VAG_PHILOX_HD inline long long nested_live_count(unsigned long long j, int n_live) {
    return (long long)n_live - (long long)(j % (unsigned long long)(n_live / 2));
}

// the shrinkage term of a point that leaves n live ones: ln X drops by 1 / n (one IEEE division)
VAG_PHILOX_HD inline double nested_shrink(long long n) { return 1.0 / (double)n; }

// the tick of draw m of iteration `it`: m = 0 the clone draw, m = 1 .. walk the walk steps
VAG_PHILOX_HD inline unsigned long long nested_tick(unsigned long long it, int walk, int m) {
    return it * (unsigned long long)(walk + 1) + (unsigned long long)m;
}

// the survivor a clone copies, j0 = floor(u K) for u in [0, 1).  u K < K in floating point (u <= 1 - 2^-53 leaves the product more
// than half an ulp below K, or exactly on a double below it); the last line holds that without the argument, as a bound on memory.
VAG_PHILOX_HD inline int nested_clone_index(double u, int k) {
    const int j0 = (int)(u * (double)k);
    return j0 < k ? j0 : k - 1;
}

// The constrained decision: the margin of a proposal with (lnl_new, lnprior_new) from a point of ln prior lnprior_old under the
// constraint ln L > lstar, log_u the logarithm of the acceptance uniform.  -inf where ln L' or ln prior' is not finite or ln L' is
// not strictly above lstar, whatever the draw; otherwise (lnprior_new - lnprior_old) - log_u.  The proposal is taken iff the margin
// is > 0: the symmetric move on the prior restricted to L > L*.  (log(0) = -inf: margin +inf, taken.)
VAG_PHILOX_HD inline double nested_margin(double lnl_new, double lnprior_new, double lnprior_old, double lstar, double log_u) {
    if (!std::isfinite(lnl_new) || !std::isfinite(lnprior_new) || !(lnl_new > lstar)) return -INFINITY;
    return (lnprior_new - lnprior_old) - log_u;
}

}  // namespace vag

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "vag_sampler.h"

namespace vag {

// order[idx] as a live slot.  What the rank kernel wrote is a permutation of 0 .. N - 1; a caller's own array is held inside the live
// set all the same, as a bound on memory.
__device__ inline int nested_slot(const int* order, int idx, int n_live) {
    const int s = order[idx];
    return (unsigned)s < (unsigned)n_live ? s : 0;
}

// The counting rank: lane i counts the slots that rank before slot i (nested_before), reading ln L through LDS in tiles of the
// workgroup's size; order[rank] = i is the scatter of a permutation, so no two lanes write one element.  The lane of rank K - 1
// writes L* = its ln L.  ln L holds no NaN (every live point is finite).
__global__ void __launch_bounds__(STRETCH_LANES)
vag_nested_rank_kernel(int n_live, const double* __restrict__ lnl /* [N] */, int* __restrict__ order /* [N] */,
                       double* __restrict__ lstar /* [1] */) {
    __shared__ double tile[STRETCH_LANES];
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    const double mine = i < n_live ? lnl[i] : 0.0;
    int rank = 0;
    for (int base = 0; base < n_live; base += STRETCH_LANES) {
        const int j = base + (int)threadIdx.x;
        tile[threadIdx.x] = j < n_live ? lnl[j] : 0.0;
        __syncthreads();
        const int count = n_live - base < STRETCH_LANES ? n_live - base : STRETCH_LANES;
        if (i < n_live)
            for (int t = 0; t < count; ++t) rank += nested_before(tile[t], base + t, mine, i) ? 1 : 0;
        __syncthreads();
    }
    if (i >= n_live) return;
    order[rank] = i;
    if (rank == n_live / 2 - 1) lstar[0] = mine;
}

// Lane r retires the point of rank r < K: it stores the point's row of the dead record, then overwrites its slot order[r] with a copy
// (theta, ln L, ln prior) of survivor order[K + j0], j0 = nested_clone_index of the uniform of stream 5 at tick (it, 0).  The same
// lane does both, in that order; survivors are only read.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_nested_retire_kernel(uint32_t seed_lo, uint32_t seed_hi, unsigned long long tick, int n_live, int ndim,
                         const int* __restrict__ order /* [N] */, double* __restrict__ live /* [N][ndim] */,
                         double* __restrict__ lnl /* [N] */, double* __restrict__ lnprior /* [N] */,
                         double* __restrict__ dead_theta /* [K][ndim] */, double* __restrict__ dead_lnl /* [K] */,
                         double* __restrict__ dead_lnprior /* [K] */) {
    const int r = blockIdx.x * STRETCH_LANES + threadIdx.x;
    const int k = n_live / 2;
    if (r >= k) return;
    const int slot = nested_slot(order, r, n_live);
    const int from = nested_slot(order, k + nested_clone_index(stream_uniform(seed_lo, seed_hi, tick, r, NESTED_STREAM_CLONE), k), n_live);
    double* mine = live + (size_t)slot * ndim;
    const double* src = live + (size_t)from * ndim;
    double* row = dead_theta + (size_t)r * ndim;
    for (int d = 0; d < ndim; ++d) row[d] = mine[d];
    dead_lnl[r] = lnl[slot];
    dead_lnprior[r] = lnprior[slot];
    for (int d = 0; d < ndim; ++d) mine[d] = src[d];
    lnl[slot] = lnl[from];
    lnprior[slot] = lnprior[from];
}

// The walk step of clone r (slot order[r]) at `tick`: survivors s1 != s2 = order[K + a], order[K + b] with (a, b) = move_pair of
// words 2, 3 of stream 0 over the K survivors, gamma as in vag_de_propose_kernel; prop[r][d] = fma(gamma, live[s1][d] - live[s2][d],
// live[slot][d]).  K >= 2.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_nested_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double gamma0, double sigma, unsigned long long tick, int n_live, int ndim,
                          const int* __restrict__ order /* [N] */, const double* __restrict__ live /* [N][ndim] */,
                          double* __restrict__ prop /* [K][ndim] */) {
    const int r = blockIdx.x * STRETCH_LANES + threadIdx.x;
    const int k = n_live / 2;
    if (r >= k) return;
    const MoveWords m = move_words(seed_lo, seed_hi, tick, r);
    const MovePair pr = move_pair(m.x[2], m.x[3], k);
    const double gamma = de_gamma(gamma0, sigma, de_quantise(de_normal(u53(m.x[0], m.x[1]), u53(m.v[0], m.v[1]))));
    const double* mine = live + (size_t)nested_slot(order, r, n_live) * ndim;
    const double* ca = live + (size_t)nested_slot(order, k + pr.a, n_live) * ndim;
    const double* cb = live + (size_t)nested_slot(order, k + pr.b, n_live) * ndim;
    double* out = prop + (size_t)r * ndim;
    for (int d = 0; d < ndim; ++d) out[d] = fma(gamma, ca[d] - cb[d], mine[d]);
}

// The decision of clone r at `tick`: taken iff nested_margin(...) > 0 with u_a from stream 1.  A taken proposal replaces the clone
// (theta, ln L, ln prior) and accepted[r] counts one.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_nested_accept_kernel(uint32_t seed_lo, uint32_t seed_hi, unsigned long long tick, int n_live, int ndim,
                         const int* __restrict__ order /* [N] */, const double* __restrict__ lstar /* [1] */,
                         const double* __restrict__ prop /* [K][ndim] */, const double* __restrict__ lnl_new /* [K] */,
                         const double* __restrict__ lnprior_new /* [K] */, double* __restrict__ live /* [N][ndim] */,
                         double* __restrict__ lnl /* [N] */, double* __restrict__ lnprior /* [N] */,
                         long long* __restrict__ accepted /* [K] */) {
    const int r = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (r >= n_live / 2) return;
    const int slot = nested_slot(order, r, n_live);
    const double u_a = stream_uniform(seed_lo, seed_hi, tick, r, STREAM_ACCEPT);
    const double l_new = lnl_new[r], p_new = lnprior_new[r];
    if (!(nested_margin(l_new, p_new, lnprior[slot], lstar[0], log(u_a)) > 0.0)) return;
    take_proposal(live + (size_t)slot * ndim, prop + (size_t)r * ndim, ndim, lnl + slot, l_new, accepted + r);
    lnprior[slot] = p_new;
}

}  // namespace vag
#endif
