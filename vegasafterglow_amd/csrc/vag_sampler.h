// vag_sampler.h -- the two kernels of the device ensemble sampler (INTEGRATION.md "the device sampler"): the Goodman & Weare stretch
// move in its parallel form with fixed halves, its draws a pure function of (seed, step, walker) through Philox4x32-10.  One lane per
// walker of the active half; the kernels are latency-sized (a half is a few hundred walkers): plain vector loads and stores, no LDS,
// no atomics.  The fused operations are explicit fma() calls and the division is an IEEE one, so that a proposal reproduces on the
// host to the bit (sampling.stretch_proposals).
#pragma once
#include <hip/hip_runtime.h>

#include "vag_philox.h"

namespace vag {

constexpr int STRETCH_LANES = 256;  // lanes per workgroup of both kernels: ceil(half / 256) groups

struct StretchDraw {  // what a walker draws for one half-step
    double z;         // the stretch factor
    int partner;      // index within the complementary half
};

// stream 0 of walker w at `step`: u_z from the first two words, the partner from the third
__device__ inline StretchDraw stretch_draw(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int w, int half, double a) {
    const uint32_t ctr[4] = {(uint32_t)w, (uint32_t)(step & 0xffffffffull), (uint32_t)(step >> 32), 0u};
    const uint32_t key[2] = {seed_lo, seed_hi};
    uint32_t x[4];
    philox4x32_10(ctr, key, x);
    return {stretch_z(a, u53(x[0], x[1])), stretch_partner(x[2], half)};
}

// prop[i][d] = fma(z, pos[w][d] - pos[partner][d], pos[partner][d]) for walker w = which * half + i of the active half `which`
__global__ void __launch_bounds__(STRETCH_LANES)
vag_stretch_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int which, int half, int ndim,
                           const double* __restrict__ pos /* [2 half][ndim] */, double* __restrict__ prop /* [half][ndim] */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    const int w = which * half + i;
    const StretchDraw dr = stretch_draw(seed_lo, seed_hi, step, w, half, a);
    const double* mine = pos + (size_t)w * ndim;
    const double* other = pos + (size_t)((1 - which) * half + dr.partner) * ndim;
    double* out = prop + (size_t)i * ndim;
    for (int d = 0; d < ndim; ++d) {
        const double q = other[d];
        out[d] = fma(dr.z, mine[d] - q, q);
    }
}

// The decision of walker w = which * half + i: reject a proposal whose ln p is not finite, otherwise accept iff
// log(u_a) < (ndim - 1) log z + (lp_new - lp[w]), u_a from stream 1 and z again from stream 0.  An accepted walker takes the
// proposal and its ln p and counts one.  chain_row / logp_row (of a stored step, or null): the walker's row of the chain and of ln p
// after the decision -- the two halves of a step fill the row between them.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_stretch_accept_kernel(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int which, int half, int ndim,
                          const double* __restrict__ prop /* [half][ndim] */, const double* __restrict__ lp_new /* [half] */,
                          double* __restrict__ pos /* [2 half][ndim] */, double* __restrict__ lp /* [2 half] */,
                          long long* __restrict__ accepted /* [2 half] */, double* __restrict__ chain_row /* [2 half][ndim] or null */,
                          double* __restrict__ logp_row /* [2 half] or null */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    const int w = which * half + i;
    const StretchDraw dr = stretch_draw(seed_lo, seed_hi, step, w, half, a);
    const uint32_t ctr[4] = {(uint32_t)w, (uint32_t)(step & 0xffffffffull), (uint32_t)(step >> 32), 1u};
    const uint32_t key[2] = {seed_lo, seed_hi};
    uint32_t y[4];
    philox4x32_10(ctr, key, y);
    const double u_a = u53(y[0], y[1]);
    const double ln_new = lp_new[i], ln_old = lp[w];
    const bool take = isfinite(ln_new) && log(u_a) < (double)(ndim - 1) * log(dr.z) + (ln_new - ln_old);  // (log(0) = -inf accepts)
    double* mine = pos + (size_t)w * ndim;
    const double* p = prop + (size_t)i * ndim;
    if (take) {
        for (int d = 0; d < ndim; ++d) mine[d] = p[d];
        lp[w] = ln_new;
        accepted[w] += 1;
    }
    if (chain_row) {
        double* row = chain_row + (size_t)w * ndim;
        for (int d = 0; d < ndim; ++d) row[d] = take ? p[d] : mine[d];
        logp_row[w] = take ? ln_new : ln_old;
    }
}

}  // namespace vag
