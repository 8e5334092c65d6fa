// vag_sampler.h -- the two kernels of the device ensemble sampler (INTEGRATION.md "the device sampler"): the Goodman & Weare stretch
// move in its parallel form with fixed halves, its draws a pure function of (seed, step, walker) through Philox4x32-10.  One lane per
// walker of the active half; the kernels are latency-sized (a half is a few hundred walkers): plain vector loads and stores, no LDS,
// no atomics.  The fused operations are explicit fma() calls and the division is an IEEE one, so that a proposal reproduces on the
// host to the bit (sampling.stretch_proposals).  The pieces every sampler kernel is written through are here too -- the draw of a
// stream, the stretch proposal of one walker, what an accepted walker takes, the walker's row of a stored step -- and vag_moves.h
// and vag_tempering.h use them: a body that two kernels share is one text.
#pragma once
#include <hip/hip_runtime.h>

#include "vag_philox.h"

namespace vag {

constexpr uint32_t STREAM_PROPOSAL = 0u, STREAM_ACCEPT = 1u, STREAM_EXCHANGE = 2u;  // (3 and 4: vag_moves.h; 5: vag_nested.h)

// the words of stream `stream` of replica r at `step`: counter (r, step lo, step hi, stream) under the key (seed_lo, seed_hi)
__device__ inline void stream_words(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int r, uint32_t stream, uint32_t out[4]) {
    const uint32_t ctr[4] = {(uint32_t)r, (uint32_t)(step & 0xffffffffull), (uint32_t)(step >> 32), stream};
    const uint32_t key[2] = {seed_lo, seed_hi};
    philox4x32_10(ctr, key, out);
}

// the uniform of the stream's first two words
__device__ inline double stream_uniform(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int r, uint32_t stream) {
    uint32_t y[4];
    stream_words(seed_lo, seed_hi, step, r, stream, y);
    return u53(y[0], y[1]);
}

struct StretchDraw {  // what a walker draws for one half-step
    double z;         // the stretch factor
    int partner;      // index within the complementary half
};

// stream 0 of replica r at `step`: u_z from the first two words, the partner from the third
__device__ inline StretchDraw stretch_draw(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int r, int half, double a) {
    uint32_t x[4];
    stream_words(seed_lo, seed_hi, step, r, STREAM_PROPOSAL, x);
    return {stretch_z(a, u53(x[0], x[1])), stretch_partner(x[2], half)};
}

// The stretch proposal of walker w = which * half + i of the ensemble ens[2 half][ndim], drawn as replica r:
// out[d] = fma(z, ens[w][d] - ens[partner][d], ens[partner][d]), the partner of the complementary half.  Returns z.
__device__ inline double stretch_proposal(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int r, int which, int half,
                                          int i, int ndim, const double* ens, double* out) {
    const StretchDraw dr = stretch_draw(seed_lo, seed_hi, step, r, half, a);
    const double* mine = ens + (size_t)(which * half + i) * ndim;
    const double* other = ens + (size_t)((1 - which) * half + dr.partner) * ndim;
    for (int d = 0; d < ndim; ++d) {
        const double q = other[d];
        out[d] = fma(dr.z, mine[d] - q, q);
    }
    return dr.z;
}

// an accepted walker takes the proposal and its ln p (ln L under tempering) and counts one
__device__ inline void take_proposal(double* mine, const double* p, int ndim, double* ln_p, double ln_new, long long* count) {
    for (int d = 0; d < ndim; ++d) mine[d] = p[d];
    *ln_p = ln_new;
    *count += 1;
}

// the walker's row of a stored step, after its decision
__device__ inline void write_row(double* row, double* ln_p_row, bool take, const double* p, const double* mine, int ndim, double ln_new,
                                 double ln_old) {
    for (int d = 0; d < ndim; ++d) row[d] = take ? p[d] : mine[d];
    *ln_p_row = take ? ln_new : ln_old;
}

// prop[i][d] = fma(z, pos[w][d] - pos[partner][d], pos[partner][d]) for walker w = which * half + i of the active half `which`
__global__ void __launch_bounds__(STRETCH_LANES)
vag_stretch_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int which, int half, int ndim,
                           const double* __restrict__ pos /* [2 half][ndim] */, double* __restrict__ prop /* [half][ndim] */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    stretch_proposal(seed_lo, seed_hi, a, step, which * half + i, which, half, i, ndim, pos, prop + (size_t)i * ndim);
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
    const double u_a = stream_uniform(seed_lo, seed_hi, step, w, STREAM_ACCEPT);
    const double ln_new = lp_new[i], ln_old = lp[w];
    const bool take = isfinite(ln_new) && log(u_a) < (double)(ndim - 1) * log(dr.z) + (ln_new - ln_old);  // (log(0) = -inf accepts)
    double* mine = pos + (size_t)w * ndim;
    const double* p = prop + (size_t)i * ndim;
    if (take) take_proposal(mine, p, ndim, lp + w, ln_new, accepted + w);
    if (chain_row) write_row(chain_row + (size_t)w * ndim, logp_row + w, take, p, mine, ndim, ln_new, ln_old);
}

}  // namespace vag
