// vag_moves.h -- the differential-evolution and snooker moves of the device ensemble sampler (INTEGRATION.md "The device sampler",
// "The move mix"): the reference's emcee configuration is DEMove at 0.8 and DESnookerMove at 0.2, both red-blue split moves, and this
// header states them in the fixed-halves framing of vag_sampler.h with the same Philox draws.  The choice of the move, the distinct
// partners, the quantised normal of the DE scale and the default scale are plain inline functions for host and device, as in
// vag_philox.h: the kernels below, the host side of the C-ABI (which chooses the kernel to launch, so no kernel branches on the kind)
// and a host program compiled with the system C++ compiler (tests/moves_check.cpp) include the same text.  The kernels follow
// vag_sampler.h: one lane per walker of the active half, 256-lane groups, plain vector loads and stores, no LDS, no atomics.  Every
// fused operation is an explicit fma() and every other product stands apart from a sum, so that a proposal reproduces on the host
// to the bit (sampling.de_proposals, sampling.snooker_proposals).
//
// Streams of the counter (w, step lo, step hi, stream): 0 the proposal, 1 the acceptance, 2 the exchange (vag_tempering.h), 3 the
// move choice (w = 0: one choice per step, shared by both halves), 4 a second block of proposal words, 5 the clone choice of nested
// sampling (vag_nested.h).
#pragma once
#include "vag_philox.h"

namespace vag {

constexpr int MOVE_STRETCH = 0, MOVE_DE = 1, MOVE_SNOOKER = 2;  // (VAG_MOVE_* of the public header)
constexpr uint32_t MOVE_STREAM_CHOICE = 3u, MOVE_STREAM_PROPOSAL2 = 4u;
constexpr double DE_QUANTUM_INV = 1048576.0, DE_QUANTUM = 1.0 / 1048576.0;  // 2^20, 2^-20
constexpr double MOVE_TWO_PI = 6.283185307179586;  // the double next to 2 pi

// The kind of a step from a uniform u in [0, 1) and the three weights (non-negative, finite, their sum > 0): u times the sum against
// the cumulative weights, which is the choice by the weights normalised by their sum.  u sum < sum in floating point (u <= 1 - 2^-53
// leaves the product more than half an ulp below the sum), so a trailing kind of weight 0 is never chosen, and a leading one never
// is because u sum >= 0.  The last line holds that without the argument, because it is a bound on memory: an ensemble may be too
// small for a kind of weight 0 (move_spec_check asks nh >= 2 or 3 only of kinds with weight), whose kernel would then index past a half.
VAG_PHILOX_HD inline int move_choice(double u, double w_stretch, double w_de, double w_snooker) {
    const double c1 = w_stretch + w_de;
    const double t = u * (c1 + w_snooker);
    if (t < w_stretch) return MOVE_STRETCH;
    if (t < c1) return MOVE_DE;
    return w_snooker > 0.0 ? MOVE_SNOOKER : (w_de > 0.0 ? MOVE_DE : MOVE_STRETCH);
}

// the uniform of the choice of `step`: the first two words of counter (0, step lo, step hi, 3)
VAG_PHILOX_HD inline double move_choice_uniform(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step) {
    const uint32_t ctr[4] = {0u, (uint32_t)(step & 0xffffffffull), (uint32_t)(step >> 32), MOVE_STREAM_CHOICE};
    const uint32_t key[2] = {seed_lo, seed_hi};
    uint32_t x[4];
    philox4x32_10(ctr, key, x);
    return u53(x[0], x[1]);
}

struct MovePair {  // two distinct walkers of the complementary half (indices within it)
    int a, b;
};
struct MoveTriple {  // three distinct ones
    int z, z1, z2;
};

// a = floor(xa nh / 2^32), b = (a + 1 + floor(xb (nh - 1) / 2^32)) mod nh: needs nh >= 2
VAG_PHILOX_HD inline MovePair move_pair(uint32_t xa, uint32_t xb, int nh) {
    const int a = stretch_partner(xa, nh);
    const int b = (a + 1 + stretch_partner(xb, nh - 1)) % nh;
    return {a, b};
}

// z and z1 as the pair; z2 = floor(xc (nh - 2) / 2^32), stepped over the two taken indices in ascending order: needs nh >= 3
VAG_PHILOX_HD inline MoveTriple move_triple(uint32_t xa, uint32_t xb, uint32_t xc, int nh) {
    const MovePair p = move_pair(xa, xb, nh);
    const int lo = p.a < p.b ? p.a : p.b, hi = p.a < p.b ? p.b : p.a;
    int c = stretch_partner(xc, nh - 2);
    if (c >= lo) ++c;
    if (c >= hi) ++c;
    return {p.a, p.b, c};
}

// the standard normal of Box & Muller from two uniforms in [0, 1): sqrt(-2 log(1 - u1)) cos(2 pi u2); 1 - u1 is exact and > 0
VAG_PHILOX_HD inline double de_normal(double u1, double u2) {
    const double r = std::sqrt(-2.0 * std::log(1.0 - u1));
    const double c = std::cos(MOVE_TWO_PI * u2);
    return r * c;
}

// n to the nearest multiple of 2^-20 (ties to even).  |n| <= 8.6, so n 2^20 < 2^24 and the scalings are exact: the quantised value is
// the same wherever log and cos round n 2^20 to the same side of a half-integer.
VAG_PHILOX_HD inline double de_quantise(double n) { return std::rint(n * DE_QUANTUM_INV) * DE_QUANTUM; }

// the customary scale of the DE move: 2.38 / sqrt(2 ndim) (ter Braak 2006)
VAG_PHILOX_HD inline double de_gamma0(int ndim) { return 2.38 / std::sqrt(2.0 * (double)ndim); }

// gamma = gamma0 (1 + sigma n_q)
VAG_PHILOX_HD inline double de_gamma(double gamma0, double sigma, double n_q) { return gamma0 * std::fma(sigma, n_q, 1.0); }

}  // namespace vag

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "vag_sampler.h"

namespace vag {

struct MoveWords {  // the proposal words of a walker: stream 0 and stream 4
    uint32_t x[4], v[4];
};

__device__ inline MoveWords move_words(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int w) {
    MoveWords m;
    stream_words(seed_lo, seed_hi, step, w, STREAM_PROPOSAL, m.x);
    stream_words(seed_lo, seed_hi, step, w, MOVE_STREAM_PROPOSAL2, m.v);
    return m;
}

// The stretch move of vag_stretch_propose_kernel (the same stretch_proposal), which also writes factor[i] = (ndim - 1) log z.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_move_stretch_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double a, unsigned long long step, int which, int half, int ndim,
                                const double* __restrict__ pos /* [2 half][ndim] */, double* __restrict__ prop /* [half][ndim] */,
                                double* __restrict__ factor /* [half] */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    const double z = stretch_proposal(seed_lo, seed_hi, a, step, which * half + i, which, half, i, ndim, pos, prop + (size_t)i * ndim);
    factor[i] = (double)(ndim - 1) * log(z);
}

// The DE move: a != b of the other half from words 2 and 3 of stream 0, the normal from u1 = u(x0, x1) of stream 0 and
// u2 = u(v0, v1) of stream 4, quantised; prop[i][d] = fma(gamma, pos[a][d] - pos[b][d], pos[w][d]); factor[i] = 0.  half >= 2.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_de_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double gamma0, double sigma, unsigned long long step, int which, int half,
                      int ndim, const double* __restrict__ pos /* [2 half][ndim] */, double* __restrict__ prop /* [half][ndim] */,
                      double* __restrict__ factor /* [half] */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    const int w = which * half + i;
    const MoveWords m = move_words(seed_lo, seed_hi, step, w);
    const MovePair pr = move_pair(m.x[2], m.x[3], half);
    const double gamma = de_gamma(gamma0, sigma, de_quantise(de_normal(u53(m.x[0], m.x[1]), u53(m.v[0], m.v[1]))));
    const double* mine = pos + (size_t)w * ndim;
    const double* ca = pos + (size_t)((1 - which) * half + pr.a) * ndim;
    const double* cb = pos + (size_t)((1 - which) * half + pr.b) * ndim;
    double* out = prop + (size_t)i * ndim;
    for (int d = 0; d < ndim; ++d) out[d] = fma(gamma, ca[d] - cb[d], mine[d]);
    factor[i] = 0.0;
}

// The snooker move: z, z1, z2 of the other half from words 2 and 3 of stream 0 and word 2 of stream 4.  With delta = s - z,
// r2 = delta . delta and proj = delta . (z1 - z2), both summed from 0 in dimension order with one fma per term,
// prop[d] = fma(gamma_s (proj / r2), delta[d], s[d]) -- the projection on the unit vector of ter Braak & Vrugt -- and
// factor = (ndim - 1) / 2 log(|prop - z|^2 / r2).  r2 = 0 or a factor that is not finite: the walker proposes its own position
// with factor -inf, which no draw accepts.  half >= 3, ndim <= 16.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_snooker_propose_kernel(uint32_t seed_lo, uint32_t seed_hi, double gamma_s, unsigned long long step, int which, int half, int ndim,
                           const double* __restrict__ pos /* [2 half][ndim] */, double* __restrict__ prop /* [half][ndim] */,
                           double* __restrict__ factor /* [half] */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    const int w = which * half + i;
    const MoveWords m = move_words(seed_lo, seed_hi, step, w);
    const MoveTriple tr = move_triple(m.x[2], m.x[3], m.v[2], half);
    const double* mine = pos + (size_t)w * ndim;
    const double* other = pos + (size_t)(1 - which) * half * ndim;
    const double* pz = other + (size_t)tr.z * ndim;
    const double* p1 = other + (size_t)tr.z1 * ndim;
    const double* p2 = other + (size_t)tr.z2 * ndim;
    double r2 = 0.0, proj = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double delta = mine[d] - pz[d];
        r2 = fma(delta, delta, r2);
        proj = fma(delta, p1[d] - p2[d], proj);
    }
    const double coef = gamma_s * (proj / r2);
    double q2 = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double q = fma(coef, mine[d] - pz[d], mine[d]);
        const double e = q - pz[d];
        q2 = fma(e, e, q2);
    }
    const double f = (0.5 * (double)(ndim - 1)) * log(q2 / r2);
    const bool ok = r2 > 0.0 && isfinite(f);
    double* out = prop + (size_t)i * ndim;
    for (int d = 0; d < ndim; ++d) out[d] = ok ? fma(coef, mine[d] - pz[d], mine[d]) : mine[d];
    factor[i] = ok ? f : -INFINITY;
}

// The decision of walker w = which * half + i for a proposal of any kind: reject one whose ln p is not finite, otherwise accept iff
// log(u_a) < factor[i] + (lp_new - lp[w]), u_a from stream 1 as in vag_stretch_accept_kernel; the rest is that kernel's: an accepted
// walker takes the proposal and its ln p and counts one, chain_row / logp_row (of a stored step, or null) receive the walker's row.
__global__ void __launch_bounds__(STRETCH_LANES)
vag_move_accept_kernel(uint32_t seed_lo, uint32_t seed_hi, unsigned long long step, int which, int half, int ndim,
                       const double* __restrict__ prop /* [half][ndim] */, const double* __restrict__ factor /* [half] */,
                       const double* __restrict__ lp_new /* [half] */, double* __restrict__ pos /* [2 half][ndim] */,
                       double* __restrict__ lp /* [2 half] */, long long* __restrict__ accepted /* [2 half] */,
                       double* __restrict__ chain_row /* [2 half][ndim] or null */, double* __restrict__ logp_row /* [2 half] or null */) {
    const int i = blockIdx.x * STRETCH_LANES + threadIdx.x;
    if (i >= half) return;
    const int w = which * half + i;
    const double u_a = stream_uniform(seed_lo, seed_hi, step, w, STREAM_ACCEPT);
    const double ln_new = lp_new[i], ln_old = lp[w];
    const bool take = isfinite(ln_new) && log(u_a) < factor[i] + (ln_new - ln_old);  // (log(0) = -inf accepts; factor -inf never does)
    double* mine = pos + (size_t)w * ndim;
    const double* p = prop + (size_t)i * ndim;
    if (take) take_proposal(mine, p, ndim, lp + w, ln_new, accepted + w);
    if (chain_row) write_row(chain_row + (size_t)w * ndim, logp_row + w, take, p, mine, ndim, ln_new, ln_old);
}

}  // namespace vag
#endif
