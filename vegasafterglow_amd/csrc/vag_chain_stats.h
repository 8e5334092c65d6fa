// vag_chain_stats.h -- the integrated autocorrelation time of a chain that lives on the device (INTEGRATION.md "Chain
// autocorrelation"): the two-pass mean of every series, its lag sums as one fma chain in ascending t, the sums pooled over the walkers
// in ascending w, Sokal's window on rho = C(l) / C(0).  The pieces of the definition are plain inline functions for host and device,
// as in vag_tempering.h and vag_moves.h: the kernels below and a host program compiled with the system C++ compiler
// (tests/chain_stats_check.cpp) include the same text.
//
// A chain view: element (t, w, d) at base[t row_stride + w D + d], row_stride >= W D; series s = w D + d, so the series of one row are
// adjacent and a wavefront of 64 series reads 512 contiguous bytes per row.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define VAG_CHAIN_HD __host__ __device__
#else
#define VAG_CHAIN_HD
#endif

#define VAG_CHAIN_TILE 16   // lags per wavefront of the lag-sum kernel: 16 accumulators and a 16-value ring of y in registers
#define VAG_CHAIN_WAVES 4   // wavefronts (consecutive lag tiles of the same 64 series) per workgroup

namespace vag {

// m1 = (sum x) / n, m = m1 + (sum (x - m1)) / n, both sums in ascending t: x[t stride], t = 0 .. n - 1
VAG_CHAIN_HD inline double chain_mean(const double* x, long long n, long long stride) {
    double s = 0.0;
    for (long long t = 0; t < n; ++t) s += x[t * stride];
    const double m1 = s / (double)n;
    double r = 0.0;
    for (long long t = 0; t < n; ++t) r += x[t * stride] - m1;
    return m1 + r / (double)n;
}

// c(lag) = sum_{t = 0}^{n - 1 - lag} (x[t] - m) (x[t + lag] - m), one fma chain in ascending t from +0
VAG_CHAIN_HD inline double chain_lag_sum(const double* x, long long n, long long stride, double m, long long lag) {
    double c = 0.0;
    for (long long t = 0; t + lag < n; ++t) c = std::fma(x[t * stride] - m, x[(t + lag) * stride] - m, c);
    return c;
}

// Sokal's window on rho[l stride], l = 0 .. L: tau(M) = 2 sum_{l <= M} rho(l) - 1 as a sequential sum, and the smallest M <= L with
// M >= c tau(M).  Returns that M with *tau = tau(M); if there is none, -1 with *tau = tau(L) (then a lower bound).  A rho that is not a
// number fails every comparison: -1 and a tau that is not a number.
VAG_CHAIN_HD inline int sokal_window(const double* rho, int L, double c, double* tau, long long stride = 1) {
    double s = 0.0, t = 0.0;
    for (int M = 0; M <= L; ++M) {
        s += rho[(long long)M * stride];
        t = 2.0 * s - 1.0;
        if ((double)M >= c * t) {
            *tau = t;
            return M;
        }
    }
    *tau = t;
    return -1;
}

// One parameter, from its pooled sums C[l stride]: rho(l) = C(l) / C(0) into rho[l stride] (rho may be C), then the window.  A C(0)
// that is zero or not finite: tau is NaN and the window -1 (rho holds whatever the divisions gave).
VAG_CHAIN_HD inline int chain_tau(const double* C, int L, double c, double* rho, double* tau, long long stride = 1) {
    const double c0 = C[0];
    for (int l = 0; l <= L; ++l) rho[(long long)l * stride] = C[(long long)l * stride] / c0;
    if (!std::isfinite(c0) || c0 == 0.0) {
        *tau = std::nan("");
        return -1;
    }
    return sokal_window(rho, L, c, tau, stride);
}

}  // namespace vag

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace vag {

constexpr int CHAIN_LANES = 64;  // one wavefront of adjacent series

// mean[s] = chain_mean of series s: one lane per series, two loops over the rows.  The sums are sequential by definition, so a series
// cannot be split over lanes and the kernel is as fast as its loads: the 32 loads of a block of rows are independent and issued
// together (16 KiB in flight per wavefront), then added in order.
constexpr int CHAIN_MEAN_ROWS = 32;
__global__ void __launch_bounds__(CHAIN_LANES)
vag_chain_mean_kernel(const double* __restrict__ chain, long long n, long long row_stride, int n_series, double* __restrict__ mean) {
    const int s = blockIdx.x * CHAIN_LANES + threadIdx.x;
    if (s >= n_series) return;
    const double* col = chain + s;
    double m1 = 0.0, shift = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double sum = 0.0;
        long long t = 0;
        for (; t + CHAIN_MEAN_ROWS <= n; t += CHAIN_MEAN_ROWS) {
            double x[CHAIN_MEAN_ROWS];
#pragma unroll
            for (int k = 0; k < CHAIN_MEAN_ROWS; ++k) x[k] = col[(t + k) * row_stride];
#pragma unroll
            for (int k = 0; k < CHAIN_MEAN_ROWS; ++k) sum += x[k] - shift;  // (x - 0 is x: the first pass is the plain sum)
        }
        for (; t < n; ++t) sum += col[t * row_stride] - shift;
        if (pass == 0)
            m1 = shift = sum / (double)n;
        else
            mean[s] = m1 + sum / (double)n;
    }
}

// Sixteen rows of the lag-sum loop, t = t0 .. t0 + 15 with t0 a multiple of 16: at row t the ring slot (t + j) % 16 holds
// y[t + l0 + j], every accumulator takes one fma with y[t], and the slot of y[t + l0] is refilled with y[t + l0 + 16].  All ring
// indices are constants after unrolling.  GUARD: rows past the end read as y = 0.
template <bool GUARD>
__device__ inline void chain_acf_rows(const double* __restrict__ col, long long row_stride, long long n, long long t0, long long lead,
                                      double m, double (&ring)[VAG_CHAIN_TILE], double (&acc)[VAG_CHAIN_TILE]) {
    double a[VAG_CHAIN_TILE], nx[VAG_CHAIN_TILE];
#pragma unroll
    for (int k = 0; k < VAG_CHAIN_TILE; ++k) {
        const long long t = t0 + k;
        if (GUARD) {
            a[k] = t < n ? col[t * row_stride] - m : 0.0;
            nx[k] = t + lead < n ? col[(t + lead) * row_stride] - m : 0.0;
        } else {
            a[k] = col[t * row_stride] - m;
            nx[k] = col[(t + lead) * row_stride] - m;
        }
    }
#pragma unroll
    for (int k = 0; k < VAG_CHAIN_TILE; ++k) {
#pragma unroll
        for (int j = 0; j < VAG_CHAIN_TILE; ++j) acc[j] = fma(a[k], ring[(k + j) % VAG_CHAIN_TILE], acc[j]);
        ring[k] = nx[k];
    }
}

// lag[l][s] = chain_lag_sum of series s at lag l, l = 0 .. L: one lane per series, one tile of VAG_CHAIN_TILE consecutive lags per
// wavefront, VAG_CHAIN_WAVES tiles of the same 64 series per workgroup (their rows meet in the L1).  Grid: n_groups series groups
// times the groups of tiles, the series group fastest.  Every accumulator is one fma chain in ascending t, whatever the launch: no
// atomics, no split of the time loop.  A product with a y past the end of the series is a product with 0, which leaves a finite
// accumulator as it is (an accumulator starts at +0 and never becomes -0).
__global__ void __launch_bounds__(CHAIN_LANES * VAG_CHAIN_WAVES)
vag_chain_acf_kernel(const double* __restrict__ chain, long long n, long long row_stride, int n_series, int n_groups, int L,
                     const double* __restrict__ mean, double* __restrict__ lag /* [L + 1][n_series] */) {
    const int s = (int)(blockIdx.x % (unsigned)n_groups) * CHAIN_LANES + threadIdx.x;
    const long long l0 = ((long long)(blockIdx.x / (unsigned)n_groups) * VAG_CHAIN_WAVES + threadIdx.y) * VAG_CHAIN_TILE;
    if (s >= n_series || l0 > L) return;  // (no barrier below)
    const double* col = chain + s;
    const double m = mean[s];
    double ring[VAG_CHAIN_TILE], acc[VAG_CHAIN_TILE];
#pragma unroll
    for (int j = 0; j < VAG_CHAIN_TILE; ++j) {
        acc[j] = 0.0;
        ring[j] = l0 + j < n ? col[(l0 + j) * row_stride] - m : 0.0;
    }
    const long long rows = n - l0;                    // t = 0 .. n - 1 - l0: the rows of the tile's smallest lag
    const long long lead = l0 + VAG_CHAIN_TILE;       // the refill reads y[t + lead]
    long long t0 = 0;
    for (; t0 + VAG_CHAIN_TILE - 1 + lead < n; t0 += VAG_CHAIN_TILE) chain_acf_rows<false>(col, row_stride, n, t0, lead, m, ring, acc);
    for (; t0 < rows; t0 += VAG_CHAIN_TILE) chain_acf_rows<true>(col, row_stride, n, t0, lead, m, ring, acc);
#pragma unroll
    for (int j = 0; j < VAG_CHAIN_TILE; ++j)
        if (l0 + j <= L) lag[(size_t)(l0 + j) * n_series + s] = acc[j];
}

// pooled[l][d] = sum_w lag[l][w D + d] in ascending w: one lane per (l, d)
__global__ void __launch_bounds__(256)
vag_chain_pool_kernel(const double* __restrict__ lag, int n_walkers, int ndim, int L, double* __restrict__ pooled /* [L + 1][D] */) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long long)(L + 1) * ndim) return;
    const long long l = item / ndim;
    const int d = (int)(item - l * ndim);
    const double* p = lag + (size_t)l * n_walkers * ndim + d;
    double sum = 0.0;
    int w = 0;
    for (; w + 8 <= n_walkers; w += 8) {
        double x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = p[(size_t)(w + k) * ndim];
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += x[k];
    }
    for (; w < n_walkers; ++w) sum += p[(size_t)w * ndim];
    pooled[item] = sum;
}

// One lane per parameter: rho = C / C(0) and the window rule (chain_tau) on the pooled sums.  rho_out[L + 1][D] is the caller's or the
// pooled buffer itself.
__global__ void __launch_bounds__(CHAIN_LANES)
vag_chain_tau_kernel(const double* pooled, int ndim, int L, double c, double* rho_out, double* __restrict__ tau,
                     int* __restrict__ window) {
    const int d = blockIdx.x * CHAIN_LANES + threadIdx.x;
    if (d >= ndim) return;
    double t;
    window[d] = chain_tau(pooled + d, L, c, rho_out + d, &t, ndim);
    tau[d] = t;
}

}  // namespace vag
#endif
