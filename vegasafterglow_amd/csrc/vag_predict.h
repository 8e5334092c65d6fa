// vag_predict.h -- quantiles of every column of an array of draws F[S][M] that lives on the device (INTEGRATION.md "Posterior-predictive
// bands"): the per-draw validity, the rank of a quantile among n values, the value between two neighbours of the sorted column.  The
// pieces of the definition are plain inline functions for host and device, as in vag_chain_stats.h, vag_moves.h and vag_tempering.h:
// the kernels below and a host program compiled with the system C++ compiler (tests/predict_check.cpp) include the same text.
//
// The definition.  A draw (row s of F) is valid when its flag is set and all M of its values are finite; n is the number of valid draws,
// the same for every column.  For a quantile q in [0, 1]: h = q * (double)(n - 1) (one FP64 multiply), lo = floor(h), g = h - lo.  With
// y the column's valid values in ascending order, Q = y[lo] when g == 0 and otherwise Q = fma(g, y[lo + 1] - y[lo], y[lo]): one FP64
// subtraction inside one fused multiply-add.  (numpy's default "linear" quantile as a distribution; the rounding is fixed here.)
// y[lo + 1] is read only when g > 0, so q = 1 and n = 1 need no special case.  n == 0: Q is NaN.  Zeros of either sign compare equal
// and nothing distinguishes them: a zero is read as +0 (predict_read), so no result depends on which zero a sort met first.  Order
// statistics are exact, so the bits of Q depend neither on the tile, nor on the workgroup size, nor on the sorting network.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "vag_common.h"  // (vag_model_params, VagGridMeta; the public header's limits)
#define VAG_PREDICT_HD __host__ __device__
#else
#define VAG_PREDICT_HD
#endif

// the loud limits (the public header states the same three): draws per call, quantiles per call, values S * M per call (1 GiB of doubles)
#ifndef VAG_PREDICT_MAX_DRAWS
#define VAG_PREDICT_MAX_DRAWS 4096
#define VAG_PREDICT_MAX_Q 16
#define VAG_PREDICT_MAX_VALUES (1ll << 27)
#endif
#define VAG_PREDICT_LDS_BYTES (128 * 1024)  // a workgroup's sorted tile: T columns of P doubles, of the CU's 160 KiB
#define VAG_PREDICT_MAX_TILE 16             // columns per workgroup at most: 128 contiguous bytes of every draw's row

namespace vag {

// g, and *lo: the rank h = q (n - 1) of quantile q among n >= 1 values, split into floor and fraction.  0 <= *lo <= n - 1, and
// *lo == n - 1 only with g == 0 (q <= 1, so the rounded product is at most n - 1).
VAG_PREDICT_HD inline double predict_rank(double q, long long n, long long* lo) {
    double h = q * (double)(n - 1);
    // h is the ROUNDED product: the subtraction below must not be contracted with the multiply into one fma (the compilers' default
    // for device code), which would subtract from the exact product.  An empty asm statement (device) or a volatile copy (host) hands
    // the optimiser a value it cannot look through.
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(h));
#else
    volatile double rounded = h;
    h = rounded;
#endif
    const double f = std::floor(h);
    *lo = (long long)f;
    return h - f;
}

// Q from the sorted column y[i stride]: y[lo] when g == 0, else fma(g, y[lo + 1] - y[lo], y[lo]); y[lo + 1] is not read when g == 0
VAG_PREDICT_HD inline double predict_value(const double* y, long long lo, double g, long long stride = 1) {
    const double a = y[lo * stride];
    if (g == 0.0) return a;
    const double d = y[(lo + 1) * stride] - a;
    return std::fma(g, d, a);
}

// a value as the sort sees it: a zero of either sign is +0
VAG_PREDICT_HD inline double predict_read(double x) { return x == 0.0 ? 0.0 : x; }

// P: the size of the sorting network for S draws, the smallest power of two >= S (S in 1 .. VAG_PREDICT_MAX_DRAWS)
VAG_PREDICT_HD inline int predict_network_size(int S) {
    int P = 1;
    while (P < S) P <<= 1;
    return P;
}

// T: adjacent columns per workgroup at S draws -- what VAG_PREDICT_LDS_BYTES holds of columns of P doubles, at most
// VAG_PREDICT_MAX_TILE (a power of two: 16 up to 1024 draws, 8 up to 2048, 4 up to 4096)
VAG_PREDICT_HD inline int predict_tile_columns(int S) {
    const int t = VAG_PREDICT_LDS_BYTES / (8 * predict_network_size(S));
    return t < 1 ? 1 : (t > VAG_PREDICT_MAX_TILE ? VAG_PREDICT_MAX_TILE : t);
}

}  // namespace vag

#ifdef __HIPCC__
namespace vag {

struct PredictQ {  // vag_quantile_spec by value
    int nq, pad;
    double q[VAG_PREDICT_MAX_Q];
};

// valid[s] = (valid_in ? valid_in[s] != 0 : 1) && every F[s][0 .. M - 1] is finite: one wavefront per draw, four draws per workgroup;
// a wavefront reads its row in pieces of 512 contiguous bytes.  valid_out (or null) receives the same flags.
__global__ void __launch_bounds__(256)
vag_predict_valid_kernel(const double* __restrict__ F, int S, int M, const int* __restrict__ valid_in, int* __restrict__ valid,
                         int* __restrict__ valid_out) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;  // (wave-uniform; no barrier below)
    bool ok = valid_in ? valid_in[s] != 0 : true;
    const double* row = F + (size_t)s * M;
    if (ok)
        for (int m = lane; m < M; m += 64) ok = ok && isfinite(row[m]);
    ok = __all(ok) != 0;
    if (lane == 0) {
        valid[s] = ok ? 1 : 0;
        if (valid_out) valid_out[s] = ok ? 1 : 0;
    }
}

// out[k][m] = quantile q[k] of column m over the valid draws.  One workgroup takes T adjacent columns m0 .. m0 + T - 1 (T a power of
// two, predict_tile_columns), so a draw's piece of the tile is 8 T contiguous bytes of F and lands as 8 T contiguous bytes of LDS:
// element i of column c lives at y[i T + c], lanes adjacent in c touch adjacent words in every phase.  Rows s >= S, invalid draws and
// columns m >= M are +inf; a valid draw's values are finite, so after the ascending sort the n valid values are y[0 .. n - 1].  The
// sort is the bitonic network on P = predict_network_size(S) elements, T (P / 2) compare-exchanges per step dealt over the lanes,
// one barrier per step.  LDS: 16 bytes (the count of valid draws, an integer atomic) + 8 P T bytes.  n_valid_out (or null): written
// by workgroup 0.
__global__ void __launch_bounds__(1024)
vag_predict_quantile_kernel(const double* __restrict__ F, int S, int M, const int* __restrict__ valid, int P, int T, PredictQ qs,
                            double* __restrict__ out, int* __restrict__ n_valid_out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    int* count = reinterpret_cast<int*>(lds);
    double* y = lds + 2;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int m0 = blockIdx.x * T;
    const int tshift = __ffs(T) - 1, tmask = T - 1;
    if (tid == 0) *count = 0;
    __syncthreads();
    int mine = 0;
    for (int w = tid; w < P * T; w += nth) {
        const int s = w >> tshift, c = w & tmask;
        const bool live = s < S && valid[s] != 0;
        double x = INFINITY;
        if (live && m0 + c < M) x = predict_read(F[(size_t)s * M + m0 + c]);
        y[w] = x;
        if (live && c == 0) ++mine;
    }
    if (mine) atomicAdd(count, mine);
    __syncthreads();
    const int n = *count;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int w = tid; w < (P >> 1) * T; w += nth) {
                const int p = w >> tshift, c = w & tmask;
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const double a = y[i * T + c], b = y[l * T + c];
                if ((a > b) == up) {
                    y[i * T + c] = b;
                    y[l * T + c] = a;
                }
            }
            __syncthreads();
        }
    for (int w = tid; w < qs.nq * T; w += nth) {
        const int k = w >> tshift, c = w & tmask;
        if (m0 + c >= M) continue;
        double Q = std::nan("");
        if (n > 0) {
            long long lo;
            const double g = predict_rank(qs.q[k], n, &lo);
            Q = predict_value(y + c, lo, g, T);
        }
        out[(size_t)k * M + m0 + c] = Q;
    }
    if (blockIdx.x == 0 && tid == 0 && n_valid_out) *n_valid_out = n;
}

// theta[S][ndim] -> params[S] and a_v[S], the transformer of vag_fit_front_kernel without bounds, priors and point data: 10^theta for
// log-scale parameters, slot VAG_P_A_V into a_v, slots above it ignored (Fitter._params_at).  A theta that is not finite makes the
// draw's parameters invalid (theta_c = NaN: the grid stage gives it a status and no work), as a walker outside its bounds is there.
struct PredictSlots {
    int slot[16], is_log[16];
};
__global__ void __launch_bounds__(128)
vag_predict_front_kernel(vag_model_params base, const double* __restrict__ theta, int S, int ndim, PredictSlots sl,
                         double a_v_fixed, vag_model_params* __restrict__ out, double* __restrict__ a_v) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S) return;
    out[b] = base;
    double* f = &out[b].theta_c;
    double av = a_v_fixed;
    bool finite = true;
    for (int d = 0; d < ndim; ++d) {
        const double v = theta[(size_t)b * ndim + d];
        finite = finite && isfinite(v);
        const double val = sl.is_log[d] ? pow(10.0, v) : v;
        if (sl.slot[d] == VAG_P_A_V)
            av = val;
        else if (sl.slot[d] < VAG_P_A_V)
            f[sl.slot[d]] = val;
    }
    if (!finite) out[b].theta_c = NAN;
    a_v[b] = av;
}

// Behind the grid request of the S models, one workgroup per draw: ok[s] = the engine evaluated the model (grid status 0 and no ODE
// row without an acceptable step, as fit_close_pass reads them); an evaluated draw's fluxes take f exp(-A_V ext[inu]) where A_V != 0
// and ext is given (the expression of vag_fit_back_kernel), a draw that was not evaluated is NaN throughout.
__global__ void __launch_bounds__(256)
vag_predict_back_kernel(double* __restrict__ draws /* [S][nnu][nt] */, int nnu, int nt, const double* __restrict__ ext /* [nnu] or null */,
                        const double* __restrict__ a_v, const VagGridMeta* __restrict__ meta, const int* __restrict__ row_status,
                        const int* __restrict__ row_off, int* __restrict__ ok) {
    __shared__ int any_bad;
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool grid_ok = meta[s].status == 0;
    if (tid == 0) any_bad = grid_ok ? 0 : 1;
    __syncthreads();
    if (grid_ok) {
        bool bad = false;
        for (int r = row_off[s] + tid; r < row_off[s + 1]; r += 256) bad = bad || row_status[r] == 1;
        if (bad) atomicOr(&any_bad, 1);
    }
    __syncthreads();
    const bool good = any_bad == 0;
    if (tid == 0) ok[s] = good ? 1 : 0;
    const double av = ext != nullptr ? a_v[s] : 0.0;
    double* row = draws + (size_t)s * nnu * nt;
    if (!good) {
        for (int i = tid; i < nnu * nt; i += 256) row[i] = NAN;
    } else if (av != 0.0) {
        for (int i = tid; i < nnu * nt; i += 256) row[i] = row[i] * exp(-av * ext[i / nt]);
    }
}

}  // namespace vag
#endif
