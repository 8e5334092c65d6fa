// vag_flux_limits.h -- the compile-time limits of the flux kernels that the host's launch decisions read (vag_flux_plan.h), and the
// measured thresholds of those decisions.  Plain C++, no device code: the kernel headers (vag_kernels.h, vag_fit_rows.h,
// vag_grid_rows.h) include it in place of definitions of their own, and tests/flux_plan_check.cpp builds it with a host compiler.
#pragma once
#include <cstddef>

namespace vag {

// ---- vag_flux_grid_kernel (vag_kernels.h) ----
constexpr int FLUX_THREADS = 512;
constexpr int FLUX_MAX_SLOTS = 8192;  // (l, idx) output slots per launch, accumulated in LDS  // (l, idx) slots per lane: nt * nnu <= FLUX_THREADS * FLUX_MAX_SLOTS

// photon source of the flux kernels
constexpr int FLUX_SYN = 0;     // synchrotron, no inverse-Compton cooling
constexpr int FLUX_SYN_IC = 1;  // synchrotron with the IC correction above nu_c
constexpr int FLUX_SSC = 2;     // SSC tables
constexpr int FLUX_FUSED = 3;   // FLUX_SYN_IC and FLUX_SSC in one pass: EAT logs, bracket search and barriers paid once

// ---- vag_flux_grid_split_kernel (vag_kernels.h: the team sizes were measured at 6 + 2, 5 + 3 and 4 + 4) ----
constexpr int FLUX_SPLIT_A = 6;                                     // wavefronts 0 .. FLUX_SPLIT_A - 1: A team
constexpr int FLUX_SPLIT_B = FLUX_THREADS / 64 - FLUX_SPLIT_A;      // the rest: B team
constexpr int FLUX_SPLIT_TIMES = 2;                                 // requested times a B lane can own
constexpr int FLUX_SPLIT_MAX_NT = FLUX_SPLIT_TIMES * FLUX_SPLIT_B * 64;
constexpr int FLUX_SPLIT_MAX_NNU = 10;                              // accumulators per owned time
// a / n (a, n > 0) from the estimate q = (int)((float)a * rcp_n) of the boundary loop's reciprocal: one compare-and-adjust each way,
// so the quotient is exact for any estimate within one of it, whatever the last bit of the hardware's reciprocal
// (tests/flux_quot_check.cpp: a = 384, every n in 1 .. 204, the reciprocal moved by up to four units in the last place)
constexpr int flux_quot_adjust(int a, int n, int q) {
    q -= q * n > a;
    q += (q + 1) * n <= a;
    return q;
}

// ---- the persistent launch and the split form: host thresholds ----
constexpr int FLUX_PERSIST_MIN_PPB = 128;  // shortest items (rows per workgroup) the persistent form takes unforced (persist_plan)
constexpr int FLUX_SPLIT_MIN_KS = 192;  // shortest staged lattice the split form takes unforced (measured at 199 nodes)
// the most dynamic LDS vag_flux_grid_split_kernel may ask for: two workgroups stay resident per CU, like the kernel it stands in for
constexpr size_t FLUX_SPLIT_LDS_BUDGET = 81920;

// ---- vag_flux_series_kernel (vag_kernels.h) ----
constexpr int SERIES_THREADS = 64;    // lanes that share one (theta, phi) row: ONE wavefront, so rows need no block barrier
constexpr int SERIES_WAVES = 4;       // most independent wavefronts per workgroup (the host picks 4, 2 or 1 by what stays resident); they only share the tables
constexpr int SERIES_MAX_SLOTS = 8;   // data points per lane: n <= 512
constexpr int SERIES_CHUNK = 8;       // (theta, phi) rows per partial sum: the unit of a model's summation tree, whatever the batch
constexpr int SERIES_MAX_BANDS = 8;   // distinct frequencies the shared-node path handles

// ---- vag_flux_fit_rows_kernel (vag_fit_rows.h) ----
constexpr int FITROWS_WAVES = 4;   // wavefronts per workgroup (they only share the tables and the data points)
constexpr int FITROWS_BANDS = 8;   // distinct frequencies handled (instantiations for <= 4 and <= 8; more: vag_flux_series_kernel)
constexpr int FITROWS_MAX_POINTS = 512;  // data points of a pass (SERIES_THREADS * SERIES_MAX_SLOTS)
constexpr int FITROWS_ROWS = 64;   // rows per block = lanes of a wavefront
constexpr int FITROWS_SEGS = 4;    // lattice segments per block: each (block, segment) is one partial sum of the model's tree

// ---- vag_flux_grid_rows_kernel (vag_grid_rows.h) ----
#ifndef VAG_GRIDROWS_WAVES
#define VAG_GRIDROWS_WAVES 4
#endif
constexpr int GRIDROWS_WAVES = VAG_GRIDROWS_WAVES;
constexpr int GRIDROWS_BANDS = 4;     // frequencies
#ifndef VAG_GRIDROWS_MAX_NT
#define VAG_GRIDROWS_MAX_NT 128
#endif
constexpr int GRIDROWS_MAX_NT = VAG_GRIDROWS_MAX_NT;  // requested times
constexpr int GRIDROWS_MAX_SLOTS = 512;

}  // namespace vag
