// vag_debug_math.h -- test-facing probe of the device math (vag_debug_device_math): evaluates one of the engine's own FP64 routines on
// caller-chosen points, on the device, in the library's translation unit, so that the code under test is the code the product kernels
// inline.  Nothing here is on a product call path.  tests/test_device_math.py holds each routine to a high-precision reference.
#pragma once
#include "vag_ic_kernels.h"
#include "vag_index.h"
#include "vag_log_ndtr.h"
#include "vag_poisson.h"
#include "vag_rs.h"
#include "vag_sky.h"

namespace vag {

constexpr int MATH_SYN_IN = 9;                        // gamma_m, gamma_c, gamma_a, gamma_M, column_den, B, p, x0, x1
constexpr int MATH_SYN_OUT = VAG_NPAR + 8;            // block, then fast (regs) x0 x1, fast (strided) x0 x1, fast2 x0 x1, exact x0 x1
constexpr int MATH_IC_IN = VAG_NPAR + VAG_NQ + 3;     // block, IC extras, p, x0, x1
constexpr int MATH_IC_OUT = 6;                        // log2_I_nu_ic x0 x1, _straight x0 x1, _pair x0 x1
constexpr int MATH_ELEC_IN = 12;                      // t_comv, r, Gamma_th, B, N_p, eps_e, p, xi_e, relic, inj.gamma_M, inj.gamma_m, inj.gamma_c
constexpr int MATH_ELEC_OUT = 11;                     // gamma_m, gamma_c, gamma_a, gamma_M, N_e, column_den, nu_m, nu_c, nu_a, nu_M, I_nu_max
constexpr int MATH_FWD_IN = 5;                        // Gamma, rho, U_th, m2, eps_B
constexpr int MATH_FWD_OUT = 4;                       // Gamma_th, B, N_p, compression

// [n_in, n_out] per point of routine `fn` (VAG_MATH_*); 0 for an unknown routine
inline int math_n_in(int fn) {
    switch (fn) {
        case VAG_MATH_SYN_CELL: return MATH_SYN_IN;
        case VAG_MATH_IC_CELL: return MATH_IC_IN;
        case VAG_MATH_LDS_ADD: return 2;  // slot (an integer in [0, 64)), value
        case VAG_MATH_POISSON_DEVIANCE: return 2;  // N, mu
        case VAG_MATH_LOG_SLOPE: return 2 * INDEX_MAX_NODES + 1;  // 8 fluxes, 8 coefficients, K
        case VAG_MATH_ELEC_CELL: return MATH_ELEC_IN;
        case VAG_MATH_FWD_STATE: return MATH_FWD_IN;
        default: return (fn >= 0 && fn < VAG_MATH_COUNT) ? 1 : 0;
    }
}
inline int math_n_out(int fn) {
    switch (fn) {
        case VAG_MATH_SYN_CELL: return MATH_SYN_OUT;
        case VAG_MATH_IC_CELL: return MATH_IC_OUT;
        case VAG_MATH_ELEC_CELL: return MATH_ELEC_OUT;
        case VAG_MATH_FWD_STATE: return MATH_FWD_OUT;
        default: return (fn >= 0 && fn < VAG_MATH_COUNT) ? 1 : 0;
    }
}
inline bool math_is_wave(int fn) {
    return fn == VAG_MATH_WAVE_PREFIX_SUM || fn == VAG_MATH_WAVE_SUM || fn == VAG_MATH_SKY_WAVE_SUM || fn == VAG_MATH_LDS_ADD;
}

// One point per lane, 64-lane workgroups (the wave routines' callers run wavefronts of 64; n % 64 == 0 for them).  The softplus / log2
// tables are copied into LDS exactly as vag_sky_terms_kernel does; `col` [VAG_NPAR][n] holds the synchrotron blocks as strided columns.
// Dynamic LDS: tables, 64 staged cell blocks, the sky_wave_sum scratch, 64 lds_add_f64 slots.
constexpr size_t MATH_PROBE_LDS = sizeof(double) * (SP_LDS_DOUBLES + 64 * VAG_NPAR + 64 + 64);
__global__ void __launch_bounds__(64) vag_math_probe_kernel(int fn, int n, const double* __restrict__ in, double* __restrict__ out,
                                                            const double* __restrict__ sp_table, double* __restrict__ col) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* s_sp = lds;
    for (int i = threadIdx.x; i < SP_LDS_DOUBLES; i += blockDim.x) s_sp[i] = sp_table[i];
    __syncthreads();
    double* s_cell = lds + SP_LDS_DOUBLES;  // 16-byte aligned: SP_LDS_DOUBLES is even
    double* s_red = s_cell + 64 * VAG_NPAR;
    double* s_slot = s_red + 64;
    const LdsTab sp = lds_tab(s_sp), lg = lds_tab(s_sp + SP_TABLE_DOUBLES);
    const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
    const bool ok = i < n;
    const int j = ok ? i : n - 1;  // a lane past the end recomputes the last point and stores nothing
    switch (fn) {
        case VAG_MATH_SYN_CELL: {
            const double* a = in + (size_t)j * MATH_SYN_IN;
            const double p = a[6], x0 = a[7], x1 = a[8];
            CellOut o;
            syn_photons_build(o, a[0], a[1], a[2], a[3], a[4], 0.0, a[5], p, 1.0, 1.0, 0.0);
            double* r = out + (size_t)j * MATH_SYN_OUT;
            for (int q = 0; q < VAG_NPAR; ++q) {
                s_cell[lane * VAG_NPAR + q] = o.par[q];
                if (ok) {
                    col[(size_t)q * n + i] = o.par[q];
                    r[q] = o.par[q];
                }
            }
            __syncthreads();
            SpecConst sc;
            sc.init(p);
            const SpecRegs regs = load_spec_regs(lds_tab(s_cell) + __mul24(lane, VAG_NPAR / 2));
            const double f0 = log2_I_nu_fast(regs, 1, sc, x0, sp), f1 = log2_I_nu_fast(regs, 1, sc, x1, sp);
            double g0, g1;
            log2_I_nu_fast2(regs, sc, x0, x1, sp, g0, g1);
            if (ok) {
                const double* cp = col + i;
                r[VAG_NPAR] = f0, r[VAG_NPAR + 1] = f1;
                r[VAG_NPAR + 2] = log2_I_nu_fast(cp, n, sc, x0, sp), r[VAG_NPAR + 3] = log2_I_nu_fast(cp, n, sc, x1, sp);
                r[VAG_NPAR + 4] = g0, r[VAG_NPAR + 5] = g1;
                r[VAG_NPAR + 6] = log2_I_nu(cp, n, sc, x0), r[VAG_NPAR + 7] = log2_I_nu(cp, n, sc, x1);
            }
            return;
        }
        case VAG_MATH_IC_CELL: {
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_IC_IN;
            const double* qv = a + VAG_NPAR;
            const double p = a[VAG_NPAR + VAG_NQ], x0 = a[VAG_NPAR + VAG_NQ + 1], x1 = a[VAG_NPAR + VAG_NQ + 2];
            SpecConst sc;
            sc.init(p);
            double* r = out + (size_t)i * MATH_IC_OUT;
            r[0] = log2_I_nu_ic(a, 1, qv, 1, sc, x0, sp), r[1] = log2_I_nu_ic(a, 1, qv, 1, sc, x1, sp);
            r[2] = log2_I_nu_ic_straight(a, 1, qv, 1, sc, x0, sp_table), r[3] = log2_I_nu_ic_straight(a, 1, qv, 1, sc, x1, sp_table);
            log2_I_nu_ic_pair(a, 1, qv, 1, sc, x0, x1, sp, r[4], r[5]);
            return;
        }
        case VAG_MATH_WAVE_PREFIX_SUM: out[i] = wave_prefix_sum(in[i]); return;
        case VAG_MATH_WAVE_SUM: out[i] = wave_sum(in[i]); return;
        case VAG_MATH_SKY_WAVE_SUM: out[i] = sky_wave_sum(in[i], s_red); return;
        case VAG_MATH_LDS_ADD: {  // 64 lanes add into the slots they name with one ds_add_f64; read back after wave_sync as the kernels do
            s_slot[lane] = 0.0;
            wave_sync();
            lds_add_f64(s_slot + ((int)in[2 * (size_t)i] & 63), in[2 * (size_t)i + 1]);
            wave_sync();
            out[i] = s_slot[lane];
            return;
        }
        case VAG_MATH_POISSON_DEVIANCE:
            if (ok) out[i] = poisson_deviance(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
            return;
        case VAG_MATH_LOG_SLOPE: {
            if (!ok) return;
            const double* a = in + (size_t)i * (2 * INDEX_MAX_NODES + 1);
            const int K = (int)a[2 * INDEX_MAX_NODES];
            out[i] = (K >= 2 && K <= INDEX_MAX_NODES) ? log_slope(a, 1, a + INDEX_MAX_NODES, K) : NAN;
            return;
        }
        case VAG_MATH_ELEC_CELL: {  // the cell as vag_cells_kernel computes it (syn_cell), details rows in the kernel's order
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_ELEC_IN;
            CellOut o;
            syn_cell(o, 0.0, a[0], a[1], 1.0, a[2], a[3], a[4], a[5], a[6], a[7], a[8] != 0, ElecBasic{a[9], a[10], a[11]});
            const double v[MATH_ELEC_OUT] = {o.gamma_m, o.gamma_c, o.gamma_a, o.gamma_M, o.N_e, o.column_den,
                                             o.nu_m, o.nu_c, o.nu_a, o.nu_M, o.I_nu_max};
            for (int q = 0; q < MATH_ELEC_OUT; ++q) out[(size_t)i * MATH_ELEC_OUT + q] = v[q];
            return;
        }
        case VAG_MATH_FWD_STATE: {
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_FWD_IN;
            const FwdState s = fwd_shock_state(a[0], a[1], a[2], a[3], a[4]);
            double* r = out + (size_t)i * MATH_FWD_OUT;
            r[0] = s.Gamma_th, r[1] = s.B, r[2] = s.N_p, r[3] = s.compression;
            return;
        }
        default: break;
    }
    if (!ok) return;
    const double x = in[i];
    double y;
    switch (fn) {
        case VAG_MATH_EXP2_FAST: y = exp2_fast(x); break;
        case VAG_MATH_EXP2_ODE: y = exp2_ode(x); break;
        case VAG_MATH_EXP2_SAT: y = exp2_sat(x); break;
        case VAG_MATH_EXP2_OR_ZERO: y = exp2_or_zero(x); break;
        case VAG_MATH_LOG2_FAST: y = log2_fast(x); break;
        case VAG_MATH_LOG2_TAB: y = log2_tab(x, lg); break;
        case VAG_MATH_LOG2_TAB_NB: y = log2_tab_nb(x, lg); break;
        case VAG_MATH_RCP_FAST: y = rcp_fast(x); break;
        case VAG_MATH_RCP_ODE: y = rcp_ode(x); break;
        case VAG_MATH_RCP1: y = rcp1(x); break;
        case VAG_MATH_SQRT_FAST: y = sqrt_fast(x); break;
        case VAG_MATH_SQRT_ODE: y = sqrt_ode(x); break;
        case VAG_MATH_SQRT1: y = sqrt1(x); break;
        case VAG_MATH_SP_FAST: y = sp_fast(x, sp); break;
        case VAG_MATH_SP_FAST_GLOBAL: y = sp_fast(x, sp_table); break;
        case VAG_MATH_SP_FAST_SEL: y = sp_fast_sel(x, sp); break;
        case VAG_MATH_LOG_NDTR: y = log_ndtr(x); break;
        default: return;
    }
    out[i] = y;
}

}  // namespace vag
