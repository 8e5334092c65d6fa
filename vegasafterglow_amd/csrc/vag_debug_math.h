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
constexpr int MATH_RVS_IN = 14;                       // Gamma, x4, x3, m3, U3, r, eps4, m4, Gamma4, eps_B, crossing, V3_comv_x, rho3_x, B3_ordered_x
constexpr int MATH_RVS_OUT = 6;                       // Gamma_th, B, N_p (rvs_shock_state), V3_comv, rho3, B3_ordered (rvs_cross_state)
constexpr int MATH_LAT_IN = 7;                        // ts, t_end, t_dec, T0, t_num, base_t_num, k
constexpr int MATH_LAT_OUT = 4;                       // node(k), n_pre, n_post, plain
constexpr int MATH_LAT_MAX = 4096;                    // largest t_num / base_t_num the probe takes
constexpr int MATH_EXT_NODES = 16;                    // nodes of a VAG_MATH_RVS_EXTRAP row
constexpr int MATH_EXT_IN = 4 * MATH_EXT_NODES + 1;   // 16 x (r, Gamma_th, B, N_p), inj
constexpr int MATH_EXT_OUT = 3 * MATH_EXT_NODES;      // 16 x (Gamma_th, B, N_p)
constexpr int MATH_INIT_IN = 10;                      // Gamma4, deps0_dt, dm0_dt, T0, t0, eps_e_th, medium type, rho_ism, A, r02
constexpr int MATH_INIT_OUT = RS_N;                   // the state of PairShock::init_state
constexpr int MATH_ICY_IN = 10;                       // gamma_m, gamma_c, p, B, Y_T, is_KN, g0, g1, nu0, nu1
constexpr int MATH_ICY_OUT = 18;                      // gamma_m_hat, gamma_c_hat, gamma_self, regime, seg.size, 3 x (slope, lg2_lower, lg2_const), Y(g0), Y(g1), Y(nu0), Y(nu1)
constexpr int MATH_STEP_IN = 8;                       // t_comv, B, gamma_m, gc, p, eps_e / eps_B, kn, gM
constexpr int MATH_STEP_OUT = 5;                      // Y_T, Y(gc), gc_new, gamma_M_of(B, Y(gc)), gamma_M_of(B, Y(gM))
constexpr int MATH_FIX_IN = 9;                        // t_comv, B, gamma_m, gc_stored, gamma_c_last, p, eps_e / eps_B, kn, gM_start
constexpr int MATH_FIX_OUT = 6;                       // gc, gc_used, Y_T, passes, gM, passes of gM
constexpr int MATH_GA_IN = 11;                        // B, column_den, gamma_m, gamma_c, gc_used, p, Y_T, kn, then a, c, m
constexpr int MATH_GA_OUT = 4;                        // gamma_a, Y_c, determine_regime(gamma_a, gamma_c, gamma_m), determine_regime(a, c, m)
constexpr int MATH_TAB_WORDS = 16;                    // table words of a VAG_MATH_IC_TABLE row
constexpr int MATH_TAB_IN = 5 + MATH_TAB_WORDS;       // n, first, th_min, th_max, x, 16 table words

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
        case VAG_MATH_REL_GAMMA: return 2;    // g1, g2
        case VAG_MATH_SHOCK_JUMP: return 2;   // gamma_rel, sigma
        case VAG_MATH_RVS_STATE: return MATH_RVS_IN;
        case VAG_MATH_CROSS_LATTICE: return MATH_LAT_IN;
        case VAG_MATH_RVS_EXTRAP: return MATH_EXT_IN;
        case VAG_MATH_PAIR_INIT: return MATH_INIT_IN;
        case VAG_MATH_KN_CORR: return 2;           // lg2_nu, lg2_x
        case VAG_MATH_IC_Y: return MATH_ICY_IN;
        case VAG_MATH_IC_STEP: return MATH_STEP_IN;
        case VAG_MATH_IC_FIXED_POINT: return MATH_FIX_IN;
        case VAG_MATH_IC_GAMMA_A: return MATH_GA_IN;
        case VAG_MATH_IC_TABLE: return MATH_TAB_IN;
        case VAG_MATH_IC_BIN_INTEGRAL: return 9;   // f_lo, f_hi, nu_lo, nu_hi, lg2f_lo, lg2f_hi, lg2r, inv_lg2r, trap
        case VAG_MATH_IC_SUFFIX_SCAN: return 4;    // the lane's four words of its wavefront's 256
        case VAG_MATH_IC_COLUMN_DEN: return 9;     // gamma, gamma_m, gamma_c, gamma_M, p, regime, column_den, Y_c, Y_at_gamma
        default: return (fn >= 0 && fn < VAG_MATH_COUNT) ? 1 : 0;
    }
}
inline int math_n_out(int fn) {
    switch (fn) {
        case VAG_MATH_SYN_CELL: return MATH_SYN_OUT;
        case VAG_MATH_IC_CELL: return MATH_IC_OUT;
        case VAG_MATH_ELEC_CELL: return MATH_ELEC_OUT;
        case VAG_MATH_FWD_STATE: return MATH_FWD_OUT;
        case VAG_MATH_REL_GAMMA: return 2;    // rel_Gamma, rel_Gamma_f
        case VAG_MATH_SHOCK_JUMP: return 3;   // downstr_4vel, jump_4vel, jump_4vel_f
        case VAG_MATH_SOUND_SPEED: return 2;  // sound_speed, sound_speed_f
        case VAG_MATH_RVS_STATE: return MATH_RVS_OUT;
        case VAG_MATH_CROSS_LATTICE: return MATH_LAT_OUT;
        case VAG_MATH_RVS_EXTRAP: return MATH_EXT_OUT;
        case VAG_MATH_PAIR_INIT: return MATH_INIT_OUT;
        case VAG_MATH_KN_LUT: return 2;            // ratio, log2 ratio
        case VAG_MATH_KN_CORR: return 4;           // corr, lg2_corr of _pair_lg2, then of _pair_node
        case VAG_MATH_IC_TABLE: return 2;          // value, breach
        case VAG_MATH_IC_SUFFIX_SCAN: return 4;
        case VAG_MATH_IC_Y: return MATH_ICY_OUT;
        case VAG_MATH_IC_STEP: return MATH_STEP_OUT;
        case VAG_MATH_IC_FIXED_POINT: return MATH_FIX_OUT;
        case VAG_MATH_IC_GAMMA_A: return MATH_GA_OUT;
        default: return (fn >= 0 && fn < VAG_MATH_COUNT) ? 1 : 0;
    }
}
inline bool math_is_wave(int fn) {
    return fn == VAG_MATH_WAVE_PREFIX_SUM || fn == VAG_MATH_WAVE_SUM || fn == VAG_MATH_SKY_WAVE_SUM || fn == VAG_MATH_LDS_ADD ||
           fn == VAG_MATH_IC_SUFFIX_SCAN;
}
// What is wrong with point `a` of routine `fn` (host side, before the launch), or nullptr: the integer and flag arguments that index or
// branch on the device, and the ranges the routines are defined on.
inline const char* math_point_error(int fn, const double* a) {
    auto whole = [](double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); };
    auto pos = [](double v) { return std::isfinite(v) && v > 0; };
    switch (fn) {
        case VAG_MATH_RVS_STATE: return (a[10] == 0 || a[10] == 1) ? nullptr : "the crossing flag must be 0 or 1";
        case VAG_MATH_CROSS_LATTICE:
            if (!(pos(a[0]) && pos(a[1]) && a[0] < a[1] && pos(a[2]) && pos(a[3]))) return "need 0 < ts < t_end and t_dec, T0 > 0, all finite";
            if (!whole(a[4], 2, MATH_LAT_MAX)) return "t_num must be an integer in [2, 4096]";
            if (!whole(a[5], 1, MATH_LAT_MAX)) return "base_t_num must be an integer in [1, 4096]";
            return whole(a[6], 0, a[4] - 1) ? nullptr : "k must be an integer in [0, t_num)";
        case VAG_MATH_RVS_EXTRAP: return whole(a[MATH_EXT_IN - 1], 0, MATH_EXT_NODES) ? nullptr : "inj must be an integer in [0, 16]";
        case VAG_MATH_PAIR_INIT:
            if (!(a[6] == VAG_MEDIUM_ISM || a[6] == VAG_MEDIUM_WIND)) return "unknown medium type";
            return (std::isfinite(a[0]) && a[0] > 1 && pos(a[3]) && pos(a[4])) ? nullptr : "need Gamma4 > 1, T0 > 0 and t0 > 0, all finite";
        case VAG_MATH_KN_LUT: return whole(a[0], 0, KN_LUT_N - 1) ? nullptr : "the node must be an integer in [0, 128)";
        case VAG_MATH_IC_TABLE: return whole(a[0], -1, MATH_TAB_WORDS) ? nullptr : "n must be an integer in [-1, 16]";
        case VAG_MATH_IC_COLUMN_DEN: return whole(a[5], 0, 6) ? nullptr : "the regime must be an integer in [0, 6]";
        case VAG_MATH_IC_Y: return (a[5] == 0 || a[5] == 1) ? nullptr : "the Klein-Nishina flag must be 0 or 1";
        case VAG_MATH_IC_STEP: return (a[6] == 0 || a[6] == 1) ? nullptr : "the Klein-Nishina flag must be 0 or 1";
        case VAG_MATH_IC_FIXED_POINT: return (a[7] == 0 || a[7] == 1) ? nullptr : "the Klein-Nishina flag must be 0 or 1";
        case VAG_MATH_IC_GAMMA_A: return (a[7] == 0 || a[7] == 1) ? nullptr : "the Klein-Nishina flag must be 0 or 1";
        default: return nullptr;
    }
}

// One point per lane, 64-lane workgroups (the wave routines' callers run wavefronts of 64; n % 64 == 0 for them).  The softplus / log2
// tables are copied into LDS exactly as vag_sky_terms_kernel does; `col` [VAG_NPAR][n] holds the synchrotron blocks as strided columns.
// Dynamic LDS: tables, 64 staged cell blocks, the sky_wave_sum scratch, 64 lds_add_f64 slots.
constexpr size_t MATH_PROBE_LDS = sizeof(double) * (SP_LDS_DOUBLES + 64 * VAG_NPAR + 64 + 64);
__global__ void __launch_bounds__(64) vag_math_probe_kernel(int fn, int n, const double* __restrict__ in, double* __restrict__ out,
                                                            const double* __restrict__ sp_table, double* __restrict__ col,
                                                            const double* __restrict__ knlut) {
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
        case VAG_MATH_REL_GAMMA:
            if (ok) out[2 * (size_t)i] = rel_Gamma(in[2 * (size_t)i], in[2 * (size_t)i + 1]), out[2 * (size_t)i + 1] = rel_Gamma_f(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
            return;
        case VAG_MATH_SHOCK_JUMP: {
            if (!ok) return;
            const double g = in[2 * (size_t)i], sigma = in[2 * (size_t)i + 1];
            double* r = out + 3 * (size_t)i;
            r[0] = downstr_4vel(g, sigma), r[1] = jump_4vel(g, sigma), r[2] = jump_4vel_f(g, sigma);
            return;
        }
        case VAG_MATH_SOUND_SPEED:
            if (ok) out[2 * (size_t)i] = sound_speed(in[i]), out[2 * (size_t)i + 1] = sound_speed_f(in[i]);
            return;
        case VAG_MATH_RVS_STATE: {
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_RVS_IN;
            const RvsCross held = {a[11], a[12], a[13]};
            const RvsState s = rvs_shock_state(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10] != 0, held);
            const RvsCross x = rvs_cross_state(a[0], a[1], a[2], a[5], a[6], a[7], a[8]);
            double* r = out + (size_t)i * MATH_RVS_OUT;
            r[0] = s.Gamma_th, r[1] = s.B, r[2] = s.N_p, r[3] = x.V3_comv, r[4] = x.rho3, r[5] = x.B3_ordered;
            return;
        }
        case VAG_MATH_CROSS_LATTICE: {
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_LAT_IN;
            CrossLattice lat;
            lat.init(a[0], a[1], a[2], a[3], (int)a[4], (int)a[5]);
            double* r = out + (size_t)i * MATH_LAT_OUT;
            r[0] = lat.node((int)a[6]), r[1] = lat.n_pre, r[2] = lat.n_post, r[3] = lat.plain;
            return;
        }
        case VAG_MATH_RVS_EXTRAP: {  // the row in this lane's own copy, nodes 4 doubles apart
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_EXT_IN;
            double w[4 * MATH_EXT_NODES];
            for (int q = 0; q < 4 * MATH_EXT_NODES; ++q) w[q] = a[q];
            rvs_early_extrap(w + 1, w + 2, w + 3, w, 4, MATH_EXT_NODES, (int)a[MATH_EXT_IN - 1]);
            double* r = out + (size_t)i * MATH_EXT_OUT;
            for (int q = 0; q < MATH_EXT_NODES; ++q) r[3 * q] = w[4 * q + 1], r[3 * q + 1] = w[4 * q + 2], r[3 * q + 2] = w[4 * q + 3];
            return;
        }
        case VAG_MATH_PAIR_INIT: {
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_INIT_IN;
            PairShock eq = {};
            eq.med.type = (int)a[6], eq.med.rho_ism = a[7], eq.med.A = a[8], eq.med.r02 = a[9], eq.med.k_m = 2;
            eq.Gamma4 = a[0], eq.deps0_dt = a[1], eq.dm0_dt = a[2], eq.T0 = a[3];
            eq.cs4 = sound_speed(eq.Gamma4);  // as vag_dynamics_pair_kernel sets them
            eq.beta4 = gamma_to_beta(eq.Gamma4);
            double s[RS_N];
            eq.init_state(s, a[4], a[5]);
            for (int q = 0; q < RS_N; ++q) out[(size_t)i * MATH_INIT_OUT + q] = s[q];
            return;
        }
        case VAG_MATH_KN_LUT:  // the context's own Klein-Nishina table, as vag_ctx_create filled it
            if (ok) out[2 * (size_t)i] = knlut[(int)in[i]], out[2 * (size_t)i + 1] = knlut[KN_LUT_N + (int)in[i]];
            return;
        case VAG_MATH_KN_CORR: {
            if (!ok) return;
            const double lg2_nu = in[2 * (size_t)i];
            double lg2_x = in[2 * (size_t)i + 1];
            if (lg2_x != lg2_x) lg2_x = lg2_nu + log2(C_H / (C_ME * C_C2));  // NaN: the argument _pair_lg2 forms from lg2_nu itself
            double* r = out + 4 * (size_t)i;
            compton_correction_pair_lg2(lg2_nu, knlut, r[0], r[1]);
            compton_correction_pair_node(lg2_x, exp2(lg2_x), knlut, r[2], r[3]);
            return;
        }
        case VAG_MATH_IC_TABLE: {  // the table is the row's own 16 words; last as vag_ic_plan_kernel forms it
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_TAB_IN;
            int breach = 0;
            const double last = ic_out_node(a[1], 0.0, (int)a[0] - 1);
            out[2 * (size_t)i] = ic_table_eval_hdr(a + 5, a[0], a[1], last, a[2], a[3], a[4], &breach);
            out[2 * (size_t)i + 1] = (double)breach;
            return;
        }
        case VAG_MATH_IC_BIN_INTEGRAL: {
            if (!ok) return;
            const double* a = in + (size_t)i * 9;
            out[i] = power_law_bin_integral(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
            return;
        }
        case VAG_MATH_IC_SUFFIX_SCAN: {  // 256 words per wavefront, in LDS as vag_ic_photon_kernel's histograms are
            for (int q = 0; q < 4; ++q) s_cell[4 * lane + q] = in[4 * (size_t)i + q];
            wave_sync();
            suffix_scan4(s_cell, lane);
            wave_sync();
            for (int q = 0; q < 4; ++q) out[4 * (size_t)i + q] = s_cell[4 * lane + q];
            return;
        }
        case VAG_MATH_IC_COLUMN_DEN: {
            if (!ok) return;
            const double* a = in + (size_t)i * 9;
            out[i] = electron_column_den(a[0], a[1], a[2], a[3], a[4], (int)a[5], a[6], a[7], a[8]);
            return;
        }
        case VAG_MATH_IC_Y: {  // the constructor as vag_photons_ic_kernel calls it, the segments as icy_store writes them
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_ICY_IN;
            IcY Ys;
            Ys.init(a[0], a[1], a[2], a[3], a[4], a[5] != 0);
            double w[VAG_NICY];
            icy_store(Ys, w, 1, 0);
            double* r = out + (size_t)i * MATH_ICY_OUT;
            r[0] = Ys.gamma_m_hat, r[1] = Ys.gamma_c_hat, r[2] = Ys.gamma_self, r[3] = (double)Ys.regime, r[4] = w[VY_NSEG];
            for (int q = 0; q < 9; ++q) r[5 + q] = w[VY_S0 + q];
            r[14] = Ys.gamma_spectrum(a[6]), r[15] = Ys.gamma_spectrum(a[7]);
            r[16] = icy_nu_spectrum(Ys, a[8]), r[17] = icy_nu_spectrum(Ys, a[9]);
            return;
        }
        case VAG_MATH_IC_STEP: {  // one pass of the body of each fixed point of ic_gamma_c_cell and of ic_gamma_M
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_STEP_IN;
            const double t_com = a[0], B = a[1], gm = a[2], gc = a[3], p = a[4];
            const bool kn = a[6] != 0;
            IcY Ys;
            Ys.init_base(gm, p, B);
            const double lg2_gc = log2_fast(gc);
            const double Y_T = thomson_Y_lg(a[5], p, gc < gm, lg2_gc - Ys.lg2_gamma_m);
            double Y = Y_T;
            if (kn) {
                Ys.update_cooling_breaks_lg(gc, lg2_gc, Y_T);
                Y = Ys.gamma_spectrum_lg(lg2_gc);
            } else {
                Ys.init(gm, gc, p, B, Y_T, false);
            }
            double* r = out + (size_t)i * MATH_STEP_OUT;
            r[0] = Y_T, r[1] = Y, r[2] = gamma_c_of(t_com, B, Y), r[3] = gamma_M_of(B, Y), r[4] = gamma_M_of(B, Ys.gamma_spectrum(a[7]));
            return;
        }
        case VAG_MATH_IC_FIXED_POINT: {  // the loops themselves: the functions vag_ic_cooling_kernel and vag_photons_ic_kernel call
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_FIX_IN;
            const bool kn = a[7] != 0;
            IcY Ys;
            double gc_used, Y_T;
            int passes = 0, passes_M = 0;
            const double gc = ic_gamma_c_cell(Ys, a[0], a[1], a[2], a[3], a[4], a[5], a[6], kn, gc_used, Y_T, &passes);
            if (!kn) Ys.init(a[2], gc_used, a[5], a[1], Y_T, false);
            const double gM = ic_gamma_M(a[1], a[8], Ys, &passes_M);
            double* r = out + (size_t)i * MATH_FIX_OUT;
            r[0] = gc, r[1] = gc_used, r[2] = Y_T, r[3] = (double)passes, r[4] = gM, r[5] = (double)passes_M;
            return;
        }
        case VAG_MATH_IC_GAMMA_A: {  // as vag_photons_ic_kernel calls them
            if (!ok) return;
            const double* a = in + (size_t)i * MATH_GA_IN;
            const double B = a[0], gm = a[2], gc = a[3], p = a[5];
            IcY Ys;
            Ys.init(gm, a[4], p, B, a[6], a[7] != 0);
            const double Y_c = Ys.gamma_spectrum(gc);
            const double ga = syn_gamma_a_ic(B, syn_I_peak(B, a[1]), gm, gc, p, Ys, Y_c);
            double* r = out + (size_t)i * MATH_GA_OUT;
            r[0] = ga, r[1] = Y_c, r[2] = (double)determine_regime(ga, gc, gm), r[3] = (double)determine_regime(a[8], a[9], a[10]);
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
        case VAG_MATH_EXP2_FAST_CHAIN: y = exp2_fast_as<EXP2_HEAD | EXP2_CHAIN>(x); break;
        case VAG_MATH_SP_FAST_RELU: y = sp_fast<true>(x, sp); break;
        case VAG_MATH_SP_FAST_RELU_VMAGIC: {  // the magic number opaque in a vector register, as flux_split_item holds it
            double magic = SP_MAGIC;
            asm volatile("" : "+v"(magic));
            y = sp_fast<true>(x, sp, magic);
            break;
        }
        default: return;
    }
    out[i] = y;
}

}  // namespace vag
