// vag_fit_kernels.h -- the kernels of a likelihood call (vag_loglike_*_batch): its front, the back kernel of every kind of pass, and
// the walkers' polarization spec.  A call is one front launch and then one pass per block of data -- the point rows, every band,
// centroid, visibility, polarization, counts, spectral-index, fold and correlated group -- each pass a model request followed by its back kernel, one
// wavefront per walker.  What the back kernels share is the pass protocol below: FitPass and the two helpers.
#pragma once
#include "vag_fold.h"
#include "vag_ic_kernels.h"
#include "vag_index.h"
#include "vag_kernels.h"
#include "vag_log_ndtr.h"
#include "vag_poisson.h"
#include "vag_robust.h"
#include "vag_sky.h"

namespace vag {

// What every back kernel receives, the same in every pass of a call but for first / last and ic_status.
struct FitPass {
    const VagGridMeta* meta;  // [nb] the pass's grids: status != 0 = not evaluated
    const int* row_status;    // the pass's ODE rows: 1 = no acceptable step
    const int* row_off;       // [nb + 1] a walker's rows in row_status
    const int* ic_status;     // [nb] the pass's SSC tables: != 0 = outside their capacity; null when the batch has no SSC
    double* chi2;             // [nb] the walker's chi^2 over the passes so far
    int* valid;               // [nb] every pass so far evaluated the walker
    const double* ln_prior;   // [nb]
    int first, last;          // the call's first / last pass
    double* out;              // [nb] ln L, by walker; written by the last pass
    int* fitstat;             // [0] walkers scored -inf, [1] of those: SSC table failures
    const int* order;         // evaluation slot -> walker, or null (identity)
};

// For the kernels that can be a call's first pass: where they leave the order the NEXT call of this batch size evaluates in.
struct FitOrderOut {
    const float* cost;  // [nb] the slots' costs of THIS call (the grid kernel's plan scan leaves them)
    int nb;
    int* next_order;    // [rank] = walker, descending cost; null: not this launch (the order is made once per call)
};

// next_order[rank] = walker, ranks by descending cost of the slot in THIS call (cost[] is in evaluation-slot order: `order` maps a slot
// back to its walker; null = identity).  Ranking by counting: the lanes compare this wavefront's slot with all others.  (Until round 5
// a launch of its own, vag_order_kernel, behind the back kernel.)  The kernels read the grid status before they call this: FitPass's
// pointers carry no __restrict__, so a wave-uniform load behind this store is a vector load, not a scalar one.
__device__ __forceinline__ void fit_hand_over_order(const FitPass& p, const FitOrderOut& o, int m, int lane) {
    if (!o.next_order) return;
    const float mine = o.cost[m];
    int rank = 0;
    for (int i0 = 0; i0 < o.nb; i0 += 64) {
        const int i = i0 + lane;
        const float c = i < o.nb ? o.cost[i] : -1.0f;
        rank += __popcll(__ballot(c > mine || (c == mine && i < m)));
    }
    if (lane == 0) o.next_order[rank] = p.order ? p.order[m] : m;
}

// The end of every back kernel.  s is the pass's chi^2 term of walker slot m (the same in every lane, or at least in lane 0), bad
// what the lane found wrong with the walker's own data so far (false for the flux kernels).
//   chi2[m] (+)= s;
//   valid[m] &= this pass evaluated the walker -- parameters valid, grid within the engine limits, no ODE row without an acceptable
//   step, SSC tables within their capacity, no lane's `bad` -- else the walker scores -inf like eval_one's except branch
//   (samplers.py:61-70);
//   last pass: out[walker] = valid ? -chi2 / 2 + ln prior : -inf, and the rejection counters.
__device__ __forceinline__ void fit_close_pass(const FitPass& p, int m, int lane, bool grid_ok, bool bad, double s) {
    if (grid_ok)
        for (int r = p.row_off[m] + lane; r < p.row_off[m + 1]; r += 64) bad = bad || p.row_status[r] == 1;
    const bool any_bad = __any(bad);
    if (lane == 0) {
        const bool ic_bad = grid_ok && p.ic_status && p.ic_status[m] != 0;
        const int ok = (p.first ? 1 : p.valid[m]) && grid_ok && !any_bad && !ic_bad;
        const double acc = p.first ? s : p.chi2[m] + s;
        p.valid[m] = ok;
        p.chi2[m] = acc;
        if (ic_bad) atomicAdd(p.fitstat + 1, 1);
        if (p.last) {
            const double lp = p.ln_prior[m];
            const bool fin = ok && isfinite(acc) && lp > -INFINITY;
            p.out[p.order ? p.order[m] : m] = fin ? -0.5 * acc + lp : -INFINITY;
            if (!fin) atomicAdd(p.fitstat, 1);
        }
    }
}

// The front of a likelihood call, one launch: bounds mask and ln prior (log_prob_batch, fitting/samplers.py:72-91), the
// transformer of fitting/utils.py:110-135 (theta[nb][ndim] -> params[nb], 10^theta for log-scale parameters), A_V per walker,
// and -- block 0 -- log2 of the point data's times / frequencies and their time extrema for the grid stage.
__global__ void __launch_bounds__(128)
vag_fit_front_kernel(vag_model_params base, const double* __restrict__ theta, int nb, int ndim, const double* __restrict__ prior,
                     int use_priors, double a_v_fixed, vag_model_params* __restrict__ out, double* __restrict__ a_v,
                     double* __restrict__ ln_prior, int* __restrict__ fitstat, const double* __restrict__ t, int n,
                     const double* __restrict__ nu, double* __restrict__ lg2_t, double* __restrict__ lg2_nu,
                     double* __restrict__ tminmax, const int* __restrict__ order /* evaluation slot -> walker, or null */) {
    const int* slot = reinterpret_cast<const int*>(prior + 64);
    const int* is_log = slot + 16;
    const int* kind = slot + 32;
    if (blockIdx.x == 0) {
        if (threadIdx.x < 4) fitstat[threadIdx.x] = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            lg2_t[i] = log2(t[i] * U_SEC);  // xt::log2(t_obs), observer.h:359
            lg2_nu[i] = log2(nu[i] * U_HZ);
        }
        if (threadIdx.x == 0 && n > 0) {  // ascending data (fitter.py:420-428)
            tminmax[0] = t[0];
            tminmax[1] = t[n - 1];
        }
    }
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    out[b] = base;  // the sampled fields are patched in place (a private copy indexed by slot would live in scratch)
    double* f = &out[b].theta_c;
    double av = a_v_fixed, lp = 0;
    bool inside = true;
    const int walker = order ? order[b] : b;
    for (int d = 0; d < ndim; ++d) {
        const double v = theta[(size_t)walker * ndim + d];
        if (use_priors) {
            const double lo = prior[d], hi = prior[16 + d];
            inside = inside && (v >= lo) && (v <= hi);
            if (kind[d] == VAG_PRIOR_GAUSSIAN) {
                const double z = (v - prior[32 + d]) / prior[48 + d];
                lp += -0.5 * z * z - log(prior[48 + d] * 2.5066282746310002);
            } else if (kind[d] == VAG_PRIOR_LOG_UNIFORM) {
                const double mn = prior[32 + d], mx = prior[48 + d];
                lp += (v >= mn && v <= mx) ? -log(v * log(mx / mn)) : -INFINITY;
            } else if (kind[d] == VAG_PRIOR_UNIFORM) {
                lp += -log(hi - lo);
            } else if (kind[d] == VAG_PRIOR_UNIFORM_RANGE) {
                const double mn = prior[32 + d], mx = prior[48 + d];
                lp += (v >= mn && v <= mx) ? -log(mx - mn) : -INFINITY;
            }
        }
        const double val = is_log[d] ? pow(10.0, v) : v;
        if (slot[d] == VAG_P_A_V)
            av = val;  // not a Model field: scales the point-data fluxes (fitter.py:512-519)
        else if (slot[d] < VAG_P_A_V)  // (VAG_P_SKY_*: read by vag_fit_sky_back_kernel)
            f[slot[d]] = val;
    }
    if (!inside) {  // never evaluated by the reference either: an invalid parameter set stops at the grid stage with no work
        out[b].theta_c = NAN;
        lp = -INFINITY;
    }
    a_v[b] = av;
    ln_prior[b] = use_priors ? lp : 0.0;
}

// The back of a flux pass (the point rows, a band group), one wavefront per walker:
//   s = sum_i w_i ((ln F_obs,i - ln max(F_model,i e^{-A_V k_i}, 1e-300)) / sigma_i)^2   (Fitter._chi2_sum, fitter.py:497-501, with the
//   extinction factor of fitter.py:512-519).
// LIM, for a pass with upper-limit rows (vag_loglike_lim_batch): a row with lim_kind[i] == VAG_OBS_UPPER_LIMIT adds
//   -2 w_i ln Phi((L_i - F_model,i e^{-A_V k_i}) / sigma_i)   (log_ndtr; no 1e-300 clamp: a model with no flux satisfies a limit)
// instead of its detection term, at the same place of the lane's sum.  A compile-time flag, so that a pass without limit rows runs
// the instructions it always ran; the three limit arguments are not read then.
template <bool LIM>
__global__ void __launch_bounds__(64)
vag_fit_back_kernel(const double* __restrict__ flux /* [nb][n] */, int n, const double* __restrict__ ln_flux,
                    const double* __restrict__ ln_err, const double* __restrict__ weight, const double* __restrict__ ext /* or null */,
                    const double* __restrict__ a_v, FitPass pass, FitOrderOut ord, const int* __restrict__ lim_kind /* [n] VAG_OBS_* */,
                    const double* __restrict__ lim_L /* [n] */, const double* __restrict__ lim_sigma /* [n] */) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    const double av = (ext != nullptr) ? a_v[m] : 0.0;
    double s = 0;
    if (grid_ok)
        for (int i = lane; i < n; i += 64) {
            double f = flux[(size_t)m * n + i];
            if (av != 0.0) f = f * exp(-av * ext[i]);
            if constexpr (LIM) {
                if (lim_kind[i] == VAG_OBS_UPPER_LIMIT) {
                    s += weight[i] * (-2.0 * log_ndtr((lim_L[i] - f) / lim_sigma[i]));
                    continue;
                }
            }
            const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
            const double q = (ln_flux[i] - log(fm)) / ln_err[i];
            s += weight[i] * (q * q);
        }
    s = wave_sum(s);
    fit_close_pass(pass, m, lane, grid_ok, false, s);
}

// The back of a flux pass with rows in noise groups (vag_loglike_noise_batch).  Rows without a group (grp[i] < 0) and upper-limit
// rows (whatever their group; lim_kind is null when the pass has none) add the terms of vag_fit_back_kernel<true>, statement for
// statement.  The detection rows of every group g the pass holds (bit g of `present`) add, with s_g the walker's systematic -- the
// free parameter with the slot VAG_P_NOISE_SYS0 + g (found as sky_placement finds pa), else noise[g] -- and c_g = noise[8 + g]:
//   v_i = sigma_i^2 + s_g^2, p_i = w_i / v_i, A = sum p_i r_i^2, B = sum p_i r_i, P = sum p_i, N = sum w_i log1p(s_g^2 / sigma_i^2),
//   c_g == 0: A + N  (separable: the group may span passes);  c_g > 0: A - c_g^2 B^2 / (1 + c_g^2 P) + N + log1p(c_g^2 P)  (the pass
//   holds all of the group: noise_scan refuses anything else).
// Every sum is a fixed lane-strided sum followed by wave_sum, group after group in ascending g: the value depends on the walker's
// row alone, not on its evaluation slot.  The groups are walked one at a time (a wave-uniform loop over the set bits), so the four
// accumulators are scalars in registers; a row's log is taken once, in the turn of its own group.  A kernel of its own so that a pass
// without grouped rows runs the instructions it always ran.
__global__ void __launch_bounds__(64)
vag_fit_back_noise_kernel(const double* __restrict__ flux /* [nb][n] */, int n, const double* __restrict__ ln_flux,
                          const double* __restrict__ ln_err, const double* __restrict__ weight, const double* __restrict__ ext /* or null */,
                          const double* __restrict__ a_v, FitPass pass, FitOrderOut ord,
                          const int* __restrict__ lim_kind /* [n] VAG_OBS_*, or null: no limit row in this pass */,
                          const double* __restrict__ lim_L /* [n] */, const double* __restrict__ lim_sigma /* [n] */,
                          const double* __restrict__ theta /* [nb][ndim] */, int ndim, const double* __restrict__ prior,
                          const double* __restrict__ noise /* [sys_fixed 8 | calib 8] */, const int* __restrict__ grp /* [n] group id or -1 */,
                          unsigned present /* bit g: some row of the pass is in group g */) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    const int walker = pass.order ? pass.order[m] : m;
    const double av = (ext != nullptr) ? a_v[m] : 0.0;
    double s = 0;
    if (grid_ok)
        for (int i = lane; i < n; i += 64) {
            const bool is_lim = lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT;
            if (grp[i] >= 0 && !is_lim) continue;  // a grouped detection: in the turn of its group below
            double f = flux[(size_t)m * n + i];
            if (av != 0.0) f = f * exp(-av * ext[i]);
            if (is_lim) {
                s += weight[i] * (-2.0 * log_ndtr((lim_L[i] - f) / lim_sigma[i]));
                continue;
            }
            const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
            const double q = (ln_flux[i] - log(fm)) / ln_err[i];
            s += weight[i] * (q * q);
        }
    s = wave_sum(s);
    if (grid_ok) {
        const int* slot = reinterpret_cast<const int*>(prior + 64);
        const int* is_log = slot + 16;
        for (int g = 0; g < VAG_NOISE_MAX_GROUPS; ++g) {
            if (!((present >> g) & 1u)) continue;
            double sg = noise[g];
            for (int d = 0; d < ndim; ++d) {
                if (slot[d] != VAG_P_NOISE_SYS0 + g) continue;
                const double v = theta[(size_t)walker * ndim + d];
                sg = is_log[d] ? pow(10.0, v) : v;
            }
            const double s2 = sg * sg, cg = noise[VAG_NOISE_MAX_GROUPS + g];
            double A = 0, B = 0, P = 0, N = 0;
            for (int i = lane; i < n; i += 64) {
                if (grp[i] != g || (lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT)) continue;
                double f = flux[(size_t)m * n + i];
                if (av != 0.0) f = f * exp(-av * ext[i]);
                const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
                const double r = ln_flux[i] - log(fm), sig2 = ln_err[i] * ln_err[i];
                const double p = weight[i] / (sig2 + s2);
                A += p * (r * r);
                B += p * r;
                P += p;
                N += weight[i] * log1p(s2 / sig2);
            }
            A = wave_sum(A);
            N = wave_sum(N);
            double term = A + N;
            if (cg > 0) {  // (wave-uniform) the calibration scale marginalised: a rank-one update of the diagonal covariance
                B = wave_sum(B);
                P = wave_sum(P);
                const double c2 = cg * cg;
                term = A - c2 * (B * B) / (1.0 + c2 * P) + N + log1p(c2 * P);
            }
            s += term;  // (every lane holds the same sums; lane 0 stores)
        }
    }
    fit_close_pass(pass, m, lane, grid_ok, false, s);
}

// The model value of row i of a flux pass with additive templates (vag_loglike_tmpl_batch): with T [.][n] the pass's template block,
// a[c] the walker's amplitudes and bit c of extm the template's `extinguished` flag,
//   e = sum a_c T_c,i over the plain templates, x = sum a_c T_c,i over the extinguished ones (both from 0 in ascending c, one fma per
//   term, only the templates of `present` read),  f = (F + x) exp(-A_V k_i) + e,
// the extinction factor applied exactly where the other back kernels apply it.  The loop over the 8 bits is unrolled: a[] is indexed
// by constants only and stays in registers.  All amplitudes 0: x = e = 0 and f is the other kernels' value, bit for bit.
__device__ __forceinline__ double tmpl_model_value(double F, int i, int n, const double* __restrict__ T, unsigned present, unsigned extm,
                                                   const double (&a)[VAG_TMPL_MAX], double av, const double* __restrict__ ext) {
    double e = 0, x = 0;
#pragma unroll
    for (int c = 0; c < VAG_TMPL_MAX; ++c) {
        if (!((present >> c) & 1u)) continue;
        const double t = T[(size_t)c * n + i];
        if ((extm >> c) & 1u)
            x = fma(a[c], t, x);
        else
            e = fma(a[c], t, e);
    }
    double f = F + x;
    if (av != 0.0) f = f * exp(-av * ext[i]);
    return f + e;
}

// The back of a flux pass with a row that a template touches (vag_loglike_tmpl_batch).  The walker's amplitudes come first, once:
// a_c is the free parameter with the slot VAG_P_TMPL_AMP0 + c (found as the noise kernel finds s_g), else amp_fixed[c], for
// c < n_tmpl; they are wave-uniform.  A free amplitude that is not finite or is negative makes the walker `bad`: it scores -inf and
// is counted like a walker whose vag_pol_spec is refused.  Then the terms of vag_fit_back_kernel<true> and vag_fit_back_noise_kernel,
// statement for statement and in the same lane-strided order, on f_i = tmpl_model_value(...) in place of the model flux; grp is null
// (and gpresent 0) when the pass has no grouped row.  A kernel of its own so that a pass no template touches runs the instructions it
// always ran.
__global__ void __launch_bounds__(64)
vag_fit_back_tmpl_kernel(const double* __restrict__ flux /* [nb][n] */, int n, const double* __restrict__ ln_flux,
                         const double* __restrict__ ln_err, const double* __restrict__ weight, const double* __restrict__ ext /* or null */,
                         const double* __restrict__ a_v, FitPass pass, FitOrderOut ord,
                         const int* __restrict__ lim_kind /* [n] VAG_OBS_*, or null: no limit row in this pass */,
                         const double* __restrict__ lim_L /* [n] */, const double* __restrict__ lim_sigma /* [n] */,
                         const double* __restrict__ theta /* [nb][ndim] */, int ndim, const double* __restrict__ prior,
                         const double* __restrict__ noise /* [sys_fixed 8 | calib 8], or null */,
                         const int* __restrict__ grp /* [n] group id or -1, or null: no grouped row in this pass */,
                         unsigned gpresent /* bit g: some row of the pass is in group g */,
                         const double* __restrict__ tmpl /* [n_tmpl][n] the pass's template values */, int n_tmpl,
                         unsigned tpresent /* bit c: template c touches some row of the pass */,
                         const double* __restrict__ amp_fixed /* [8] */, unsigned extm /* bit c: template c is extinguished */) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    const int walker = pass.order ? pass.order[m] : m;
    const double av = (ext != nullptr) ? a_v[m] : 0.0;
    const int* slot = reinterpret_cast<const int*>(prior + 64);
    const int* is_log = slot + 16;
    double a[VAG_TMPL_MAX];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < VAG_TMPL_MAX; ++c) {
        a[c] = 0.0;
        if (c >= n_tmpl) continue;
        a[c] = amp_fixed[c];
        for (int d = 0; d < ndim; ++d) {
            if (slot[d] != VAG_P_TMPL_AMP0 + c) continue;
            const double v = theta[(size_t)walker * ndim + d];
            a[c] = is_log[d] ? pow(10.0, v) : v;
            bad = bad || !isfinite(a[c]) || a[c] < 0;
        }
    }
    // The rounding of the lane's sum is stated, not left to the compiler, so that all amplitudes 0 is the pass without templates bit
    // for bit: vag_fit_back_kernel<false> (no limit row, no group: a straight-line loop) accumulates with one fma per row,
    // s = fma(w, q^2, s); the kernels whose loop branches on a limit row add the rounded product, s = s + w q^2.
    const bool fused = !lim_kind && !grp;
    double s = 0;
    if (grid_ok)
        for (int i = lane; i < n; i += 64) {
            const bool is_lim = lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT;
            if (grp && grp[i] >= 0 && !is_lim) continue;  // a grouped detection: in the turn of its group below
            const double f = tmpl_model_value(flux[(size_t)m * n + i], i, n, tmpl, tpresent, extm, a, av, ext);
            {
#pragma clang fp contract(off)
                if (is_lim) {
                    s = s + weight[i] * (-2.0 * log_ndtr((lim_L[i] - f) / lim_sigma[i]));
                    continue;
                }
                const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
                const double q = (ln_flux[i] - log(fm)) / ln_err[i];
                s = fused ? fma(weight[i], q * q, s) : s + weight[i] * (q * q);
            }
        }
    s = wave_sum(s);
    if (grid_ok && grp) {
        for (int g = 0; g < VAG_NOISE_MAX_GROUPS; ++g) {
            if (!((gpresent >> g) & 1u)) continue;
            double sg = noise[g];
            for (int d = 0; d < ndim; ++d) {
                if (slot[d] != VAG_P_NOISE_SYS0 + g) continue;
                const double v = theta[(size_t)walker * ndim + d];
                sg = is_log[d] ? pow(10.0, v) : v;
            }
            const double s2 = sg * sg, cg = noise[VAG_NOISE_MAX_GROUPS + g];
            double A = 0, B = 0, P = 0, N = 0;
            for (int i = lane; i < n; i += 64) {
                if (grp[i] != g || (lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT)) continue;
                const double f = tmpl_model_value(flux[(size_t)m * n + i], i, n, tmpl, tpresent, extm, a, av, ext);
                const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
                const double r = ln_flux[i] - log(fm), sig2 = ln_err[i] * ln_err[i];
                const double p = weight[i] / (sig2 + s2);
                A += p * (r * r);
                B += p * r;
                P += p;
                N += weight[i] * log1p(s2 / sig2);
            }
            A = wave_sum(A);
            N = wave_sum(N);
            double term = A + N;
            if (cg > 0) {  // (wave-uniform) the calibration scale marginalised, as in vag_fit_back_noise_kernel
                B = wave_sum(B);
                P = wave_sum(P);
                const double c2 = cg * cg;
                term = A - c2 * (B * B) / (1.0 + c2 * P) + N + log1p(c2 * P);
            }
            s += term;  // (every lane holds the same sums; lane 0 stores)
        }
    }
    fit_close_pass(pass, m, lane, grid_ok, bad, s);
}

// The back of a flux pass that holds a detection row of a robust noise group (vag_loglike_robust_batch; INTEGRATION.md "Outlier
// groups").  It is vag_fit_back_tmpl_kernel statement for statement and in the same lane-strided order -- n_tmpl = 0: no template,
// tmpl and amp_fixed are not read and f_i is the other kernels' value -- but for the group walk: a group whose bit is set in rmask takes
// the single sum R = sum w_i l_i, l_i = robust_row_lnl(...) (vag_robust.h), in place of A, B, P, N and adds -2 wave_sum(R); it has no
// calibration (robust_scan refuses one).  The group's P, b, mu are found as s_g is found: the free parameters with the slots
// VAG_P_ROBUST_FRAC0 / _SCALE0 / _SHIFT0 + g, else robust[g], robust[8 + g], robust[16 + g]; log1p(-P) and ln P are formed once per
// group and are wave-uniform, as is the branch on the group's bit.  A free P that is not finite or lies outside [0, 1), a free b that is
// not finite or is negative and a free mu that is not finite make the walker `bad`, like a refused template amplitude.  A kernel of its
// own so that a pass without such a row runs the instructions it always ran.
__global__ void __launch_bounds__(64)
vag_fit_back_robust_kernel(const double* __restrict__ flux /* [nb][n] */, int n, const double* __restrict__ ln_flux,
                           const double* __restrict__ ln_err, const double* __restrict__ weight, const double* __restrict__ ext /* or null */,
                           const double* __restrict__ a_v, FitPass pass, FitOrderOut ord,
                           const int* __restrict__ lim_kind /* [n] VAG_OBS_*, or null: no limit row in this pass */,
                           const double* __restrict__ lim_L /* [n] */, const double* __restrict__ lim_sigma /* [n] */,
                           const double* __restrict__ theta /* [nb][ndim] */, int ndim, const double* __restrict__ prior,
                           const double* __restrict__ noise /* [sys_fixed 8 | calib 8] */, const int* __restrict__ grp /* [n] group id or -1 */,
                           unsigned gpresent /* bit g: some row of the pass is in group g */,
                           const double* __restrict__ tmpl /* [n_tmpl][n] the pass's template values, or null */, int n_tmpl,
                           unsigned tpresent /* bit c: template c touches some row of the pass */,
                           const double* __restrict__ amp_fixed /* [8], or null */, unsigned extm /* bit c: template c is extinguished */,
                           const double* __restrict__ robust /* [frac_fixed 8 | scale_fixed 8 | shift_fixed 8] */,
                           unsigned rmask /* bit g: group g is robust */) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    const int walker = pass.order ? pass.order[m] : m;
    const double av = (ext != nullptr) ? a_v[m] : 0.0;
    const int* slot = reinterpret_cast<const int*>(prior + 64);
    const int* is_log = slot + 16;
    double a[VAG_TMPL_MAX];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < VAG_TMPL_MAX; ++c) {
        a[c] = 0.0;
        if (c >= n_tmpl) continue;
        a[c] = amp_fixed[c];
        for (int d = 0; d < ndim; ++d) {
            if (slot[d] != VAG_P_TMPL_AMP0 + c) continue;
            const double v = theta[(size_t)walker * ndim + d];
            a[c] = is_log[d] ? pow(10.0, v) : v;
            bad = bad || !isfinite(a[c]) || a[c] < 0;
        }
    }
    double s = 0;
    if (grid_ok)
        for (int i = lane; i < n; i += 64) {
            const bool is_lim = lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT;
            if (grp[i] >= 0 && !is_lim) continue;  // a grouped detection: in the turn of its group below
            const double f = tmpl_model_value(flux[(size_t)m * n + i], i, n, tmpl, tpresent, extm, a, av, ext);
            {
#pragma clang fp contract(off)
                if (is_lim) {
                    s = s + weight[i] * (-2.0 * log_ndtr((lim_L[i] - f) / lim_sigma[i]));
                    continue;
                }
                const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
                const double q = (ln_flux[i] - log(fm)) / ln_err[i];
                s = s + weight[i] * (q * q);
            }
        }
    s = wave_sum(s);
    if (grid_ok) {
        for (int g = 0; g < VAG_NOISE_MAX_GROUPS; ++g) {
            if (!((gpresent >> g) & 1u)) continue;
            const bool rob = (rmask >> g) & 1u;  // (wave-uniform: a kernel argument)
            double sg = noise[g], P = 0, b = 0, mu = 0;
            if (rob) P = robust[g], b = robust[VAG_NOISE_MAX_GROUPS + g], mu = robust[2 * VAG_NOISE_MAX_GROUPS + g];
            for (int d = 0; d < ndim; ++d) {
                const int sl = slot[d];
                const bool mine = sl == VAG_P_NOISE_SYS0 + g ||
                                  (rob && (sl == VAG_P_ROBUST_FRAC0 + g || sl == VAG_P_ROBUST_SCALE0 + g || sl == VAG_P_ROBUST_SHIFT0 + g));
                if (!mine) continue;
                const double v = theta[(size_t)walker * ndim + d];
                const double val = is_log[d] ? pow(10.0, v) : v;
                if (sl == VAG_P_NOISE_SYS0 + g) {
                    sg = val;
                } else if (sl == VAG_P_ROBUST_FRAC0 + g) {
                    P = val;
                    bad = bad || !isfinite(val) || val < 0 || !(val < 1);
                } else if (sl == VAG_P_ROBUST_SCALE0 + g) {
                    b = val;
                    bad = bad || !isfinite(val) || val < 0;
                } else {
                    mu = val;
                    bad = bad || !isfinite(val);
                }
            }
            const double s2 = sg * sg;
            if (rob) {  // (wave-uniform) the mixture: one sum, no calibration
                const double b2 = b * b, ln_good = log1p(-P), ln_bad = log(P);
                double R = 0;
                for (int i = lane; i < n; i += 64) {
                    if (grp[i] != g || (lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT)) continue;
                    const double f = tmpl_model_value(flux[(size_t)m * n + i], i, n, tmpl, tpresent, extm, a, av, ext);
                    const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
                    const double r = ln_flux[i] - log(fm), sig2 = ln_err[i] * ln_err[i];
                    R += weight[i] * robust_row_lnl(r, sig2, s2, b2, mu, ln_good, ln_bad);
                }
                s += -2.0 * wave_sum(R);
                continue;
            }
            const double cg = noise[VAG_NOISE_MAX_GROUPS + g];
            double A = 0, B = 0, Pw = 0, N = 0;
            for (int i = lane; i < n; i += 64) {
                if (grp[i] != g || (lim_kind && lim_kind[i] == VAG_OBS_UPPER_LIMIT)) continue;
                const double f = tmpl_model_value(flux[(size_t)m * n + i], i, n, tmpl, tpresent, extm, a, av, ext);
                const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
                const double r = ln_flux[i] - log(fm), sig2 = ln_err[i] * ln_err[i];
                const double p = weight[i] / (sig2 + s2);
                A += p * (r * r);
                B += p * r;
                Pw += p;
                N += weight[i] * log1p(s2 / sig2);
            }
            A = wave_sum(A);
            N = wave_sum(N);
            double term = A + N;
            if (cg > 0) {  // (wave-uniform) the calibration scale marginalised, as in vag_fit_back_noise_kernel
                B = wave_sum(B);
                Pw = wave_sum(Pw);
                const double c2 = cg * cg;
                term = A - c2 * (B * B) / (1.0 + c2 * Pw) + N + log1p(c2 * Pw);
            }
            s += term;  // (every lane holds the same sums; lane 0 stores)
        }
    }
    fit_close_pass(pass, m, lane, grid_ok, bad, s);
}

// The back of a counts pass (vag_loglike_counts_batch).  flux [nb][ns] holds the walker's band-integrated flux at the group's ns
// sample times; row i gathers its m samples in k order, mu_i = B_i + a_i sum_k F[idx[i m + k]], and adds w_i D(N_i, mu_i)
// (poisson_deviance) to the lane's sum; a row with w_i = 0 adds nothing.  The lanes' sums are closed by wave_sum in the fixed order of
// the other back kernels, so the value depends on the walker's own row of flux alone.  The pass adds 2 sum_i w_i D_i + const2 to
// chi^2, const2 = -2 sum_i w_i S_i being the walker-independent half the host formed (counts_scan).
__global__ void __launch_bounds__(64)
vag_fit_back_counts_kernel(const double* __restrict__ flux /* [nb][ns] */, int ns, int n, int mm, const int* __restrict__ idx /* [n][mm] */,
                           const double* __restrict__ counts, const double* __restrict__ background, const double* __restrict__ scale,
                           const double* __restrict__ weight, double const2, FitPass pass, FitOrderOut ord) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    double s = 0;
    if (grid_ok) {
        const double* f = flux + (size_t)m * ns;
        for (int i = lane; i < n; i += 64) {
            const double w = weight[i];
            if (w == 0.0) continue;
            const int* ix = idx + (size_t)i * mm;
            double sum = 0;
            for (int k = 0; k < mm; ++k) sum += f[ix[k]];
            const double mu = background[i] + scale[i] * sum;
            s += w * poisson_deviance(counts[i], mu);
        }
    }
    s = 2.0 * wave_sum(s) + const2;
    fit_close_pass(pass, m, lane, grid_ok, false, s);
}

// The back of a spectral-index pass (vag_loglike_index_batch).  flux [nb][n K] holds the walker's flux density at the group's points
// (t_i, nu_k), i outer; lane i strides the rows, reads its K consecutive values, forms S_i = log_slope - A_V ext_slope and adds
// w_i ((S_i - s_i) / sigma_i)^2 to the lane's sum; a row with w_i = 0 adds nothing.  A row whose slope is undefined (some F <= 0 or
// not finite) makes the sum NaN, which the last pass turns into -inf and counts.  The lanes' sums are closed by wave_sum in the fixed
// order of the other back kernels, so the value depends on the walker's own row of flux alone.
__global__ void __launch_bounds__(64)
vag_fit_back_index_kernel(const double* __restrict__ flux /* [nb][n K] */, int n, int K, const double* __restrict__ value,
                          const double* __restrict__ err, const double* __restrict__ weight, const double* __restrict__ coef /* [K] */,
                          double ext_slope, const double* __restrict__ a_v, FitPass pass, FitOrderOut ord) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    const double shift = ext_slope != 0.0 ? a_v[m] * ext_slope : 0.0;
    double s = 0;
    if (grid_ok) {
        const double* f = flux + (size_t)m * n * K;
        for (int i = lane; i < n; i += 64) {
            const double w = weight[i];
            if (w == 0.0) continue;
            const double q = (log_slope(f + (size_t)i * K, 1, coef, K) - shift - value[i]) / err[i];
            s += w * (q * q);
        }
    }
    s = wave_sum(s);
    fit_close_pass(pass, m, lane, grid_ok, false, s);
}

// The back of a fold pass (vag_loglike_fold_batch).  flux [nb][ns J] holds the walker's flux density at the group's points
// (t_sample_s, nu_j), s outer.  The walker's N_H is the free parameter with the slot VAG_P_N_H (found as sky_placement finds pa), else
// n_h_fixed; lane j < J keeps T_j = exp(-N_H sigma_j) (1 without sigma).  Row after row: lane j gathers its bin's m samples in s
// order and writes G[i][j] = T_j ((exposure_i / m) sum) to the LDS row; after the barrier the lanes stride the channels, lane c
// running j = 0 .. J-1 over the LDS broadcast and A[j][c] (fold_mu: the wavefront's loads of A are consecutive in c), and adds
// w D(N, mu) (poisson_deviance) to its sum; a channel with w = 0 adds nothing.  The second barrier keeps the next row's writes behind
// this row's reads.  The lanes' sums are closed by wave_sum in the fixed order of the other back kernels, so the value depends on
// the walker's own row of flux alone.  The pass adds 2 sum w D + const2 to chi^2, const2 the walker-independent half the host
// formed (fold_scan).  One wavefront per block: the barriers are wave-uniform (grid_ok and the row loop are).
__global__ void __launch_bounds__(64)
vag_fit_back_fold_kernel(const double* __restrict__ flux /* [nb][ns J] */, int ns, int J, int C, int n, int mm,
                         const int* __restrict__ idx /* [n][mm] */, const double* __restrict__ A /* [J][C] */,
                         const double* __restrict__ sigma /* [J] or null */, const double* __restrict__ eom /* [n] exposure / m */,
                         const double* __restrict__ counts /* [n][C] */, const double* __restrict__ background,
                         const double* __restrict__ weight, double const2, const double* __restrict__ theta /* [nb][ndim] */, int ndim,
                         const double* __restrict__ prior, double n_h_fixed, FitPass pass, FitOrderOut ord) {
    __shared__ double s_g[FOLD_MAX_BINS];
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    double s = 0;
    if (grid_ok) {
        double T = 1.0;
        if (sigma != nullptr && lane < J) {
            const int walker = pass.order ? pass.order[m] : m;
            const int* slot = reinterpret_cast<const int*>(prior + 64);
            const int* is_log = slot + 16;
            double nh = n_h_fixed;
            for (int d = 0; d < ndim; ++d) {
                if (slot[d] != VAG_P_N_H) continue;
                const double v = theta[(size_t)walker * ndim + d];
                nh = is_log[d] ? pow(10.0, v) : v;
            }
            T = exp(-(nh * sigma[lane]));
        }
        const double* f = flux + (size_t)m * ns * J;
        for (int i = 0; i < n; ++i) {
            if (lane < J) {
                const int* ix = idx + (size_t)i * mm;
                double sum = 0;
                for (int k = 0; k < mm; ++k) sum += f[(size_t)ix[k] * J + lane];
                s_g[lane] = T * (eom[i] * sum);
            }
            __syncthreads();
            for (int c = lane; c < C; c += 64) {
                const size_t at = (size_t)i * C + c;
                const double w = weight[at];
                if (w == 0.0) continue;
                s += w * poisson_deviance(counts[at], fold_mu(background[at], A + c, C, s_g, J));
            }
            __syncthreads();
        }
    }
    s = 2.0 * wave_sum(s) + const2;
    fit_close_pass(pass, m, lane, grid_ok, false, s);
}

// The back of a correlated group's pass (vag_loglike_cov_batch).  flux [nb][n] holds the walker's flux density at the group's rows.
// Phase 1: the lanes stride the rows and write r_i = ln F_obs,i - ln max(F_i e^{-A_V k_i}, 1e-300) (the statements of
// vag_fit_back_kernel: a NaN stays NaN) to the LDS row.  Phase 2, behind the barrier: lane l takes the rows i = l, l + 64, ... in
// ascending order and forms y_i = sum_{j=0..i} W_ij r_j from 0 in ascending j with one fma per term, r_j the LDS broadcast and W_ij
// read from the transposed copy Wt[j n + i] (the wavefront's loads are consecutive doubles), then s = fma(y_i, y_i, s).  The j loop
// is wave-uniform: it runs to the largest row of the wavefront's block of 64, and a lane keeps its y where j > i (a select, not a
// product with the stored zero: the value is that of a loop to the lane's own i, whatever r_j holds); a lane past n reads row n - 1
// and keeps nothing.  The lanes' sums are closed by wave_sum in the fixed order of the other back kernels, so the value depends on
// the walker's own row of flux alone; the pass adds w sum y^2, and 0 without reading a row when w = 0.  One wavefront per block: the
// barrier is wave-uniform (grid_ok and w are).
__global__ void __launch_bounds__(64)
vag_fit_back_cov_kernel(const double* __restrict__ flux /* [nb][n] */, int n, const double* __restrict__ ln_flux,
                        const double* __restrict__ ext /* [n] or null */, const double* __restrict__ Wt /* [n][n]: Wt[j n + i] = W_ij */,
                        double w, const double* __restrict__ a_v, FitPass pass, FitOrderOut ord) {
    __shared__ double s_r[VAG_COV_MAX_ROWS];
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    fit_hand_over_order(pass, ord, m, lane);
    const double av = (ext != nullptr) ? a_v[m] : 0.0;
    double s = 0;
    if (grid_ok && w != 0.0) {  // (w = 0: the pass's validity alone, the term is 0)
        for (int i = lane; i < n; i += 64) {
            double f = flux[(size_t)m * n + i];
            if (av != 0.0) f = f * exp(-av * ext[i]);
            const double fm = (f != f) ? f : (f > 1e-300 ? f : 1e-300);
            s_r[i] = ln_flux[i] - log(fm);
        }
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < n;
            const double* col = Wt + (on ? i : n - 1);
            const int j_end = min(i0 + 64, n);  // one past the block's largest row
            double y = 0;
#pragma unroll 4
            for (int j = 0; j < j_end; ++j) {
                const double yj = fma(col[(size_t)j * n], s_r[j], y);
                y = j <= i ? yj : y;
            }
            s = on ? fma(y, y, s) : s;
        }
    }
    s = w * wave_sum(s);
    fit_close_pass(pass, m, lane, grid_ok, false, s);
}

// The back of one centroid pass: the walker's sky placement (free parameters with slots VAG_P_SKY_*, else the fixed values), the
// group's chi^2 term, and its own validity condition -- F > 0 and finite moments at every epoch.
__global__ void __launch_bounds__(64)
vag_fit_sky_back_kernel(const double* __restrict__ mom /* [nb][n][6] */, int n, const double* __restrict__ obs /* [t|e|n|ee|en|w] */,
                        const double* __restrict__ theta, int ndim, const double* __restrict__ prior, double pa_fixed, double east0_fixed,
                        double north0_fixed, FitPass pass) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const int walker = pass.order ? pass.order[m] : m;
    double pa = pa_fixed, e0 = east0_fixed, n0 = north0_fixed;
    sky_placement(theta, walker, ndim, prior, pa, e0, n0);
    double sp, cp;
    sincos(pa, &sp, &cp);
    const double *e_obs = obs + n, *n_obs = obs + 2 * (size_t)n, *e_err = obs + 3 * (size_t)n, *n_err = obs + 4 * (size_t)n,
                 *w = obs + 5 * (size_t)n;
    const bool grid_ok = pass.meta[m].status == 0;
    double s = 0;
    bool bad = false;
    if (grid_ok)
        for (int i = lane; i < n; i += 64) {
            const double* mo = mom + ((size_t)m * n + i) * 6;
            const double F = mo[0], X = mo[1], Y = mo[2];
            bad = bad || !(F > 0) || !isfinite(F) || !isfinite(X) || !isfinite(Y);
            const double east = e0 + (X * sp + Y * cp), north = n0 + (X * cp - Y * sp);
            const double qe = (e_obs[i] - east) / e_err[i], qn = (n_obs[i] - north) / n_err[i];
            s += w[i] * (qe * qe + qn * qn);
        }
    s = wave_sum(s);
    fit_close_pass(pass, m, lane, grid_ok, bad, s);
}

// The back of one visibility pass: the walker's block partials in a fixed order (lane-strided, then the wavefront sum), and its own
// validity condition -- finite V_mod at every datum.  A model with no flux is valid: its V_mod is 0.
__global__ void __launch_bounds__(64)
vag_fit_vis_back_kernel(const double* __restrict__ partial /* [nb][n_blk][2] */, int n_blk, FitPass pass) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const bool grid_ok = pass.meta[m].status == 0;
    double s = 0;
    bool bad = false;
    if (grid_ok)
        for (int i = lane; i < n_blk; i += 64) {
            const double* p = partial + ((size_t)m * n_blk + i) * 2;
            s += p[0];
            bad = bad || p[1] != 0.0;
        }
    s = wave_sum(s);
    fit_close_pass(pass, m, lane, grid_ok, bad, s);
}

// The walkers' polarization spec, one thread per evaluation slot: spec[m] = {b - 1 of the forward, reverse shock, Pi_max of the forward,
// reverse shock} as pol_spec() resolves a vag_pol_spec -- free parameters with the slots VAG_P_POL_*, else the fixed values; a reverse
// b that is neither free nor given (< 0) follows the walker's forward b; a Pi_max < 0 is (p + 1) / (p + 7/3) with the p of the walker's
// transformed parameters.  bad[m] = 1 where pol_spec() would refuse the walker (its spec is then 0: unpolarized, never read back).
__global__ void __launch_bounds__(128)
vag_fit_pol_spec_kernel(const double* __restrict__ theta, int nb, int ndim, const double* __restrict__ prior,
                        const vag_model_params* __restrict__ params, double b0, double b1, double pm0, double pm1,
                        const int* __restrict__ order, double* __restrict__ spec, int* __restrict__ bad) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nb) return;
    const int walker = order ? order[m] : m;
    const int* slot = reinterpret_cast<const int*>(prior + 64);
    const int* is_log = slot + 16;
    bool b1_given = !(b1 < 0);
    for (int d = 0; d < ndim; ++d) {
        const int sl = slot[d];
        if (sl < VAG_P_POL_B || sl > VAG_P_POL_PI_MAX_RVS) continue;
        const double v = theta[(size_t)walker * ndim + d];
        const double val = is_log[d] ? pow(10.0, v) : v;
        b0 = sl == VAG_P_POL_B ? val : b0;  // (selects, as in sky_placement)
        pm0 = sl == VAG_P_POL_PI_MAX ? val : pm0;
        b1 = sl == VAG_P_POL_B_RVS ? val : b1;
        pm1 = sl == VAG_P_POL_PI_MAX_RVS ? val : pm1;
        b1_given = b1_given || sl == VAG_P_POL_B_RVS;
    }
    if (!b1_given) b1 = b0;
    const bool ok = isfinite(b0) && b0 >= 0 && isfinite(b1) && b1 >= 0 && !(pm0 != pm0) && !(pm0 > 1) && !(pm1 != pm1) && !(pm1 > 1);
    const double p0 = params[m].p, p1 = params[m].rvs_p;
    if (pm0 < 0) pm0 = (p0 + 1) / (p0 + 7.0 / 3.0);
    if (pm1 < 0) pm1 = (p1 + 1) / (p1 + 7.0 / 3.0);
    double* o = spec + 4 * (size_t)m;
    o[0] = ok ? b0 - 1 : 0.0;
    o[1] = ok ? b1 - 1 : 0.0;
    o[2] = ok ? pm0 : 0.0;
    o[3] = ok ? pm1 : 0.0;
    bad[m] = ok ? 0 : 1;
}

// The back of one polarization pass: the walker's position angle (the free parameter with the slot VAG_P_SKY_PA, else the fixed
// value), the turn of the jet-frame Q, U by 2 pa, the residuals of up to 64 epochs at a time, one per lane, added in epoch order, and
// its own validity condition -- a valid spec, I > 0 and finite I, Q, U at every epoch.  A DEGREE group reads hypot(Q, U) of the jet
// frame: the position angle does not enter.
// LIM, for a DEGREE group with upper-limit epochs (vag_loglike_lim_batch): an epoch with lim_kind[i] == VAG_OBS_UPPER_LIMIT adds
// -2 w_i ln Phi((q_i - hypot(Q, U) / I) / err_q_i) instead of its detection term (q holds the limit, err_q its noise level); the
// I <= 0 rule stays.  A compile-time flag, so that a group without limit epochs runs the instructions it always ran; lim_kind is not
// read then.
template <bool LIM>
__global__ void __launch_bounds__(64)
vag_fit_pol_back_kernel(const double* __restrict__ stokes /* [nb][n][3] jet frame */, int n, int kind,
                        const double* __restrict__ obs /* [t|q|u|eq|eu|w] */, const int* __restrict__ spec_bad,
                        const double* __restrict__ theta, int ndim, const double* __restrict__ prior, double pa_fixed, FitPass pass,
                        const int* __restrict__ lim_kind /* [n] VAG_OBS_* */) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const int walker = pass.order ? pass.order[m] : m;
    double pa = pa_fixed, e0 = 0, n0 = 0;
    sky_placement(theta, walker, ndim, prior, pa, e0, n0);
    double s2, c2;
    sincos(2 * pa, &s2, &c2);
    const double *q_obs = obs + n, *u_obs = obs + 2 * (size_t)n, *q_err = obs + 3 * (size_t)n, *u_err = obs + 4 * (size_t)n,
                 *w = obs + 5 * (size_t)n;
    const bool grid_ok = pass.meta[m].status == 0;
    double s = 0;
    bool bad = spec_bad[m] != 0;
    if (grid_ok)
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane, cnt = min(64, n - i0);
            double term = 0;
            if (i < n) {
                const double* sk = stokes + ((size_t)m * n + i) * 3;
                const double I = sk[0], Q = sk[1], U = sk[2];
                bad = bad || !(I > 0) || !isfinite(I) || !isfinite(Q) || !isfinite(U);
                if (kind == VAG_POL_DEGREE) {
                    const double r = (q_obs[i] - hypot(Q, U) / I) / q_err[i];
                    if constexpr (LIM)
                        term = w[i] * (lim_kind[i] == VAG_OBS_UPPER_LIMIT ? -2.0 * log_ndtr(r) : r * r);
                    else
                        term = w[i] * (r * r);
                } else {
                    const double Qs = Q * c2 - U * s2, Us = Q * s2 + U * c2;
                    const double rq = (q_obs[i] - Qs / I) / q_err[i], ru = (u_obs[i] - Us / I) / u_err[i];
                    term = w[i] * (rq * rq + ru * ru);
                }
            }
            for (int j = 0; j < cnt; ++j) s += wave_bcast(term, j);  // every lane: the epochs in order
        }
    fit_close_pass(pass, m, lane, grid_ok, bad, s);
}

}  // namespace vag
