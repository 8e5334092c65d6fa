// vag_sampler_plan.h -- the host side of the device sampler between "an entry point was called" and "a kernel is in the queue": what
// the four specs (stretch move, move mix, parallel tempering, nested sampling) refuse, the kind of a step of the mix, what a run entry refuses of its
// arguments, and the integer arithmetic the launchers and the step loop share -- the seed's halves, the half, workgroups, stored
// rows, exchange pairs, row offsets.  Plain C++17: no device header, no context, no allocation -- a host compiler builds it, and
// tests/sampler_plan_check.cpp holds every decision at its threshold and on each side of it.  vag_capi.hip keeps the locks, the
// launches and the step loop.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "vag_fit_request.h"  // set_err
#include "vag_moves.h"        // move_choice, move_choice_uniform
#include "vag_nested.h"       // VAG_NESTED_MAX_LIVE_POINTS
#include "vag_tempering.h"    // TemperLadder

namespace vag {

static_assert(VAG_MOVE_STRETCH == MOVE_STRETCH && VAG_MOVE_DE == MOVE_DE && VAG_MOVE_SNOOKER == MOVE_SNOOKER, "the public kinds are the header's");
static_assert(VAG_TEMPER_MAX == VAG_TEMPER_MAX_RUNGS, "the public ladder limit is the kernels'");
static_assert(VAG_NESTED_MAX_LIVE == VAG_NESTED_MAX_LIVE_POINTS, "the public live-point limit is the kernels'");

// ---- what the specs refuse ----

// the shape every spec shares; the other two specs inherit the texts with their "stretch move:" prefix
inline int ensemble_check(int ndim, int n_walkers, double a, int thin) {
    if (ndim < 1 || ndim > 16) return set_err(VAG_E_INVALID, "stretch move: ndim must be 1..16, got %d", ndim);
    if (n_walkers < 2 * ndim || (n_walkers & 1))
        return set_err(VAG_E_INVALID, "stretch move: need an even number of walkers, at least 2 * ndim = %d, got %d", 2 * ndim, n_walkers);
    if (!std::isfinite(a) || !(a > 1.0)) return set_err(VAG_E_INVALID, "stretch move: the scale a must be finite and > 1, got %g", a);
    if (thin < 1) return set_err(VAG_E_INVALID, "stretch move: thin must be >= 1, got %d", thin);
    return VAG_OK;
}

inline int stretch_spec_check(const vag_stretch_spec* sp) { return ensemble_check(sp->ndim, sp->n_walkers, sp->a, sp->thin); }  // (not null)

inline int move_spec_check(const vag_move_spec* sp) {  // (not null)
    if (const int rc = ensemble_check(sp->ndim, sp->n_walkers, sp->a, sp->thin)) return rc;
    double sum = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(sp->weights[k]) || sp->weights[k] < 0.0)
            return set_err(VAG_E_INVALID, "move mix: weight %d must be finite and >= 0, got %g", k, sp->weights[k]);
        sum += sp->weights[k];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return set_err(VAG_E_INVALID, "move mix: the weights must have a finite sum > 0");
    const int half = sp->n_walkers / 2;
    if (sp->weights[MOVE_DE] > 0.0 && half < 2)
        return set_err(VAG_E_INVALID, "move mix: the DE move needs two walkers of the other half, n_walkers >= 4, got %d", sp->n_walkers);
    if (sp->weights[MOVE_SNOOKER] > 0.0 && half < 3)
        return set_err(VAG_E_INVALID, "move mix: the snooker move needs three walkers of the other half, n_walkers >= 6, got %d", sp->n_walkers);
    if (!std::isfinite(sp->gamma0) || sp->gamma0 < 0.0)
        return set_err(VAG_E_INVALID, "move mix: gamma0 must be finite and >= 0 (0: 2.38 / sqrt(2 ndim)), got %g", sp->gamma0);
    if (!std::isfinite(sp->sigma)) return set_err(VAG_E_INVALID, "move mix: sigma must be finite, got %g", sp->sigma);
    if (!std::isfinite(sp->gamma_snooker)) return set_err(VAG_E_INVALID, "move mix: gamma_snooker must be finite, got %g", sp->gamma_snooker);
    return VAG_OK;
}

// the checks of a tempered spec (not null); fills the ladder the kernels take by value, zero beyond n_temps
inline int tempered_spec_check(const vag_tempered_spec* sp, TemperLadder& ladder) {
    if (const int rc = ensemble_check(sp->ndim, sp->n_walkers, sp->a, sp->thin)) return rc;
    if (sp->n_temps < 1 || sp->n_temps > VAG_TEMPER_MAX)
        return set_err(VAG_E_INVALID, "tempering: n_temps must be 1..%d, got %d", VAG_TEMPER_MAX, sp->n_temps);
    if ((long long)sp->n_temps * sp->n_walkers > (1ll << 30))
        return set_err(VAG_E_INVALID, "tempering: n_temps * n_walkers must not exceed 2^30, got %lld", (long long)sp->n_temps * sp->n_walkers);
    if (!sp->betas) return set_err(VAG_E_INVALID, "tempering: null betas");
    if (sp->betas[0] != 1.0) return set_err(VAG_E_INVALID, "tempering: betas[0] must be 1, got %g", sp->betas[0]);
    for (int t = 0; t < VAG_TEMPER_MAX; ++t) ladder.beta[t] = 0.0;
    for (int t = 0; t < sp->n_temps; ++t) {
        const double b = sp->betas[t];
        if (!std::isfinite(b) || b < 0.0 || (t > 0 && !(b < sp->betas[t - 1])))
            return set_err(VAG_E_INVALID, "tempering: betas must be finite, strictly descending and >= 0; betas[%d] = %g", t, b);
        ladder.beta[t] = b;
    }
    return VAG_OK;
}

// the checks of a nested spec (not null)
inline int nested_spec_check(const vag_nested_spec* sp) {
    if (sp->ndim < 1 || sp->ndim > 16) return set_err(VAG_E_INVALID, "nested sampling: ndim must be 1..16, got %d", sp->ndim);
    if (sp->n_live < 4 || sp->n_live > VAG_NESTED_MAX_LIVE || (sp->n_live & 1))
        return set_err(VAG_E_INVALID, "nested sampling: need an even number of live points, 4..%d, got %d", VAG_NESTED_MAX_LIVE, sp->n_live);
    if (sp->walk < 1) return set_err(VAG_E_INVALID, "nested sampling: walk must be >= 1, got %d", sp->walk);
    if (!std::isfinite(sp->gamma0) || sp->gamma0 < 0.0)
        return set_err(VAG_E_INVALID, "nested sampling: gamma0 must be finite and >= 0 (0: 2.38 / sqrt(2 ndim)), got %g", sp->gamma0);
    if (!std::isfinite(sp->sigma)) return set_err(VAG_E_INVALID, "nested sampling: sigma must be finite, got %g", sp->sigma);
    return VAG_OK;
}

// the walk step of a nested building block: 1 .. walk (0 is the clone draw, which retire makes)
inline int nested_walk_step_check(const vag_nested_spec* sp, int m) {
    if (m < 1 || m > sp->walk) return set_err(VAG_E_INVALID, "nested sampling: the walk step m must be 1..walk = %d, got %d", sp->walk, m);
    return VAG_OK;
}

// `who`: "stretch move", "move mix" or "tempering", the prefix of the entry's own refusals
inline int half_check(const char* who, int half) {
    if (half != 0 && half != 1) return set_err(VAG_E_INVALID, "%s: half must be 0 or 1, got %d", who, half);
    return VAG_OK;
}

// ---- what a run entry refuses of its arguments: before the spec's checks, the chain pointers (`set` of them are not null; `what`
//      names them: "the chain and its ln p"), which come all or none; behind them, ndim against the fit spec's and n_steps ----

inline int run_chain_check(const char* who, const char* what, int set, int of) {
    if (set != 0 && set != of) return set_err(VAG_E_INVALID, "%s: %s are stored together or not at all", who, what);
    return VAG_OK;
}

inline int run_steps_check(const char* who, int ndim, int fit_ndim, int n_steps) {
    if (ndim != fit_ndim) return set_err(VAG_E_INVALID, "%s: ndim %d is not the fit spec's %d", who, ndim, fit_ndim);
    if (n_steps < 0) return set_err(VAG_E_INVALID, "%s: n_steps must be >= 0, got %d", who, n_steps);
    return VAG_OK;
}

// ---- the phases of a step of the shared step loop: each is propose, ONE likelihood call, accept ----

constexpr int HALF_PHASES = 2;  // the three moves: half 0, then half 1
inline int nested_phases(const vag_nested_spec* sp) { return sp->walk; }  // nested sampling: the walk steps m = phase + 1

// ---- the kind of `step` of the mix, chosen on the host: the kernels do not branch on it ----

struct SeedWords {  // the Philox key of a seed
    uint32_t lo, hi;
};
inline SeedWords seed_words(uint64_t seed) { return {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)}; }

inline int move_kind(const vag_move_spec* sp, uint64_t step) {
    const SeedWords key = seed_words(sp->seed);
    const double u = move_choice_uniform(key.lo, key.hi, (unsigned long long)step);
    return move_choice(u, sp->weights[MOVE_STRETCH], sp->weights[MOVE_DE], sp->weights[MOVE_SNOOKER]);
}

// ---- the arithmetic of the launchers and of the step loop ----

inline int half_of(int n_walkers) { return n_walkers / 2; }  // walkers of a half (n_walkers is even)

inline unsigned lane_groups(long long items) { return (unsigned)((items + STRETCH_LANES - 1) / STRETCH_LANES); }  // one lane per item

inline bool step_is_stored(uint64_t step, int thin) { return (step + 1) % (uint64_t)thin == 0; }

// the exchange pairs (t, t + 1) of `step`: those with t + step even
inline int swap_pairs(int n_temps, uint64_t step) { return (n_temps - (int)(step & 1u)) / 2; }

// the element offset of stored row `row`: of an array [rows][n_walkers][width] (a plain ensemble) and [rows][n_temps][n_walkers][width]
// (a ladder); width is ndim for positions and 1 for ln p, ln L and ln prior
inline size_t ensemble_row_offset(size_t row, int n_walkers, int width) { return row * (size_t)n_walkers * (size_t)width; }
inline size_t ladder_row_offset(size_t row, int n_temps, int n_walkers, int width) {
    return row * ((size_t)n_temps * (size_t)n_walkers) * (size_t)width;
}
// of the dead record and the counts of nested sampling, [rows][n_live / 2][width]: an iteration retires half the live points
inline size_t dead_row_offset(size_t row, int n_live, int width) { return ensemble_row_offset(row, half_of(n_live), width); }

}  // namespace vag
