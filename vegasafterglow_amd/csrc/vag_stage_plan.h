// vag_stage_plan.h -- the arithmetic of the model stages (run_model_stages, finish_speculation) and of the split of a batch by
// flags: what a planned-ahead call is sized for and when it has to be repeated, which dynamics kernel takes a batch with how many
// rows per wavefront, where the refill kernel's arrays lie in d_dynrec, and which models form a group.  Integer arithmetic on the
// numbers of a batch summary (VagDevPlan) and the hooks, which come in parsed as FluxHooks does it.
// Plain C++17: no device header, no context, no environment access, no HIP call -- a host compiler builds it, and
// tests/stage_plan_check.cpp holds every threshold at the value and on each side of it.  vag_capi.hip keeps the launches, the
// allocations and the context updates.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vag_common.h"
#include "vag_flux_plan.h"  // HOOK_UNSET, hook_set

namespace vag {

// VAG_FLAG_* a batch summary stands for (flags_first is -1 where no model is valid)
inline int plan_flags(const VagDevPlan& p) { return p.flags_first < 0 ? 0 : p.flags_first; }

// ---- planning ahead (VAG_PLAN_AHEAD): a call sized from the previous call's summary, verified at its end ----

// same batch size as the hint, a valid hint, no details, the hook and the caller's switch on
inline bool may_plan_ahead(bool hook_on, bool allowed, bool want_details, bool hint_valid, int hint_nb, int nb) {
    return hook_on && allowed && !want_details && hint_valid && hint_nb == nb;
}

// what the grid kernel may hand out before it reports an overflow; the defaults are those of a call that waits for its summary
struct StageCaps {
    int rows = INT32_MAX, k = INT32_MAX, pairs = INT32_MAX;
    long long cells = INT64_MAX;
};
inline StageCaps plan_ahead_caps(const VagDevPlan& hint, int margin_k) {
    StageCaps c;
    c.rows = hint.rows + hint.rows / 4 + 64;
    c.cells = hint.cells + hint.cells / 4 + 4096;
    c.k = std::min(VAG_MAX_TIME, hint.max_k + margin_k);  // LDS of the flux kernels scales with it: keep it tight
    c.pairs = hint.max_pairs + hint.max_pairs / 2 + 64;
    return c;
}

// The end of a planned-ahead call.  repeat: a capacity was exceeded (the device then skipped every model), the batch mixes flags,
// or its flags / dynamics class are not the hint's.  margin_k: the lattice head room of the next planned-ahead calls -- more where
// the lattice outgrew the one this call had.
struct PlanVerdict {
    bool repeat;
    int margin_k;
};
inline PlanVerdict plan_ahead_verdict(const VagDevPlan& got, const VagDevPlan& hint, int cap_k, int margin_k) {
    const bool repeat = got.overflow || got.flags_mixed ||
                        (got.n_ok > 0 && (plan_flags(got) != plan_flags(hint) || got.dyn_class != hint.dyn_class));
    const bool grow = repeat && got.overflow && got.max_k > cap_k;
    return {repeat, grow ? std::min(32, 2 * margin_k + 2) : margin_k};
}

// ---- the dynamics stage ----

struct DynHooks {
    int general = HOOK_UNSET;      // VAG_DYN_GENERAL (switch): the general solver also where the fast one applies
    int refill = HOOK_UNSET;       // VAG_DYN_REFILL: 0 / not 0 forces the plain / the refill form of the fast solver
    int refill_min = HOOK_UNSET;   // VAG_DYN_REFILL_MIN: finished lanes a wavefront collects before it takes new rows, 1..64
    int refill_wgs = HOOK_UNSET;   // VAG_DYN_REFILL_WGS: workgroups of the refill kernel, at least 1
    int pair_rpw = HOOK_UNSET;     // VAG_PAIR_RPW: > 0 overrides the pair solver's rows per wavefront, at most 64
    int dyn_rpw = HOOK_UNSET;      // VAG_DYN_RPW: the same for the fast and the general solver
};

// ODE rows per wavefront of the dynamics kernels (one lane integrates one row).  Measured (profiles/r02_rpw.txt): fewer
// rows per wavefront do NOT pay for the general kernel -- at 256 VGPRs only one wavefront fits a SIMD and the dispatcher
// does not spread single-wavefront workgroups evenly -- so full wavefronts stay the default; the knob remains for tuning.
// The coupled forward + reverse shock solver keeps its retry loop inside the step (a wavefront repeats an attempt while ANY of its
// lanes rejects) and one wavefront fills a SIMD (256 VGPRs): fewer rows per wavefront mean fewer repeated attempts and -- while the
// batch has fewer wavefronts than the chip has SIMDs -- more SIMDs at work.  The general solver retries inside the step likewise.
inline int pair_rows_per_wave(int rows, int hook) {
    if (hook_set(hook) && hook > 0) return std::min(hook, 64);
    // Measured (profiles/debug/pair_rpw_probe.py: one configs[2] model = 65 rows / 512 models = 33 k rows; general_rpw_probe.py: one
    // spreading Gaussian jet = 49 rows / 256 of them = 12.5 k rows; same bits whatever the choice): 64 rows per wavefront 3.18 / 3.48 ms
    // and 1.85 / 1.98 ms, 32: 2.83 / 5.35 and 1.57 / 2.28, 16: 2.68 / 5.89 and 1.77 / 2.30, 8: 2.32 / 16.3 and 1.41 / 4.36 -- fewer rows pay
    // for a handful of models and cost as soon as there are a few hundred wavefronts (a 256-VGPR wavefront owns its SIMD and the
    // dispatcher does not spread them evenly), so only small batches are split up.
    for (int rpw = 8; rpw < 64; rpw *= 2)
        if ((rows + rpw - 1) / rpw <= 64) return rpw;
    return 64;
}
inline int dyn_rows_per_wave(int hook) { return hook_set(hook) && hook > 0 ? std::min(hook, 64) : 64; }

enum DynFamily {
    DYN_PAIR,     // vag_dynamics_pair_kernel: both shocks from one ODE state per row (VAG_FLAG_RVS)
    DYN_FAST,     // vag_dynamics_fast_kernel: the common case, flat attempt loop, raw saves
    DYN_REFILL,   // vag_dynamics_refill_kernel: the fast solver, persistent, its lanes refilled from a row queue
    DYN_GENERAL   // vag_dynamics_kernel<spreading, inject>
};
struct DynPlan {
    DynFamily family;
    bool spreading, inject;  // VAG_FLAG_SPREADING / VAG_FLAG_MAGNETAR of the batch (the general solver's two switches)
    int rows_per_wave;       // of the pair, fast and general kernel (the refill kernel's wavefronts are full)
    int refill_min;          // DYN_REFILL: finished lanes a wavefront collects before it takes new rows
};
// Batches beyond one and a half rounds of the plain fast kernel's integrator slots (four two-wavefront workgroups per CU) take the
// persistent kernel whose lanes refill from a row queue and save inline (two integrators per SIMD instead of one integrator and
// its saver); smaller ones keep the plain kernel, which is built for the latency of one row (no preparation pass on the chain).
// Measured (profiles/r06_refill_probe.txt, C4 walkers, ODE stage plain / refill): 53.9 k rows 0.37 / 0.41 ms, 108.6 k rows
// 0.72 / 0.62, 218 k rows 1.22 / 0.89, 433.8 k rows 2.28 / 1.73.  VAG_DYN_REFILL=0 / 1 forces either; same bits
// (tests/test_gpu_parity.py).  refill_min 1 / 4 / 8 / 16: 1.97 / 1.80 / 1.80 / 1.73 ms per 8192 walkers (a refill is ~200
// instructions for the whole wavefront).
inline DynPlan dyn_plan(int batch_flags, int dyn_class, int rows, int n_cus, const DynHooks& h) {
    DynPlan p{DYN_GENERAL, (batch_flags & VAG_FLAG_SPREADING) != 0, (batch_flags & VAG_FLAG_MAGNETAR) != 0, 64, 16};
    if (batch_flags & VAG_FLAG_RVS) {
        p.family = DYN_PAIR;
        p.rows_per_wave = pair_rows_per_wave(rows, h.pair_rpw);
    } else if (dyn_class == 0 && !hook_set(h.general)) {
        const bool refill = hook_set(h.refill) ? h.refill != 0 : rows >= 96 * 4LL * n_cus;
        p.family = refill ? DYN_REFILL : DYN_FAST;
        p.rows_per_wave = dyn_rows_per_wave(h.dyn_rpw);
        if (hook_set(h.refill_min)) p.refill_min = std::max(1, std::min(64, h.refill_min));
    } else {
        p.rows_per_wave = pair_rows_per_wave(rows, h.dyn_rpw);
    }
    return p;
}

// workgroups (one wavefront each) of the refill kernel: what stays resident, no more than there are wavefronts of rows
inline unsigned refill_workgroups(int rows, int wg_per_cu, int n_cus, int hook) {
    const long long slots = hook_set(hook) ? std::max(1, hook) : (long long)wg_per_cu * n_cus;
    return (unsigned)std::max<long long>(1, std::min<long long>((rows + 63) / 64, slots));
}

// d_dynrec of the refill form, in bytes from its start: the start records (at 0) | the sorted queue (rows ints, an even number of
// them) | the queue's two counters (16 bytes) | histogram / offsets [buckets][chunks] | length class per row (a byte each)
struct DynRecShape {
    int rowrec, buckets, chunk;  // DYN_ROWREC doubles per record, DYN_BUCKETS, DYN_CHUNK rows per chunk (vag_dyn_fast.h)
};
struct DynRecLayout {
    size_t n_chunks, order, queue, hist, cls, bytes;
};
inline DynRecLayout dynrec_layout(int rows, const DynRecShape& s) {
    DynRecLayout l;
    l.n_chunks = ((size_t)rows + s.chunk - 1) / s.chunk;
    l.order = sizeof(double) * (size_t)rows * s.rowrec;
    l.queue = l.order + sizeof(int) * (((size_t)rows + 1) & ~(size_t)1);
    l.hist = l.queue + 16;
    l.cls = l.hist + sizeof(unsigned) * s.buckets * l.n_chunks;
    l.bytes = l.cls + (size_t)rows;
    return l;
}

// ---- a batch whose models differ in their flags: the models of every flag set, the sets in the order in which they are first
//      seen, the models of a set in batch order.  flags_of(m): VAG_FLAG_* of model m. ----
template <class FlagsOf>
inline std::vector<std::vector<int>> group_by_flags(int nb, FlagsOf flags_of) {
    std::vector<int> keys;
    std::vector<std::vector<int>> groups;
    for (int m = 0; m < nb; ++m) {
        const int f = flags_of(m);
        size_t g = 0;
        while (g < keys.size() && keys[g] != f) ++g;
        if (g == keys.size()) {
            keys.push_back(f);
            groups.emplace_back();
        }
        groups[g].push_back(m);
    }
    return groups;
}

}  // namespace vag
