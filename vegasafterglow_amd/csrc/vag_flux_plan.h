// vag_flux_plan.h -- the decisions between "the model stages have run" and "a flux kernel is in the queue": which kernel family and
// variant takes a request, with how many rows per workgroup, whether the launch goes persistent, split or fused.  Every one is integer
// arithmetic on a dozen numbers of the batch, the request and the hooks; the thresholds are measured ones (vag_flux_limits.h).
// Plain C++17: no device header, no context, no environment access, no allocation -- a host compiler builds it, and
// tests/flux_plan_check.cpp holds every threshold at the value and on each side of it.  LDS sizes and occupancy figures come in as
// numbers, computed next to the kernels; vag_capi.hip, the one translation unit of the library, maps the variants to kernels.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>

#include "vag_flux_limits.h"

namespace vag {

constexpr size_t CU_LDS_BYTES = 160 * 1024;  // LDS of a CU: the most a workgroup can ask for

// the numbers of the context's current batch the decisions read
struct FluxBatch {
    int nb = 0;       // models
    int n_rows = 0;   // (theta, phi) rows with work (0: nothing is launched)
    int max_k = 0, max_pairs = 0;  // longest lattice, most (theta, phi) pairs of one model
    long long total_pairs = 0;     // (theta, phi) pairs of all models
    int n_cus = 0;
    bool count_work = false;  // vag_ctx_count_work
    int ppb_pin = 0;          // > 0: pairs per workgroup pinned (a counts pass of the likelihood)
    bool spreading = false;   // VAG_FLAG_SPREADING
};

// the hooks, parsed once per launch: std::atoi of the variable, HOOK_UNSET where it is not in the environment.  Hooks that only
// switch something act by being set, whatever their value (VAG_FLUX_WIDE=0 is still wide).
constexpr int HOOK_UNSET = INT_MIN;
struct FluxHooks {
    int pairs_per_block = HOOK_UNSET;         // VAG_PAIRS_PER_BLOCK: > 0 overrides
    int k_cap = HOOK_UNSET;                   // VAG_FLUX_K_CAP: staged lattice nodes (at least 4)
    int wide = HOOK_UNSET;                    // VAG_FLUX_WIDE (switch): no 256-lane form
    int grid_rowwise = HOOK_UNSET;            // VAG_GRID_ROWWISE (switch): small grids through the wavefront-per-row series kernel
    int grid_row_per_workgroup = HOOK_UNSET;  // VAG_GRID_ROW_PER_WORKGROUP (switch): no row-per-lane grid kernel
    int persistent = HOOK_UNSET;              // VAG_FLUX_PERSISTENT: 0 never, 1 (default) where measured to win, 2 always
    int split = HOOK_UNSET;                   // VAG_FLUX_SPLIT: 0 never, 1 (default) where measured to win, 2 wherever legal
    int no_fused = HOOK_UNSET;                // VAG_NO_FUSED (switch)
    int force_fused = HOOK_UNSET;             // VAG_FORCE_FUSED (switch)
    int series_row_per_wave = HOOK_UNSET;     // VAG_SERIES_ROW_PER_WAVE (switch): no row-per-lane fit kernel
    int fit_waves_per_block = HOOK_UNSET;     // VAG_FIT_WAVES_PER_BLOCK: 4, 2, anything else 1
    int series_ppb = HOOK_UNSET;              // VAG_SERIES_PPB: rows per series wavefront, in chunks
    int series_waves = HOOK_UNSET;            // VAG_SERIES_WAVES: wavefronts per series workgroup
};
inline bool hook_set(int v) { return v != HOOK_UNSET; }
inline int hook_or(int v, int dflt) { return hook_set(v) ? v : dflt; }

// ---- rows per workgroup, staged lattice nodes ----

// (theta, phi) pairs per workgroup of vag_flux_grid_kernel
inline int choose_pairs_per_block(const FluxBatch& b, const FluxHooks& h) {
    if (hook_set(h.pairs_per_block) && h.pairs_per_block > 0)  // tuning/debug override
        return std::min(h.pairs_per_block, std::max(1, b.max_pairs));
    // a pinned value (a counts pass of the likelihood): the partial sums of a model are then cut at the same pairs in every batch -- a
    // model with fewer pairs than the value is one workgroup either way.  With grid_rows_plan keeping such a request off the
    // row-per-lane kernel, this is what makes the flux independent of the rest of the batch; the other launch choices the batch
    // decides -- 256 or 512 lanes, the persistent form -- do not change the sums (tests/test_counts.py holds them to the bits), and
    // the piece loop of lattices longer than the staged row (max_k > 512) is outside the guarantee
    if (b.ppb_pin > 0) return std::min(b.ppb_pin, std::max(1, b.max_pairs));
    // enough workgroups to fill 256 CUs several times over, but not so many that staging the photon rows
    // and the partial grids dominate
    long long ppb = (b.total_pairs + 16383) / 16384;
    long long lo = 4;
    if (b.total_pairs / 16 >= 2048) lo = 16;
    if (b.total_pairs / 64 >= 4096) lo = 64;
    ppb = std::max(ppb, lo);
    ppb = std::min<long long>(ppb, std::max(1, b.max_pairs));
    return (int)std::max<long long>(1, ppb);
}

// Lattice nodes the flux kernels stage at a time (their LDS scales with it).  Longer lattices are taken in overlapping pieces
// inside the kernels; VAG_FLUX_K_CAP is a test hook that makes ordinary models take that path.
inline int flux_ks(const FluxBatch& b, const FluxHooks& h) {
    const int cap = hook_set(h.k_cap) ? std::max(4, h.k_cap) : 512;
    return std::max(2, std::min(b.max_k, cap));
}

// ---- a (t, nu) grid request ----

// VAG_GRID_ROWWISE=1 sends a small plain grid to the wavefront-per-row series kernel (an experiment switch: measured slower on every
// such shape, see run_flux_grid)
inline bool grid_rowwise(const FluxBatch& b, const FluxHooks& h, int mode, int nt, int nnu, bool band_weighted) {
    return nt * nnu <= SERIES_THREADS * SERIES_MAX_SLOTS && nnu <= SERIES_MAX_BANDS && !band_weighted && mode != FLUX_FUSED &&
           !b.count_work && hook_set(h.grid_rowwise) && !b.spreading;
}

// Small grids of large batches: a (theta, phi) row per lane (vag_grid_rows.h).  A lone model would walk its lattice as one
// sequential chain there, so the batch must bring blocks of 64 rows enough to fill the GPU; models of a few rows (on-axis
// top hats: 32 rows) would leave lanes empty.  The choice is the batch's (total_pairs) and the kernel sums in another order, so
// a request whose result must not depend on the batch (ppb_pin, a counts pass) stays on the workgroup kernel.
struct GridRowsPlan {
    bool take = false;
    long long blocks = 0;     // blocks of 64 rows in the batch
    int max_blocks = 0;       // ... of one model at most
    bool persistent = false;  // workgroups that take blocks until none is left
    unsigned wg_all = 0;      // workgroups per model of the launch that is not persistent (grid.x; grid.y = nb)
    unsigned wg_persistent = 0;
};
inline GridRowsPlan grid_rows_plan(const FluxBatch& b, const FluxHooks& h, int mode, int nt, int nnu) {
    GridRowsPlan p;
    p.blocks = (b.total_pairs + FITROWS_ROWS - 1) / FITROWS_ROWS;
    p.take = mode != FLUX_FUSED && !b.spreading && !b.count_work && nt * nnu <= GRIDROWS_MAX_SLOTS && nnu <= GRIDROWS_BANDS &&
             nt <= GRIDROWS_MAX_NT && p.blocks >= 4096 && b.total_pairs >= 128LL * b.nb && b.n_rows > 0 && !b.ppb_pin &&
             !hook_set(h.grid_row_per_workgroup);
    p.max_blocks = std::max(1, (b.max_pairs + FITROWS_ROWS - 1) / FITROWS_ROWS);
    // The plain-synchrotron pass is a persistent launch like vag_flux_fit_rows_kernel (three workgroups per CU that take blocks
    // until none is left: vag_grid_rows.h); the IC-corrected and the tabulated-SSC pass keep one workgroup per four blocks (the
    // first has no registers for the loop -- 61 against 47 ms per 1024 C5 members, measured -- the second nothing to gain).
    p.persistent = mode != FLUX_SYN_IC && mode != FLUX_SSC;
    const long long wg_need = (p.blocks + b.nb + GRIDROWS_WAVES - 1) / GRIDROWS_WAVES;  // (total_pairs may be the previous call's)
    p.wg_all = (unsigned)((p.max_blocks + GRIDROWS_WAVES - 1) / GRIDROWS_WAVES);
    p.wg_persistent = (unsigned)std::max<long long>(1, std::min<long long>(wg_need, 3LL * b.n_cus));
    return p;
}

// The variant of the workgroup kernel, vag_flux_grid_kernel<count, mode, spread, lanes, pieces>.  Exactly 21 exist (each as the
// one-item and the persistent kernel):
//   pieces (some lattice is longer than the staged row)   4 modes x {spread, not}, 512 lanes, no tally           8
//   256 lanes ("small")                                   4 modes, not spreading, no tally, one piece            4
//   512 lanes, spreading                                  4 modes                                                4
//   512 lanes, not spreading                              4 modes, and FLUX_SYN with the tally                   5
struct GridVariant {
    int mode = FLUX_SYN;
    bool spread = false;
    int lanes = FLUX_THREADS;  // 256 | 512
    bool pieces = false;
    bool count = false;  // the tallying instantiation (vag_ctx_count_work)
};
inline GridVariant grid_variant(const FluxBatch& b, const FluxHooks& h, int mode, int nt, int nnu, int ks) {
    GridVariant v;
    v.mode = mode;
    v.spread = b.spreading;
    v.pieces = b.max_k > ks;  // the instantiations with the piece loop; the tallying one has none: the plan keeps the upper bounds
    // the tally exists only for FLUX_SYN, 512 lanes, no spreading and no pieces
    v.count = b.count_work && mode == FLUX_SYN && !b.spreading && !v.pieces;
    // requests with few (nu, t) slots and short rows keep less than half of a 512-lane workgroup busy: use 256 lanes
    // (+47 % on the C5 / C1b shapes; a 128-lane variant measured slower).  Never spreading, tallying or in pieces.
    const bool small = !b.spreading && !v.count && !v.pieces && (long long)nt * nnu <= 512 && (long long)ks * ((nnu + 1) / 2) <= 512 &&
                       !hook_set(h.wide);
    v.lanes = small ? 256 : FLUX_THREADS;
    return v;
}
// the one variant the split form can stand in for: plain synchrotron, non-spreading, one piece, 512 lanes, no tally
inline bool grid_variant_plain(const GridVariant& v) {
    return v.mode == FLUX_SYN && !v.spread && v.lanes == FLUX_THREADS && !v.pieces && !v.count;
}

// Whether a launch of `n_items` work items goes persistent, and with how many workgroups: as many as stay resident (wg_per_cu from
// the occupancy query x CUs), the items dealt from a counter.  persist: 0 never, 1 where it wins, 2 (or more) whatever the shape.
// A launch that fits in one round gains nothing from a deal order, and the item loop's spills cost the short ones up to 5 %.
// Short items lose too: every item starts with a round trip to the counter and two barriers, and on items of 32 rows (16384
// configs[0] top hats, ppb 64) the persistent form took 6.1 against 4.6 ms.  Measured to win at ppb 128 (configs[1], 512 models).
struct PersistPlan {
    bool persistent = false;
    long long n_wg = 0;
};
inline PersistPlan persist_plan(int persist, long long n_items, int wg_per_cu, int n_cus, int pairs_per_block) {
    const long long resident = (long long)wg_per_cu * n_cus;
    if (!persist || (persist == 1 && (n_items <= resident || pairs_per_block < FLUX_PERSIST_MIN_PPB))) return {};
    return {true, std::min(n_items, resident)};
}

// Whether the split form (vag_flux_grid_split_kernel) may take a launch of the plain variant (grid_variant_plain) that may go
// persistent (persist != 0); persist_plan with the split kernel's own occupancy then still has to say that it does.
// split = 1: the shapes it is measured to win on; 2 (test hook): wherever it is legal; 0: never.
inline bool split_takes(int split, int persist, bool has_rowgeo, size_t lds_split, int nt, int nnu, int ks) {
    if (!split || !persist || !has_rowgeo) return false;
    if (lds_split > FLUX_SPLIT_LDS_BUDGET || nnu > FLUX_SPLIT_MAX_NNU || nt > FLUX_SPLIT_MAX_NT) return false;
    // Unforced only on what was measured, the headline shape (lattices of 199 nodes, 200 times x 10 frequencies): all ten frequencies
    // (fewer take the B team's chain-after-chain loop, which lost), times in the range where B lanes own two, and a lattice about as
    // long -- the A team's work scales with the lattice, the B team's two wavefronts carry every (nu, t) slot whatever its length,
    // so on shorter lattices they are what a row waits for.  The LDS budget bounds the lattice from above (204 nodes at this grid).
    if (split == 1 && (nnu != FLUX_SPLIT_MAX_NNU || nt <= FLUX_SPLIT_B * 64 || ks < FLUX_SPLIT_MIN_KS)) return false;
    return true;
}

// Synchrotron (IC-cooled) and SSC components of one emitter in ONE flux pass, or two passes: lds_fused / lds_two are the workgroup
// kernel's LDS in FLUX_FUSED and in FLUX_SYN_IC mode.
inline bool fused_fits(const FluxBatch& b, const FluxHooks& h, int nt, int nnu, size_t lds_fused, size_t lds_two) {
    if (hook_set(h.no_fused)) return false;
    if (hook_set(h.grid_rowwise) && nt * nnu <= SERIES_THREADS * SERIES_MAX_SLOTS && nnu <= SERIES_MAX_BANDS && !b.count_work)
        return false;  // experiment switch of run_flux_grid: two passes of the wavefront-per-row kernel
    // the second set of buffers must not cost a resident workgroup: on the C5 / C3 shapes it does (63 vs 51 KB: two
    // workgroups per CU instead of three) and the fused pass measured 18 % SLOWER than two passes there
    const size_t cu = CU_LDS_BYTES;
    if (hook_set(h.force_fused)) return lds_fused <= cu;
    return lds_fused <= cu && std::min<size_t>(cu / lds_fused, 4) >= std::min<size_t>(cu / lds_two, 4);
}

// ---- a series request ----

// A fit's shape (plain synchrotron, <= 512 points in a few bands): the row-per-lane kernel (vag_fit_rows.h)
inline bool fit_rows_takes(const FluxHooks& h, int mode, int grid_nt, int n, int n_bands) {
    return mode != FLUX_FUSED && grid_nt == 0 && n <= FITROWS_MAX_POINTS && n_bands > 0 && n_bands <= FITROWS_BANDS &&
           !hook_set(h.series_row_per_wave);
}

// vag_flux_fit_rows_kernel<mode, bands, spread, tally>: 3 modes x {4, 8 bands} x {spread, not} and ONE tallying instantiation,
// <FLUX_SYN, 4, false, true> (plain synchrotron, <= 4 bands, no spreading: the walker metric's case) -- 13
struct FitRowsVariant {
    int mode = FLUX_SYN;
    int bands = 4;  // 4 | 8
    bool spread = false;
    bool tally = false;
};
struct FitRowsPlan {
    int max_blocks = 0;    // blocks of 64 rows of one model at most
    long long blocks = 0;  // ... in the batch
    int waves_per_block = 0;
    int workgroups = 0;  // of the persistent launch
    FitRowsVariant v;
};
inline FitRowsPlan fit_rows_plan(const FluxBatch& b, const FluxHooks& h, int mode, int n_bands) {
    FitRowsPlan p;
    p.max_blocks = std::max(1, (b.max_pairs + FITROWS_ROWS - 1) / FITROWS_ROWS);
    // wavefronts per block of 64 rows: four while the batch leaves the GPU room (each walks a quarter of the lattice),
    // one when there are blocks enough to fill it (one prologue per block).  The partial sums are the same either way.
    p.blocks = (b.total_pairs + FITROWS_ROWS - 1) / FITROWS_ROWS;
    p.waves_per_block = p.blocks <= 1024 ? 4 : (p.blocks <= 4608 ? 2 : 1);  // measured (persistent launch, 4 / 2 / 1): 0.8 k blocks 0.072 / 0.088 / 0.140 ms, 1.6 k 0.115 / 0.105 / 0.142, 6.2 k 0.333 / 0.267 / 0.269
    if (hook_set(h.fit_waves_per_block)) p.waves_per_block = h.fit_waves_per_block == 4 ? 4 : (h.fit_waves_per_block == 2 ? 2 : 1);
    // persistent workgroups: as many as the GPU holds (three per CU), fewer when there are fewer items (blocks x wavefronts per block)
    const long long items = (p.blocks + b.nb) * p.waves_per_block;  // (total_pairs may be the previous call's: every model can own one block more)
    p.workgroups = (int)std::max<long long>(1, std::min<long long>((items + FITROWS_WAVES - 1) / FITROWS_WAVES, 3LL * b.n_cus));
    p.v.tally = b.count_work && mode == FLUX_SYN && !b.spreading && n_bands <= 4;
    p.v.mode = mode == FLUX_SYN || mode == FLUX_SYN_IC ? mode : FLUX_SSC;
    p.v.bands = n_bands <= 4 ? 4 : 8;
    p.v.spread = b.spreading;
    return p;
}

// vag_flux_series_kernel<mode, spread, points per lane, grid>: 3 modes x {spread, not} x {1, SERIES_MAX_SLOTS} for point series
// and 3 modes of the grid form -- 15.  A grid served by this kernel launches the NON-spreading <M, false, SERIES_MAX_SLOTS, true>
// whatever the batch is: that path never takes a spreading batch (grid_rowwise).
struct SeriesVariant {
    int mode = FLUX_SYN;
    bool spread = false;
    int slots = SERIES_MAX_SLOTS;  // data points per lane: 1 | SERIES_MAX_SLOTS
    bool grid = false;
};
struct SeriesPlan {
    long long ppb = 0;   // rows per wavefront
    int max_blocks = 0;  // wavefronts per model at most
    int chunk = 0;       // rows per partial sum
    int max_chunks = 0;
    int n_bands = 0;  // as the kernel gets it: 0 turns the shared-node path off
    SeriesVariant v;
};
inline SeriesPlan series_plan(const FluxBatch& b, const FluxHooks& h, int mode, int n, int n_bands, int grid_nt) {
    SeriesPlan p;
    // series work per (theta, phi) row is small: fewer, longer wavefronts as the batch grows.  The partial sums are kept per
    // SERIES_CHUNK rows whatever this choice is, so a model's result does not depend on what else is in the batch (a walker
    // scores the same bits alone, in a block of 64, or among 1024).
    p.ppb = std::max<long long>(SERIES_CHUNK, (b.total_pairs + 32767) / 32768);
    p.ppb = (p.ppb + SERIES_CHUNK - 1) / SERIES_CHUNK * SERIES_CHUNK;
    if (hook_set(h.series_ppb)) p.ppb = std::max(1, h.series_ppb) * SERIES_CHUNK;  // tuning override (in chunks)
    p.max_blocks = std::max(1, (int)((b.max_pairs + p.ppb - 1) / p.ppb));
    // a small (nu, t) grid served by this kernel keeps one partial per wavefront (its 128 x 128 rows would need thousands of
    // 8-row chunks per model); a grid request makes no batch-independence promise, as the workgroup kernel does not either
    p.chunk = grid_nt > 0 ? (int)p.ppb : SERIES_CHUNK;
    p.max_chunks = std::max(1, (b.max_pairs + p.chunk - 1) / p.chunk);
    p.n_bands = n > SERIES_THREADS && grid_nt == 0 ? 0 : n_bands;  // a fit's shared-node path keeps one point per lane
    p.v.mode = mode == FLUX_SYN_IC || mode == FLUX_SSC ? mode : FLUX_SYN;
    p.v.grid = grid_nt > 0;
    p.v.spread = !p.v.grid && b.spreading;
    p.v.slots = !p.v.grid && n <= SERIES_THREADS ? 1 : SERIES_MAX_SLOTS;  // one data point per lane
    return p;
}

// Wavefronts per series workgroup: the shape that keeps the most wavefronts resident on a CU (each workgroup carries one copy of
// the tables); ties go to the LARGER workgroup looked at later.  wg_per_cu[i]: resident workgroups of 1 << i wavefronts (always the
// occupancy of vag_flux_series_kernel<FLUX_SYN, false, 1>, whatever variant is launched), negative where that workgroup's LDS
// exceeds a CU's -- nothing larger is looked at then.
inline int series_waves(const FluxHooks& h, const int (&wg_per_cu)[3]) {
    static_assert(SERIES_WAVES == 4, "workgroups of 1, 2 and 4 wavefronts");
    int waves = 1, best = 0;
    for (int i = 0, w = 1; w <= SERIES_WAVES; ++i, w <<= 1) {
        if (wg_per_cu[i] < 0) break;
        const int resident = std::min(wg_per_cu[i] * w, 16);
        if (resident >= best) best = resident, waves = w;
    }
    if (hook_set(h.series_waves)) waves = std::max(1, std::min(SERIES_WAVES, h.series_waves));
    return waves;
}

}  // namespace vag
