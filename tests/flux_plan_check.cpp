// flux_plan_check.cpp -- the launch decisions of the flux stage (csrc/vag_flux_plan.h over csrc/vag_flux_limits.h) run on their own,
// for the host sanitizers: tests/test_flux_plan_host.py builds it with -fsanitize=address,undefined and runs it.  No device, no
// context, no HIP.
//
// Every expected value is a literal worked out by hand from the launch code as it stood before the decisions moved into the header
// (commit c27b3a4, vag_capi.hip; "was NNNN" cites its line), never computed through the header.  Every threshold is held at the
// value and one on each side.  One "ok <case>" line per case.
#include <cstdio>

#include "../vegasafterglow_amd/csrc/vag_flux_limits.h"
#include "../vegasafterglow_amd/csrc/vag_flux_plan.h"

using namespace vag;

static int g_failed = 0;
#define EQ(got, want)                                                                                                     \
    do {                                                                                                                  \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                    \
        if (g_ != w_) {                                                                                                   \
            std::printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #got, g_, w_);                          \
            ++g_failed;                                                                                                   \
        }                                                                                                                 \
    } while (0)
static void done(const char* name, int failed_before) {
    if (g_failed == failed_before) std::printf("ok %s\n", name);
}

static FluxBatch batch(int nb, int max_k, int max_pairs, long long total_pairs) {
    FluxBatch b;
    b.nb = nb;
    b.n_rows = 1;
    b.max_k = max_k;
    b.max_pairs = max_pairs;
    b.total_pairs = total_pairs;
    b.n_cus = 256;
    return b;
}
static const FluxHooks NONE;

// a variant as {mode, spread, lanes, pieces, count}
static void variant_is(const GridVariant& v, int mode, bool spread, int lanes, bool pieces, bool count, int line) {
    if (v.mode != mode || v.spread != spread || v.lanes != lanes || v.pieces != pieces || v.count != count) {
        std::printf("FAIL %s:%d: variant {%d, %d, %d, %d, %d}, want {%d, %d, %d, %d, %d}\n", __FILE__, line, v.mode, (int)v.spread, v.lanes,
                    (int)v.pieces, (int)v.count, mode, (int)spread, lanes, (int)pieces, (int)count);
        ++g_failed;
    }
}
#define VARIANT(v, ...) variant_is(v, __VA_ARGS__, __LINE__)

static void limits() {
    const int f = g_failed;
    // the values the literals below rest on (vag_kernels.h 681-682, 719-722, 1502-1506, 1890-1894; vag_fit_rows.h 28-32;
    // vag_grid_rows.h 20-29; vag_capi.hip 1305, 1331-1332)
    EQ(FLUX_THREADS, 512); EQ(FLUX_MAX_SLOTS, 8192);
    EQ(FLUX_SYN, 0); EQ(FLUX_SYN_IC, 1); EQ(FLUX_SSC, 2); EQ(FLUX_FUSED, 3);
    EQ(FLUX_SPLIT_A, 6); EQ(FLUX_SPLIT_B, 2); EQ(FLUX_SPLIT_TIMES, 2); EQ(FLUX_SPLIT_MAX_NT, 256); EQ(FLUX_SPLIT_MAX_NNU, 10);
    EQ(FLUX_PERSIST_MIN_PPB, 128); EQ(FLUX_SPLIT_MIN_KS, 192); EQ(FLUX_SPLIT_LDS_BUDGET, 81920);
    EQ(SERIES_THREADS, 64); EQ(SERIES_WAVES, 4); EQ(SERIES_MAX_SLOTS, 8); EQ(SERIES_CHUNK, 8); EQ(SERIES_MAX_BANDS, 8);
    EQ(FITROWS_WAVES, 4); EQ(FITROWS_BANDS, 8); EQ(FITROWS_MAX_POINTS, 512); EQ(FITROWS_ROWS, 64); EQ(FITROWS_SEGS, 4);
    EQ(GRIDROWS_WAVES, 4); EQ(GRIDROWS_BANDS, 4); EQ(GRIDROWS_MAX_NT, 128); EQ(GRIDROWS_MAX_SLOTS, 512);
    done("limits", f);
}

// 512 models of 4096 rows and 199 lattice nodes, 200 times x 10 frequencies, plain synchrotron
static void headline() {
    const int f = g_failed;
    const FluxBatch b = batch(512, 199, 4096, 512LL * 4096);
    // was 1274-1280: (2097152 + 16383) / 16384 = 128 (129 x 16384 = 2113536 is one more), lo = 64, max_pairs 4096 does not clamp
    EQ(choose_pairs_per_block(b, NONE), 128);
    EQ(flux_ks(b, NONE), 199);                                   // was 1286-1288: min(199, 512)
    EQ(grid_rowwise(b, NONE, FLUX_SYN, 200, 10, false), false);  // was 1409-1410: no hook (and 2000 slots)
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 200, 10).take, false);  // was 1420: 2000 slots > 512
    const GridVariant v = grid_variant(b, NONE, FLUX_SYN, 200, 10, 199);
    VARIANT(v, FLUX_SYN, false, 512, false, false);  // was 1533: 2000 slots > 512, so the last branch of the ladder, 1607-1610
    EQ(grid_variant_plain(v), true);
    // was 1350 / 1356, 1386 / 1387: 512 x 32 = 16384 items of 128 rows against 2 x 256 resident workgroups
    const PersistPlan p = persist_plan(1, 512 * 32, 2, 256, 128);
    EQ(p.persistent, true); EQ(p.n_wg, 512);
    EQ(split_takes(1, 1, true, 81920, 200, 10, 199), true);  // was 1369-1376 (the LDS at its budget, 1371: >)
    // one number at a time
    EQ(split_takes(1, 1, true, 81920, 200, 10, 191), false);  // was 1376: k_stride < 192
    EQ(split_takes(1, 1, true, 81920, 200, 10, 192), true);
    EQ(split_takes(1, 1, true, 81920, 200, 10, 193), true);
    EQ(split_takes(1, 1, true, 81920, 200, 9, 199), false);   // was 1376: nnu != 10
    EQ(split_takes(1, 1, true, 81920, 200, 11, 199), false);  // was 1371: nnu > 10
    EQ(split_takes(1, 1, true, 81920, 127, 10, 199), false);  // was 1376: nt <= 2 x 64
    EQ(split_takes(1, 1, true, 81920, 128, 10, 199), false);
    EQ(split_takes(1, 1, true, 81920, 129, 10, 199), true);
    EQ(split_takes(1, 1, true, 81920, 256, 10, 199), true);   // was 1371: nt > 256
    EQ(split_takes(1, 1, true, 81920, 257, 10, 199), false);
    EQ(split_takes(1, 1, true, 81919, 200, 10, 199), true);
    EQ(split_takes(1, 1, true, 81921, 200, 10, 199), false);  // was 1371: one byte over the budget
    EQ(split_takes(0, 1, true, 81920, 200, 10, 199), false);  // was 1369: VAG_FLUX_SPLIT=0
    EQ(split_takes(1, 0, true, 81920, 200, 10, 199), false);  // was 1369: VAG_FLUX_PERSISTENT=0
    EQ(split_takes(1, 2, true, 81920, 200, 10, 199), true);
    EQ(split_takes(1, 1, false, 81920, 200, 10, 199), false);  // was 1369: no row-geometry records (a spreading batch)
    // VAG_FLUX_SPLIT=2: wherever it is legal (was 1371, 1376 skipped)
    EQ(split_takes(2, 1, true, 20000, 40, 4, 60), true);
    EQ(split_takes(2, 1, true, 20000, 256, 4, 60), true);
    EQ(split_takes(2, 1, true, 20000, 257, 4, 60), false);
    EQ(split_takes(2, 1, true, 20000, 40, 11, 60), false);
    EQ(split_takes(2, 1, true, 81921, 40, 4, 60), false);
    EQ(split_takes(2, 0, true, 20000, 40, 4, 60), false);
    done("headline shape", f);
}

static void persistence() {
    const int f = g_failed;
    // 16384 top hats of 32 rows: was 1274-1280, (524288 + 16383) / 16384 = 32, lo = 64, clamped to the 32 rows a model has
    EQ(choose_pairs_per_block(batch(16384, 100, 32, 16384LL * 32), NONE), 32);
    // was 1350: items shorter than 128 rows stay one per workgroup however many there are (the measured case: ppb 64)
    EQ(persist_plan(1, 16384, 2, 256, 64).persistent, false);
    EQ(persist_plan(1, 16384, 2, 256, 127).persistent, false);
    EQ(persist_plan(1, 16384, 2, 256, 128).persistent, true);
    EQ(persist_plan(1, 16384, 2, 256, 129).persistent, true);
    // was 1350: n_items <= wg * n_cus fits in one round
    EQ(persist_plan(1, 511, 2, 256, 128).persistent, false);
    EQ(persist_plan(1, 512, 2, 256, 128).persistent, false);
    EQ(persist_plan(1, 513, 2, 256, 128).persistent, true);
    EQ(persist_plan(1, 513, 2, 256, 128).n_wg, 512);      // was 1356
    EQ(persist_plan(1, 769, 3, 256, 128).n_wg, 768);
    EQ(persist_plan(1, 768, 3, 256, 128).persistent, false);
    // VAG_FLUX_PERSISTENT=0 (was 1337, 1350: no query, wg = -1) and =2 (was 1350: whatever the shape; 1356: min(items, resident))
    EQ(persist_plan(0, 100000, -1, 256, 512).persistent, false);
    EQ(persist_plan(2, 10, 2, 256, 4).persistent, true);
    EQ(persist_plan(2, 10, 2, 256, 4).n_wg, 10);
    EQ(persist_plan(2, 100000, 1, 256, 4).n_wg, 256);
    done("persistence", f);
}

static void lanes256() {
    const int f = g_failed;
    FluxBatch b = batch(64, 128, 1000, 64000);
    auto grid_variant = [](FluxBatch b, const FluxHooks& h, int mode, int nt, int nnu, int ks) {
        b.max_k = ks;
        return vag::grid_variant(b, h, mode, nt, nnu, ks);
    };
    FluxHooks wide;
    wide.wide = 1;
    // was 1533-1534: nt * nnu <= 512
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 128, 4, 128), FLUX_SYN, false, 256, false, false);  // 512 slots, 128 x 2 = 256
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 171, 3, 128), FLUX_SYN, false, 512, false, false);  // 513 slots
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 73, 7, 128), FLUX_SYN, false, 256, false, false);   // 511 slots, 128 x 4 = 512
    // was 1533: ks * ((nnu + 1) / 2) <= 512 (lattices as long as the staged row: one piece)
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 4, 256), FLUX_SYN, false, 256, false, false);  // 256 x 2 = 512
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 3, 256), FLUX_SYN, false, 256, false, false);  // 256 x (4 / 2) = 512
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 1, 512), FLUX_SYN, false, 256, false, false);  // 512 x 1
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 5, 171), FLUX_SYN, false, 512, false, false);  // 171 x 3 = 513
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 5, 170), FLUX_SYN, false, 256, false, false);  // 170 x 3 = 510
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 4, 257), FLUX_SYN, false, 512, false, false);  // 257 x 2 = 514
    // off under the hook, spreading, the tally
    VARIANT(grid_variant(b, wide, FLUX_SYN, 100, 4, 256), FLUX_SYN, false, 512, false, false);
    FluxHooks wide0;
    wide0.wide = 0;  // (was 1534: the hook acts by being set)
    VARIANT(grid_variant(b, wide0, FLUX_SYN, 100, 4, 256), FLUX_SYN, false, 512, false, false);
    FluxBatch s = b;
    s.spreading = true;
    VARIANT(grid_variant(s, NONE, FLUX_SYN, 100, 4, 256), FLUX_SYN, true, 512, false, false);
    FluxBatch t = b;
    t.count_work = true;
    VARIANT(grid_variant(t, NONE, FLUX_SYN, 100, 4, 256), FLUX_SYN, false, 512, false, true);
    VARIANT(grid_variant(t, NONE, FLUX_SSC, 100, 4, 256), FLUX_SSC, false, 256, false, false);  // (was 1518: a tally only for FLUX_SYN)
    done("256-lane form", f);
}

static void variants21() {
    const int f = g_failed;
    const int modes[4] = {FLUX_SYN, FLUX_SYN_IC, FLUX_SSC, FLUX_FUSED};
    FluxBatch b = batch(64, 200, 1000, 64000), s = b, c = b;
    s.spreading = true;
    c.count_work = true;
    for (int m : modes) {
        VARIANT(grid_variant(b, NONE, m, 200, 10, 200), m, false, 512, false, false);  // was 1587-1588, 1601-1604, 1610
        VARIANT(grid_variant(s, NONE, m, 200, 10, 200), m, true, 512, false, false);   // was 1585-1586, 1595-1600
        VARIANT(grid_variant(b, NONE, m, 100, 4, 200), m, false, 256, false, false);   // was 1583-1584, 1589-1594
        VARIANT(grid_variant(b, NONE, m, 200, 10, 150), m, false, 512, true, false);   // was 1565-1581: max_k 200 > ks 150
        VARIANT(grid_variant(s, NONE, m, 200, 10, 150), m, true, 512, true, false);
    }
    VARIANT(grid_variant(c, NONE, FLUX_SYN, 200, 10, 200), FLUX_SYN, false, 512, false, true);  // was 1605-1606: the 21st
    // what does not exist maps to what the ladder gave
    VARIANT(grid_variant(c, NONE, FLUX_FUSED, 200, 10, 200), FLUX_FUSED, false, 512, false, false);  // fused + count (was 1518, 1587)
    VARIANT(grid_variant(c, NONE, FLUX_SYN_IC, 200, 10, 200), FLUX_SYN_IC, false, 512, false, false);
    VARIANT(grid_variant(b, NONE, FLUX_SYN, 100, 4, 8), FLUX_SYN, false, 512, true, false);   // small + pieces (was 1565: pieces first)
    VARIANT(grid_variant(c, NONE, FLUX_SYN, 200, 10, 150), FLUX_SYN, false, 512, true, false);  // count + pieces (was 1566)
    FluxBatch cs = c;
    cs.spreading = true;
    VARIANT(grid_variant(cs, NONE, FLUX_SYN, 200, 10, 200), FLUX_SYN, true, 512, false, false);  // count + spreading (was 1518, 1599)
    VARIANT(grid_variant(s, NONE, FLUX_SYN, 100, 4, 200), FLUX_SYN, true, 512, false, false);    // small + spreading (was 1533)
    // only the plain variant can be the split form's (was 1607: the ladder's last branch but one)
    EQ(grid_variant_plain(grid_variant(b, NONE, FLUX_SYN, 200, 10, 200)), true);
    EQ(grid_variant_plain(grid_variant(b, NONE, FLUX_SYN_IC, 200, 10, 200)), false);
    EQ(grid_variant_plain(grid_variant(s, NONE, FLUX_SYN, 200, 10, 200)), false);
    EQ(grid_variant_plain(grid_variant(b, NONE, FLUX_SYN, 100, 4, 200)), false);
    EQ(grid_variant_plain(grid_variant(b, NONE, FLUX_SYN, 200, 10, 150)), false);
    EQ(grid_variant_plain(grid_variant(c, NONE, FLUX_SYN, 200, 10, 200)), false);
    done("21 grid variants", f);
}

static void grid_rows() {
    const int f = g_failed;
    // was 1419-1422: blocks = (total_pairs + 63) / 64 >= 4096, total_pairs >= 128 * nb
    FluxBatch b = batch(1024, 100, 300, 262081);  // (262081 + 63) / 64 = 4096
    GridRowsPlan p = grid_rows_plan(b, NONE, FLUX_SYN, 128, 4);
    EQ(p.take, true); EQ(p.blocks, 4096);
    EQ(p.max_blocks, 5);         // was 1423: (300 + 63) / 64
    EQ(p.persistent, true);      // was 1452
    EQ(p.wg_all, 2);             // was 1456: (5 + 3) / 4
    EQ(p.wg_persistent, 768);    // was 1455, 1457: (4096 + 1024 + 3) / 4 = 1280 against 3 x 256
    b.n_cus = 1000;
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 128, 4).wg_persistent, 1280);
    b.n_cus = 256;
    EQ(grid_rows_plan(b, NONE, FLUX_SYN_IC, 128, 4).take, true); EQ(grid_rows_plan(b, NONE, FLUX_SYN_IC, 128, 4).persistent, false);
    EQ(grid_rows_plan(b, NONE, FLUX_SSC, 128, 4).take, true); EQ(grid_rows_plan(b, NONE, FLUX_SSC, 128, 4).persistent, false);
    b.total_pairs = 262080;  // 4095 blocks
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 128, 4).blocks, 4095); EQ(grid_rows_plan(b, NONE, FLUX_SYN, 128, 4).take, false);
    FluxBatch w = batch(4096, 100, 300, 128LL * 4096);  // 8192 blocks
    EQ(grid_rows_plan(w, NONE, FLUX_SYN, 128, 4).take, true);
    w.total_pairs = 128LL * 4096 - 1;  // still (524287 + 63) / 64 = 8192 blocks
    EQ(grid_rows_plan(w, NONE, FLUX_SYN, 128, 4).blocks, 8192); EQ(grid_rows_plan(w, NONE, FLUX_SYN, 128, 4).take, false);
    w.total_pairs = 128LL * 4096 + 1;
    EQ(grid_rows_plan(w, NONE, FLUX_SYN, 128, 4).take, true);
    // the request: slots 512 / 513, nnu 4 / 5, nt 128 / 129
    b.total_pairs = 262081;
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 171, 3).take, false);  // 513 slots
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 100, 5).take, false);  // 500 slots in 5 frequencies
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 100, 4).take, true);
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 128, 1).take, true);
    EQ(grid_rows_plan(b, NONE, FLUX_SYN, 129, 1).take, false);
    // off
    EQ(grid_rows_plan(b, NONE, FLUX_FUSED, 128, 4).take, false);
    FluxBatch o = b;
    o.ppb_pin = 64;
    EQ(grid_rows_plan(o, NONE, FLUX_SYN, 128, 4).take, false);
    o = b, o.spreading = true;
    EQ(grid_rows_plan(o, NONE, FLUX_SYN, 128, 4).take, false);
    o = b, o.count_work = true;
    EQ(grid_rows_plan(o, NONE, FLUX_SYN, 128, 4).take, false);
    o = b, o.n_rows = 0;
    EQ(grid_rows_plan(o, NONE, FLUX_SYN, 128, 4).take, false);
    FluxHooks h;
    h.grid_row_per_workgroup = 0;  // (acts by being set)
    EQ(grid_rows_plan(b, h, FLUX_SYN, 128, 4).take, false);
    // the wavefront-per-row series kernel for a grid: only with its hook (was 1409-1410)
    FluxHooks r;
    r.grid_rowwise = 1;
    EQ(grid_rowwise(b, NONE, FLUX_SYN, 64, 8, false), false);
    EQ(grid_rowwise(b, r, FLUX_SYN, 64, 8, false), true);    // 512 slots, 8 frequencies
    EQ(grid_rowwise(b, r, FLUX_SYN, 171, 3, false), false);  // 513 slots
    EQ(grid_rowwise(b, r, FLUX_SYN, 50, 9, false), false);
    EQ(grid_rowwise(b, r, FLUX_SSC, 64, 8, false), true);
    EQ(grid_rowwise(b, r, FLUX_FUSED, 64, 8, false), false);
    EQ(grid_rowwise(b, r, FLUX_SYN, 64, 8, true), false);  // band-weighted
    o = b, o.count_work = true;
    EQ(grid_rowwise(o, r, FLUX_SYN, 64, 8, false), false);
    o = b, o.spreading = true;
    EQ(grid_rowwise(o, r, FLUX_SYN, 64, 8, false), false);
    done("row-per-lane grid kernel", f);
}

static void pairs_per_block() {
    const int f = g_failed;
    // was 1274-1280.  total_pairs / 16 >= 2048 at 32768: lo 4 -> 16
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 32767), NONE), 4);   // (32767 + 16383) / 16384 = 2, lo 4
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 32768), NONE), 16);  // still 2, lo 16
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 32769), NONE), 16);
    // total_pairs / 64 >= 4096 at 262144: lo 16 -> 64
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 262143), NONE), 16);  // (262143 + 16383) / 16384 = 16
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 262144), NONE), 64);
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 262145), NONE), 64);
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 200LL * 16384), NONE), 200);  // (3276800 + 16383) / 16384 = 200 above lo
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 0), NONE), 4);
    // the max_pairs clamp (was 1279-1280)
    EQ(choose_pairs_per_block(batch(8, 100, 40, 262144), NONE), 40);
    EQ(choose_pairs_per_block(batch(8, 100, 0, 262144), NONE), 1);
    // the pin (was 1271) and the hook, which goes first (was 1262-1265)
    FluxBatch pin = batch(8, 100, 1000, 262144);
    pin.ppb_pin = 128;
    EQ(choose_pairs_per_block(pin, NONE), 128);
    pin.max_pairs = 100;
    EQ(choose_pairs_per_block(pin, NONE), 100);
    FluxHooks h;
    h.pairs_per_block = 7;
    EQ(choose_pairs_per_block(pin, h), 7);
    h.pairs_per_block = 5000;
    EQ(choose_pairs_per_block(pin, h), 100);
    h.pairs_per_block = 0;  // not > 0: as if unset
    EQ(choose_pairs_per_block(pin, h), 100);
    h.pairs_per_block = -3;
    EQ(choose_pairs_per_block(batch(8, 100, 1000, 262144), h), 64);
    // staged lattice nodes (was 1286-1288)
    EQ(flux_ks(batch(8, 511, 1, 1), NONE), 511);
    EQ(flux_ks(batch(8, 512, 1, 1), NONE), 512);
    EQ(flux_ks(batch(8, 513, 1, 1), NONE), 512);
    EQ(flux_ks(batch(8, 0, 1, 1), NONE), 2);
    FluxHooks k;
    k.k_cap = 8;
    EQ(flux_ks(batch(8, 100, 1, 1), k), 8);
    k.k_cap = 2;  // at least 4
    EQ(flux_ks(batch(8, 100, 1, 1), k), 4);
    k.k_cap = 1000;
    EQ(flux_ks(batch(8, 600, 1, 1), k), 600);
    done("choose_pairs_per_block", f);
}

static void fit_rows_and_series() {
    const int f = g_failed;
    // was 2478-2479
    EQ(fit_rows_takes(NONE, FLUX_SYN, 0, 512, 8), true);
    EQ(fit_rows_takes(NONE, FLUX_SYN, 0, 513, 8), false);
    EQ(fit_rows_takes(NONE, FLUX_SYN, 0, 512, 9), false);
    EQ(fit_rows_takes(NONE, FLUX_SYN, 0, 512, 0), false);
    EQ(fit_rows_takes(NONE, FLUX_SSC, 0, 1, 1), true);
    EQ(fit_rows_takes(NONE, FLUX_FUSED, 0, 64, 4), false);
    EQ(fit_rows_takes(NONE, FLUX_SYN, 16, 64, 4), false);  // a grid
    FluxHooks rpw;
    rpw.series_row_per_wave = 1;
    EQ(fit_rows_takes(rpw, FLUX_SYN, 0, 64, 4), false);
    // wavefronts per block (was 2515-2517) and persistent workgroups (was 2522-2523), 64 walkers
    FitRowsPlan p = fit_rows_plan(batch(64, 100, 300, 65536), NONE, FLUX_SYN, 4);  // 1024 blocks
    EQ(p.blocks, 1024); EQ(p.waves_per_block, 4); EQ(p.max_blocks, 5);
    EQ(p.workgroups, 768);  // (1024 + 64) x 4 = 4352 items, 1088 workgroups of four wavefronts, 3 x 256 hold
    p = fit_rows_plan(batch(64, 100, 300, 65537), NONE, FLUX_SYN, 4);
    EQ(p.blocks, 1025); EQ(p.waves_per_block, 2);
    EQ(p.workgroups, 545);  // (1025 + 64) x 2 = 2178, (2178 + 3) / 4
    p = fit_rows_plan(batch(64, 100, 300, 294912), NONE, FLUX_SYN, 4);
    EQ(p.blocks, 4608); EQ(p.waves_per_block, 2);
    p = fit_rows_plan(batch(64, 100, 300, 294913), NONE, FLUX_SYN, 4);
    EQ(p.blocks, 4609); EQ(p.waves_per_block, 1); EQ(p.workgroups, 768);  // (4609 + 64 + 3) / 4 = 1169
    p = fit_rows_plan(batch(1, 100, 64, 64), NONE, FLUX_SYN, 4);
    EQ(p.blocks, 1); EQ(p.waves_per_block, 4); EQ(p.workgroups, 2); EQ(p.max_blocks, 1);  // (1 + 1) x 4 = 8 items
    EQ(fit_rows_plan(batch(1, 100, 0, 0), NONE, FLUX_SYN, 4).workgroups, 1);              // 4 items, max_blocks at least 1
    EQ(fit_rows_plan(batch(1, 100, 0, 0), NONE, FLUX_SYN, 4).max_blocks, 1);
    FluxHooks w;
    w.fit_waves_per_block = 4;
    EQ(fit_rows_plan(batch(64, 100, 300, 294913), w, FLUX_SYN, 4).waves_per_block, 4);
    w.fit_waves_per_block = 2;
    EQ(fit_rows_plan(batch(64, 100, 300, 64), w, FLUX_SYN, 4).waves_per_block, 2);
    w.fit_waves_per_block = 3;  // anything else: 1
    EQ(fit_rows_plan(batch(64, 100, 300, 64), w, FLUX_SYN, 4).waves_per_block, 1);
    // the variant (was 2529, 2545-2563): 4 | 8 bands at n_bands 4 / 5, the one tallying instantiation
    FluxBatch b = batch(64, 100, 300, 65536), s = b, c = b;
    s.spreading = true;
    c.count_work = true;
    auto is = [](const FitRowsVariant& v, int mode, int bands, bool spread, bool tally) {
        return v.mode == mode && v.bands == bands && v.spread == spread && v.tally == tally;
    };
    const int modes[3] = {FLUX_SYN, FLUX_SYN_IC, FLUX_SSC};
    for (int m : modes) {
        EQ(is(fit_rows_plan(b, NONE, m, 4).v, m, 4, false, false), true);
        EQ(is(fit_rows_plan(b, NONE, m, 5).v, m, 8, false, false), true);
        EQ(is(fit_rows_plan(b, NONE, m, 8).v, m, 8, false, false), true);
        EQ(is(fit_rows_plan(s, NONE, m, 1).v, m, 4, true, false), true);
        EQ(is(fit_rows_plan(s, NONE, m, 5).v, m, 8, true, false), true);
    }
    EQ(is(fit_rows_plan(c, NONE, FLUX_SYN, 4).v, FLUX_SYN, 4, false, true), true);
    EQ(is(fit_rows_plan(c, NONE, FLUX_SYN, 5).v, FLUX_SYN, 8, false, false), true);  // more than 4 bands: no tally
    EQ(is(fit_rows_plan(c, NONE, FLUX_SYN_IC, 4).v, FLUX_SYN_IC, 4, false, false), true);
    EQ(is(fit_rows_plan(c, NONE, FLUX_SSC, 4).v, FLUX_SSC, 4, false, false), true);
    FluxBatch cs = c;
    cs.spreading = true;
    EQ(is(fit_rows_plan(cs, NONE, FLUX_SYN, 4).v, FLUX_SYN, 4, true, false), true);

    // the shared-node series kernel: rows per wavefront (was 2577-2580), 8 * 32768 = 262144
    SeriesPlan q = series_plan(batch(64, 100, 300, 262144), NONE, FLUX_SYN, 64, 3, 0);
    EQ(q.ppb, 8);  // (262144 + 32767) / 32768 = 8
    EQ(q.max_blocks, 38); EQ(q.chunk, 8); EQ(q.max_chunks, 38);  // (300 + 7) / 8
    q = series_plan(batch(64, 100, 300, 262145), NONE, FLUX_SYN, 64, 3, 0);
    EQ(q.ppb, 16);  // 9, rounded up to whole chunks of 8
    EQ(q.max_blocks, 19); EQ(q.chunk, 8); EQ(q.max_chunks, 38);  // (300 + 15) / 16; a point series keeps 8-row partial sums (was 2583)
    q = series_plan(batch(64, 100, 300, 262145), NONE, FLUX_SYN, 500, 5, 100);
    EQ(q.ppb, 16); EQ(q.chunk, 16); EQ(q.max_chunks, 19);  // a grid: one partial per wavefront
    EQ(series_plan(batch(64, 100, 300, 0), NONE, FLUX_SYN, 64, 3, 0).ppb, 8);
    EQ(series_plan(batch(64, 100, 0, 0), NONE, FLUX_SYN, 64, 3, 0).max_blocks, 1);
    EQ(series_plan(batch(64, 100, 0, 0), NONE, FLUX_SYN, 64, 3, 0).max_chunks, 1);
    FluxHooks sp;
    sp.series_ppb = 3;  // in chunks (was 2579)
    EQ(series_plan(batch(64, 100, 300, 262145), sp, FLUX_SYN, 64, 3, 0).ppb, 24);
    sp.series_ppb = 0;
    EQ(series_plan(batch(64, 100, 300, 262145), sp, FLUX_SYN, 64, 3, 0).ppb, 8);
    // n_bands = 0 above 64 points of a point series (was 2587)
    EQ(series_plan(b, NONE, FLUX_SYN, 64, 3, 0).n_bands, 3);
    EQ(series_plan(b, NONE, FLUX_SYN, 65, 3, 0).n_bands, 0);
    EQ(series_plan(b, NONE, FLUX_SYN, 500, 5, 100).n_bands, 5);
    // the variant (was 2644-2665)
    auto ser = [](const SeriesVariant& v, int mode, bool spread, int slots, bool grid) {
        return v.mode == mode && v.spread == spread && v.slots == slots && v.grid == grid;
    };
    for (int m : modes) {
        EQ(ser(series_plan(b, NONE, m, 64, 3, 0).v, m, false, 1, false), true);
        EQ(ser(series_plan(b, NONE, m, 65, 3, 0).v, m, false, 8, false), true);
        EQ(ser(series_plan(s, NONE, m, 1, 0, 0).v, m, true, 1, false), true);
        EQ(ser(series_plan(s, NONE, m, 512, 0, 0).v, m, true, 8, false), true);
        EQ(ser(series_plan(b, NONE, m, 60, 4, 15).v, m, false, 8, true), true);  // a grid of 60 slots: eight per lane all the same
        EQ(ser(series_plan(s, NONE, m, 60, 4, 15).v, m, false, 8, true), true);  // was 2648: the non-spreading kernel whatever S_ is
    }
    EQ(ser(series_plan(b, NONE, FLUX_FUSED, 64, 3, 0).v, FLUX_SYN, false, 1, false), true);  // was 2664-2665: the ladder's last branch
    // wavefronts per workgroup (was 2595-2601): most resident wavefronts, at most 16 counted, >= lets the later shape win a tie
    FluxHooks none;
    EQ(series_waves(none, {4, 2, 1}), 4);    // 4, 4, 4
    EQ(series_waves(none, {16, 8, 3}), 2);   // 16, 16, 12
    EQ(series_waves(none, {20, 8, 4}), 4);   // 16 (capped), 16, 16
    EQ(series_waves(none, {3, 1, 0}), 1);    // 3, 2, 0
    EQ(series_waves(none, {2, 2, -1}), 2);   // four wavefronts do not fit the LDS
    EQ(series_waves(none, {2, -1, 9}), 1);   // ... nothing larger is looked at
    EQ(series_waves(none, {-1, -1, -1}), 1);
    EQ(series_waves(none, {0, 0, 0}), 4);
    FluxHooks sw;
    sw.series_waves = 2;
    EQ(series_waves(sw, {4, 2, 1}), 2);
    sw.series_waves = 9;
    EQ(series_waves(sw, {4, 2, 1}), 4);
    sw.series_waves = 0;
    EQ(series_waves(sw, {4, 2, 1}), 1);
    done("fit rows and series", f);
}

static void fused() {
    const int f = g_failed;
    const FluxBatch b = batch(64, 100, 300, 65536);
    // was 1841-1844, cu = 163840.  63 against 51 KB: 163840 / 64512 = 2 resident against 163840 / 52224 = 3 -- two passes
    EQ(fused_fits(b, NONE, 100, 4, 63 * 1024, 51 * 1024), false);
    EQ(fused_fits(b, NONE, 100, 4, 40000, 30000), true);     // 4 against min(5, 4)
    EQ(fused_fits(b, NONE, 100, 4, 54613, 50000), true);     // 163840 / 54613 = 3 against 3
    EQ(fused_fits(b, NONE, 100, 4, 54614, 50000), false);    // 163840 / 54614 = 2
    EQ(fused_fits(b, NONE, 100, 4, 163840, 100000), true);   // 1 against 1
    EQ(fused_fits(b, NONE, 100, 4, 163841, 100000), false);  // does not fit at all
    FluxHooks h;
    h.force_fused = 1;  // was 1843
    EQ(fused_fits(b, h, 100, 4, 63 * 1024, 51 * 1024), true);
    EQ(fused_fits(b, h, 100, 4, 163841, 51 * 1024), false);
    h.no_fused = 1;  // was 1836: goes first
    EQ(fused_fits(b, h, 100, 4, 40000, 30000), false);
    FluxHooks r;
    r.grid_rowwise = 1;  // was 1837-1838
    EQ(fused_fits(b, r, 64, 8, 40000, 30000), false);  // 512 slots: the experiment takes it in two passes
    EQ(fused_fits(b, r, 171, 3, 40000, 30000), true);  // 513
    EQ(fused_fits(b, r, 50, 9, 40000, 30000), true);
    FluxBatch c = b;
    c.count_work = true;
    EQ(fused_fits(c, r, 64, 8, 40000, 30000), true);
    done("fused_fits", f);
}

int main() {
    limits();
    headline();
    persistence();
    lanes256();
    variants21();
    grid_rows();
    pairs_per_block();
    fit_rows_and_series();
    fused();
    if (g_failed) std::printf("FAIL: %d checks\n", g_failed);
    return g_failed ? 1 : 0;
}
