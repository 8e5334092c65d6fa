// stage_plan_check.cpp -- the arithmetic of the model stages (csrc/vag_stage_plan.h) run on its own, for the host sanitizers:
// tests/test_stage_plan_host.py builds it with -fsanitize=address,undefined and runs it.  No device, no context, no HIP.
//
// Every expected value is a literal worked out by hand from run_model_stages, finish_speculation, run_flag_groups and
// flux_dev_by_flags of vag_capi.hip as they stood before the arithmetic moved into the header (commit 19f0a66), never computed
// through the header.  Every threshold is held at the value and on each side.  One "ok <case>" line per case.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../vegasafterglow_amd/csrc/vag_stage_plan.h"

using namespace vag;

static int g_failed = 0;
#define EQ(got, want)                                                                            \
    do {                                                                                         \
        const long long g_ = (long long)(got), w_ = (long long)(want);                           \
        if (g_ != w_) {                                                                          \
            std::printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #got, g_, w_); \
            ++g_failed;                                                                          \
        }                                                                                        \
    } while (0)
static void done(const char* name, int failed_before) {
    if (g_failed == failed_before) std::printf("ok %s\n", name);
}

static VagDevPlan summary(int rows, long long cells, int max_k, int max_pairs, int flags_first = 0, int dyn_class = 0, int n_ok = 5) {
    VagDevPlan p{};
    p.rows = rows, p.cells = cells, p.max_k = max_k, p.max_pairs = max_pairs;
    p.flags_first = flags_first, p.dyn_class = dyn_class, p.n_ok = n_ok;
    return p;
}

static void capacities() {
    const int f = g_failed;
    StageCaps none;  // a call that waits for its summary: no capacity at all
    EQ(none.rows, 2147483647);
    EQ(none.k, 2147483647);
    EQ(none.pairs, 2147483647);
    EQ(none.cells, 9223372036854775807LL);
    StageCaps c = plan_ahead_caps(summary(100, 1000, 50, 10), 2);  // small totals: the additive head room dominates
    EQ(c.rows, 189);     // 100 + 25 + 64
    EQ(c.cells, 5346);   // 1000 + 250 + 4096
    EQ(c.k, 52);
    EQ(c.pairs, 79);     // 10 + 5 + 64
    c = plan_ahead_caps(summary(3, 3, 1, 1), 6);  // the integer divisions give 0
    EQ(c.rows, 67);
    EQ(c.cells, 4099);
    EQ(c.k, 7);
    EQ(c.pairs, 65);
    c = plan_ahead_caps(summary(1000003, 5000000001LL, 4000, 100001), 14);  // large totals: a quarter / a half; the cells beyond 2^32
    EQ(c.rows, 1250067);          // 1000003 + 250000 + 64
    EQ(c.cells, 6250004097LL);    // 5000000001 + 1250000000 + 4096
    EQ(c.k, 4014);
    EQ(c.pairs, 150065);          // 100001 + 50000 + 64
    // the lattice cap at VAG_MAX_TIME = 1048576
    EQ(plan_ahead_caps(summary(1, 1, 1048573, 1), 2).k, 1048575);
    EQ(plan_ahead_caps(summary(1, 1, 1048574, 1), 2).k, 1048576);
    EQ(plan_ahead_caps(summary(1, 1, 1048575, 1), 2).k, 1048576);
    EQ(plan_ahead_caps(summary(1, 1, 1048570, 1), 32).k, 1048576);
    // whether a call may be planned ahead: hook, the caller's switch, no details, a valid hint, the hint's batch size
    EQ(may_plan_ahead(true, true, false, true, 128, 128), 1);
    EQ(may_plan_ahead(false, true, false, true, 128, 128), 0);
    EQ(may_plan_ahead(true, false, false, true, 128, 128), 0);
    EQ(may_plan_ahead(true, true, true, true, 128, 128), 0);
    EQ(may_plan_ahead(true, true, false, false, 128, 128), 0);
    EQ(may_plan_ahead(true, true, false, true, 128, 127), 0);
    EQ(may_plan_ahead(true, true, false, true, 128, 129), 0);
    // the flags a summary stands for
    EQ(plan_flags(summary(1, 1, 1, 1, -1)), 0);
    EQ(plan_flags(summary(1, 1, 1, 1, 0)), 0);
    EQ(plan_flags(summary(1, 1, 1, 1, 37)), 37);
    done("capacities", f);
}

static void verdict() {
    const int f = g_failed;
    const VagDevPlan hint = summary(100, 1000, 50, 10, /* flags */ 1, /* dyn_class */ 0);
    const int cap_k = 52;
    VagDevPlan got = summary(110, 1100, 52, 11, 1, 0);  // no cause: kept, the margin as it was
    PlanVerdict v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 0);
    EQ(v.margin_k, 2);
    got.overflow = 1;  // 1: a capacity exceeded, the lattice within its head room (at the cap)
    v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 1);
    EQ(v.margin_k, 2);
    got.max_k = 53;  // 2: ... the lattice beyond it: the margin grows
    v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 1);
    EQ(v.margin_k, 6);
    got = summary(110, 1100, 53, 11, 1, 0);  // (a longer lattice without an overflow is no cause: the device found room)
    v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 0);
    EQ(v.margin_k, 2);
    got = summary(110, 1100, 50, 11, 1, 0);
    got.flags_mixed = 1;  // 3: mixed flags
    v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 1);
    EQ(v.margin_k, 2);
    got = summary(110, 1100, 50, 11, 5, 0);  // 4: other flags than the hint's
    v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 1);
    EQ(v.margin_k, 2);
    got = summary(110, 1100, 50, 11, 1, 1);  // 5: another dynamics class
    v = plan_ahead_verdict(got, hint, cap_k, 2);
    EQ(v.repeat, 1);
    EQ(v.margin_k, 2);
    got = summary(0, 0, 0, 0, -1, 1, /* n_ok */ 0);  // no valid model: flags and class are nobody's, kept
    EQ(plan_ahead_verdict(got, hint, cap_k, 2).repeat, 0);
    got = summary(110, 1100, 50, 11, 0, 0);  // a hint without flags (-1) against a batch of flags 0: the same
    EQ(plan_ahead_verdict(got, summary(100, 1000, 50, 10, -1, 0), cap_k, 2).repeat, 0);
    done("verdict", f);
}

static void margin() {
    const int f = g_failed;
    VagDevPlan got = summary(1, 1, 100, 1);
    got.overflow = 1;
    const int want[6] = {2, 6, 14, 30, 32, 32};
    int m = 2;
    for (int i = 0; i < 6; ++i) {
        EQ(m, want[i]);
        m = plan_ahead_verdict(got, summary(1, 1, 10, 1), /* cap_k */ 99, m).margin_k;
    }
    done("margin", f);
}

static void family() {
    const int f = g_failed;
    // index bits: 16 reverse shock | 8 dyn_class not 0 | 4 spreading | 2 magnetar | 1 VAG_DYN_GENERAL set.  P pair, F fast, G general
    const char* want = "FGFGFGFGGGGGGGGGPPPPPPPPPPPPPPPP";
    for (int i = 0; i < 32; ++i) {
        const int flags = ((i & 16) ? VAG_FLAG_RVS : 0) | ((i & 4) ? VAG_FLAG_SPREADING : 0) | ((i & 2) ? VAG_FLAG_MAGNETAR : 0) | VAG_FLAG_KN;
        DynHooks h;
        if (i & 1) h.general = 0;  // a switch: set is on, whatever the value
        const DynPlan p = dyn_plan(flags, (i & 8) ? 3 : 0, /* rows */ 100, /* n_cus */ 256, h);
        EQ(p.family, want[i] == 'P' ? DYN_PAIR : want[i] == 'F' ? DYN_FAST : DYN_GENERAL);
        EQ(p.spreading, (i & 4) != 0);
        EQ(p.inject, (i & 2) != 0);
    }
    // whose rows per wavefront: the pair solver's hook is VAG_PAIR_RPW, the fast and the general solver's VAG_DYN_RPW
    DynHooks h;
    h.pair_rpw = 4, h.dyn_rpw = 32;
    EQ(dyn_plan(VAG_FLAG_RVS, 0, 100, 256, h).rows_per_wave, 4);
    EQ(dyn_plan(0, 0, 100, 256, h).rows_per_wave, 32);
    EQ(dyn_plan(0, 1, 100, 256, h).rows_per_wave, 32);
    const DynHooks none;
    EQ(dyn_plan(VAG_FLAG_RVS, 0, 100, 256, none).rows_per_wave, 8);  // 100 rows: 13 wavefronts of 8
    EQ(dyn_plan(0, 0, 100, 256, none).rows_per_wave, 64);            // the fast solver: full wavefronts
    EQ(dyn_plan(0, 1, 100, 256, none).rows_per_wave, 8);             // the general solver: as the pair solver
    EQ(dyn_rows_per_wave(HOOK_UNSET), 64);
    EQ(dyn_rows_per_wave(-1), 64);
    EQ(dyn_rows_per_wave(0), 64);
    EQ(dyn_rows_per_wave(1), 1);
    EQ(dyn_rows_per_wave(64), 64);
    EQ(dyn_rows_per_wave(65), 64);
    done("dynamics family", f);
}

static void refill() {
    const int f = g_failed;
    const DynHooks none;
    EQ(dyn_plan(0, 0, 98303, 256, none).family, DYN_FAST);  // 96 * 4 * 256 = 98304 rows
    EQ(dyn_plan(0, 0, 98304, 256, none).family, DYN_REFILL);
    EQ(dyn_plan(0, 0, 98305, 256, none).family, DYN_REFILL);
    EQ(dyn_plan(0, 0, 1535, 4, none).family, DYN_FAST);  // 96 * 4 * 4 = 1536
    EQ(dyn_plan(0, 0, 1536, 4, none).family, DYN_REFILL);
    EQ(dyn_plan(VAG_FLAG_RVS, 0, 98304, 256, none).family, DYN_PAIR);  // (the fast solver's form only)
    EQ(dyn_plan(0, 1, 98304, 256, none).family, DYN_GENERAL);
    DynHooks h;
    h.refill = 0;  // VAG_DYN_REFILL: 0 never, anything else always
    EQ(dyn_plan(0, 0, 98304, 256, h).family, DYN_FAST);
    h.refill = 1;
    EQ(dyn_plan(0, 0, 10, 256, h).family, DYN_REFILL);
    h.refill = -3;
    EQ(dyn_plan(0, 0, 10, 256, h).family, DYN_REFILL);
    // VAG_DYN_REFILL_MIN: 16 by default, held to 1..64
    EQ(dyn_plan(0, 0, 98304, 256, none).refill_min, 16);
    const int mins[6][2] = {{-5, 1}, {0, 1}, {1, 1}, {8, 8}, {64, 64}, {65, 64}};
    for (const auto& m : mins) {
        DynHooks hm;
        hm.refill_min = m[0];
        EQ(dyn_plan(0, 0, 98304, 256, hm).refill_min, m[1]);
    }
    // workgroups: what stays resident (wg_per_cu * n_cus), no more than the wavefronts of rows, at least 1; VAG_DYN_REFILL_WGS: at least 1
    EQ(refill_workgroups(98304, 8, 256, HOOK_UNSET), 1536);    // 1536 wavefronts < 2048 slots
    EQ(refill_workgroups(131072, 8, 256, HOOK_UNSET), 2048);   // 2048 = 2048
    EQ(refill_workgroups(131073, 8, 256, HOOK_UNSET), 2048);   // 2049 > 2048
    EQ(refill_workgroups(1000000, 8, 256, HOOK_UNSET), 2048);
    EQ(refill_workgroups(1, 8, 256, HOOK_UNSET), 1);
    EQ(refill_workgroups(64, 8, 256, HOOK_UNSET), 1);
    EQ(refill_workgroups(65, 8, 256, HOOK_UNSET), 2);
    EQ(refill_workgroups(1000000, 8, 256, 5), 5);
    EQ(refill_workgroups(1000000, 8, 256, 1), 1);
    EQ(refill_workgroups(1000000, 8, 256, 0), 1);
    EQ(refill_workgroups(1000000, 8, 256, -2), 1);
    EQ(refill_workgroups(640, 8, 256, 100000), 10);
    done("refill", f);
}

static void pair_rpw() {
    const int f = g_failed;
    const int want[7][2] = {{512, 8}, {513, 16}, {1024, 16}, {1025, 32}, {2048, 32}, {2049, 64}, {4097, 64}};
    for (const auto& w : want) EQ(pair_rows_per_wave(w[0], HOOK_UNSET), w[1]);
    EQ(pair_rows_per_wave(1, HOOK_UNSET), 8);
    EQ(pair_rows_per_wave(4097, 4), 4);   // VAG_PAIR_RPW: > 0 overrides, at most 64
    EQ(pair_rows_per_wave(100, 64), 64);
    EQ(pair_rows_per_wave(100, 70), 64);
    EQ(pair_rows_per_wave(100, 0), 8);
    EQ(pair_rows_per_wave(100, -1), 8);
    done("pair_rows_per_wave", f);
}

static void dynrec() {
    const int f = g_failed;
    const DynRecShape s{20, 16, 256};  // DYN_ROWREC, DYN_BUCKETS, DYN_CHUNK
    // rows, chunks, order, queue, hist, cls, bytes
    const long long want[4][7] = {{7, 1, 1120, 1152, 1168, 1232, 1239},               // odd: the queue is padded to 8 ints
                                  {512, 2, 81920, 83968, 83984, 84112, 84624},        // even, whole chunks
                                  {1000, 4, 160000, 164000, 164016, 164272, 165272},  // even, the last chunk not full
                                  {257, 2, 41120, 42152, 42168, 42296, 42553}};       // odd, one row into the second chunk
    for (const auto& w : want) {
        const int rows = (int)w[0];
        const DynRecLayout l = dynrec_layout(rows, s);
        EQ(l.n_chunks, w[1]);
        EQ(l.order, w[2]);
        EQ(l.queue, w[3]);
        EQ(l.hist, w[4]);
        EQ(l.cls, w[5]);
        EQ(l.bytes, w[6]);
        // every offset a multiple of its element's size (doubles at 0, ints, unsigned, unsigned, bytes)
        EQ(l.order % 4, 0);
        EQ(l.queue % 4, 0);
        EQ(l.hist % 4, 0);
        // no region reaches into the next
        EQ(l.order >= 8ull * 20 * rows, 1);
        EQ(l.queue - l.order >= 4ull * rows, 1);
        EQ(l.hist - l.queue, 16);
        EQ(l.cls - l.hist, 4ll * 16 * w[1]);
        EQ(l.bytes - l.cls, rows);
        // the total as the allocation was written: records + queue + 16 + histogram + rows
        const size_t rec = sizeof(double) * (size_t)rows * 20, ord = sizeof(int) * (((size_t)rows + 1) & ~(size_t)1);
        const size_t hist = sizeof(unsigned) * 16 * (((size_t)rows + 256 - 1) / 256);
        EQ(l.bytes, rec + ord + 16 + hist + (size_t)rows);
    }
    done("d_dynrec layout", f);
}

static void grouping() {
    const int f = g_failed;
    const std::vector<int> none;
    EQ(group_by_flags(0, [&](int m) { return none[m]; }).size(), 0);
    const std::vector<int> one = {5, 5, 5};
    std::vector<std::vector<int>> g = group_by_flags(3, [&](int m) { return one[m]; });
    EQ(g.size(), 1);
    EQ(g[0].size(), 3);
    EQ(g[0][0], 0);
    EQ(g[0][1], 1);
    EQ(g[0][2], 2);
    const std::vector<int> abacb = {1, 4, 1, 0, 4};  // A B A C B: first-seen order of the sets, batch order within a set
    g = group_by_flags(5, [&](int m) { return abacb[m]; });
    EQ(g.size(), 3);
    EQ(g[0].size(), 2);
    EQ(g[0][0], 0);
    EQ(g[0][1], 2);
    EQ(g[1].size(), 2);
    EQ(g[1][0], 1);
    EQ(g[1][1], 4);
    EQ(g[2].size(), 1);
    EQ(g[2][0], 3);
    done("grouping", f);
}

int main() {
    capacities();
    verdict();
    margin();
    family();
    refill();
    pair_rpw();
    dynrec();
    grouping();
    return g_failed ? 1 : 0;
}
