// sampler_plan_check.cpp -- the host-side decisions of the device sampler (csrc/vag_sampler_plan.h) run on their own, for the host
// sanitizers: tests/test_sampler_plan_host.py builds it with -fsanitize=address,undefined and runs it.  No device, no context, no
// HIP.
//
// Every expected value is a literal worked out by hand from the sampler section of vag_capi.hip as it stood before the decisions
// moved into the header (commit d62d631: stretch_spec_check, move_spec_check, move_kind, tempered_spec_check, the three run entries
// and their launchers), never computed through the header.  Every threshold is held at the value and on each side.  One
// "ok <case>" line per case.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/vegasafterglow_amd.h"
#include "../vegasafterglow_amd/csrc/vag_sampler_plan.h"

using namespace vag;

static int g_failed = 0;
#define EQ(got, want)                                                                                \
    do {                                                                                             \
        const long long g_ = (long long)(got), w_ = (long long)(want);                               \
        if (g_ != w_) {                                                                              \
            std::printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #got, g_, w_);     \
            ++g_failed;                                                                              \
        }                                                                                            \
    } while (0)
// a refusal: VAG_E_INVALID with this text
#define REFUSED(call, text)                                                                                       \
    do {                                                                                                          \
        g_err.clear();                                                                                            \
        const int rc_ = (call);                                                                                   \
        if (rc_ != VAG_E_INVALID || g_err != (text)) {                                                            \
            std::printf("FAIL %s:%d: %s = %d \"%s\", want %d \"%s\"\n", __FILE__, __LINE__, #call, rc_, g_err.c_str(), \
                        (int)VAG_E_INVALID, text);                                                                \
            ++g_failed;                                                                                           \
        }                                                                                                         \
    } while (0)
static void done(const char* name, int failed_before) {
    if (g_failed == failed_before) std::printf("ok %s\n", name);
}

static const double INF = std::numeric_limits<double>::infinity(), NAN_ = std::numeric_limits<double>::quiet_NaN();

static vag_stretch_spec stretch(int ndim, int nw, double a = 2.0, int thin = 1) { return vag_stretch_spec{5, a, nw, ndim, thin}; }

static void shape() {
    const int f = g_failed;
    vag_stretch_spec s;
    // ndim 1..16
    s = stretch(0, 4);
    REFUSED(stretch_spec_check(&s), "stretch move: ndim must be 1..16, got 0");
    s = stretch(1, 2);
    EQ(stretch_spec_check(&s), VAG_OK);
    s = stretch(16, 32);
    EQ(stretch_spec_check(&s), VAG_OK);
    s = stretch(17, 34);
    REFUSED(stretch_spec_check(&s), "stretch move: ndim must be 1..16, got 17");
    // an even number of walkers, at least 2 ndim
    s = stretch(3, 7);
    REFUSED(stretch_spec_check(&s), "stretch move: need an even number of walkers, at least 2 * ndim = 6, got 7");
    s = stretch(3, 4);
    REFUSED(stretch_spec_check(&s), "stretch move: need an even number of walkers, at least 2 * ndim = 6, got 4");
    s = stretch(3, 6);
    EQ(stretch_spec_check(&s), VAG_OK);
    // a finite and > 1
    s = stretch(3, 6, 1.0);
    REFUSED(stretch_spec_check(&s), "stretch move: the scale a must be finite and > 1, got 1");
    s = stretch(3, 6, 1.0000000000000002);  // the double after 1
    EQ(stretch_spec_check(&s), VAG_OK);
    s = stretch(3, 6, INF);
    REFUSED(stretch_spec_check(&s), "stretch move: the scale a must be finite and > 1, got inf");
    s = stretch(3, 6, NAN_);
    EQ(stretch_spec_check(&s), VAG_E_INVALID);  // (the text of a NaN carries the C library's sign)
    // thin >= 1
    s = stretch(3, 6, 2.0, 0);
    REFUSED(stretch_spec_check(&s), "stretch move: thin must be >= 1, got 0");
    s = stretch(3, 6, 2.0, 1);
    EQ(stretch_spec_check(&s), VAG_OK);
    // the fields directly, and the order of the checks: ndim, walkers, a, thin
    REFUSED(ensemble_check(0, 7, 1.0, 0), "stretch move: ndim must be 1..16, got 0");
    REFUSED(ensemble_check(1, 7, 1.0, 0), "stretch move: need an even number of walkers, at least 2 * ndim = 2, got 7");
    REFUSED(ensemble_check(1, 8, 1.0, 0), "stretch move: the scale a must be finite and > 1, got 1");
    REFUSED(ensemble_check(1, 8, 2.0, -3), "stretch move: thin must be >= 1, got -3");
    // half 0 or 1, under the entry's own prefix
    REFUSED(half_check("stretch move", -1), "stretch move: half must be 0 or 1, got -1");
    EQ(half_check("stretch move", 0), VAG_OK);
    EQ(half_check("tempering", 1), VAG_OK);
    REFUSED(half_check("move mix", 2), "move mix: half must be 0 or 1, got 2");
    done("common shape", f);
}

static vag_move_spec mix(int ndim, int nw, double w_s, double w_de, double w_sn) {
    return vag_move_spec{7, 2.0, 0.0, 1e-5, 1.7, {w_s, w_de, w_sn}, nw, ndim, 1};
}

static void moves() {
    const int f = g_failed;
    vag_move_spec m;
    m = mix(3, 6, 0.0, 0.8, 0.2);
    EQ(move_spec_check(&m), VAG_OK);
    // the common checks come first, under the stretch move's prefix
    m = mix(3, 7, 0.0, 0.8, 0.2);
    REFUSED(move_spec_check(&m), "stretch move: need an even number of walkers, at least 2 * ndim = 6, got 7");
    m = mix(3, 6, 0.0, 0.8, 0.2);
    m.a = 1.0;
    REFUSED(move_spec_check(&m), "stretch move: the scale a must be finite and > 1, got 1");
    // weights: finite, >= 0, a sum > 0
    m = mix(3, 6, 0.5, -0.1, 0.2);
    REFUSED(move_spec_check(&m), "move mix: weight 1 must be finite and >= 0, got -0.1");
    m = mix(3, 6, NAN_, 0.8, 0.2);
    EQ(move_spec_check(&m), VAG_E_INVALID);
    m = mix(3, 6, 0.0, 0.8, INF);
    REFUSED(move_spec_check(&m), "move mix: weight 2 must be finite and >= 0, got inf");
    m = mix(3, 6, 0.0, 0.0, 0.0);
    REFUSED(move_spec_check(&m), "move mix: the weights must have a finite sum > 0");
    m = mix(3, 6, 1e308, 1e308, 0.0);  // (each finite, the sum is not)
    REFUSED(move_spec_check(&m), "move mix: the weights must have a finite sum > 0");
    // the DE move: halves of 1 and 2
    m = mix(1, 2, 0.0, 1.0, 0.0);
    REFUSED(move_spec_check(&m), "move mix: the DE move needs two walkers of the other half, n_walkers >= 4, got 2");
    m = mix(1, 4, 0.0, 1.0, 0.0);
    EQ(move_spec_check(&m), VAG_OK);
    // the snooker move: halves of 2 and 3, whatever the size of its weight
    m = mix(1, 4, 0.0, 0.0, 1.0);
    REFUSED(move_spec_check(&m), "move mix: the snooker move needs three walkers of the other half, n_walkers >= 6, got 4");
    m = mix(1, 4, 1.0, 0.0, 1e-300);
    REFUSED(move_spec_check(&m), "move mix: the snooker move needs three walkers of the other half, n_walkers >= 6, got 4");
    m = mix(1, 6, 0.0, 0.0, 1.0);
    EQ(move_spec_check(&m), VAG_OK);
    m = mix(1, 6, 1.0, 0.0, 1e-300);
    EQ(move_spec_check(&m), VAG_OK);
    // a kind of weight 0 asks nothing of the ensemble
    m = mix(1, 2, 1.0, 0.0, 0.0);
    EQ(move_spec_check(&m), VAG_OK);
    m = mix(1, 4, 0.0, 1.0, 0.0);
    EQ(move_spec_check(&m), VAG_OK);
    // gamma0 finite and >= 0 (0: the default), sigma and gamma_snooker finite
    m = mix(3, 6, 0.0, 0.8, 0.2);
    m.gamma0 = -1e-300;
    REFUSED(move_spec_check(&m), "move mix: gamma0 must be finite and >= 0 (0: 2.38 / sqrt(2 ndim)), got -1e-300");
    m.gamma0 = NAN_;
    EQ(move_spec_check(&m), VAG_E_INVALID);
    m.gamma0 = 0.0;
    EQ(move_spec_check(&m), VAG_OK);
    m.sigma = INF;
    REFUSED(move_spec_check(&m), "move mix: sigma must be finite, got inf");
    m.sigma = 1e-5;
    m.gamma_snooker = -INF;
    REFUSED(move_spec_check(&m), "move mix: gamma_snooker must be finite, got -inf");
    done("move spec", f);
}

static void kinds() {
    const int f = g_failed;
    // RUN_SEED = 7 of tests/test_moves.py, the reference mix: DE, snooker, DE, snooker, DE, DE (its run130 asserts the same of
    // sampling.move_kind)
    const vag_move_spec m = mix(3, 130, 0.0, 0.8, 0.2);
    const int want[6] = {1, 2, 1, 2, 1, 1};
    for (int s = 0; s < 6; ++s) EQ(move_kind(&m, (uint64_t)s), want[s]);
    // one kind with weight: that kind at every step
    const vag_move_spec only_stretch = mix(3, 130, 1.0, 0.0, 0.0), only_snooker = mix(3, 130, 0.0, 0.0, 1.0);
    for (int s = 0; s < 6; ++s) {
        EQ(move_kind(&only_stretch, (uint64_t)s), 0);
        EQ(move_kind(&only_snooker, (uint64_t)s), 2);
    }
    done("move_kind", f);
}

static void ladders() {
    const int f = g_failed;
    double betas[65];
    for (int t = 0; t < 65; ++t) betas[t] = 1.0 - t / 128.0;  // strictly descending from 1, all > 0
    TemperLadder ladder;
    vag_tempered_spec s{5, 2.0, 3, 8, 3, 1, betas};
    EQ(tempered_spec_check(&s, ladder), VAG_OK);
    // the common checks come first, under the stretch move's prefix
    s.thin = 0;
    REFUSED(tempered_spec_check(&s, ladder), "stretch move: thin must be >= 1, got 0");
    s.thin = 1;
    // n_temps 1..64
    s.n_temps = 0;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: n_temps must be 1..64, got 0");
    s.n_temps = 1;
    EQ(tempered_spec_check(&s, ladder), VAG_OK);
    s.n_temps = 64;
    EQ(tempered_spec_check(&s, ladder), VAG_OK);
    s.n_temps = 65;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: n_temps must be 1..64, got 65");
    // n_temps * n_walkers <= 2^30: 64 * 2^24 is 2^30, two walkers more per rung are 128 above
    s.n_temps = 64;
    s.n_walkers = 16777216;
    EQ(tempered_spec_check(&s, ladder), VAG_OK);
    s.n_walkers = 16777218;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: n_temps * n_walkers must not exceed 2^30, got 1073741952");
    s.n_walkers = 8;
    // the ladder: there, from 1, finite, strictly descending, >= 0
    s.n_temps = 3;
    s.betas = nullptr;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: null betas");
    const double from_half[3] = {0.5, 0.25, 0.125}, equal[3] = {1.0, 0.5, 0.5}, rising[3] = {1.0, 0.5, 0.75}, negative[2] = {1.0, -0.1},
                 infinite[2] = {1.0, -INF}, to_zero[3] = {1.0, 0.5, 0.0}, plain[3] = {1.0, 0.5, 0.25};
    s.betas = from_half;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: betas[0] must be 1, got 0.5");
    s.betas = equal;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: betas must be finite, strictly descending and >= 0; betas[2] = 0.5");
    s.betas = rising;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: betas must be finite, strictly descending and >= 0; betas[2] = 0.75");
    s.n_temps = 2;
    s.betas = negative;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: betas must be finite, strictly descending and >= 0; betas[1] = -0.1");
    s.betas = infinite;
    REFUSED(tempered_spec_check(&s, ladder), "tempering: betas must be finite, strictly descending and >= 0; betas[1] = -inf");
    s.n_temps = 3;
    s.betas = to_zero;
    EQ(tempered_spec_check(&s, ladder), VAG_OK);
    // filled, and zero beyond n_temps whatever it held
    for (int t = 0; t < 64; ++t) ladder.beta[t] = 7.0;
    s.betas = plain;
    EQ(tempered_spec_check(&s, ladder), VAG_OK);
    EQ(ladder.beta[0] == 1.0 && ladder.beta[1] == 0.5 && ladder.beta[2] == 0.25, 1);
    for (int t = 3; t < 64; ++t) EQ(ladder.beta[t] == 0.0, 1);
    EQ(sizeof(TemperLadder), 512);
    done("tempered spec", f);
}

static void run_arguments() {
    const int f = g_failed;
    // the chain pointers: all or none
    EQ(run_chain_check("stretch move", "the chain and its ln p", 0, 2), VAG_OK);
    EQ(run_chain_check("stretch move", "the chain and its ln p", 2, 2), VAG_OK);
    REFUSED(run_chain_check("stretch move", "the chain and its ln p", 1, 2),
            "stretch move: the chain and its ln p are stored together or not at all");
    REFUSED(run_chain_check("move mix", "the chain and its ln p", 1, 2), "move mix: the chain and its ln p are stored together or not at all");
    EQ(run_chain_check("tempering", "the chain, its ln L and its ln prior", 0, 3), VAG_OK);
    EQ(run_chain_check("tempering", "the chain, its ln L and its ln prior", 3, 3), VAG_OK);
    REFUSED(run_chain_check("tempering", "the chain, its ln L and its ln prior", 1, 3),
            "tempering: the chain, its ln L and its ln prior are stored together or not at all");
    REFUSED(run_chain_check("tempering", "the chain, its ln L and its ln prior", 2, 3),
            "tempering: the chain, its ln L and its ln prior are stored together or not at all");
    // ndim is the fit spec's; n_steps >= 0
    EQ(run_steps_check("stretch move", 3, 3, 0), VAG_OK);
    EQ(run_steps_check("stretch move", 3, 3, 1), VAG_OK);
    REFUSED(run_steps_check("stretch move", 3, 2, 1), "stretch move: ndim 3 is not the fit spec's 2");
    REFUSED(run_steps_check("move mix", 2, 3, -1), "move mix: ndim 2 is not the fit spec's 3");  // (ndim is looked at first)
    REFUSED(run_steps_check("tempering", 3, 3, -1), "tempering: n_steps must be >= 0, got -1");
    done("run arguments", f);
}

static void arithmetic() {
    const int f = g_failed;
    // the key: the seed's low and high word
    const SeedWords k = seed_words(0x0123456789abcdefull);
    EQ(k.lo, 0x89abcdefll);
    EQ(k.hi, 0x01234567ll);
    const SeedWords small = seed_words(7);
    EQ(small.lo, 7);
    EQ(small.hi, 0);
    EQ(half_of(2), 1);
    EQ(half_of(6), 3);
    EQ(half_of(130), 65);
    // 256 lanes a group
    EQ(STRETCH_LANES, 256);
    EQ(lane_groups(1), 1);
    EQ(lane_groups(256), 1);
    EQ(lane_groups(257), 2);
    EQ(lane_groups(512), 2);
    EQ(lane_groups(1ll << 30), 4194304);  // the largest ladder, were it one half
    // step s is stored when (s + 1) % thin == 0: thin 1, 2, 3 from step0 = 0 and from step0 = 5
    const int thin2_from0[6] = {0, 1, 0, 1, 0, 1}, thin3_from0[6] = {0, 0, 1, 0, 0, 1};
    const int thin2_from5[6] = {1, 0, 1, 0, 1, 0}, thin3_from5[6] = {1, 0, 0, 1, 0, 0};
    for (int k2 = 0; k2 < 6; ++k2) {
        EQ(step_is_stored((uint64_t)k2, 1), 1);
        EQ(step_is_stored((uint64_t)(5 + k2), 1), 1);
        EQ(step_is_stored((uint64_t)k2, 2), thin2_from0[k2]);
        EQ(step_is_stored((uint64_t)k2, 3), thin3_from0[k2]);
        EQ(step_is_stored((uint64_t)(5 + k2), 2), thin2_from5[k2]);
        EQ(step_is_stored((uint64_t)(5 + k2), 3), thin3_from5[k2]);
    }
    EQ(step_is_stored(0xffffffffull, 2), 1);  // (2^32 is even: the sum is taken in 64 bits)
    // the pairs (t, t + 1) with t + step even, T = 1..5
    const int even_step[5] = {0, 1, 1, 2, 2}, odd_step[5] = {0, 0, 1, 1, 2};
    for (int T = 1; T <= 5; ++T) {
        EQ(swap_pairs(T, 0), even_step[T - 1]);
        EQ(swap_pairs(T, 4), even_step[T - 1]);
        EQ(swap_pairs(T, 1), odd_step[T - 1]);
        EQ(swap_pairs(T, 0x100000001ull), odd_step[T - 1]);
    }
    // row `row` of [rows][nw][width] and of [rows][T][nw][width]
    EQ(ensemble_row_offset(0, 130, 3), 0);
    EQ(ensemble_row_offset(3, 130, 3), 1170);
    EQ(ensemble_row_offset(3, 130, 1), 390);
    EQ(ladder_row_offset(0, 3, 130, 3), 0);
    EQ(ladder_row_offset(2, 3, 130, 3), 2340);
    EQ(ladder_row_offset(2, 3, 130, 1), 780);
    EQ(ensemble_row_offset(1u << 20, 1 << 20, 16), 17592186044416ll);   // 2^44: in size_t, not in int
    EQ(ladder_row_offset(1u << 10, 64, 1 << 24, 16), 17592186044416ll);  // 2^10 2^30 2^4
    done("arithmetic", f);
}

int main() {
    shape();
    moves();
    kinds();
    ladders();
    run_arguments();
    arithmetic();
    if (g_failed) std::printf("FAIL %d checks\n", g_failed);
    return g_failed ? 1 : 0;
}
