// robust_check.cpp -- the host side of the outlier groups (csrc/vag_fit_request.h: robust_scan, RobustLayout, the request's twelfth
// block, the slot acceptance of fit_accepts) and their row term (csrc/vag_robust.h) run on their own, for the host sanitizers:
// tests/test_outliers_host.py builds it with -fsanitize=address,undefined and runs it.  No device, no context, no HIP.
//
// The fit spec has 3 point rows and two band groups of 2 and 3 rows; the noise spec three groups: 0 (point rows 0 and 2, band group
// 1), 1 (point row 1) and 2 (band group 0, calibration 0.1).  Every input array lives on the heap at exactly its advertised length.
// One "ok <case>" line per case.
#include <cstdio>
#include <initializer_list>
#include <memory>

#include "../include/vegasafterglow_amd.h"
#include "../vegasafterglow_amd/csrc/vag_fit_request.h"
#include "../vegasafterglow_amd/csrc/vag_robust.h"

static std::vector<std::shared_ptr<void>> g_keep;
static int g_failed = 0;

template <class T>
static T* heap(std::initializer_list<T> v) {
    T* p = new T[v.size()];
    std::copy(v.begin(), v.end(), p);
    g_keep.emplace_back(p, [](void* q) { delete[] static_cast<T*>(q); });
    return p;
}
static const double* D(std::initializer_list<double> v) { return heap<double>(v); }
static const int32_t* I(std::initializer_list<int32_t> v) { return heap<int32_t>(v); }

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

static void done(const char* name, int failed_before) {
    if (g_failed == failed_before) std::printf("ok %s\n", name);
}

static vag_fit_spec fit_spec() {
    vag_fit_spec s{};
    s.ndim = 1;
    s.slot[0] = 0;
    s.n_data = 3;
    s.t = D({1e5, 2e5, 3e5});
    s.n_bands = 2;
    vag_band_obs b0{}, b1{};
    b0.n = 2, b0.t = D({1e5, 2e5}), b0.ln_flux = D({-1.0, -2.0}), b0.ln_err = D({0.1, 0.1}), b0.weight = D({1.0, 1.0});
    b1.n = 3, b1.t = D({1e5, 2e5, 3e5}), b1.ln_flux = D({-1.0, -2.0, -3.0}), b1.ln_err = D({0.1, 0.1, 0.1}), b1.weight = D({1.0, 1.0, 1.0});
    s.bands = heap<vag_band_obs>({b0, b1});
    return s;
}

static vag_noise_fit_spec noise_spec() {
    vag_noise_fit_spec nz{};
    nz.n_groups = 3;
    nz.n_bands = 2;
    nz.point_group = I({0, 1, 0});
    nz.band_group = I({2, 0});
    nz.calib[2] = 0.1;
    return nz;
}

static vag_robust_fit_spec robust_spec() {  // groups 0 and 1 robust
    vag_robust_fit_spec rb{};
    rb.n_groups = 3;
    rb.mask = 0x3u;
    rb.frac_fixed[0] = 0.25, rb.frac_fixed[1] = 0.5;
    rb.scale_fixed[0] = 1.5, rb.scale_fixed[1] = 0.0;
    rb.shift_fixed[0] = -0.75, rb.shift_fixed[1] = 2.0;
    return rb;
}

static bool refused(int rc, const char* word) {
    const bool ok = rc == VAG_E_INVALID && g_err.find(word) != std::string::npos;
    if (!ok) std::printf("  got rc %d, message \"%s\", wanted \"%s\"\n", rc, g_err.c_str(), word);
    return ok;
}

static void scan_layout() {
    const int before = g_failed;
    const vag_fit_spec spec = fit_spec();
    const vag_noise_fit_spec nz = noise_spec();
    const vag_robust_fit_spec rb = robust_spec();
    std::vector<double> stage;
    RobustLayout lay;
    CHECK(robust_scan(&spec, &nz, nullptr, &rb, stage, lay) == VAG_OK);
    CHECK(stage.size() == 24 && lay.doubles == 24 && ROBUST_STAGE_DOUBLES == 24);
    const double want[24] = {0.25, 0.5, 0, 0, 0, 0, 0, 0, 1.5, 0.0, 0, 0, 0, 0, 0, 0, -0.75, 2.0, 0, 0, 0, 0, 0, 0};
    CHECK(stage.size() == 24 && std::memcmp(stage.data(), want, sizeof want) == 0);
    CHECK(lay.any && lay.mask == 0x3u && lay.point && lay.band.size() == 2 && !lay.band[0] && lay.band[1]);
    // the key: the same bytes under another mask are another block; another value is another block
    vag_robust_fit_spec other = rb;
    other.mask = 0x1u;
    std::vector<double> stage2;
    RobustLayout lay2;
    CHECK(robust_scan(&spec, &nz, nullptr, &other, stage2, lay2) == VAG_OK && stage2 == stage && lay2.hash != lay.hash);
    CHECK(lay2.point && lay2.band[1] && lay2.mask == 0x1u);
    other = rb;
    other.shift_fixed[1] = 2.5;
    RobustLayout lay3;
    CHECK(robust_scan(&spec, &nz, nullptr, &other, stage2, lay3) == VAG_OK && lay3.hash != lay.hash);
    RobustLayout lay4;
    CHECK(robust_scan(&spec, &nz, nullptr, &rb, stage2, lay4) == VAG_OK && lay4.hash == lay.hash && lay4.doubles == lay.doubles);
    // limit rows are no detection rows: group 1 holds point row 1 alone; with that row a limit and the mask naming group 1 only,
    // nothing is left; band group 1 with every row a limit leaves the point rows
    vag_limit_fit_spec lim{};
    lim.point = {I({VAG_OBS_DETECTION, VAG_OBS_UPPER_LIMIT, VAG_OBS_DETECTION}), D({0.0, 2.5, 0.0}), D({1.0, 0.5, 1.0})};
    other = rb;
    other.mask = 0x2u;
    RobustLayout lay5;
    CHECK(robust_scan(&spec, &nz, &lim, &other, stage2, lay5) == VAG_OK && !lay5.any && !lay5.point && !lay5.band[0] && !lay5.band[1]);
    const int32_t lm = VAG_OBS_UPPER_LIMIT;
    lim.n_bands = 2;
    lim.bands = heap<vag_limit_rows>({{nullptr, nullptr, nullptr}, {I({lm, lm, lm}), D({1.0, 1.0, 1.0}), D({0.5, 0.5, 0.5})}});
    RobustLayout lay6;
    CHECK(robust_scan(&spec, &nz, &lim, &rb, stage2, lay6) == VAG_OK && lay6.any && lay6.point && !lay6.band[1]);
    // no group is robust: accepted, and nothing to do
    other = rb;
    other.mask = 0;
    RobustLayout lay7;
    CHECK(robust_scan(&spec, &nz, nullptr, &other, stage2, lay7) == VAG_OK && !lay7.any && lay7.mask == 0);
    done("robust_scan layout", before);
}

static void scan_refusals() {
    const int before = g_failed;
    const vag_fit_spec spec = fit_spec();
    vag_noise_fit_spec nz = noise_spec();
    std::vector<double> stage;
    auto scan = [&](const vag_robust_fit_spec& rb, const vag_noise_fit_spec* noise) {
        RobustLayout lay;
        return robust_scan(&spec, noise, nullptr, &rb, stage, lay);
    };
    vag_robust_fit_spec rb = robust_spec();
    CHECK(scan(rb, &nz) == VAG_OK);
    CHECK(refused(scan(rb, nullptr), "need a noise block"));
    rb.n_groups = 2;
    CHECK(refused(scan(rb, &nz), "n_groups must be the noise spec's 3, got 2"));
    rb = robust_spec();
    rb.mask = 0x8u;
    CHECK(refused(scan(rb, &nz), "at or above n_groups = 3"));
    rb.mask = 0x80000000u;
    CHECK(refused(scan(rb, &nz), "at or above n_groups = 3"));
    rb = robust_spec();
    rb.mask = 0x4u;
    CHECK(refused(scan(rb, &nz), "outlier group 2 has a calibration fraction"));
    const double nan = std::nan(""), inf = INFINITY;
    for (double v : {nan, inf, -inf, -0.1, 1.0, 1.5}) {
        rb = robust_spec();
        rb.frac_fixed[1] = v;
        CHECK(refused(scan(rb, &nz), "outlier group 1: the outlier fraction"));
    }
    for (double v : {nan, inf, -1e-300}) {
        rb = robust_spec();
        rb.scale_fixed[0] = v;
        CHECK(refused(scan(rb, &nz), "outlier group 0: the outlier scatter"));
    }
    for (double v : {nan, inf, -inf}) {
        rb = robust_spec();
        rb.shift_fixed[1] = v;
        CHECK(refused(scan(rb, &nz), "outlier group 1: the outlier offset"));
    }
    rb = robust_spec();  // the edges that are accepted
    rb.frac_fixed[0] = 0.0, rb.frac_fixed[1] = std::nextafter(1.0, 0.0), rb.scale_fixed[0] = 0.0, rb.shift_fixed[0] = -1e300;
    CHECK(scan(rb, &nz) == VAG_OK);
    // through fit_request_prepare, behind the noise scan's own refusals
    {
        FitRequest r = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &rb);
        CHECK(refused(fit_request_prepare(r), "need a noise block"));
        rb.mask = 0x4u;
        FitRequest q = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz, nullptr, nullptr, nullptr, nullptr, nullptr, &rb);
        CHECK(refused(fit_request_prepare(q), "outlier group 2"));
        nz.n_groups = 9;
        FitRequest p = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz, nullptr, nullptr, nullptr, nullptr, nullptr, &rb);
        CHECK(refused(fit_request_prepare(p), "noise groups: n_groups"));
    }
    done("robust_scan refusal", before);
}

static bool accepts(FitRequest& r) { return fit_scan(r.spec, r.spec->ndim, fit_accepts(r), r.fit) == VAG_OK; }

static void prepare_and_slots() {
    int before = g_failed;
    vag_fit_spec spec = fit_spec();
    const vag_noise_fit_spec nz = noise_spec();
    vag_robust_fit_spec rb = robust_spec();
    {  // a full block stays, and the eleven-block spelling of the request leaves the member null
        FitRequest r = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz, nullptr, nullptr, nullptr, nullptr, nullptr, &rb);
        CHECK(fit_request_prepare(r) == VAG_OK && r.robust == &rb && r.noise == &nz && r.rlay.any && r.rstage.size() == 24);
        FitRequest narrow = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz);
        CHECK(fit_request_prepare(narrow) == VAG_OK && narrow.robust == nullptr && !narrow.rlay.any && narrow.rlay.mask == 0);
    }
    {  // no robust group: the block is nulled, the request is the noise request
        vag_robust_fit_spec none = rb;
        none.mask = 0;
        FitRequest r = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz, nullptr, nullptr, nullptr, nullptr, nullptr, &none);
        CHECK(fit_request_prepare(r) == VAG_OK && r.robust == nullptr && r.noise == &nz);
    }
    {  // the only robust group's only row is a limit: nulled, its slots still accepted
        vag_limit_fit_spec lim{};
        lim.point = {I({VAG_OBS_DETECTION, VAG_OBS_UPPER_LIMIT, VAG_OBS_DETECTION}), D({0.0, 2.5, 0.0}), D({1.0, 0.5, 1.0})};
        vag_robust_fit_spec one = rb;
        one.mask = 0x2u;
        FitRequest r = fit_request(&spec, nullptr, nullptr, nullptr, &lim, &nz, nullptr, nullptr, nullptr, nullptr, nullptr, &one);
        CHECK(fit_request_prepare(r) == VAG_OK && r.robust == nullptr && r.noise == &nz && r.lim == &lim && r.rlay.mask == 0x2u);
        spec.slot[0] = VAG_P_ROBUST_SCALE0 + 1;
        CHECK(accepts(r));
        spec.slot[0] = VAG_P_ROBUST_SCALE0 + 0;
        CHECK(!accepts(r) && g_err == "bad parameter slot");
    }
    done("fit_request_prepare robust block", before);

    before = g_failed;
    CHECK(VAG_P_ROBUST_FRAC0 == VAG_P_TMPL_AMP0 + VAG_TMPL_MAX && VAG_P_ROBUST_SCALE0 == VAG_P_ROBUST_FRAC0 + VAG_NOISE_MAX_GROUPS &&
          VAG_P_ROBUST_SHIFT0 == VAG_P_ROBUST_SCALE0 + VAG_NOISE_MAX_GROUPS);
    CHECK(robust_slot_group(VAG_P_ROBUST_FRAC0) == 0 && robust_slot_group(VAG_P_ROBUST_FRAC0 + 7) == 7 &&
          robust_slot_group(VAG_P_ROBUST_SCALE0 + 3) == 3 && robust_slot_group(VAG_P_ROBUST_SHIFT0 + 7) == 7 &&
          robust_slot_group(VAG_P_ROBUST_SHIFT0 + 8) == -1 && robust_slot_group(VAG_P_TMPL_AMP0 + 7) == -1 && robust_slot_group(0) == -1);
    FitRequest with = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz, nullptr, nullptr, nullptr, nullptr, nullptr, &rb);
    FitRequest noise_only = fit_request(&spec, nullptr, nullptr, nullptr, nullptr, &nz);
    FitRequest plain = fit_request(&spec);
    CHECK(fit_request_prepare(with) == VAG_OK && fit_request_prepare(noise_only) == VAG_OK && fit_request_prepare(plain) == VAG_OK);
    CHECK(fit_accepts(with).robust_mask == 0x3u && fit_accepts(noise_only).robust_mask == 0 && fit_accepts(plain).robust_mask == 0);
    for (int base : {VAG_P_ROBUST_FRAC0, VAG_P_ROBUST_SCALE0, VAG_P_ROBUST_SHIFT0})
        for (int g = 0; g < VAG_NOISE_MAX_GROUPS; ++g) {
            spec.slot[0] = base + g;
            CHECK(accepts(with) == (g < 2));  // groups 0 and 1 are robust; 2 is a plain noise group; 3 .. 7 do not exist
            CHECK(!accepts(noise_only) && g_err == "bad parameter slot");
            CHECK(!accepts(plain));
        }
    spec.slot[0] = VAG_P_ROBUST_SHIFT0 + VAG_NOISE_MAX_GROUPS;  // the first slot behind the three families
    CHECK(!accepts(with) && g_err == "bad parameter slot");
    spec.slot[0] = VAG_P_NOISE_SYS0 + 2;  // the systematic of every noise group stays accepted
    CHECK(accepts(with) && accepts(noise_only) && !accepts(plain));
    done("robust slots", before);
}

// the definition in long double, from the group's P itself
static long double ref_lnl(double r, double sig, double s, double b, double mu, double P) {
    const long double sig2 = (long double)sig * sig, s2 = (long double)s * s, b2 = (long double)b * b, rr = r, d = (long double)r - mu;
    const long double g = log1pl(-(long double)P) - 0.5L * rr * rr / (sig2 + s2) - 0.5L * log1pl(s2 / sig2);
    if (P == 0.0) return g;
    const long double o = logl((long double)P) - 0.5L * d * d / (sig2 + s2 + b2) - 0.5L * log1pl((s2 + b2) / sig2);
    const long double hi = g > o ? g : o, lo = g > o ? o : g;
    return hi + log1pl(expl(lo - hi));
}

static void row_term() {
    const int before = g_failed;
    // Every term of g and of o is <= 0, so neither sum cancels: each of the dozen roundings (and the C library's log, log1p and exp,
    // below 1 ulp each) is at most an ulp of a quantity no larger than max(1, |l|) up to a factor 2.  32 eps covers that with room;
    // an algebra error shows at 1e-3 and above.
    const double gate = 32 * 2.220446049250313e-16;
    double worst = 0;
    int cases = 0;
    const double sig = 0.1;
    for (double P : {0.0, 1e-300, 1e-12, 0.15, 0.5, 1.0 - 1e-12, std::nextafter(1.0, 0.0)})
        for (double b : {0.0, 0.3, 1.5, 50.0})
            for (double s : {0.0, 0.05, 2.0})
                for (double mu : {0.0, 0.7, -3.0})
                    for (double k : {0.0, 1e-3, 0.5, 1.0, 3.0, 10.0, 37.0, 100.0, 1e3})
                        for (double sign : {1.0, -1.0}) {
                            const double r = sign * k * sig;
                            const double got = vag::robust_row_lnl(r, sig * sig, s * s, b * b, mu, std::log1p(-P), std::log(P));
                            const long double want = ref_lnl(r, sig, s, b, mu, P);
                            const double err = (double)(fabsl((long double)got - want) / fmaxl(1.0L, fabsl(want)));
                            worst = std::fmax(worst, err);
                            ++cases;
                            if (!(std::isfinite(got) && err <= gate))
                                std::printf("  P %g b %g s %g mu %g r %g: got %.17g want %.17Lg err %g\n", P, b, s, mu, r, got, want, err);
                            CHECK(std::isfinite(got) && err <= gate);
                            if (P == 0.0) {  // l = g to the bit: the noise group's term of the row
                                const double g = std::log1p(-0.0) - 0.5 * (r * r) / (sig * sig + s * s) - 0.5 * std::log1p(s * s / (sig * sig));
                                CHECK(got == g);
                            }
                        }
    std::printf("  robust_row_lnl: %d cases, worst |got - want| / max(1, |want|) = %.3g (gate %.3g)\n", cases, worst, gate);
    // b = 0 with mu = 0: both components are the same Gaussian, l = g(P = 0) for every P
    for (double P : {1e-12, 0.3, 1.0 - 1e-12}) {
        const double a = vag::robust_row_lnl(0.25, 0.01, 0.0025, 0.0, 0.0, std::log1p(-P), std::log(P));
        const double z = vag::robust_row_lnl(0.25, 0.01, 0.0025, 0.0, 0.0, 0.0, -INFINITY);
        CHECK(std::fabs(a - z) <= gate * std::fmax(1.0, std::fabs(z)));
    }
    // a NaN or infinite residual stays NaN, whatever P
    for (double P : {0.0, 0.15})
        for (double r : {(double)NAN, (double)INFINITY, -(double)INFINITY})
            CHECK(std::isnan(vag::robust_row_lnl(r, 0.01, 0.0, 2.25, 0.0, std::log1p(-P), std::log(P))));
    done("robust_row_lnl", before);
}

int main() {
    scan_layout();
    scan_refusals();
    prepare_and_slots();
    row_term();
    if (g_failed) std::printf("FAIL %d checks\n", g_failed);
    return g_failed ? 1 : 0;
}
