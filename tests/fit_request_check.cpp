// fit_request_check.cpp -- the host side of a likelihood request (csrc/vag_fit_request.h) run on its own, for the host sanitizers:
// tests/test_fit_request_host.py builds it with -fsanitize=address,undefined and runs it.  No device, no context, no HIP.
//
// Every scan lays out one accepted spec at the smallest shapes that reach every branch of its layout arithmetic; the offsets of its
// *Layout and every staged double and int32 are compared with what this file writes down from the documented layout, not with anything
// the scan computed.  Every input array lives on the heap at exactly its advertised length, so a read one element past it is an
// AddressSanitizer report.  Then two requests through fit_request_prepare, and one refusal per scan.  One "ok <case>" line per case.
#include <cstdio>
#include <initializer_list>
#include <memory>

#include "../include/vegasafterglow_amd.h"
#include "../vegasafterglow_amd/csrc/vag_fit_request.h"

static std::vector<std::shared_ptr<void>> g_keep;
static int g_failed = 0;

// a heap array of exactly these elements
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

// what a block must hold, written down field by field: doubles, and int32 arrays in (n + 1) / 2 doubles whose padding is zero
struct Want {
    std::vector<double> v;
    Want& d(std::initializer_list<double> x) {
        v.insert(v.end(), x);
        return *this;
    }
    Want& i(std::initializer_list<int32_t> x) {
        const size_t at = v.size();
        v.resize(at + (x.size() + 1) / 2, 0.0);
        std::memcpy(v.data() + at, x.begin(), sizeof(int32_t) * x.size());
        return *this;
    }
};

static bool same_bytes(const std::vector<double>& got, const Want& w) {
    return got.size() == w.v.size() && std::memcmp(got.data(), w.v.data(), sizeof(double) * got.size()) == 0;
}

// the int32 view of the block at `off` doubles: what the kernels read there
static bool ints_at(const std::vector<double>& stage, long off, std::initializer_list<int32_t> want) {
    if (off < 0 || (size_t)off + (want.size() + 1) / 2 > stage.size()) return false;
    size_t k = 0;
    for (int32_t w : want) {
        int32_t got;
        std::memcpy(&got, reinterpret_cast<const char*>(stage.data() + off) + sizeof(int32_t) * k++, sizeof got);
        if (got != w) return false;
    }
    return true;
}

static bool longs(const std::vector<long>& got, std::initializer_list<long> want) { return got == std::vector<long>(want); }

static void done(const char* name, int failed_before) {
    if (g_failed == failed_before) std::printf("ok %s\n", name);
}

// S(N) = N ln N - N - ln N! from the C library, to hold const2 = -2 sum w S against
static double S_ref(double N) { return N > 0 ? N * std::log(N) - N - std::lgamma(N + 1.0) : 0.0; }
static bool near_eq(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(1.0, std::fabs(b)); }

// the fit spec every case annotates: 3 point rows (n odd) and two band groups of 2 and 3 rows; the scans read the shapes only
static vag_fit_spec fit_spec() {
    vag_fit_spec s{};
    s.ndim = 1;
    s.slot[0] = VAG_P_N_H;
    s.n_data = 3;
    s.t = D({1e5, 2e5, 3e5});
    s.n_bands = 2;
    vag_band_obs b0{}, b1{};
    b0.n = 2;
    b1.n = 3;
    s.bands = heap<vag_band_obs>({b0, b1});
    return s;
}

static vag_pol_fit_spec pol_spec() {  // one degree group of 3 epochs
    vag_polarization_obs o{};
    o.nu = 3e9, o.n = 3, o.kind = VAG_POL_DEGREE;
    o.t = D({1e5, 2e5, 3e5});
    o.q = D({0.1, 0.2, 0.3});
    o.err_q = D({0.01, 0.02, 0.03});
    o.weight = D({1.0, 1.0, 1.0});
    vag_pol_fit_spec p{};
    p.n_groups = 1;
    p.groups = heap<vag_polarization_obs>({o});
    return p;
}

// ---- the accepted specs
static vag_limit_fit_spec lim_spec() {  // a limit row among the point rows, in the second band group only, and a limit epoch
    const int32_t det = VAG_OBS_DETECTION, lim = VAG_OBS_UPPER_LIMIT;
    vag_limit_fit_spec l{};
    l.point = {I({det, lim, det}), D({9.0, 2.5, 9.0}), D({9.0, 0.5, 9.0})};
    l.n_bands = 2;
    l.bands = heap<vag_limit_rows>({{I({det, det}), nullptr, nullptr}, {I({lim, det, det}), D({1.5, 7.0, 7.0}), D({0.25, 7.0, 7.0})}});
    l.n_pol_groups = 1;
    l.pol_kind = heap<const int32_t*>({I({det, det, lim})});
    return l;
}

static vag_noise_fit_spec noise_spec() {  // point rows in both groups and in none; the first band group in group 1, the second in none
    vag_noise_fit_spec z{};
    z.n_groups = 2, z.n_bands = 2;
    z.point_group = I({0, -1, 1});
    z.band_group = I({1, -1});
    z.sys_fixed[0] = 0.1, z.sys_fixed[1] = 0.2;
    z.calib[0] = 0.05;
    return z;
}

static vag_template_fit_spec tmpl_spec() {  // template 0 extinguished and nowhere, template 1 on two point rows; no band row touched
    vag_template_fit_spec t{};
    t.n_templates = 2, t.n_bands = 2;
    t.point = D({0.0, 0.0, 0.0, 0.5, 0.0, 1.5});
    t.bands = heap<const double*>({D({0.0, 0.0, 0.0, 0.0}), nullptr});
    t.amp_fixed[0] = 2.0, t.amp_fixed[1] = 3.0;
    t.extinguished[0] = 1;
    return t;
}

static vag_counts_fit_spec counts_spec() {  // n m = 3 (odd) and 6 (even)
    vag_counts_obs a{}, b{};
    a.nu_min = 1e17, a.nu_max = 2e17, a.num_points = 5, a.n = 3, a.m = 1, a.n_samples = 3;
    a.t_sample = D({1e4, 2e4, 3e4});
    a.sample_idx = I({0, 1, 2});
    a.counts = D({0.0, 5.0, 40.0}), a.background = D({0.5, 0.25, 0.0}), a.scale = D({1.0, 2.0, 3.0}), a.weight = D({1.0, 0.0, 0.5});
    b.nu_min = 2e17, b.nu_max = 3e17, b.num_points = 2, b.n = 2, b.m = 3, b.n_samples = 4;
    b.t_sample = D({1e4, 2e4, 3e4, 4e4});
    b.sample_idx = I({0, 1, 2, 1, 2, 3});
    b.counts = D({17.0, 3.0}), b.background = D({0.0, 1.0}), b.scale = D({4.0, 5.0}), b.weight = D({2.0, 1.0});
    vag_counts_fit_spec c{};
    c.n_groups = 2;
    c.groups = heap<vag_counts_obs>({a, b});
    return c;
}

static vag_index_fit_spec index_spec() {  // n = 3, K = 2 and n = 1, K = VAG_INDEX_MAX_NODES
    static_assert(VAG_INDEX_MAX_NODES == 8, "the second group below has 8 frequencies");
    vag_index_obs a{}, b{};
    a.n = 3, a.k = 2, a.ext_slope = 0.0;
    a.nu = D({1e9, 2e9}), a.coef = D({-1.0, 1.0});
    a.t = D({1e5, 2e5, 3e5}), a.value = D({-0.5, -0.6, -0.7}), a.err = D({0.1, 0.2, 0.3}), a.weight = D({1.0, 0.0, 2.0});
    b.n = 1, b.k = 8, b.ext_slope = 0.25;
    b.nu = D({1e9, 2e9, 3e9, 4e9, 5e9, 6e9, 7e9, 8e9}), b.coef = D({0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0});
    b.t = D({5e5}), b.value = D({0.3}), b.err = D({0.05}), b.weight = D({1.5});
    vag_index_fit_spec s{};
    s.n_groups = 2;
    s.groups = heap<vag_index_obs>({a, b});
    return s;
}

static vag_fold_fit_spec fold_spec() {  // J = C = n = m = 1 without sigma; J = 3, C = 2, n = 3, m = 3, 5 sample times, with sigma
    vag_fold_obs a{}, b{};
    a.J = 1, a.C = 1, a.n = 1, a.m = 1, a.n_samples = 1;
    a.nu = D({1e17}), a.A = D({50.0}), a.t_sample = D({1e4}), a.sample_idx = I({0}), a.exposure_over_m = D({100.0});
    a.counts = D({7.0}), a.background = D({0.5}), a.weight = D({1.0});
    b.J = 3, b.C = 2, b.n = 3, b.m = 3, b.n_samples = 5;
    b.nu = D({1e17, 2e17, 3e17}), b.A = D({1.0, 2.0, 3.0, 4.0, 5.0, 6.0}), b.sigma = D({3e-22, 2e-22, 1e-22});
    b.t_sample = D({1e4, 2e4, 3e4, 4e4, 5e4});
    b.sample_idx = I({0, 1, 2, 1, 2, 3, 2, 3, 4});
    b.exposure_over_m = D({10.0, 20.0, 30.0});
    b.counts = D({0.0, 1.0, 20.0, 3.0, 4.0, 100.0}), b.background = D({0.1, 0.2, 0.3, 0.4, 0.5, 0.6});
    b.weight = D({1.0, 0.0, 2.0, 1.0, 0.5, 1.0});
    vag_fold_fit_spec f{};
    f.n_groups = 2;
    f.groups = heap<vag_fold_obs>({a, b});
    f.n_h_fixed = 1e21;
    return f;
}

static vag_cov_fit_spec cov_spec() {  // n = 1 without ext; n = 3 with ext, the whitener's unread upper half not finite
    vag_cov_obs a{}, b{};
    a.n = 1, a.weight = 1.0;
    a.t = D({1e5}), a.nu = D({3e9}), a.ln_flux = D({-60.0}), a.whitener = D({4.0});
    b.n = 3, b.weight = 0.5;
    b.t = D({1e5, 2e5, 2e5}), b.nu = D({1e9, 5e9, 1e9}), b.ln_flux = D({-61.0, -62.0, -63.0}), b.ext = D({0.1, 0.2, 0.3});
    b.whitener = D({1.0, NAN, INFINITY, 2.0, 3.0, NAN, 4.0, 5.0, 6.0});
    vag_cov_fit_spec c{};
    c.n_groups = 2;
    c.groups = heap<vag_cov_obs>({a, b});
    return c;
}

// ---- one case per scan: the layout of the accepted spec
static void check_lim(const vag_fit_spec& spec) {
    const int before = g_failed;
    const vag_pol_fit_spec pol = pol_spec();
    const vag_limit_fit_spec lim = lim_spec();
    std::vector<double> stage;
    LimLayout lay;
    CHECK(lim_scan(&spec, &pol, &lim, stage, lay) == VAG_OK);
    // point rows at 0: [limit 3 | sigma 3 | kind 3 in 2]; band group 0 not stored; band group 1 at 8: [3 | 3 | 3 in 2]; pol group at 16
    CHECK(lay.any && lay.point == 0 && longs(lay.band, {-1, 8}) && longs(lay.pol, {16}));
    CHECK(same_bytes(stage, Want().d({0.0, 2.5, 0.0, 1.0, 0.5, 1.0}).i({0, 1, 0}).d({1.5, 0.0, 0.0, 0.25, 1.0, 1.0}).i({1, 0, 0}).i({0, 0, 1})));
    CHECK(ints_at(stage, 6, {0, 1, 0, 0}) && ints_at(stage, 14, {1, 0, 0, 0}) && ints_at(stage, 16, {0, 0, 1, 0}));
    done("lim_scan layout", before);
}

static void check_noise(const vag_fit_spec& spec) {
    const int before = g_failed;
    const vag_noise_fit_spec nz = noise_spec();
    std::vector<double> stage;
    NoiseLayout lay;
    CHECK(noise_scan(&spec, &nz, stage, lay) == VAG_OK);
    // [sys_fixed 8 | calib 8], the point rows' ids at 16 (3 in 2), band group 0's at 18 (2 in 1); band group 1 not stored
    CHECK(lay.any && lay.n_groups == 2 && lay.point == 16 && longs(lay.band, {18, -1}));
    CHECK(lay.point_present == 3u && lay.band_present == std::vector<unsigned>({2u, 0u}));
    CHECK(same_bytes(stage, Want().d({0.1, 0.2, 0, 0, 0, 0, 0, 0}).d({0.05, 0, 0, 0, 0, 0, 0, 0}).i({0, -1, 1}).i({1, 1})));
    CHECK(ints_at(stage, 16, {0, -1, 1, 0}) && ints_at(stage, 18, {1, 1}));
    done("noise_scan layout", before);
}

static void check_tmpl(const vag_fit_spec& spec) {
    const int before = g_failed;
    const vag_template_fit_spec tp = tmpl_spec();
    std::vector<double> stage;
    TmplLayout lay;
    CHECK(tmpl_scan(&spec, &tp, stage, lay) == VAG_OK);
    // [amp_fixed 8], the point rows' values [2][3] at 8; neither band group stored
    CHECK(lay.any && lay.n_templates == 2 && lay.ext_mask == 1u && lay.point == 8 && longs(lay.band, {-1, -1}));
    CHECK(lay.point_present == 2u && lay.band_present == std::vector<unsigned>({0u, 0u}));
    CHECK(same_bytes(stage, Want().d({2.0, 3.0, 0, 0, 0, 0, 0, 0}).d({0.0, 0.0, 0.0, 0.5, 0.0, 1.5})));
    done("tmpl_scan layout", before);
}

static void check_counts() {
    const int before = g_failed;
    const vag_counts_fit_spec cs = counts_spec();
    std::vector<double> stage;
    CountsLayout lay;
    CHECK(counts_scan(&cs, stage, lay) == VAG_OK);
    // per group [t_sample ns | N n | B n | a n | w n | idx n m]: 3 + 12 + 2 = 17, then 4 + 8 + 3
    CHECK(lay.n_groups == 2 && longs(lay.off, {0, 17}) && lay.const2.size() == 2);
    CHECK(same_bytes(stage, Want().d({1e4, 2e4, 3e4}).d({0.0, 5.0, 40.0}).d({0.5, 0.25, 0.0}).d({1.0, 2.0, 3.0}).d({1.0, 0.0, 0.5}).i({0, 1, 2})
                                .d({1e4, 2e4, 3e4, 4e4}).d({17.0, 3.0}).d({0.0, 1.0}).d({4.0, 5.0}).d({2.0, 1.0}).i({0, 1, 2, 1, 2, 3})));
    CHECK(ints_at(stage, 15, {0, 1, 2, 0}) && ints_at(stage, 29, {0, 1, 2, 1, 2, 3}));
    if (lay.const2.size() == 2) {
        CHECK(near_eq(lay.const2[0], -2.0 * (1.0 * S_ref(0.0) + 0.5 * S_ref(40.0))));  // (the row of weight 0 is left out)
        CHECK(near_eq(lay.const2[1], -2.0 * (2.0 * S_ref(17.0) + 1.0 * S_ref(3.0))));
    }
    done("counts_scan layout", before);
}

static void check_index() {
    const int before = g_failed;
    const vag_index_fit_spec is = index_spec();
    std::vector<double> stage;
    IndexLayout lay;
    CHECK(index_scan(&is, stage, lay) == VAG_OK);
    // per group [t n K | nu n K | s n | sigma n | w n | c K], the points row-major with the row outer: 6 + 6 + 9 + 2 = 23, then 27
    CHECK(lay.n_groups == 2 && longs(lay.off, {0, 23}));
    CHECK(same_bytes(stage, Want().d({1e5, 1e5, 2e5, 2e5, 3e5, 3e5}).d({1e9, 2e9, 1e9, 2e9, 1e9, 2e9}).d({-0.5, -0.6, -0.7}).d({0.1, 0.2, 0.3})
                                .d({1.0, 0.0, 2.0}).d({-1.0, 1.0})
                                .d({5e5, 5e5, 5e5, 5e5, 5e5, 5e5, 5e5, 5e5}).d({1e9, 2e9, 3e9, 4e9, 5e9, 6e9, 7e9, 8e9}).d({0.3}).d({0.05}).d({1.5})
                                .d({0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0})));
    done("index_scan layout", before);
}

static void check_fold(const vag_fit_spec& spec) {
    const int before = g_failed;
    const vag_fold_fit_spec fs = fold_spec();
    std::vector<double> stage;
    FoldLayout lay;
    CHECK(fold_scan(&spec, &fs, stage, lay) == VAG_OK);  // (the spec frees N_H: accepted, a group has a cross-section)
    // per group [t ns J | nu ns J | A J C | sigma J | exposure / m n | N n C | B n C | w n C | idx n m]: 9 doubles, then
    // 15 + 15 + 6 + 3 + 3 + 6 + 6 + 6 + 5 = 65
    CHECK(lay.n_groups == 2 && lay.any_sigma && longs(lay.off, {0, 9}) && lay.const2.size() == 2);
    CHECK(same_bytes(stage, Want().d({1e4}).d({1e17}).d({50.0}).d({0.0}).d({100.0}).d({7.0}).d({0.5}).d({1.0}).i({0})
                                .d({1e4, 1e4, 1e4, 2e4, 2e4, 2e4, 3e4, 3e4, 3e4, 4e4, 4e4, 4e4, 5e4, 5e4, 5e4})
                                .d({1e17, 2e17, 3e17, 1e17, 2e17, 3e17, 1e17, 2e17, 3e17, 1e17, 2e17, 3e17, 1e17, 2e17, 3e17})
                                .d({1.0, 2.0, 3.0, 4.0, 5.0, 6.0}).d({3e-22, 2e-22, 1e-22}).d({10.0, 20.0, 30.0})
                                .d({0.0, 1.0, 20.0, 3.0, 4.0, 100.0}).d({0.1, 0.2, 0.3, 0.4, 0.5, 0.6}).d({1.0, 0.0, 2.0, 1.0, 0.5, 1.0})
                                .i({0, 1, 2, 1, 2, 3, 2, 3, 4})));
    CHECK(ints_at(stage, 8, {0, 0}) && ints_at(stage, 69, {0, 1, 2, 1, 2, 3, 2, 3, 4, 0}));
    if (lay.const2.size() == 2) {
        CHECK(near_eq(lay.const2[0], -2.0 * S_ref(7.0)));
        CHECK(near_eq(lay.const2[1], -2.0 * (S_ref(0.0) + 2.0 * S_ref(20.0) + S_ref(3.0) + 0.5 * S_ref(4.0) + S_ref(100.0))));
    }
    done("fold_scan layout", before);
}

static void check_cov() {
    const int before = g_failed;
    const vag_cov_fit_spec cs = cov_spec();
    std::vector<double> stage;
    CovLayout lay;
    CHECK(cov_scan(&cs, stage, lay) == VAG_OK);
    // per group [t n | nu n | ln_flux n | ext n | Wt n n], Wt[j n + i] = W_ij for j <= i and 0 elsewhere: 5 doubles, then 12 + 9
    CHECK(lay.n_groups == 2 && longs(lay.off, {0, 5}));
    CHECK(same_bytes(stage, Want().d({1e5}).d({3e9}).d({-60.0}).d({0.0}).d({4.0})
                                .d({1e5, 2e5, 2e5}).d({1e9, 5e9, 1e9}).d({-61.0, -62.0, -63.0}).d({0.1, 0.2, 0.3})
                                .d({1.0, 2.0, 4.0, 0.0, 3.0, 5.0, 0.0, 0.0, 6.0})));
    if (stage.size() == 26) {
        const double* W = cs.groups[1].whitener;
        const double* Wt = stage.data() + 5 + 12;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) CHECK(r <= c ? Wt[r * 3 + c] == W[c * 3 + r] : Wt[r * 3 + c] == 0.0);
    }
    done("cov_scan layout", before);
}

// ---- through fit_request_prepare
static void check_prepare(const vag_fit_spec& spec) {
    int before = g_failed;
    {  // every optional block present, and empty or flagging no row
        const vag_sky_fit_spec sky{};
        const vag_vis_fit_spec vis{};
        const vag_pol_fit_spec pol{};
        vag_limit_fit_spec lim{};
        lim.point.kind = I({VAG_OBS_DETECTION, VAG_OBS_DETECTION, VAG_OBS_DETECTION});
        vag_noise_fit_spec nz{};
        nz.n_bands = 2;
        nz.point_group = I({-1, -1, -1});
        nz.band_group = I({-1, -1});
        vag_template_fit_spec tp{};
        tp.n_templates = 1;
        tp.point = D({0.0, 0.0, 0.0});
        const vag_counts_fit_spec counts{};
        const vag_index_fit_spec index{};
        const vag_fold_fit_spec fold{};
        const vag_cov_fit_spec cov{};
        FitRequest r = fit_request(&spec, &sky, &vis, &pol, &lim, &nz, &counts, &index, &fold, &tp, &cov);
        CHECK(fit_request_prepare(r) == VAG_OK && r.prepared);
        CHECK(!r.sky && !r.vis && !r.pol && !r.lim && !r.noise && !r.counts && !r.index && !r.fold && !r.tmpl && !r.cov && !r.placed);
        CHECK(r.tlay.n_templates == 1);  // (stays: the amplitude slot of the spec's template is still accepted)
        done("fit_request_prepare empty blocks", before);
    }
    before = g_failed;
    {  // every optional block with data
        vag_centroid_obs cen{};
        cen.nu = 3e9, cen.n = 1;
        vag_sky_fit_spec sky{};
        sky.n_groups = 1;
        sky.groups = heap<vag_centroid_obs>({cen});
        vag_visibility_obs vo{};
        vo.n_epochs = 1, vo.n_vis = 1;
        vag_vis_fit_spec vis{};
        vis.n_groups = 1;
        vis.groups = heap<vag_visibility_obs>({vo});
        const vag_pol_fit_spec pol = pol_spec();
        const vag_limit_fit_spec lim = lim_spec();
        const vag_noise_fit_spec nz = noise_spec();
        const vag_template_fit_spec tp = tmpl_spec();
        const vag_counts_fit_spec counts = counts_spec();
        const vag_index_fit_spec index = index_spec();
        const vag_fold_fit_spec fold = fold_spec();
        const vag_cov_fit_spec cov = cov_spec();
        FitRequest r = fit_request(&spec, &sky, &vis, &pol, &lim, &nz, &counts, &index, &fold, &tp, &cov);
        CHECK(fit_request_prepare(r) == VAG_OK && r.prepared && r.placed);
        CHECK(r.sky && r.vis && r.pol && r.lim && r.noise && r.counts && r.index && r.fold && r.tmpl && r.cov);
        CHECK(r.lstage.size() == 18 && r.nstage.size() == 19 && r.tstage.size() == 14 && r.cstage.size() == 32 && r.istage.size() == 50 &&
              r.fstage.size() == 74 && r.vstage.size() == 26);
        done("fit_request_prepare full request", before);
    }
}

// ---- one refusal per scan (the exhaustive lists are the Python host tests', through the C ABI)
static void check_refusals(const vag_fit_spec& spec) {
    auto refused = [](const char* name, int rc) {
        const int before = g_failed;
        CHECK(rc == VAG_E_INVALID);
        CHECK(!g_err.empty());
        g_err.clear();
        done(name, before);
    };
    std::vector<double> stage;
    {
        vag_limit_fit_spec lim{};
        lim.n_bands = 2;  // ... and no band list
        LimLayout lay;
        refused("lim_scan refusal", lim_scan(&spec, nullptr, &lim, stage, lay));
    }
    {
        vag_noise_fit_spec nz{};
        nz.n_bands = 2;
        NoiseLayout lay;
        refused("noise_scan refusal", noise_scan(&spec, &nz, stage, lay));
    }
    {
        vag_template_fit_spec tp{};
        tp.n_bands = 2;
        TmplLayout lay;
        refused("tmpl_scan refusal", tmpl_scan(&spec, &tp, stage, lay));
    }
    {
        vag_counts_fit_spec cs{};
        cs.n_groups = 1;
        CountsLayout lay;
        refused("counts_scan refusal", counts_scan(&cs, stage, lay));
    }
    {
        vag_index_fit_spec is{};
        is.n_groups = 1;
        IndexLayout lay;
        refused("index_scan refusal", index_scan(&is, stage, lay));
    }
    {
        vag_fold_fit_spec fs{};
        fs.n_groups = 1;
        FoldLayout lay;
        refused("fold_scan refusal", fold_scan(&spec, &fs, stage, lay));
    }
    {
        vag_cov_fit_spec cs{};
        cs.n_groups = 1;
        CovLayout lay;
        refused("cov_scan refusal", cov_scan(&cs, stage, lay));
    }
}

int main() {
    const vag_fit_spec spec = fit_spec();
    check_lim(spec);
    check_noise(spec);
    check_tmpl(spec);
    check_counts();
    check_index();
    check_fold(spec);
    check_cov();
    check_prepare(spec);
    check_refusals(spec);
    if (g_failed) std::printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
