// fit_request_check.cpp -- the host side of a likelihood request (csrc/vag_fit_request.h) run on its own, for the host sanitizers:
// tests/test_fit_request_host.py builds it with -fsanitize=address,undefined and runs it.  No device, no context, no HIP.
//
// Every scan lays out one accepted spec at the smallest shapes that reach every branch of its layout arithmetic; the offsets of its
// *Layout and every staged double and int32 are compared with what this file writes down from the documented layout, not with anything
// the scan computed.  Every input array lives on the heap at exactly its advertised length, so a read one element past it is an
// AddressSanitizer report.  The four blocks that are hashed in place (fit, sky, pol, vis) are filled into a heap buffer of exactly the
// scan's size; their hashes are compared across equal and changed content, and every one of their refusals is reached with its text.
// Then two requests through fit_request_prepare, one refusal per scan, the block views (*_cols) against offsets worked out by hand
// with every array read back through them, and the pass list of five requests.  One "ok <case>" line per case.
#include <cstdio>
#include <functional>
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
    Want& z(size_t n) {  // n doubles of zeros
        v.resize(v.size() + n, 0.0);
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

// ---- the four blocks hashed in place (fit, sky, pol, vis): the scan's offsets and size, then the miss half's fill into a heap buffer of
//      exactly that size, against the documented layout; the hashes; every refusal with its text
template <class T>
static T* heap_v(const std::vector<T>& v) {  // a heap copy of exactly these elements, for the caller to change
    T* p = new T[v.size()];
    std::copy(v.begin(), v.end(), p);
    g_keep.emplace_back(p, [](void* q) { delete[] static_cast<T*>(q); });
    return p;
}
template <class T>
static T* own(const T*& p, size_t n) {  // re-seats p on a copy of its n elements and hands the copy out
    T* q = heap_v(std::vector<T>(p, p + n));
    p = q;
    return q;
}
static std::vector<double> ramp(size_t n, double first) {  // first, first + 1, ...
    std::vector<double> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = first + (double)i;
    return v;
}
static Want& operator+=(Want& w, const std::vector<double>& x) {
    w.v.insert(w.v.end(), x.begin(), x.end());
    return w;
}
static bool sizes(const std::vector<size_t>& got, std::initializer_list<size_t> want) { return got == std::vector<size_t>(want); }

// 3 point rows (odd), two band groups of 2 and 3 rows, two free parameters with priors
static vag_fit_spec fit_full(bool with_ext, int n_point = 3) {
    vag_fit_spec s{};
    s.ndim = 2, s.slot[0] = 0, s.slot[1] = 1, s.is_log[0] = 1;
    if ((s.n_data = n_point)) {
        s.t = D({1e5, 2e5, 3e5}), s.nu = D({1e9, 2e9, 3e9}), s.ln_flux = D({-60.0, -61.0, -62.0}), s.ln_err = D({0.1, 0.2, 0.3});
        s.weight = D({1.0, 0.5, 0.25});
        if (with_ext) s.ext_kernel = D({0.7, 0.8, 0.9});
    }
    vag_band_obs b0{}, b1{};
    b0.n = 2, b0.t = D({1e4, 2e4}), b0.ln_flux = D({-50.0, -51.0}), b0.ln_err = D({0.01, 0.02}), b0.weight = D({1.0, 2.0});
    b1.n = 3, b1.t = D({1e4, 1e4, 3e4}), b1.ln_flux = D({-52.0, -53.0, -54.0}), b1.ln_err = D({0.03, 0.04, 0.05}), b1.weight = D({3.0, 4.0, 5.0});
    s.n_bands = 2;
    s.bands = heap<vag_band_obs>({b0, b1});
    s.use_priors = 1;
    s.lower[0] = 0.1, s.lower[1] = -1.0, s.upper[0] = 1.0, s.upper[1] = 2.0;
    s.prior_kind[0] = VAG_PRIOR_LOG_UNIFORM, s.prior_kind[1] = VAG_PRIOR_GAUSSIAN;
    s.prior_a[0] = 0.1, s.prior_a[1] = 0.5, s.prior_b[0] = 1.0, s.prior_b[1] = 0.25;
    return s;
}

static Want& fit_tail(Want& w) {  // the band groups and the prior block of fit_full
    w.d({1e4, 2e4, -50.0, -51.0, 0.01, 0.02, 1.0, 2.0}).d({1e4, 1e4, 3e4, -52.0, -53.0, -54.0, 0.03, 0.04, 0.05, 3.0, 4.0, 5.0});
    w.d({0.1, -1.0}).z(14).d({1.0, 2.0}).z(14).d({0.1, 0.5}).z(14).d({1.0, 0.25}).z(14);  // lower | upper | prior_a | prior_b
    return w.i({0, 1}).z(7).i({1, 0}).z(7).i({VAG_PRIOR_LOG_UNIFORM, VAG_PRIOR_GAUSSIAN}).z(7);  // slot | is_log | prior_kind
}

static std::vector<double> filled(size_t n, const std::function<void(double*)>& fill) {
    std::vector<double> got(n, NAN);  // (exactly the scan's size: a write past it is a report; NAN: a double the fill leaves is seen)
    fill(got.data());
    return got;
}

static void check_fit() {
    const int before = g_failed;
    FitLayout lay;
    for (const bool with_ext : {true, false}) {
        const vag_fit_spec s = fit_full(with_ext);
        CHECK(fit_scan(&s, 2, FitAccepts{}, lay) == VAG_OK && fit_rows(&s) == VAG_OK);
        // the point block 6 * 3 = 18, band group 0 at 18 (4 * 2), band group 1 at 26 (4 * 3), the priors at 38, then 64 + 24
        CHECK(lay.nu == 3 && lay.ln_flux == 6 && lay.ln_err == 9 && lay.weight == 12 && lay.ext == 15);
        CHECK(sizes(lay.band, {18, 26}) && lay.prior == 38 && lay.doubles == 126);
        Want w;
        w.d({1e5, 2e5, 3e5, 1e9, 2e9, 3e9, -60.0, -61.0, -62.0, 0.1, 0.2, 0.3, 1.0, 0.5, 0.25});
        with_ext ? w.d({0.7, 0.8, 0.9}) : w.z(3);
        CHECK(same_bytes(filled(lay.doubles, [&](double* hp) { fit_fill(&s, lay, hp); }), fit_tail(w)));
    }
    const vag_fit_spec s = fit_full(false, 0);  // no point row: the point block is 6 * max(n, 1) = 6 doubles of zeros
    CHECK(fit_scan(&s, 2, FitAccepts{}, lay) == VAG_OK && fit_rows(&s) == VAG_OK);
    CHECK(sizes(lay.band, {6, 14}) && lay.prior == 26 && lay.doubles == 114);
    Want w;
    const std::vector<double> got = filled(lay.doubles, [&](double* hp) { fit_fill(&s, lay, hp); });
    CHECK(same_bytes(got, fit_tail(w.z(6))));
    CHECK(ints_at(got, 26 + 64, {0, 1, 0, 0}) && ints_at(got, 26 + 64 + 8, {1, 0}) && ints_at(got, 26 + 64 + 16, {2, 1}));  // three int32[16]
    // the accepted slots
    vag_fit_spec a = fit_full(true);
    a.slot[0] = VAG_P_SKY_EAST0, a.slot[1] = VAG_P_TMPL_AMP0 + 1;
    FitAccepts acc;
    acc.sky = true, acc.n_templates = 2;
    CHECK(fit_scan(&a, 2, acc, lay) == VAG_OK);
    a.n_data = a.n_bands = 0;  // no flux row at all: data only through another block
    acc.counts = true;
    CHECK(fit_scan(&a, 2, acc, lay) == VAG_OK && lay.prior == 6 && lay.doubles == 94);
    done("fit block layout", before);
}

static vag_sky_fit_spec sky_full() {  // two centroid groups of 1 and 2 epochs
    vag_centroid_obs a{}, b{};
    a.nu = 5e9, a.n = 1, a.t = D({1e6}), a.east = D({0.1}), a.north = D({0.2}), a.err_east = D({0.01}), a.err_north = D({0.02}), a.weight = D({1.0});
    b.nu = 8e9, b.n = 2, b.t = D({2e6, 3e6}), b.east = D({0.3, 0.4}), b.north = D({0.5, 0.6}), b.err_east = D({0.03, 0.04});
    b.err_north = D({0.05, 0.06}), b.weight = D({2.0, 3.0});
    vag_sky_fit_spec s{};
    s.n_groups = 2;
    s.groups = heap<vag_centroid_obs>({a, b});
    return s;
}

static void check_sky() {
    const int before = g_failed;
    const vag_sky_fit_spec s = sky_full();
    SkyLayout lay;
    CHECK(sky_scan(&s, lay) == VAG_OK && sky_rows(&s) == VAG_OK);
    CHECK(sizes(lay.off, {0, 7}) && lay.doubles == 20);  // per group [nu | six arrays of n]: 1 + 6, then 1 + 12
    CHECK(same_bytes(filled(lay.doubles, [&](double* hp) { six_fill(&s, lay, hp); }),
                     Want().d({5e9, 1e6, 0.1, 0.2, 0.01, 0.02, 1.0}).d({8e9, 2e6, 3e6, 0.3, 0.4, 0.5, 0.6, 0.03, 0.04, 0.05, 0.06, 2.0, 3.0})));
    vag_sky_fit_spec none{};  // no group, a fixed placement: nothing to hold
    none.pa_fixed = 0.3;
    CHECK(sky_scan(&none, lay) == VAG_OK && sky_rows(&none) == VAG_OK && lay.off.empty() && lay.doubles == 0);
    CHECK(filled(0, [&](double* hp) { six_fill(&none, lay, hp); }).empty());
    done("sky block layout", before);
}

static vag_pol_fit_spec pol_full() {  // a QU group of 2 epochs, a DEGREE group of 1 epoch without u and err_u
    vag_polarization_obs a{}, b{};
    a.nu = 3e9, a.n = 2, a.kind = VAG_POL_QU, a.t = D({1e5, 2e5}), a.q = D({0.1, 0.2}), a.u = D({-0.1, -0.2}), a.err_q = D({0.01, 0.02});
    a.err_u = D({0.03, 0.04}), a.weight = D({1.0, 2.0});
    b.nu = 4e9, b.n = 1, b.kind = VAG_POL_DEGREE, b.t = D({3e5}), b.q = D({0.3}), b.err_q = D({0.05}), b.weight = D({3.0});
    vag_pol_fit_spec p{};
    p.n_groups = 2;
    p.groups = heap<vag_polarization_obs>({a, b});
    return p;
}

static void check_pol() {
    const int before = g_failed;
    const vag_pol_fit_spec p = pol_full();
    PolLayout lay;
    CHECK(pol_scan(&p, lay) == VAG_OK && pol_rows(&p) == VAG_OK);
    CHECK(sizes(lay.off, {0, 13}) && lay.doubles == 20);  // [nu | t | q | u | err_q | err_u | weight]: 1 + 12, then 1 + 6 with two zeros
    CHECK(same_bytes(filled(lay.doubles, [&](double* hp) { six_fill(&p, lay, hp); }),
                     Want().d({3e9, 1e5, 2e5, 0.1, 0.2, -0.1, -0.2, 0.01, 0.02, 0.03, 0.04, 1.0, 2.0}).d({4e9, 3e5, 0.3, 0.0, 0.05, 0.0, 3.0})));
    done("pol block layout", before);
}

// a COMPLEX group with three epochs of 1, 64 and 65 visibilities, an AMPLITUDE group of one epoch of 2 without im
static vag_vis_fit_spec vis_full() {
    vag_visibility_obs a{}, b{};
    a.nu = 2e10, a.n_epochs = 3, a.n_vis = 130, a.kind = VAG_VIS_COMPLEX, a.t = D({1e5, 2e5, 3e5}), a.first = I({0, 1, 65, 130});
    a.u = heap_v(ramp(130, 1000.0)), a.v = heap_v(ramp(130, 2000.0)), a.re = heap_v(ramp(130, 3000.0)), a.im = heap_v(ramp(130, 4000.0));
    a.err = heap_v(ramp(130, 5000.0)), a.weight = heap_v(ramp(130, 6000.0));
    b.nu = 4e10, b.n_epochs = 1, b.n_vis = 2, b.kind = VAG_VIS_AMPLITUDE, b.t = D({4e5}), b.first = I({0, 2});
    b.u = D({1.0, 2.0}), b.v = D({3.0, 4.0}), b.re = D({5.0, 6.0}), b.err = D({7.0, 8.0}), b.weight = D({9.0, 10.0});
    vag_vis_fit_spec s{};
    s.n_groups = 2;
    s.groups = heap<vag_visibility_obs>({a, b});
    return s;
}

static void check_vis() {
    const int before = g_failed;
    const vag_vis_fit_spec s = vis_full();
    BlockKey key;
    std::vector<VisLayout> lay;
    std::vector<int> blocks;
    CHECK(vis_scan(&s, key) == VAG_OK && vis_rows(&s, lay, blocks) == VAG_OK);
    // per group [nu | t n_epochs | six arrays of n_vis]: 1 + 3 + 780 = 784, then 1 + 1 + 12; the first group's epochs are cut into
    // blocks of at most 64 -- 1, 1 and 2 of them -- so the second group's blocks start at 4
    CHECK(key.doubles == 798 && lay.size() == 2 && lay[0].obs_off == 0 && lay[1].obs_off == 784 && lay[0].blk_off == 0 && lay[1].blk_off == 4);
    CHECK(lay[0].epoch_blk == std::vector<int>({0, 1, 2, 4}) && lay[1].epoch_blk == std::vector<int>({0, 1}));
    CHECK(blocks == std::vector<int>({0, 0, 1, 1, 1, 64, 2, 65, 64, 2, 129, 1, 0, 0, 2}));
    Want w;
    w.d({2e10, 1e5, 2e5, 3e5});
    for (const double first : {1000.0, 2000.0, 3000.0, 4000.0, 5000.0, 6000.0}) w += ramp(130, first);
    w.d({4e10, 4e5}).d({1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.0, 0.0, 7.0, 8.0, 9.0, 10.0});
    CHECK(same_bytes(filled(key.doubles, [&](double* hp) { vis_fill(&s, lay, hp); }), w));
    done("vis block layout", before);
}

template <class Spec, class Hash>
static void hashes_of(Spec (*make)(), Hash hash, void (*one_double)(Spec&)) {
    Spec a = make(), b = make();  // equal content in other arrays
    CHECK(hash(a) == hash(b));
    one_double(b);
    CHECK(hash(a) != hash(b));
}

static void check_hashes() {
    const int before = g_failed;
    auto fit_hash = [](const vag_fit_spec& s) {
        FitLayout lay;
        CHECK(fit_scan(&s, 2, FitAccepts{}, lay) == VAG_OK);
        return lay.hash;
    };
    auto sky_hash = [](const vag_sky_fit_spec& s) {
        SkyLayout lay;
        CHECK(sky_scan(&s, lay) == VAG_OK);
        return lay.hash;
    };
    auto pol_hash = [](const vag_pol_fit_spec& s) {
        PolLayout lay;
        CHECK(pol_scan(&s, lay) == VAG_OK);
        return lay.hash;
    };
    auto vis_hash = [](const vag_vis_fit_spec& s) {
        BlockKey key;
        CHECK(vis_scan(&s, key) == VAG_OK);
        return key.hash;
    };
    hashes_of<vag_fit_spec>([] { return fit_full(true); }, fit_hash, [](vag_fit_spec& s) { own(own(s.bands, 2)[1].weight, 3)[2] = 5.5; });
    hashes_of<vag_sky_fit_spec>(sky_full, sky_hash, [](vag_sky_fit_spec& s) { own(own(s.groups, 2)[1].north, 2)[1] = 0.61; });
    hashes_of<vag_pol_fit_spec>(pol_full, pol_hash, [](vag_pol_fit_spec& s) { own(own(s.groups, 2)[0].err_u, 2)[0] = 0.031; });
    hashes_of<vag_vis_fit_spec>(vis_full, vis_hash, [](vag_vis_fit_spec& s) { own(own(s.groups, 2)[0].im, 130)[129] = 0.5; });
    // a kind
    vag_fit_spec f = fit_full(true);
    f.prior_kind[1] = VAG_PRIOR_NONE;
    CHECK(fit_hash(f) != fit_hash(fit_full(true)));
    vag_pol_fit_spec p = pol_full();
    own(p.groups, 2)[0].kind = VAG_POL_DEGREE;
    CHECK(pol_hash(p) != pol_hash(pol_full()));
    vag_vis_fit_spec v = vis_full();
    own(v.groups, 2)[0].kind = VAG_VIS_AMPLITUDE;
    CHECK(vis_hash(v) != vis_hash(vis_full()));
    // n_az: 0 is the default the code substitutes, 1024 for a visibility group and 256 for a polarization group
    own(v.groups, 2)[0].kind = VAG_VIS_COMPLEX;
    own(v.groups, 2)[1].n_az = 512;
    CHECK(vis_hash(v) != vis_hash(vis_full()));
    own(v.groups, 2)[1].n_az = 1024;
    CHECK(vis_hash(v) == vis_hash(vis_full()));
    p = pol_full();
    own(p.groups, 2)[1].n_az = 256;
    CHECK(pol_hash(p) == pol_hash(pol_full()));
    own(p.groups, 2)[1].n_az = 128;
    CHECK(pol_hash(p) != pol_hash(pol_full()));
    done("block hashes", before);
}

// The scanned blocks: the key a scan leaves is the stage vector's size and a hash of the shapes and the staged bytes.
static void check_scan_keys(const vag_fit_spec& spec) {
    const int before = g_failed;
    auto cov_key = [](const vag_cov_fit_spec& cs) {
        std::vector<double> stage;
        CovLayout lay;
        CHECK(cov_scan(&cs, stage, lay) == VAG_OK && lay.doubles == stage.size() && lay.doubles == 26);
        return lay.hash;
    };
    vag_cov_fit_spec c = cov_spec();
    CHECK(cov_key(c) == cov_key(cov_spec()));  // equal content in other arrays
    own(own(c.groups, 2)[1].ln_flux, 3)[2] = -63.5;
    CHECK(cov_key(c) != cov_key(cov_spec()));
    c = cov_spec();
    own(own(c.groups, 2)[1].whitener, 9)[1] = 7.0;  // (the unread upper half is not staged: not content)
    CHECK(cov_key(c) == cov_key(cov_spec()));
    const vag_pol_fit_spec pol = pol_spec();
    const vag_limit_fit_spec lim = lim_spec();
    vag_limit_fit_spec lim2 = lim_spec();
    own(own(lim2.bands, 2)[1].sigma, 3)[0] = 0.3;
    std::vector<double> s1, s2, s3;
    LimLayout l1, l2, l3;
    CHECK(lim_scan(&spec, &pol, &lim, s1, l1) == VAG_OK && lim_scan(&spec, &pol, &lim, s2, l2) == VAG_OK && lim_scan(&spec, &pol, &lim2, s3, l3) == VAG_OK);
    CHECK(l1.doubles == 18 && l1.hash == l2.hash && l3.doubles == 18 && l3.hash != l1.hash);
    const vag_counts_fit_spec cs = counts_spec();
    const vag_index_fit_spec is = index_spec();
    const vag_fold_fit_spec fs = fold_spec();
    const vag_noise_fit_spec nz = noise_spec();
    const vag_template_fit_spec tp = tmpl_spec();
    std::vector<double> stage;
    CountsLayout cl;
    IndexLayout il;
    FoldLayout fl;
    NoiseLayout nl;
    TmplLayout tl;
    CHECK(counts_scan(&cs, stage, cl) == VAG_OK && cl.doubles == 32 && cl.hash != 0);
    CHECK(index_scan(&is, stage, il) == VAG_OK && il.doubles == 50 && il.hash != cl.hash);
    CHECK(fold_scan(&spec, &fs, stage, fl) == VAG_OK && fl.doubles == 74 && fl.hash != il.hash);
    CHECK(noise_scan(&spec, &nz, stage, nl) == VAG_OK && nl.doubles == 19 && nl.hash != fl.hash);
    CHECK(tmpl_scan(&spec, &tp, stage, tl) == VAG_OK && tl.doubles == 14 && tl.hash != nl.hash);
    done("scan keys", before);
}

// Every refusal of one block: a change to the accepted spec, where it must be refused (the scan, or the rows behind a scan that
// accepts), and the text, word for word.
template <class Spec>
struct Refusal {
    const char* text;
    bool in_rows;
    std::function<void(Spec&)> change;
};

template <class Spec>
static void refusals_of(const char* name, Spec (*make)(), int (*scan)(const Spec&), int (*rows)(const Spec&),
                        std::initializer_list<Refusal<Spec>> table) {
    const int before = g_failed;
    for (const Refusal<Spec>& r : table) {
        Spec s = make();
        r.change(s);
        g_err.clear();
        const int rc = scan(s);
        if (r.in_rows) CHECK(rc == VAG_OK && rows(s) == VAG_E_INVALID);
        else CHECK(rc == VAG_E_INVALID);
        if (g_err != r.text) {
            std::printf("FAIL %s: wanted \"%s\", got \"%s\"\n", name, r.text, g_err.c_str());
            ++g_failed;
        }
    }
    done(name, before);
}

static void check_block_refusals() {
    using F = vag_fit_spec;
    refusals_of<F>(
        "fit block refusals", [] { return fit_full(true); },
        [](const F& s) {
            FitLayout lay;
            return fit_scan(&s, 2, FitAccepts{}, lay);
        },
        [](const F& s) { return fit_rows(&s); },
        {{"ndim must match spec and be in 1..16", false, [](F& s) { s.ndim = 3; }},
         {"fit spec has no data", false, [](F& s) { s.n_data = s.n_bands = 0; }},
         {"bad parameter slot", false, [](F& s) { s.slot[1] = VAG_P_SKY_PA; }},
         {"prior bounds of parameter 1: need lower < upper", false, [](F& s) { s.upper[1] = s.lower[1]; }},
         {"unknown prior kind 7", false, [](F& s) { s.prior_kind[0] = 7; }},
         {"Uniform prior needs maximum > minimum", false, [](F& s) { s.prior_kind[0] = VAG_PRIOR_UNIFORM_RANGE, s.prior_b[0] = s.prior_a[0]; }},
         {"Gaussian prior needs sigma > 0", false, [](F& s) { s.prior_b[1] = 0.0; }},
         {"LogUniform prior needs 0 < minimum < maximum", false, [](F& s) { s.prior_a[0] = 0.0; }},
         {"band group 1 has no observations", false, [](F& s) { own(s.bands, 2)[1].n = 0; }},
         {"data times must be positive", true, [](F& s) { own(s.t, 3)[1] = -2e5; }},
         {"data times must be ascending (fitter.py:420-428)", true, [](F& s) { own(s.t, 3)[2] = 1.5e5; }},
         {"band group 1: times must be positive and ascending", true, [](F& s) { own(own(s.bands, 2)[1].t, 3)[1] = 0.5e4; }}});
    using S = vag_sky_fit_spec;
    refusals_of<S>(
        "sky block refusals", sky_full,
        [](const S& s) {
            SkyLayout lay;
            return sky_scan(&s, lay);
        },
        [](const S& s) { return sky_rows(&s); },
        {{"bad centroid group list", false, [](S& s) { s.n_groups = -1; }},
         {"fixed sky placement values must be finite", false, [](S& s) { s.north0_fixed = INFINITY; }},
         {"centroid group 1 has no observations", false, [](S& s) { own(s.groups, 2)[1].n = 0; }},
         {"centroid group 0: null array", false, [](S& s) { own(s.groups, 2)[0].east = nullptr; }},
         {"centroid group 1: frequency must be positive", true, [](S& s) { own(s.groups, 2)[1].nu = -8e9; }},
         {"centroid group 1: times must be positive and ascending", true, [](S& s) { own(own(s.groups, 2)[1].t, 2)[1] = 1e6; }},
         {"centroid group 0: positions and weights must be finite", true, [](S& s) { own(own(s.groups, 2)[0].north, 1)[0] = INFINITY; }},
         {"centroid group 0: errors must be positive and finite", true, [](S& s) { own(own(s.groups, 2)[0].err_east, 1)[0] = 0.0; }}});
    using P = vag_pol_fit_spec;
    refusals_of<P>(
        "pol block refusals", pol_full,
        [](const P& s) {
            PolLayout lay;
            return pol_scan(&s, lay);
        },
        [](const P& s) { return pol_rows(&s); },
        {{"bad polarization group list", false, [](P& s) { s.groups = nullptr; }},
         {"at most 64 polarization groups", false, [](P& s) { s.n_groups = VAG_POL_MAX_GROUPS + 1; }},
         {"fixed polarization values must not be NaN", false, [](P& s) { s.pi_max_fixed[1] = NAN; }},
         {"polarization group 0 has no observations", false, [](P& s) { own(s.groups, 2)[0].n = 0; }},
         {"polarization group 1: at most 4096 epochs", false, [](P& s) { own(s.groups, 2)[1].n = VAG_VIS_MAX_EPOCHS + 1; }},
         {"polarization group 0: unknown kind 5", false, [](P& s) { own(s.groups, 2)[0].kind = 5; }},
         {"polarization group 0: null array", false, [](P& s) { own(s.groups, 2)[0].err_u = nullptr; }},
         {"polarization group 1: frequency must be positive", true, [](P& s) { own(s.groups, 2)[1].nu = INFINITY; }},
         {"polarization group 0: times must be positive and ascending", true, [](P& s) { own(own(s.groups, 2)[0].t, 2)[1] = 0.5e5; }},
         {"polarization group 1: measurements must be finite, weights finite and >= 0", true, [](P& s) { own(own(s.groups, 2)[1].weight, 1)[0] = -1.0; }},
         {"polarization group 0: errors must be positive and finite", true, [](P& s) { own(own(s.groups, 2)[0].err_u, 2)[1] = 0.0; }}});
    using V = vag_vis_fit_spec;
    static_assert(VAG_VIS_MAX_GROUPS == 64 && VAG_VIS_MAX_EPOCHS == 4096 && VAG_VIS_MAX_PER_EPOCH == 65536, "the texts below hold these");
    refusals_of<V>(
        "vis block refusals", vis_full,
        [](const V& s) {
            BlockKey key;
            return vis_scan(&s, key);
        },
        [](const V& s) {
            std::vector<VisLayout> lay;
            std::vector<int> blocks;
            return vis_rows(&s, lay, blocks);
        },
        {{"bad visibility group list", false, [](V& s) { s.groups = nullptr; }},
         {"at most 64 visibility groups", false, [](V& s) { s.n_groups = VAG_VIS_MAX_GROUPS + 1; }},
         {"visibility group 1 has no observations", false, [](V& s) { own(s.groups, 2)[1].n_epochs = 0; }},
         {"visibility group 0: at most 4096 epochs", false, [](V& s) { own(s.groups, 2)[0].n_epochs = VAG_VIS_MAX_EPOCHS + 1; }},
         {"visibility group 1: unknown kind 2", false, [](V& s) { own(s.groups, 2)[1].kind = 2; }},
         {"visibility group 1: null array", false, [](V& s) { own(s.groups, 2)[1].kind = VAG_VIS_COMPLEX; }},  // (and no im)
         {"visibility group 1: frequency must be positive", true, [](V& s) { own(s.groups, 2)[1].nu = 0.0; }},
         {"visibility group 0: first[0] must be 0 and first[n_epochs] n_vis", true, [](V& s) { own(own(s.groups, 2)[0].first, 4)[3] = 129; }},
         {"visibility group 0: times must be positive and strictly ascending", true, [](V& s) { own(own(s.groups, 2)[0].t, 3)[2] = 2e5; }},
         {"visibility group 0: epoch 1 is empty or first[] is not ascending", true, [](V& s) { own(own(s.groups, 2)[0].first, 4)[2] = 1; }},
         {"visibility group 0: at most 65536 visibilities per epoch", true,
          [](V& s) {  // one epoch of 65537
              vag_visibility_obs& o = own(s.groups, 2)[0];
              o.n_epochs = 1, o.n_vis = VAG_VIS_MAX_PER_EPOCH + 1, o.first = I({0, VAG_VIS_MAX_PER_EPOCH + 1});
              o.u = o.v = o.re = o.im = o.err = o.weight = heap_v(std::vector<double>(o.n_vis, 1.0));
          }},
         {"visibility group 0: baselines and visibilities must be finite", true, [](V& s) { own(own(s.groups, 2)[0].im, 130)[129] = NAN; }},
         {"visibility group 1: errors must be positive and finite", true, [](V& s) { own(own(s.groups, 2)[1].err, 2)[1] = 0.0; }},
         {"visibility group 1: weights must be finite and >= 0", true, [](V& s) { own(own(s.groups, 2)[1].weight, 2)[0] = -9.0; }}});
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

// ---- the block views: every *_cols against offsets worked out by hand from the layout comment, at the smallest shapes where two
//      columns can be confused, two groups of different shapes per block (with one group every off[g] is 0); then every input array
//      read back through the view, element for element, from a heap copy of exactly the block's length
static bool col_is(const double* block, size_t at, const double* src, size_t n) { return std::memcmp(block + at, src, sizeof(double) * n) == 0; }
static bool icol_is(const double* block, size_t at, const int32_t* src, size_t n) { return std::memcmp(block + at, src, sizeof(int32_t) * n) == 0; }
static bool col_zero(const double* block, size_t at, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (block[at + i] != 0.0) return false;
    return true;
}

static void check_block_columns() {
    const int before = g_failed;
    {  // counts: [t_sample ns | N n | B n | a n | w n | idx n m]; n = 3, m = 2, ns = 5: 5 + 12 + 3 = 20; then n = 1, m = 3, ns = 2 (n m odd:
       // the int32 tail has a pad): 2 + 4 + 2 = 8
        vag_counts_obs a{}, b{};
        a.nu_min = 1e17, a.nu_max = 2e17, a.num_points = 3, a.n = 3, a.m = 2, a.n_samples = 5;
        a.t_sample = D({1e4, 2e4, 3e4, 4e4, 5e4}), a.sample_idx = I({0, 1, 2, 3, 3, 4});
        a.counts = D({1.0, 2.0, 3.0}), a.background = D({0.1, 0.2, 0.3}), a.scale = D({4.0, 5.0, 6.0}), a.weight = D({7.0, 8.0, 9.0});
        b.nu_min = 1e17, b.nu_max = 2e17, b.num_points = 2, b.n = 1, b.m = 3, b.n_samples = 2;
        b.t_sample = D({6e4, 7e4}), b.sample_idx = I({1, 0, 1}), b.counts = D({11.0}), b.background = D({12.0}), b.scale = D({13.0}), b.weight = D({14.0});
        vag_counts_fit_spec cs{};
        cs.n_groups = 2, cs.groups = heap<vag_counts_obs>({a, b});
        const CountsCols ka = counts_cols(a), kb = counts_cols(b);
        CHECK(ka.N == 5 && ka.B == 8 && ka.a == 11 && ka.w == 14 && ka.idx == 17 && ka.doubles == 20);
        CHECK(kb.N == 2 && kb.B == 3 && kb.a == 4 && kb.w == 5 && kb.idx == 6 && kb.doubles == 8);
        std::vector<double> stage;
        CountsLayout lay;
        CHECK(counts_scan(&cs, stage, lay) == VAG_OK && longs(lay.off, {0, 20}) && (size_t)lay.off[1] == ka.doubles && stage.size() == 28);
        if (stage.size() == 28) {
            const double* blk = heap_v(stage);
            for (int g = 0; g < 2; ++g) {
                const vag_counts_obs& o = cs.groups[g];
                const CountsCols k = counts_cols(o);
                const double* p = blk + lay.off[g];
                CHECK(col_is(p, 0, o.t_sample, o.n_samples) && col_is(p, k.N, o.counts, o.n) && col_is(p, k.B, o.background, o.n));
                CHECK(col_is(p, k.a, o.scale, o.n) && col_is(p, k.w, o.weight, o.n) && icol_is(p, k.idx, o.sample_idx, (size_t)o.n * o.m));
            }
        }
    }
    {  // index: [t n K | nu n K | s n | sigma n | w n | c K]; n = 2, K = 3: 6 + 6 + 6 + 3 = 21; then n = 1, K = 2: 2 + 2 + 3 + 2 = 9
        vag_index_obs a{}, b{};
        a.n = 2, a.k = 3, a.nu = D({1e9, 2e9, 3e9}), a.coef = D({-1.0, 0.5, 1.0});
        a.t = D({1e5, 2e5}), a.value = D({-0.5, -0.6}), a.err = D({0.1, 0.2}), a.weight = D({1.0, 2.0});
        b.n = 1, b.k = 2, b.nu = D({4e9, 5e9}), b.coef = D({-2.0, 2.0}), b.t = D({3e5}), b.value = D({0.3}), b.err = D({0.05}), b.weight = D({1.5});
        vag_index_fit_spec is{};
        is.n_groups = 2, is.groups = heap<vag_index_obs>({a, b});
        const IndexCols ka = index_cols(a), kb = index_cols(b);
        CHECK(ka.nu == 6 && ka.value == 12 && ka.err == 14 && ka.weight == 16 && ka.coef == 18 && ka.doubles == 21);
        CHECK(kb.nu == 2 && kb.value == 4 && kb.err == 5 && kb.weight == 6 && kb.coef == 7 && kb.doubles == 9);
        std::vector<double> stage;
        IndexLayout lay;
        CHECK(index_scan(&is, stage, lay) == VAG_OK && longs(lay.off, {0, 21}) && (size_t)lay.off[1] == ka.doubles && stage.size() == 30);
        if (stage.size() == 30) {
            const double* blk = heap_v(stage);
            for (int g = 0; g < 2; ++g) {
                const vag_index_obs& o = is.groups[g];
                const IndexCols k = index_cols(o);
                const double* p = blk + lay.off[g];
                for (int i = 0; i < o.n; ++i)
                    for (int q = 0; q < o.k; ++q) CHECK(p[i * o.k + q] == o.t[i] && p[k.nu + i * o.k + q] == o.nu[q]);
                CHECK(col_is(p, k.value, o.value, o.n) && col_is(p, k.err, o.err, o.n) && col_is(p, k.weight, o.weight, o.n));
                CHECK(col_is(p, k.coef, o.coef, o.k));
            }
        }
    }
    for (const bool first_has_sigma : {true, false}) {
        // fold: [t ns J | nu ns J | A J C | sigma J | exposure / m n | N n C | B n C | w n C | idx n m]; n = 2, C = 3, J = 2, ns = 3,
        // m = 1: 6 + 6 + 6 + 2 + 2 + 18 + 1 = 41; then J = C = n = m = ns = 1: 9.  One of the two has a cross-section, the other zeros.
        vag_fold_obs a{}, b{};
        a.J = 2, a.C = 3, a.n = 2, a.m = 1, a.n_samples = 3;
        a.nu = D({1e17, 2e17}), a.A = D({1.0, 2.0, 3.0, 4.0, 5.0, 6.0}), a.t_sample = D({1e4, 2e4, 3e4}), a.sample_idx = I({2, 1});
        a.exposure_over_m = D({10.0, 20.0}), a.counts = D({0.0, 1.0, 2.0, 3.0, 4.0, 5.0}), a.background = D({0.1, 0.2, 0.3, 0.4, 0.5, 0.6});
        a.weight = D({1.0, 0.0, 2.0, 1.0, 0.5, 1.0});
        b.J = 1, b.C = 1, b.n = 1, b.m = 1, b.n_samples = 1;
        b.nu = D({3e17}), b.A = D({50.0}), b.t_sample = D({4e4}), b.sample_idx = I({0}), b.exposure_over_m = D({100.0});
        b.counts = D({7.0}), b.background = D({0.5}), b.weight = D({1.5});
        (first_has_sigma ? a.sigma : b.sigma) = first_has_sigma ? D({3e-22, 2e-22}) : D({1e-22});
        vag_fold_fit_spec fs{};
        fs.n_groups = 2, fs.groups = heap<vag_fold_obs>({a, b});
        const FoldCols ka = fold_cols(a), kb = fold_cols(b);
        CHECK(ka.nu == 6 && ka.A == 12 && ka.sigma == 18 && ka.eom == 20 && ka.N == 22 && ka.B == 28 && ka.w == 34 && ka.idx == 40 && ka.doubles == 41);
        CHECK(kb.nu == 1 && kb.A == 2 && kb.sigma == 3 && kb.eom == 4 && kb.N == 5 && kb.B == 6 && kb.w == 7 && kb.idx == 8 && kb.doubles == 9);
        vag_fit_spec spec = fit_spec();  // (frees N_H: a group has a cross-section)
        std::vector<double> stage;
        FoldLayout lay;
        CHECK(fold_scan(&spec, &fs, stage, lay) == VAG_OK && longs(lay.off, {0, 41}) && (size_t)lay.off[1] == ka.doubles && stage.size() == 50);
        if (stage.size() == 50) {
            const double* blk = heap_v(stage);
            for (int g = 0; g < 2; ++g) {
                const vag_fold_obs& o = fs.groups[g];
                const FoldCols k = fold_cols(o);
                const double* p = blk + lay.off[g];
                for (int s = 0; s < o.n_samples; ++s)
                    for (int j = 0; j < o.J; ++j) CHECK(p[s * o.J + j] == o.t_sample[s] && p[k.nu + s * o.J + j] == o.nu[j]);
                CHECK(col_is(p, k.A, o.A, (size_t)o.J * o.C) && (o.sigma ? col_is(p, k.sigma, o.sigma, o.J) : col_zero(p, k.sigma, o.J)));
                CHECK(col_is(p, k.eom, o.exposure_over_m, o.n) && col_is(p, k.N, o.counts, (size_t)o.n * o.C));
                CHECK(col_is(p, k.B, o.background, (size_t)o.n * o.C) && col_is(p, k.w, o.weight, (size_t)o.n * o.C));
                CHECK(icol_is(p, k.idx, o.sample_idx, (size_t)o.n * o.m));
            }
        }
    }
    {  // cov: [t n | nu n | ln_flux n | ext n | Wt n n]; n = 2 without ext: 8 + 4 = 12; then n = 65 with ext: 260 + 4225 = 4485
        vag_cov_obs a{}, b{};
        a.n = 2, a.weight = 1.0, a.t = D({1e5, 2e5}), a.nu = D({1e9, 2e9}), a.ln_flux = D({-60.0, -61.0}), a.whitener = D({1.0, NAN, 2.0, 3.0});
        std::vector<double> W(65 * 65, NAN);
        for (int i = 0; i < 65; ++i)
            for (int j = 0; j <= i; ++j) W[i * 65 + j] = 1.0 + i * 65 + j;
        b.n = 65, b.weight = 0.5, b.t = heap_v(ramp(65, 1e5)), b.nu = heap_v(ramp(65, 1e9)), b.ln_flux = heap_v(ramp(65, -100.0));
        b.ext = heap_v(ramp(65, 0.5)), b.whitener = heap_v(W);
        vag_cov_fit_spec cs{};
        cs.n_groups = 2, cs.groups = heap<vag_cov_obs>({a, b});
        const CovCols ka = cov_cols(a), kb = cov_cols(b);
        CHECK(ka.nu == 2 && ka.ln_flux == 4 && ka.ext == 6 && ka.Wt == 8 && ka.doubles == 12);
        CHECK(kb.nu == 65 && kb.ln_flux == 130 && kb.ext == 195 && kb.Wt == 260 && kb.doubles == 4485);
        std::vector<double> stage;
        CovLayout lay;
        CHECK(cov_scan(&cs, stage, lay) == VAG_OK && longs(lay.off, {0, 12}) && (size_t)lay.off[1] == ka.doubles && stage.size() == 4497);
        if (stage.size() == 4497) {
            const double* blk = heap_v(stage);
            for (int g = 0; g < 2; ++g) {
                const vag_cov_obs& o = cs.groups[g];
                const CovCols k = cov_cols(o);
                const double* p = blk + lay.off[g];
                CHECK(col_is(p, 0, o.t, o.n) && col_is(p, k.nu, o.nu, o.n) && col_is(p, k.ln_flux, o.ln_flux, o.n));
                CHECK(o.ext ? col_is(p, k.ext, o.ext, o.n) : col_zero(p, k.ext, o.n));
                bool same = true;
                for (int i = 0; i < o.n; ++i)
                    for (int j = 0; j < o.n; ++j) same = same && p[k.Wt + (size_t)j * o.n + i] == (j <= i ? o.whitener[(size_t)i * o.n + j] : 0.0);
                CHECK(same);
            }
        }
    }
    {  // a flux block of limit rows: [limit n | sigma n | kind n]; the point rows, n = 3: 6 + 2 = 8; then band group 0, n = 2: 4 + 1 = 5
        const int32_t det = VAG_OBS_DETECTION, lim = VAG_OBS_UPPER_LIMIT;
        const vag_fit_spec spec = fit_spec();
        vag_limit_fit_spec l{};
        l.point = {I({lim, lim, det}), D({2.5, 3.5, 9.0}), D({0.5, 0.25, 9.0})};
        l.n_bands = 2;
        l.bands = heap<vag_limit_rows>({{I({det, lim}), D({7.0, 1.5}), D({7.0, 0.125})}, {I({det, det, det}), nullptr, nullptr}});
        const LimCols ka = lim_cols(3), kb = lim_cols(2);
        CHECK(ka.sigma == 3 && ka.kind == 6 && ka.doubles == 8);
        CHECK(kb.sigma == 2 && kb.kind == 4 && kb.doubles == 5);
        std::vector<double> stage;
        LimLayout lay;
        CHECK(lim_scan(&spec, nullptr, &l, stage, lay) == VAG_OK && lay.point == 0 && longs(lay.band, {8, -1}) && stage.size() == 13);
        CHECK((size_t)lay.band[0] == ka.doubles);
        if (stage.size() == 13) {
            const double* blk = heap_v(stage);
            const double* p = blk + lay.point;  // (a detection holds limit 0 and sigma 1)
            CHECK(col_is(p, 0, D({2.5, 3.5, 0.0}), 3) && col_is(p, ka.sigma, D({0.5, 0.25, 1.0}), 3) && icol_is(p, ka.kind, l.point.kind, 3));
            p = blk + lay.band[0];
            CHECK(col_is(p, 0, D({0.0, 1.5}), 2) && col_is(p, kb.sigma, D({1.0, 0.125}), 2) && icol_is(p, kb.kind, l.bands[0].kind, 2));
        }
    }
    {  // a band group in the fit block: [t n | ln_flux n | ln_err n | weight n]; n = 2 behind point rows of n = 3 (at 18): 8; then n = 3: 12
        const vag_fit_spec s = fit_full(true);
        const BandCols ka = band_cols(2), kb = band_cols(3);
        CHECK(ka.ln_flux == 2 && ka.ln_err == 4 && ka.weight == 6 && ka.doubles == 8);
        CHECK(kb.ln_flux == 3 && kb.ln_err == 6 && kb.weight == 9 && kb.doubles == 12);
        FitLayout lay;
        CHECK(fit_scan(&s, 2, FitAccepts{}, lay) == VAG_OK && sizes(lay.band, {18, 26}) && lay.band[1] == lay.band[0] + ka.doubles);
        CHECK(lay.prior == lay.band[1] + kb.doubles);
        const std::vector<double> got = filled(lay.doubles, [&](double* hp) { fit_fill(&s, lay, hp); });
        for (int g = 0; g < 2 && lay.band.size() == 2; ++g) {
            const vag_band_obs& bd = s.bands[g];
            const BandCols k = band_cols(bd.n);
            const double* p = got.data() + lay.band[g];
            CHECK(col_is(p, 0, bd.t, bd.n) && col_is(p, k.ln_flux, bd.ln_flux, bd.n) && col_is(p, k.ln_err, bd.ln_err, bd.n));
            CHECK(col_is(p, k.weight, bd.weight, bd.n));
        }
    }
    {  // a centroid group: [nu | t n | east n | north n | err_east n | err_north n | weight n]; n = 1: 7; then n = 2: 13
        const vag_sky_fit_spec s = sky_full();
        const SixCols ka = six_cols(1), kb = six_cols(2);
        CHECK(ka.rows == 1 && ka.col[0] == 1 && ka.col[1] == 2 && ka.col[2] == 3 && ka.col[3] == 4 && ka.col[4] == 5 && ka.col[5] == 6 && ka.doubles == 7);
        CHECK(kb.rows == 1 && kb.col[0] == 1 && kb.col[1] == 3 && kb.col[2] == 5 && kb.col[3] == 7 && kb.col[4] == 9 && kb.col[5] == 11 && kb.doubles == 13);
        SkyLayout lay;
        CHECK(sky_scan(&s, lay) == VAG_OK && sizes(lay.off, {0, 7}) && lay.off[1] == ka.doubles && lay.doubles == 20);
        const std::vector<double> got = filled(lay.doubles, [&](double* hp) { six_fill(&s, lay, hp); });
        for (int g = 0; g < 2 && lay.off.size() == 2; ++g) {
            const vag_centroid_obs& o = s.groups[g];
            const SixCols k = six_cols(o.n);
            const double* p = got.data() + lay.off[g];
            const double* col[6] = {o.t, o.east, o.north, o.err_east, o.err_north, o.weight};
            CHECK(p[0] == o.nu);
            for (int q = 0; q < 6; ++q) CHECK(col_is(p, k.col[q], col[q], o.n));
        }
    }
    {  // a visibility group: [nu | t n_epochs | u | v | re | im | err | weight] (n_vis each); 3 epochs, 130 visibilities: 4 + 780; then 1, 2: 14
        const vag_vis_fit_spec s = vis_full();
        const VisCols ka = vis_cols(s.groups[0]), kb = vis_cols(s.groups[1]);
        CHECK(ka.t == 1 && ka.six == 4 && ka.doubles == 784 && kb.t == 1 && kb.six == 2 && kb.doubles == 14);
        CHECK(six_cols(130, ka.six).col[0] == 4 && six_cols(130, ka.six).col[5] == 654 && six_cols(2, kb.six).col[5] == 12);
        BlockKey key;
        std::vector<VisLayout> lay;
        std::vector<int> blocks;
        CHECK(vis_scan(&s, key) == VAG_OK && vis_rows(&s, lay, blocks) == VAG_OK && key.doubles == 798 && lay[1].obs_off == ka.doubles);
        const std::vector<double> got = filled(key.doubles, [&](double* hp) { vis_fill(&s, lay, hp); });
        for (int g = 0; g < 2; ++g) {
            const vag_visibility_obs& o = s.groups[g];
            const VisCols k = vis_cols(o);
            const SixCols six = six_cols(o.n_vis, k.six);
            const double* p = got.data() + lay[g].obs_off;
            const double* col[6] = {o.u, o.v, o.re, o.im, o.err, o.weight};
            CHECK(p[0] == o.nu && col_is(p, k.t, o.t, o.n_epochs));
            for (int q = 0; q < 6; ++q) CHECK(col[q] ? col_is(p, six.col[q], col[q], o.n_vis) : col_zero(p, six.col[q], o.n_vis));
        }
    }
    {  // the host copy of a short series' frequencies: point i at nu[i % K], as the index and fold scans lay the nu column out
        const double* nu = D({1e9, 2e9, 3e9});
        double* pts = heap_v(std::vector<double>(6, NAN));
        CHECK(short_series_nu(nu, 3, 6, 6, pts) == pts && col_is(pts, 0, D({1e9, 2e9, 3e9, 1e9, 2e9, 3e9}), 6));
        CHECK(short_series_nu(nu, 3, 9, 6, pts) == nullptr);  // (above the bound: no shared-node test, nothing written)
    }
    done("block columns", before);
}

// ---- the pass list of a prepared request: kinds and groups in order, the size, the first and the last position; a request fit_scan
//      accepts has a pass (the last pass writes the call's output), and the one with an empty list is the one it refuses
static bool passes_are(const std::vector<PassItem>& got, std::initializer_list<PassItem> want) {
    if (got.size() != want.size()) return false;
    size_t i = 0;
    for (const PassItem& w : want) {
        if (got[i].kind != w.kind || got[i].group != w.group) return false;
        ++i;
    }
    return true;
}

static bool scan_accepts(FitRequest& r) { return fit_scan(r.spec, r.spec->ndim, fit_accepts(r), r.fit) == VAG_OK; }

static void check_pass_list() {
    const int before = g_failed;
    using K = PassKind;
    vag_fit_spec point = fit_full(false);  // 3 point rows alone
    point.n_bands = 0;
    {
        FitRequest r = fit_request(&point);
        CHECK(fit_request_prepare(r) == VAG_OK && scan_accepts(r));
        CHECK(passes_are(fit_pass_list(r), {{K::Point, 0}}));  // one pass: the first and the last
    }
    {  // no point row, two band groups
        const vag_fit_spec s = fit_full(false, 0);
        FitRequest r = fit_request(&s);
        CHECK(fit_request_prepare(r) == VAG_OK && scan_accepts(r));
        const std::vector<PassItem> list = fit_pass_list(r);
        CHECK(passes_are(list, {{K::Band, 0}, {K::Band, 1}}));
        CHECK(list.size() == 2 && list.front().kind == K::Band && list.front().group == 0 && list.back().group == 1);
    }
    {  // a visibility group without centroid groups: sky carries the placement only
        vag_sky_fit_spec sky{};
        sky.pa_fixed = 0.3;
        const vag_vis_fit_spec vis = vis_full();
        FitRequest r = fit_request(&point, &sky, &vis);
        CHECK(fit_request_prepare(r) == VAG_OK && r.sky && r.placed && scan_accepts(r));
        const std::vector<PassItem> list = fit_pass_list(r);
        CHECK(passes_are(list, {{K::Point, 0}, {K::Vis, 0}, {K::Vis, 1}}));
        CHECK(list.size() == 3 && list.front().kind == K::Point && list.back().kind == K::Vis && list.back().group == 1);
    }
    {  // empty group lists given as present specs: normalised away, the list is the narrower request's
        const vag_fit_spec s = fit_full(false);
        const vag_sky_fit_spec sky{};
        const vag_vis_fit_spec vis{};
        const vag_pol_fit_spec pol{};
        const vag_counts_fit_spec counts{};
        const vag_index_fit_spec index{};
        const vag_fold_fit_spec fold{};
        const vag_cov_fit_spec cov{};
        FitRequest r = fit_request(&s, &sky, &vis, &pol, nullptr, nullptr, &counts, &index, &fold, nullptr, &cov), narrow = fit_request(&s);
        CHECK(fit_request_prepare(r) == VAG_OK && fit_request_prepare(narrow) == VAG_OK && scan_accepts(r) && scan_accepts(narrow));
        const std::vector<PassItem> list = fit_pass_list(r), want = fit_pass_list(narrow);
        CHECK(passes_are(list, {{K::Point, 0}, {K::Band, 0}, {K::Band, 1}}) && passes_are(want, {{K::Point, 0}, {K::Band, 0}, {K::Band, 1}}));
        CHECK(list.front().kind == K::Point && list.back().kind == K::Band && list.back().group == 1);
    }
    {  // every kind at once, two groups of each list kind
        const vag_fit_spec s = fit_full(true);
        const vag_sky_fit_spec sky = sky_full();
        const vag_vis_fit_spec vis = vis_full();
        const vag_pol_fit_spec pol = pol_full();
        const vag_counts_fit_spec counts = counts_spec();
        const vag_index_fit_spec index = index_spec();
        const vag_fold_fit_spec fold = fold_spec();
        const vag_cov_fit_spec cov = cov_spec();
        FitRequest r = fit_request(&s, &sky, &vis, &pol, nullptr, nullptr, &counts, &index, &fold, nullptr, &cov);
        CHECK(fit_request_prepare(r) == VAG_OK && scan_accepts(r));
        const std::vector<PassItem> list = fit_pass_list(r);
        CHECK(passes_are(list, {{K::Point, 0}, {K::Band, 0}, {K::Band, 1}, {K::Centroid, 0}, {K::Centroid, 1}, {K::Vis, 0}, {K::Vis, 1},
                                {K::Pol, 0}, {K::Pol, 1}, {K::Counts, 0}, {K::Counts, 1}, {K::Index, 0}, {K::Index, 1}, {K::Fold, 0},
                                {K::Fold, 1}, {K::Cov, 0}, {K::Cov, 1}}));
        CHECK(list.size() == 17 && list.front().kind == K::Point && list.back().kind == K::Cov && list.back().group == 1);
    }
    {  // nothing at all: the empty list is the request fit_scan refuses
        vag_fit_spec s = fit_full(false, 0);
        s.n_bands = 0;
        FitRequest r = fit_request(&s);
        CHECK(fit_request_prepare(r) == VAG_OK && fit_pass_list(r).empty() && !scan_accepts(r));
    }
    done("pass list", before);
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
    check_fit();
    check_sky();
    check_pol();
    check_vis();
    check_hashes();
    check_scan_keys(spec);
    check_prepare(spec);
    check_refusals(spec);
    check_block_refusals();
    check_block_columns();
    check_pass_list();
    if (g_failed) std::printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
