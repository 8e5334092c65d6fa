// vag_fit_request.h -- the host side of one likelihood request: what is done to its twelve spec blocks before a HIP call, the request
// that carries them, and its normalisation.  Two conventions.  Scanned every call (lim, noise, robust, tmpl, counts, index, fold, cov): *_scan
// validates the block and lays it out in a stage vector (int32 arrays packed into doubles, transposed whiteners, ...); a miss copies
// it.  Hashed in place, filled on a miss (fit, sky, vis, pol): *_scan makes the cheap checks and hashes the caller's arrays where they
// lie; only a miss runs *_rows (the row validation), then *_fill (into the pinned buffer).  Either way the scan leaves the block's
// BlockKey and its offsets in a *Layout, which the passes read.  Plain C++17, no device header and no context: a host compiler builds
// it, and tests/fit_request_check.cpp runs it under the host sanitizers.  vag_capi.hip keeps the uploads and the launches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vag_common.h"
#include "vag_poisson_const.h"

// the calling thread's last error text (vag_last_error); set_err formats it and hands the code back
static thread_local std::string g_err;

static int set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// content hash of a spec block (FNV-1a, 64 bit): what decides whether the block is resident already
static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
constexpr uint64_t FNV_SEED = 1469598103934665603ull;

// what says whether a block is resident already: the hash of its content, and its size.  Every *Layout is one.
struct BlockKey { uint64_t hash = 0; size_t doubles = 0; };

// The key of a block a scan has staged: what tells two layouts of the same bytes apart is in h already -- the passes' offsets, or the
// groups' shapes -- and the bytes follow.
static void key_staged(BlockKey& k, uint64_t h, const std::vector<double>& stage) {
    k.hash = fnv1a(h, stage.data(), sizeof(double) * stage.size());
    k.doubles = stage.size();
}
static uint64_t hash_offsets(long point, const std::vector<long>& band) {
    const uint64_t h = fnv1a(FNV_SEED, &point, sizeof point);
    return band.empty() ? h : fnv1a(h, band.data(), sizeof(long) * band.size());
}

// Block views.  Beside each layout below stands one *_cols function: the offsets of a group's columns, in doubles from the group's
// start, and the group's length.  The scan or fill that writes the block and the pass that reads it (loglike_passes, vag_capi.hip)
// both place every column through it; an int32 column is `(n + 1) / 2` doubles (ints_in).
static size_t ints_in(size_t n) { return (n + 1) / 2; }
static void put_doubles(double* dst, const double* src, size_t n) { std::memcpy(dst, src, sizeof(double) * n); }

// ---- upper-limit rows (vag_loglike_lim_batch): the blocks that hold a limit row, in one device buffer, uploaded like the other spec
//      blocks when the hash changes.  Layout in doubles: a flux block (the point rows, a band group) of n rows is
//      [limit | sigma | kind] (n, n, int32 [n] in (n + 1) / 2 doubles), a polarization group's block [kind] alone (its L and sigma are
//      the group's q and err_q in the pol block).  A block without a limit row is not stored (offset -1): its pass is the pass without
//      limits.  Rows that are detections hold limit 0 and sigma 1, whatever the caller's arrays hold there. ----
struct LimCols { size_t sigma, kind, doubles; };  // of a flux block of n rows (limit at 0)
static LimCols lim_cols(int n) { return {(size_t)n, 2 * (size_t)n, 2 * (size_t)n + ints_in(n)}; }

struct LimLayout : BlockKey {
    long point = -1;              // offset of the point rows' block in the lim block, or -1
    std::vector<long> band, pol;  // the same per band group / polarization group
    bool any = false;             // some limit row exists
};

static void lim_push_kinds(std::vector<double>& stage, const int32_t* kind, int n) {
    const size_t at = stage.size();
    stage.resize(at + ints_in(n), 0.0);
    std::memcpy(stage.data() + at, kind, sizeof(int32_t) * n);
}

// Checks one flux block of lim (what / g name it in messages) and appends it to stage when it holds a limit row.
static int lim_flux_block(const vag_limit_rows& r, int n, const char* what, int g, std::vector<double>& stage, long& off, bool& any) {
    off = -1;
    if (!r.kind || n <= 0) return VAG_OK;
    bool here = false;
    for (int i = 0; i < n; ++i) {
        if (r.kind[i] != VAG_OBS_DETECTION && r.kind[i] != VAG_OBS_UPPER_LIMIT)
            return set_err(VAG_E_INVALID, "limit rows, %s %d, row %d: unknown kind %d", what, g, i, r.kind[i]);
        if (r.kind[i] != VAG_OBS_UPPER_LIMIT) continue;
        if (!r.limit || !r.sigma) return set_err(VAG_E_INVALID, "limit rows, %s %d: null limit or sigma array", what, g);
        if (!std::isfinite(r.limit[i]) || r.limit[i] < 0)
            return set_err(VAG_E_INVALID, "limit rows, %s %d, row %d: the limit must be finite and >= 0", what, g, i);
        if (!std::isfinite(r.sigma[i]) || !(r.sigma[i] > 0))
            return set_err(VAG_E_INVALID, "limit rows, %s %d, row %d: sigma must be finite and > 0", what, g, i);
        here = true;
    }
    if (!here) return VAG_OK;
    any = true;
    const LimCols k = lim_cols(n);
    off = (long)stage.size();
    stage.resize(off + k.doubles, 0.0);
    double* dst = stage.data() + off;
    for (int i = 0; i < n; ++i) {
        dst[i] = r.kind[i] == VAG_OBS_UPPER_LIMIT ? r.limit[i] : 0.0;
        dst[k.sigma + i] = r.kind[i] == VAG_OBS_UPPER_LIMIT ? r.sigma[i] : 1.0;
    }
    std::memcpy(dst + k.kind, r.kind, sizeof(int32_t) * n);
    return VAG_OK;
}

// Validates lim against its partners and lays its blocks out in stage (host work only: no context is touched).
static int lim_scan(const vag_fit_spec* spec, const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, std::vector<double>& stage,
                    LimLayout& lay) {
    const int n_pol = pol ? pol->n_groups : 0;
    if (lim->n_bands != 0 && lim->n_bands != spec->n_bands)
        return set_err(VAG_E_INVALID, "limit rows: n_bands must be 0 or the fit spec's %d, got %d", spec->n_bands, lim->n_bands);
    if (lim->n_pol_groups != 0 && lim->n_pol_groups != n_pol)
        return set_err(VAG_E_INVALID, "limit rows: n_pol_groups must be 0 or the %d polarization groups, got %d", n_pol, lim->n_pol_groups);
    if ((lim->n_bands > 0 && !lim->bands) || (lim->n_pol_groups > 0 && !lim->pol_kind))
        return set_err(VAG_E_INVALID, "limit rows: null band or polarization list");
    if (lim->point.kind && spec->n_data > 0 && !spec->t) return set_err(VAG_E_INVALID, "limit rows: the fit spec has no point rows");
    int rc = lim_flux_block(lim->point, spec->n_data, "point rows", 0, stage, lay.point, lay.any);
    if (rc) return rc;
    lay.band.assign(std::max(spec->n_bands, 0), -1);
    for (int g = 0; g < lim->n_bands; ++g) {
        if (!spec->bands) return set_err(VAG_E_INVALID, "limit rows: the fit spec has no band groups");
        rc = lim_flux_block(lim->bands[g], spec->bands[g].n, "band group", g, stage, lay.band[g], lay.any);
        if (rc) return rc;
    }
    lay.pol.assign(std::max(n_pol, 0), -1);
    for (int g = 0; g < lim->n_pol_groups; ++g) {
        const int32_t* kind = lim->pol_kind[g];
        if (!kind) continue;
        if (!pol->groups) return set_err(VAG_E_INVALID, "bad polarization group list");
        const vag_polarization_obs& o = pol->groups[g];
        bool here = false;
        for (int i = 0; i < o.n; ++i) {
            if (kind[i] != VAG_OBS_DETECTION && kind[i] != VAG_OBS_UPPER_LIMIT)
                return set_err(VAG_E_INVALID, "limit rows, polarization group %d, epoch %d: unknown kind %d", g, i, kind[i]);
            if (kind[i] != VAG_OBS_UPPER_LIMIT) continue;
            if (o.kind != VAG_POL_DEGREE)
                return set_err(VAG_E_INVALID, "limit rows, polarization group %d, epoch %d: only VAG_POL_DEGREE groups take upper limits", g, i);
            if (!o.q || !o.err_q) return set_err(VAG_E_INVALID, "polarization group %d: null array", g);
            if (!std::isfinite(o.q[i]) || o.q[i] < 0 || o.q[i] > 1)
                return set_err(VAG_E_INVALID, "limit rows, polarization group %d, epoch %d: the limit must lie in [0, 1]", g, i);
            if (!std::isfinite(o.err_q[i]) || !(o.err_q[i] > 0))
                return set_err(VAG_E_INVALID, "limit rows, polarization group %d, epoch %d: sigma must be finite and > 0", g, i);
            here = true;
        }
        if (!here) continue;
        lay.any = true;
        lay.pol[g] = (long)stage.size();
        lim_push_kinds(stage, kind, o.n);
    }
    const uint64_t h = hash_offsets(lay.point, lay.band);
    key_staged(lay, lay.pol.empty() ? h : fnv1a(h, lay.pol.data(), sizeof(long) * lay.pol.size()), stage);
    return VAG_OK;
}

// ---- noise groups (vag_loglike_noise_batch): one device buffer, uploaded like the other spec blocks when the hash changes.  Layout
//      in doubles: [sys_fixed 8 | calib 8], then for every pass that holds a grouped row -- the point rows, a band group -- the rows'
//      group ids (int32 [n] in (n + 1) / 2 doubles).  A pass without a grouped row is not stored (offset -1): it is the pass without
//      noise groups. ----
struct NoiseLayout : BlockKey {
    long point = -1;                    // offset of the point rows' ids in the noise block, or -1
    std::vector<long> band;             // the same per band group
    unsigned point_present = 0;         // bit g: some point row is in group g
    std::vector<unsigned> band_present; // the same per band group
    int n_groups = 0;
    bool any = false;                   // some row is grouped
};

// Validates noise against the fit spec and lays its blocks out in stage (host work only: no context is touched).
static int noise_scan(const vag_fit_spec* spec, const vag_noise_fit_spec* nz, std::vector<double>& stage, NoiseLayout& lay) {
    if (nz->n_groups < 0 || nz->n_groups > VAG_NOISE_MAX_GROUPS)
        return set_err(VAG_E_INVALID, "noise groups: n_groups must be in 0..%d, got %d", VAG_NOISE_MAX_GROUPS, nz->n_groups);
    if (nz->n_bands != spec->n_bands)
        return set_err(VAG_E_INVALID, "noise groups: n_bands must be the fit spec's %d, got %d", spec->n_bands, nz->n_bands);
    if (nz->n_bands > 0 && (!nz->band_group || !spec->bands)) return set_err(VAG_E_INVALID, "noise groups: null band list");
    for (int g = 0; g < nz->n_groups; ++g) {
        if (!std::isfinite(nz->sys_fixed[g]) || nz->sys_fixed[g] < 0)
            return set_err(VAG_E_INVALID, "noise group %d: the systematic must be finite and >= 0", g);
        if (!std::isfinite(nz->calib[g]) || nz->calib[g] < 0)
            return set_err(VAG_E_INVALID, "noise group %d: the calibration fraction must be finite and >= 0", g);
    }
    lay.n_groups = nz->n_groups;
    stage.assign(2 * VAG_NOISE_MAX_GROUPS, 0.0);
    for (int g = 0; g < nz->n_groups; ++g) {
        stage[g] = nz->sys_fixed[g];
        stage[VAG_NOISE_MAX_GROUPS + g] = nz->calib[g];
    }
    int passes[VAG_NOISE_MAX_GROUPS] = {0};  // in how many passes a group has rows
    auto push_ids = [&](const int32_t* ids, int32_t same, int n) -> long {
        const long at = (long)stage.size();
        stage.resize(at + ((size_t)n + 1) / 2, 0.0);
        int32_t* dst = reinterpret_cast<int32_t*>(stage.data() + at);
        for (int i = 0; i < n; ++i) dst[i] = ids ? ids[i] : same;
        return at;
    };
    const int n = spec->n_data;
    if (nz->point_group && n > 0) {
        for (int i = 0; i < n; ++i) {
            const int id = nz->point_group[i];
            if (id < -1 || id >= nz->n_groups)
                return set_err(VAG_E_INVALID, "noise groups, point row %d: group %d is outside [-1, %d)", i, id, nz->n_groups);
            if (id >= 0) lay.point_present |= 1u << id;
        }
        if (lay.point_present) {
            lay.any = true;
            lay.point = push_ids(nz->point_group, 0, n);
            for (int g = 0; g < nz->n_groups; ++g) passes[g] += (lay.point_present >> g) & 1u;
        }
    }
    lay.band.assign(std::max(spec->n_bands, 0), -1);
    lay.band_present.assign(std::max(spec->n_bands, 0), 0u);
    for (int b = 0; b < nz->n_bands; ++b) {
        const int id = nz->band_group[b];
        if (id < -1 || id >= nz->n_groups)
            return set_err(VAG_E_INVALID, "noise groups, band group %d: group %d is outside [-1, %d)", b, id, nz->n_groups);
        if (id < 0 || spec->bands[b].n <= 0) continue;
        lay.any = true;
        lay.band_present[b] = 1u << id;
        lay.band[b] = push_ids(nullptr, id, spec->bands[b].n);
        ++passes[id];
    }
    for (int g = 0; g < nz->n_groups; ++g)
        if (nz->calib[g] > 0 && passes[g] > 1)
            return set_err(VAG_E_INVALID,
                           "noise group %d has a calibration fraction and rows in %d passes: such a group must hold point rows only or "
                           "exactly one band group", g, passes[g]);
    key_staged(lay, hash_offsets(lay.point, lay.band), stage);
    return VAG_OK;
}

// ---- outlier groups (vag_loglike_robust_batch): one device buffer, uploaded like the other spec blocks when the hash changes.  Layout
//      in doubles: [frac_fixed 8 | scale_fixed 8 | shift_fixed 8].  The rows' group ids are the noise block's. ----
constexpr size_t ROBUST_STAGE_DOUBLES = 3 * VAG_NOISE_MAX_GROUPS;

struct RobustLayout : BlockKey {
    bool any = false;             // some detection row lies in a robust group
    unsigned mask = 0;            // bit g: group g is robust
    bool point = false;           // the point rows hold a detection row of a robust group
    std::vector<char> band;       // the same per band group
};

// Validates the robust block against the fit spec, the noise block (which noise_scan has accepted) and the limit rows (which lim_scan
// has accepted; null: no limit row), and lays its fixed values out in stage (host work only: no context is touched).
static int robust_scan(const vag_fit_spec* spec, const vag_noise_fit_spec* nz, const vag_limit_fit_spec* lim, const vag_robust_fit_spec* rb,
                       std::vector<double>& stage, RobustLayout& lay) {
    if (!nz) return set_err(VAG_E_INVALID, "outlier groups need a noise block: a robust group is a noise group");
    if (rb->n_groups != nz->n_groups)
        return set_err(VAG_E_INVALID, "outlier groups: n_groups must be the noise spec's %d, got %d", nz->n_groups, rb->n_groups);
    if ((rb->mask >> rb->n_groups) != 0u)  // (n_groups is the noise spec's: 0 .. 8)
        return set_err(VAG_E_INVALID, "outlier groups: the mask 0x%x names a group at or above n_groups = %d", rb->mask, rb->n_groups);
    for (int g = 0; g < rb->n_groups; ++g) {
        if (((rb->mask >> g) & 1u) && nz->calib[g] > 0)
            return set_err(VAG_E_INVALID, "outlier group %d has a calibration fraction: the marginalised scale does not commute with the mixture", g);
        if (!std::isfinite(rb->frac_fixed[g]) || rb->frac_fixed[g] < 0 || !(rb->frac_fixed[g] < 1))
            return set_err(VAG_E_INVALID, "outlier group %d: the outlier fraction must be finite and in [0, 1)", g);
        if (!std::isfinite(rb->scale_fixed[g]) || rb->scale_fixed[g] < 0)
            return set_err(VAG_E_INVALID, "outlier group %d: the outlier scatter must be finite and >= 0", g);
        if (!std::isfinite(rb->shift_fixed[g])) return set_err(VAG_E_INVALID, "outlier group %d: the outlier offset must be finite", g);
    }
    lay.mask = rb->mask;
    stage.assign(ROBUST_STAGE_DOUBLES, 0.0);
    for (int g = 0; g < rb->n_groups; ++g) {
        stage[g] = rb->frac_fixed[g];
        stage[VAG_NOISE_MAX_GROUPS + g] = rb->scale_fixed[g];
        stage[2 * VAG_NOISE_MAX_GROUPS + g] = rb->shift_fixed[g];
    }
    auto robust_id = [&](int id) { return id >= 0 && ((rb->mask >> id) & 1u); };
    const int n = spec->n_data;
    const int32_t* pk = lim ? lim->point.kind : nullptr;
    if (nz->point_group)
        for (int i = 0; i < n && !lay.point; ++i)
            lay.point = robust_id(nz->point_group[i]) && !(pk && pk[i] == VAG_OBS_UPPER_LIMIT);
    lay.band.assign(std::max(spec->n_bands, 0), 0);
    for (int b = 0; b < nz->n_bands; ++b) {
        if (!robust_id(nz->band_group[b])) continue;
        const int32_t* bk = (lim && b < lim->n_bands) ? lim->bands[b].kind : nullptr;
        for (int i = 0; i < spec->bands[b].n && !lay.band[b]; ++i) lay.band[b] = !(bk && bk[i] == VAG_OBS_UPPER_LIMIT);
    }
    lay.any = lay.point || std::find(lay.band.begin(), lay.band.end(), (char)1) != lay.band.end();
    key_staged(lay, fnv1a(FNV_SEED, &lay.mask, sizeof lay.mask), stage);
    return VAG_OK;
}

// ---- additive templates (vag_loglike_tmpl_batch): one device buffer, uploaded like the other spec blocks when the hash changes.
//      Layout in doubles: [amp_fixed 8], then for every pass with a touched row -- the point rows, a band group -- its values
//      [n_templates][n].  A pass no template touches is not stored (offset -1): it is the pass without templates. ----
struct TmplLayout : BlockKey {
    long point = -1;                    // offset of the point rows' values in the tmpl block, or -1
    std::vector<long> band;             // the same per band group
    unsigned point_present = 0;         // bit c: template c touches some point row
    std::vector<unsigned> band_present; // the same per band group
    unsigned ext_mask = 0;              // bit c: template c is extinguished
    int n_templates = 0;
    bool any = false;                   // some row is touched
};

// Validates tmpl against the fit spec and lays its blocks out in stage (host work only: no context is touched).
static int tmpl_scan(const vag_fit_spec* spec, const vag_template_fit_spec* tp, std::vector<double>& stage, TmplLayout& lay) {
    if (tp->n_templates < 0 || tp->n_templates > VAG_TMPL_MAX)
        return set_err(VAG_E_INVALID, "templates: n_templates must be in 0..%d, got %d", VAG_TMPL_MAX, tp->n_templates);
    if (tp->n_bands != 0 && tp->n_bands != spec->n_bands)
        return set_err(VAG_E_INVALID, "templates: n_bands must be 0 or the fit spec's %d, got %d", spec->n_bands, tp->n_bands);
    if (tp->n_bands > 0 && (!tp->bands || !spec->bands)) return set_err(VAG_E_INVALID, "templates: null band list");
    const int nt = tp->n_templates;
    for (int c = 0; c < nt; ++c) {
        if (!std::isfinite(tp->amp_fixed[c]) || tp->amp_fixed[c] < 0)
            return set_err(VAG_E_INVALID, "template %d: the fixed amplitude must be finite and >= 0", c);
        if (tp->extinguished[c] != 0 && tp->extinguished[c] != 1)
            return set_err(VAG_E_INVALID, "template %d: extinguished must be 0 or 1, got %d", c, tp->extinguished[c]);
        lay.ext_mask |= (unsigned)tp->extinguished[c] << c;
    }
    lay.n_templates = nt;
    stage.assign(VAG_TMPL_MAX, 0.0);
    for (int c = 0; c < nt; ++c) stage[c] = tp->amp_fixed[c];
    // one pass's block: checked, and stored when some value is not 0
    auto push = [&](const double* T, int n, const char* what, int b, long& at, unsigned& present) -> int {
        for (int c = 0; c < nt; ++c)
            for (int i = 0; i < n; ++i) {
                const double v = T[(size_t)c * n + i];
                if (!std::isfinite(v) || v < 0) {
                    if (b < 0) return set_err(VAG_E_INVALID, "template %d, %s %d: the value must be finite and >= 0", c, what, i);
                    return set_err(VAG_E_INVALID, "template %d, %s %d, row %d: the value must be finite and >= 0", c, what, b, i);
                }
                if (v != 0.0) present |= 1u << c;
            }
        if (present) {
            lay.any = true;
            at = (long)stage.size();
            stage.insert(stage.end(), T, T + (size_t)nt * n);
        }
        return VAG_OK;
    };
    int rc = VAG_OK;
    if (tp->point && nt > 0 && spec->n_data > 0 && (rc = push(tp->point, spec->n_data, "point row", -1, lay.point, lay.point_present)))
        return rc;
    lay.band.assign(std::max(spec->n_bands, 0), -1);
    lay.band_present.assign(std::max(spec->n_bands, 0), 0u);
    for (int b = 0; b < tp->n_bands && nt > 0; ++b) {
        if (!tp->bands[b] || spec->bands[b].n <= 0) continue;
        if ((rc = push(tp->bands[b], spec->bands[b].n, "band group", b, lay.band[b], lay.band_present[b]))) return rc;
    }
    key_staged(lay, hash_offsets(lay.point, lay.band), stage);
    return VAG_OK;
}

// ---- counts groups (vag_loglike_counts_batch): one device buffer, uploaded like the other spec blocks when the hash changes.  Layout
//      in doubles, per group: [t_sample ns | N n | B n | a n | w n], then the sample indices (int32 [n m] in (n m + 1) / 2 doubles). ----
struct CountsCols { size_t N, B, a, w, idx, doubles; };  // (t_sample at 0)
static CountsCols counts_cols(const vag_counts_obs& o) {
    const size_t ns = (size_t)o.n_samples, n = (size_t)o.n;
    return {ns, ns + n, ns + 2 * n, ns + 3 * n, ns + 4 * n, ns + 4 * n + ints_in(n * (size_t)o.m)};
}

struct CountsLayout : BlockKey {
    std::vector<long> off;       // where group g starts in the counts block
    std::vector<double> const2;  // -2 sum_i w_i S_i of group g (vag::poisson_const): the walker-independent half of its chi^2
    int n_groups = 0;
};

// Validates the counts groups and lays their blocks out in stage (host work only: no context is touched).
static int counts_scan(const vag_counts_fit_spec* cs, std::vector<double>& stage, CountsLayout& lay) {
    if (cs->n_groups < 0 || !cs->groups) return set_err(VAG_E_INVALID, "counts groups: n_groups must be >= 0 with a group list, got %d", cs->n_groups);
    lay.n_groups = cs->n_groups;
    stage.clear();
    uint64_t h = FNV_SEED;  // (the shapes: two groups whose blocks hold the same bytes are still two layouts; so index, fold, cov)
    for (int g = 0; g < cs->n_groups; ++g) {
        const vag_counts_obs& o = cs->groups[g];
        const int head[4] = {o.n, o.m, o.n_samples, o.num_points};
        h = fnv1a(h, head, sizeof head);
        if (!(std::isfinite(o.nu_min) && std::isfinite(o.nu_max) && o.nu_min > 0 && o.nu_max > o.nu_min))
            return set_err(VAG_E_INVALID, "counts group %d: the band needs 0 < nu_min < nu_max, both finite", g);
        if (o.num_points < 2 || o.num_points > VAG_MAX_NU)
            return set_err(VAG_E_INVALID, "counts group %d: num_points must be in 2..%d, got %d", g, VAG_MAX_NU, o.num_points);
        if (o.n < 1) return set_err(VAG_E_INVALID, "counts group %d has no rows", g);
        if (o.m < 1) return set_err(VAG_E_INVALID, "counts group %d: m (samples per row) must be >= 1, got %d", g, o.m);
        if (o.n_samples < 1) return set_err(VAG_E_INVALID, "counts group %d has no sample times", g);
        if (!o.t_sample || !o.sample_idx || !o.counts || !o.background || !o.scale || !o.weight)
            return set_err(VAG_E_INVALID, "counts group %d: null array", g);
        for (int j = 0; j < o.n_samples; ++j)
            if (!std::isfinite(o.t_sample[j]) || !(o.t_sample[j] > 0) || (j > 0 && !(o.t_sample[j] > o.t_sample[j - 1])))
                return set_err(VAG_E_INVALID, "counts group %d, sample %d: sample times must be finite, > 0 and strictly ascending", g, j);
        double wS = 0;
        for (int i = 0; i < o.n; ++i) {
            const double N = o.counts[i];
            if (!std::isfinite(N) || N < 0 || N != std::floor(N))
                return set_err(VAG_E_INVALID, "counts group %d, row %d: counts must be a finite integer >= 0, got %g", g, i, N);
            if (N > 9007199254740992.0) return set_err(VAG_E_INVALID, "counts group %d, row %d: counts above 2^53", g, i);
            if (!std::isfinite(o.background[i]) || o.background[i] < 0)
                return set_err(VAG_E_INVALID, "counts group %d, row %d: the background must be finite and >= 0", g, i);
            if (!std::isfinite(o.scale[i]) || !(o.scale[i] > 0))
                return set_err(VAG_E_INVALID, "counts group %d, row %d: the scale must be finite and > 0", g, i);
            if (!std::isfinite(o.weight[i]) || o.weight[i] < 0)
                return set_err(VAG_E_INVALID, "counts group %d, row %d: the weight must be finite and >= 0", g, i);
            for (int k = 0; k < o.m; ++k) {
                const int j = o.sample_idx[(size_t)i * o.m + k];
                if (j < 0 || j >= o.n_samples)
                    return set_err(VAG_E_INVALID, "counts group %d, row %d: sample index %d is outside [0, %d)", g, i, j, o.n_samples);
            }
            if (o.weight[i] > 0) wS += o.weight[i] * vag::poisson_const(N);
        }
        const CountsCols k = counts_cols(o);
        const size_t at = stage.size(), n = (size_t)o.n;
        lay.off.push_back((long)at);
        lay.const2.push_back(-2.0 * wS);
        stage.resize(at + k.doubles, 0.0);
        double* dst = stage.data() + at;
        put_doubles(dst, o.t_sample, o.n_samples);
        put_doubles(dst + k.N, o.counts, n);
        put_doubles(dst + k.B, o.background, n);
        put_doubles(dst + k.a, o.scale, n);
        put_doubles(dst + k.w, o.weight, n);
        std::memcpy(dst + k.idx, o.sample_idx, sizeof(int32_t) * n * o.m);
    }
    key_staged(lay, h, stage);
    return VAG_OK;
}

// ---- spectral-index groups (vag_loglike_index_batch): one device buffer, uploaded like the other spec blocks when the hash changes.
//      Layout in doubles, per group: [t n K | nu n K | s n | sigma n | w n | c K]; the first two are the series points (t_i, nu_k), i
//      outer, as prep_times takes them. ----
struct IndexCols { size_t nu, value, err, weight, coef, doubles; };  // (t at 0; t and nu hold the n K series points)
static IndexCols index_cols(const vag_index_obs& o) {
    const size_t n = (size_t)o.n, K = (size_t)o.k, np = n * K;
    return {np, 2 * np, 2 * np + n, 2 * np + 2 * n, 2 * np + 3 * n, 2 * np + 3 * n + K};
}

struct IndexLayout : BlockKey {
    std::vector<long> off;  // where group g starts in the index block
    int n_groups = 0;
};

// Validates the spectral-index groups and lays their blocks out in stage (host work only: no context is touched).
static int index_scan(const vag_index_fit_spec* is, std::vector<double>& stage, IndexLayout& lay) {
    if (is->n_groups < 0 || !is->groups) return set_err(VAG_E_INVALID, "index groups: n_groups must be >= 0 with a group list, got %d", is->n_groups);
    lay.n_groups = is->n_groups;
    lay.off.clear();
    stage.clear();
    uint64_t h = FNV_SEED;
    for (int g = 0; g < is->n_groups; ++g) {
        const vag_index_obs& o = is->groups[g];
        const int head[2] = {o.n, o.k};
        h = fnv1a(h, head, sizeof head);
        if (o.k < 2 || o.k > VAG_INDEX_MAX_NODES)
            return set_err(VAG_E_INVALID, "index group %d: k (frequencies) must be in 2..%d, got %d", g, VAG_INDEX_MAX_NODES, o.k);
        if (o.n < 1) return set_err(VAG_E_INVALID, "index group %d has no rows", g);
        if (o.n > (1 << 24)) return set_err(VAG_E_INVALID, "index group %d: more than %d rows", g, 1 << 24);
        if (!o.nu || !o.coef || !o.t || !o.value || !o.err || !o.weight) return set_err(VAG_E_INVALID, "index group %d: null array", g);
        for (int k = 0; k < o.k; ++k) {
            if (!std::isfinite(o.nu[k]) || !(o.nu[k] > 0) || (k > 0 && !(o.nu[k] > o.nu[k - 1])))
                return set_err(VAG_E_INVALID, "index group %d, frequency %d: frequencies must be finite, > 0 and strictly ascending", g, k);
            if (!std::isfinite(o.coef[k])) return set_err(VAG_E_INVALID, "index group %d, coefficient %d is not finite", g, k);
        }
        if (!std::isfinite(o.ext_slope)) return set_err(VAG_E_INVALID, "index group %d: ext_slope is not finite", g);
        for (int i = 0; i < o.n; ++i) {
            if (!std::isfinite(o.t[i]) || !(o.t[i] > 0) || (i > 0 && o.t[i] < o.t[i - 1]))
                return set_err(VAG_E_INVALID, "index group %d, row %d: times must be finite, > 0 and ascending", g, i);
            if (!std::isfinite(o.value[i])) return set_err(VAG_E_INVALID, "index group %d, row %d: the index is not finite", g, i);
            if (!std::isfinite(o.err[i]) || !(o.err[i] > 0))
                return set_err(VAG_E_INVALID, "index group %d, row %d: the error must be finite and > 0", g, i);
            if (!std::isfinite(o.weight[i]) || o.weight[i] < 0)
                return set_err(VAG_E_INVALID, "index group %d, row %d: the weight must be finite and >= 0", g, i);
        }
        const IndexCols c = index_cols(o);
        const size_t at = stage.size(), n = (size_t)o.n, K = (size_t)o.k;
        lay.off.push_back((long)at);
        stage.resize(at + c.doubles, 0.0);
        double* dst = stage.data() + at;
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < K; ++k) {
                dst[i * K + k] = o.t[i];
                dst[c.nu + i * K + k] = o.nu[k];
            }
        put_doubles(dst + c.value, o.value, n);
        put_doubles(dst + c.err, o.err, n);
        put_doubles(dst + c.weight, o.weight, n);
        put_doubles(dst + c.coef, o.coef, K);
    }
    key_staged(lay, h, stage);
    return VAG_OK;
}

// ---- fold groups (vag_loglike_fold_batch): one device buffer, uploaded like the other spec blocks when the hash changes.  Layout in
//      doubles, per group: [t ns J | nu ns J | A J C | sigma J | exposure / m n | N n C | B n C | w n C], then the sample indices
//      (int32 [n m] in (n m + 1) / 2 doubles); the first two are the series points (t_sample_s, nu_j), s outer, as prep_times takes
//      them; sigma is zeros for a group without one (the kernel is handed a null pointer then). ----
struct FoldCols { size_t nu, A, sigma, eom, N, B, w, idx, doubles; };  // (t at 0; t and nu hold the n_samples J series points)
static FoldCols fold_cols(const vag_fold_obs& o) {
    const size_t J = (size_t)o.J, n = (size_t)o.n, nc = n * (size_t)o.C, np = (size_t)o.n_samples * J;
    const size_t sigma = 2 * np + J * (size_t)o.C, N = sigma + J + n, idx = N + 3 * nc;
    return {np, 2 * np, sigma, sigma + J, N, N + nc, N + 2 * nc, idx, idx + ints_in(n * (size_t)o.m)};
}

struct FoldLayout : BlockKey {
    std::vector<long> off;       // where group g starts in the fold block
    std::vector<double> const2;  // -2 sum_{i,c} w S of group g (vag::poisson_const): the walker-independent half of its chi^2
    bool any_sigma = false;      // some group carries a cross-section: N_H is read
    int n_groups = 0;
};

// Validates the fold groups and lays their blocks out in stage (host work only: no context is touched).
static int fold_scan(const vag_fit_spec* spec, const vag_fold_fit_spec* fs, std::vector<double>& stage, FoldLayout& lay) {
    if (fs->n_groups < 0 || !fs->groups) return set_err(VAG_E_INVALID, "fold groups: n_groups must be >= 0 with a group list, got %d", fs->n_groups);
    if (!std::isfinite(fs->n_h_fixed) || fs->n_h_fixed < 0) return set_err(VAG_E_INVALID, "fold groups: n_h_fixed must be finite and >= 0");
    lay.n_groups = fs->n_groups;
    lay.off.clear();
    lay.const2.clear();
    lay.any_sigma = false;
    stage.clear();
    uint64_t h = FNV_SEED;
    for (int g = 0; g < fs->n_groups; ++g) {
        const vag_fold_obs& o = fs->groups[g];
        const int head[6] = {o.J, o.C, o.n, o.m, o.n_samples, o.sigma ? 1 : 0};
        h = fnv1a(h, head, sizeof head);
        if (o.J < 1 || o.J > VAG_FOLD_MAX_BINS)
            return set_err(VAG_E_INVALID, "fold group %d: J (energy bins) must be in 1..%d, got %d", g, VAG_FOLD_MAX_BINS, o.J);
        if (o.C < 1 || o.C > VAG_FOLD_MAX_CHANNELS)
            return set_err(VAG_E_INVALID, "fold group %d: C (channels) must be in 1..%d, got %d", g, VAG_FOLD_MAX_CHANNELS, o.C);
        if (o.n < 1) return set_err(VAG_E_INVALID, "fold group %d has no rows", g);
        if (o.m < 1) return set_err(VAG_E_INVALID, "fold group %d: m (samples per row) must be >= 1, got %d", g, o.m);
        if (o.n_samples < 1) return set_err(VAG_E_INVALID, "fold group %d has no sample times", g);
        if (o.n > (1 << 16) || o.m > (1 << 10) || o.n_samples > (1 << 18))
            return set_err(VAG_E_INVALID, "fold group %d: more than %d rows, %d samples per row or %d sample times", g, 1 << 16, 1 << 10, 1 << 18);
        if (!o.nu || !o.A || !o.t_sample || !o.sample_idx || !o.exposure_over_m || !o.counts || !o.background || !o.weight)
            return set_err(VAG_E_INVALID, "fold group %d: null array", g);
        for (int j = 0; j < o.J; ++j) {
            if (!std::isfinite(o.nu[j]) || !(o.nu[j] > 0) || (j > 0 && !(o.nu[j] > o.nu[j - 1])))
                return set_err(VAG_E_INVALID, "fold group %d, bin %d: frequencies must be finite, > 0 and strictly ascending", g, j);
            if (o.sigma && (!std::isfinite(o.sigma[j]) || o.sigma[j] < 0))
                return set_err(VAG_E_INVALID, "fold group %d, bin %d: the cross-section must be finite and >= 0", g, j);
            for (int ch = 0; ch < o.C; ++ch) {
                const double a = o.A[(size_t)j * o.C + ch];
                if (!std::isfinite(a) || a < 0)
                    return set_err(VAG_E_INVALID, "fold group %d, bin %d, channel %d: the response must be finite and >= 0", g, j, ch);
            }
        }
        for (int j = 0; j < o.n_samples; ++j)
            if (!std::isfinite(o.t_sample[j]) || !(o.t_sample[j] > 0) || (j > 0 && !(o.t_sample[j] > o.t_sample[j - 1])))
                return set_err(VAG_E_INVALID, "fold group %d, sample %d: sample times must be finite, > 0 and strictly ascending", g, j);
        double wS = 0;
        for (int i = 0; i < o.n; ++i) {
            if (!std::isfinite(o.exposure_over_m[i]) || !(o.exposure_over_m[i] > 0))
                return set_err(VAG_E_INVALID, "fold group %d, row %d: exposure_over_m must be finite and > 0", g, i);
            for (int k = 0; k < o.m; ++k) {
                const int j = o.sample_idx[(size_t)i * o.m + k];
                if (j < 0 || j >= o.n_samples)
                    return set_err(VAG_E_INVALID, "fold group %d, row %d: sample index %d is outside [0, %d)", g, i, j, o.n_samples);
            }
            for (int ch = 0; ch < o.C; ++ch) {
                const size_t at = (size_t)i * o.C + ch;
                const double N = o.counts[at];
                if (!std::isfinite(N) || N < 0 || N != std::floor(N))
                    return set_err(VAG_E_INVALID, "fold group %d, row %d, channel %d: counts must be a finite integer >= 0, got %g", g, i, ch, N);
                if (N > 9007199254740992.0) return set_err(VAG_E_INVALID, "fold group %d, row %d, channel %d: counts above 2^53", g, i, ch);
                if (!std::isfinite(o.background[at]) || o.background[at] < 0)
                    return set_err(VAG_E_INVALID, "fold group %d, row %d, channel %d: the background must be finite and >= 0", g, i, ch);
                if (!std::isfinite(o.weight[at]) || o.weight[at] < 0)
                    return set_err(VAG_E_INVALID, "fold group %d, row %d, channel %d: the weight must be finite and >= 0", g, i, ch);
                if (o.weight[at] > 0) wS += o.weight[at] * vag::poisson_const(N);
            }
        }
        if (o.sigma) lay.any_sigma = true;
        const FoldCols k = fold_cols(o);
        const size_t at = stage.size(), J = (size_t)o.J, C = (size_t)o.C, n = (size_t)o.n, ns = (size_t)o.n_samples;
        lay.off.push_back((long)at);
        lay.const2.push_back(-2.0 * wS);
        stage.resize(at + k.doubles, 0.0);
        double* dst = stage.data() + at;
        for (size_t q = 0; q < ns; ++q)
            for (size_t j = 0; j < J; ++j) {
                dst[q * J + j] = o.t_sample[q];
                dst[k.nu + q * J + j] = o.nu[j];
            }
        put_doubles(dst + k.A, o.A, J * C);
        if (o.sigma) put_doubles(dst + k.sigma, o.sigma, J);
        put_doubles(dst + k.eom, o.exposure_over_m, n);
        put_doubles(dst + k.N, o.counts, n * C);
        put_doubles(dst + k.B, o.background, n * C);
        put_doubles(dst + k.w, o.weight, n * C);
        std::memcpy(dst + k.idx, o.sample_idx, sizeof(int32_t) * n * o.m);
    }
    // (N_H is read by groups with a cross-section only: without one it is refused as a free parameter, the rule of east0 / north0)
    if (!lay.any_sigma)
        for (int d = 0; d < spec->ndim && d < 16; ++d)
            if (spec->slot[d] == VAG_P_N_H) return set_err(VAG_E_INVALID, "bad parameter slot");
    key_staged(lay, h, stage);
    return VAG_OK;
}

// ---- correlated groups (vag_loglike_cov_batch): one device buffer, uploaded like the other spec blocks when the hash changes.  Layout
//      in doubles, per group: [t n | nu n | ln_flux n | ext n | Wt n n]; the first two are the series points as prep_times takes
//      them; ext is zeros for a group without one (the kernel is handed a null pointer then); Wt[j n + i] = W_ij for j <= i, else 0:
//      the whitener transposed, so that a wavefront whose lanes hold consecutive rows i loads consecutive doubles. ----
struct CovCols { size_t nu, ln_flux, ext, Wt, doubles; };  // (t at 0)
static CovCols cov_cols(const vag_cov_obs& o) {
    const size_t n = (size_t)o.n;
    return {n, 2 * n, 3 * n, 4 * n, 4 * n + n * n};
}

struct CovLayout : BlockKey {
    std::vector<long> off;  // where group g starts in the cov block
    int n_groups = 0;
};

// Validates the correlated groups and lays their blocks out in stage (host work only: no context is touched).
static int cov_scan(const vag_cov_fit_spec* cs, std::vector<double>& stage, CovLayout& lay) {
    if (cs->n_groups < 0 || cs->n_groups > VAG_COV_MAX_GROUPS)
        return set_err(VAG_E_INVALID, "correlated groups: n_groups must be in 0..%d, got %d", VAG_COV_MAX_GROUPS, cs->n_groups);
    if (!cs->groups) return set_err(VAG_E_INVALID, "correlated groups: null group list");
    lay.n_groups = cs->n_groups;
    lay.off.clear();
    stage.clear();
    uint64_t h = FNV_SEED;
    for (int g = 0; g < cs->n_groups; ++g) {
        const vag_cov_obs& o = cs->groups[g];
        const int head[2] = {o.n, o.ext ? 1 : 0};
        h = fnv1a(h, head, sizeof head);
        if (o.n < 1 || o.n > VAG_COV_MAX_ROWS)
            return set_err(VAG_E_INVALID, "correlated group %d: n (rows) must be in 1..%d, got %d", g, VAG_COV_MAX_ROWS, o.n);
        if (!o.t || !o.nu || !o.ln_flux || !o.whitener) return set_err(VAG_E_INVALID, "correlated group %d: null array", g);
        if (!std::isfinite(o.weight) || o.weight < 0)
            return set_err(VAG_E_INVALID, "correlated group %d: the weight must be finite and >= 0", g);
        const size_t n = (size_t)o.n;
        for (int i = 0; i < o.n; ++i) {
            if (!std::isfinite(o.t[i]) || !(o.t[i] > 0) || (i > 0 && o.t[i] < o.t[i - 1]))
                return set_err(VAG_E_INVALID, "correlated group %d, row %d: times must be finite, > 0 and ascending", g, i);
            if (!std::isfinite(o.nu[i]) || !(o.nu[i] > 0))
                return set_err(VAG_E_INVALID, "correlated group %d, row %d: the frequency must be finite and > 0", g, i);
            if (!std::isfinite(o.ln_flux[i])) return set_err(VAG_E_INVALID, "correlated group %d, row %d: ln_flux is not finite", g, i);
            if (o.ext && !std::isfinite(o.ext[i])) return set_err(VAG_E_INVALID, "correlated group %d, row %d: ext is not finite", g, i);
            for (int j = 0; j <= i; ++j)
                if (!std::isfinite(o.whitener[i * n + j]))
                    return set_err(VAG_E_INVALID, "correlated group %d, row %d: whitener entry %d is not finite", g, i, j);
            if (!(o.whitener[i * n + i] > 0))
                return set_err(VAG_E_INVALID, "correlated group %d, row %d: the whitener's diagonal entry must be > 0", g, i);
        }
        const CovCols k = cov_cols(o);
        const size_t at = stage.size();
        lay.off.push_back((long)at);
        stage.resize(at + k.doubles, 0.0);
        double* dst = stage.data() + at;
        put_doubles(dst, o.t, n);
        put_doubles(dst + k.nu, o.nu, n);
        put_doubles(dst + k.ln_flux, o.ln_flux, n);
        if (o.ext) put_doubles(dst + k.ext, o.ext, n);
        double* Wt = dst + k.Wt;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j <= i; ++j) Wt[j * n + i] = o.whitener[i * n + j];
    }
    key_staged(lay, h, stage);
    return VAG_OK;
}

// ---- the fit spec (every vag_loglike_*_batch): the observation arrays, the slot map and the priors in one device buffer.  Layout in
//      doubles: [t | nu | ln_flux | ln_err | weight | ext] (n each, in 6 max(n, 1); ext is zeros without an ext_kernel), then per band
//      group [t | ln_flux | ln_err | weight] (bd.n each), then [lower | upper | prior_a | prior_b] (16 each), then int32
//      [slot | is_log | prior_kind] (16 each). ----
struct BandCols { size_t ln_flux, ln_err, weight, doubles; };  // of a band group of n rows (t at 0)
static BandCols band_cols(int n) { return {(size_t)n, 2 * (size_t)n, 3 * (size_t)n, 4 * (size_t)n}; }

struct FitLayout : BlockKey {
    size_t nu = 0, ln_flux = 0, ln_err = 0, weight = 0, ext = 0;  // the point rows' columns (t is at 0)
    std::vector<size_t> band;                                     // where band group g starts
    size_t prior = 0;                                             // where the prior block starts
};

// The slots a fit spec may free beyond the model's own, by what else the request holds: the placement (some group reads it), the
// field of polarization groups, N_H (a fold group with a cross-section), the systematic of a noise group and the amplitude of a
// template that exist, and the three outlier parameters of a robust group.  counts: some group is data without a flux row (counts,
// index, fold, cov).
struct FitAccepts {
    bool sky = false, pol = false, n_h = false, counts = false;
    int noise_groups = 0, n_templates = 0;
    unsigned robust_mask = 0;  // bit g: noise group g is robust
};

// the group of an outlier-parameter slot (VAG_P_ROBUST_FRAC0 / _SCALE0 / _SHIFT0 + g), or -1
static int robust_slot_group(int s) {
    for (int base : {VAG_P_ROBUST_FRAC0, VAG_P_ROBUST_SCALE0, VAG_P_ROBUST_SHIFT0})
        if (s >= base && s < base + VAG_NOISE_MAX_GROUPS) return s - base;
    return -1;
}

static int fit_scan(const vag_fit_spec* spec, int ndim, const FitAccepts& acc, FitLayout& lay) {
    if (ndim != spec->ndim || ndim <= 0 || ndim > 16) return set_err(VAG_E_INVALID, "ndim must match spec and be in 1..16");
    const int n = spec->n_data;
    if (n < 0 || spec->n_bands < 0 || (n == 0 && spec->n_bands == 0 && !acc.sky && !acc.pol && !acc.counts))
        return set_err(VAG_E_INVALID, "fit spec has no data");
    for (int d = 0; d < ndim; ++d) {
        const int s = spec->slot[d];
        if (s == VAG_P_A_V) continue;
        if (acc.sky && s >= VAG_P_SKY_PA && s <= VAG_P_SKY_NORTH0) continue;
        if (acc.pol && (s == VAG_P_SKY_PA || (s >= VAG_P_POL_B && s <= VAG_P_POL_PI_MAX_RVS))) continue;
        if (s >= VAG_P_NOISE_SYS0 && s < VAG_P_NOISE_SYS0 + acc.noise_groups) continue;
        if (acc.n_h && s == VAG_P_N_H) continue;
        if (s >= VAG_P_TMPL_AMP0 && s < VAG_P_TMPL_AMP0 + acc.n_templates) continue;
        if (robust_slot_group(s) >= 0 && ((acc.robust_mask >> robust_slot_group(s)) & 1u)) continue;
        if (s < 0 || (s >= VAG_P_COUNT && (s < VAG_P_RVS_EPS_E || s > VAG_P_MAG_Q))) return set_err(VAG_E_INVALID, "bad parameter slot");
    }
    if (spec->use_priors)
        for (int d = 0; d < ndim; ++d) {
            if (!(spec->lower[d] < spec->upper[d])) return set_err(VAG_E_INVALID, "prior bounds of parameter %d: need lower < upper", d);
            const int k = spec->prior_kind[d];
            if (k < VAG_PRIOR_UNIFORM || k > VAG_PRIOR_UNIFORM_RANGE) return set_err(VAG_E_INVALID, "unknown prior kind %d", k);
            if (k == VAG_PRIOR_UNIFORM_RANGE && !(spec->prior_b[d] > spec->prior_a[d])) return set_err(VAG_E_INVALID, "Uniform prior needs maximum > minimum");
            if (k == VAG_PRIOR_GAUSSIAN && !(spec->prior_b[d] > 0)) return set_err(VAG_E_INVALID, "Gaussian prior needs sigma > 0");
            if (k == VAG_PRIOR_LOG_UNIFORM && !(spec->prior_a[d] > 0 && spec->prior_b[d] > spec->prior_a[d]))
                return set_err(VAG_E_INVALID, "LogUniform prior needs 0 < minimum < maximum");
        }
    const int head[4] = {n, spec->n_bands, ndim, spec->ext_kernel ? 1 : 0};
    uint64_t& h = lay.hash = fnv1a(FNV_SEED, head, sizeof head);
    lay.nu = n, lay.ln_flux = 2 * (size_t)n, lay.ln_err = 3 * (size_t)n, lay.weight = 4 * (size_t)n, lay.ext = 5 * (size_t)n;
    size_t total = 6 * (size_t)std::max(n, 1);
    for (const double* arr : {spec->t, spec->nu, spec->ln_flux, spec->ln_err, spec->weight, spec->ext_kernel})
        if (arr && n > 0) h = fnv1a(h, arr, sizeof(double) * n);
    lay.band.clear();
    for (int g = 0; g < spec->n_bands; ++g) {
        const vag_band_obs& bd = spec->bands[g];
        if (bd.n <= 0) return set_err(VAG_E_INVALID, "band group %d has no observations", g);
        h = fnv1a(h, &bd.n, sizeof bd.n);
        for (const double* arr : {bd.t, bd.ln_flux, bd.ln_err, bd.weight}) h = fnv1a(h, arr, sizeof(double) * bd.n);
        lay.band.push_back(total);
        total += band_cols(bd.n).doubles;
    }
    h = fnv1a(h, spec->slot, sizeof spec->slot);
    h = fnv1a(h, spec->is_log, sizeof spec->is_log);
    h = fnv1a(h, &spec->use_priors, sizeof spec->use_priors);
    if (spec->use_priors) {
        h = fnv1a(fnv1a(h, spec->lower, sizeof spec->lower), spec->upper, sizeof spec->upper);
        h = fnv1a(h, spec->prior_kind, sizeof spec->prior_kind);
        h = fnv1a(fnv1a(h, spec->prior_a, sizeof spec->prior_a), spec->prior_b, sizeof spec->prior_b);
    }
    lay.prior = total;
    lay.doubles = total + 4 * 16 + 3 * 16 / 2;  // four double[16] + three int32[16]
    return VAG_OK;
}

static int fit_rows(const vag_fit_spec* spec) {
    const int n = spec->n_data;
    for (int i = 0; i < n; ++i)
        if (!(spec->t[i] > 0)) return set_err(VAG_E_INVALID, "data times must be positive");
    for (int i = 1; i < n; ++i)
        if (spec->t[i] < spec->t[i - 1]) return set_err(VAG_E_INVALID, "data times must be ascending (fitter.py:420-428)");
    for (int g = 0; g < spec->n_bands; ++g) {
        const vag_band_obs& bd = spec->bands[g];
        for (int i = 0; i < bd.n; ++i)
            if (!(bd.t[i] > 0) || (i > 0 && bd.t[i] < bd.t[i - 1]))
                return set_err(VAG_E_INVALID, "band group %d: times must be positive and ascending", g);
    }
    return VAG_OK;
}

static void fit_fill(const vag_fit_spec* spec, const FitLayout& lay, double* hp) {
    const size_t n = (size_t)spec->n_data;
    std::memset(hp, 0, sizeof(double) * lay.doubles);
    const double* src[6] = {spec->t, spec->nu, spec->ln_flux, spec->ln_err, spec->weight, spec->ext_kernel};
    const size_t at[6] = {0, lay.nu, lay.ln_flux, lay.ln_err, lay.weight, lay.ext};
    for (int q = 0; q < 6 && n > 0; ++q)
        if (src[q]) std::memcpy(hp + at[q], src[q], sizeof(double) * n);
    for (int g = 0; g < spec->n_bands; ++g) {
        const vag_band_obs& bd = spec->bands[g];
        const BandCols k = band_cols(bd.n);
        double* dst = hp + lay.band[g];
        put_doubles(dst, bd.t, bd.n);
        put_doubles(dst + k.ln_flux, bd.ln_flux, bd.n);
        put_doubles(dst + k.ln_err, bd.ln_err, bd.n);
        put_doubles(dst + k.weight, bd.weight, bd.n);
    }
    const double* pd[4] = {spec->lower, spec->upper, spec->prior_a, spec->prior_b};
    for (int q = 0; q < 4; ++q) std::memcpy(hp + lay.prior + 16 * q, pd[q], sizeof spec->lower);
    const int32_t* pi[3] = {spec->slot, spec->is_log, spec->prior_kind};
    for (int q = 0; q < 3; ++q) std::memcpy(hp + lay.prior + 64 + 8 * q, pi[q], sizeof spec->slot);
}

// ---- centroid groups (vag_loglike_sky_batch) and polarization groups (vag_loglike_pol_batch): one device buffer each, of one shape.
//      Layout in doubles, per group: [nu | six arrays of n] (1 + 6 n) -- [t | east | north | err_east | err_north | weight] of a centroid
//      group, [t | q | u | err_q | err_u | weight] of a polarization group, u and err_u of a DEGREE group zeros. ----
struct SixGroup {  // one such group; a null array is stored as zeros
    double nu;
    int n;
    const double* col[6];
};
struct SixCols { size_t rows, col[6], doubles; };  // rows: the `+ 1` past nu, where the six arrays start (col[0], the times)
static SixCols six_cols(int n, size_t rows = 1) {  // (rows: 1 behind nu; a visibility group's arrays lie behind its epochs' times)
    SixCols k{rows, {}, rows + 6 * (size_t)n};
    for (int q = 0; q < 6; ++q) k.col[q] = rows + (size_t)q * n;
    return k;
}
static void six_put(const double* const col[6], size_t n, const SixCols& k, double* dst) {  // n doubles of each array, zeros for a null one
    for (int q = 0; q < 6; ++q) {
        if (col[q])
            put_doubles(dst + k.col[q], col[q], n);
        else
            std::memset(dst + k.col[q], 0, sizeof(double) * n);
    }
}
static SixGroup six_group(const vag_centroid_obs& o) { return {o.nu, o.n, {o.t, o.east, o.north, o.err_east, o.err_north, o.weight}}; }
static SixGroup six_group(const vag_polarization_obs& o) {
    const bool qu = o.kind == VAG_POL_QU;
    return {o.nu, o.n, {o.t, o.q, qu ? o.u : nullptr, o.err_q, qu ? o.err_u : nullptr, o.weight}};
}

struct SixLayout : BlockKey { std::vector<size_t> off; };  // off: where group g starts in the block
using SkyLayout = SixLayout;
using PolLayout = SixLayout;

static void six_begin(SixLayout& lay, int n_groups) { lay = {}, lay.hash = fnv1a(FNV_SEED, &n_groups, sizeof n_groups); }
// hash and place of the next group: nu, its shape integers, the arrays it has
static void six_push(SixLayout& lay, const SixGroup& g, const int* head, size_t n_head) {
    lay.hash = fnv1a(fnv1a(lay.hash, &g.nu, sizeof g.nu), head, sizeof(int) * n_head);
    for (const double* arr : g.col)
        if (arr) lay.hash = fnv1a(lay.hash, arr, sizeof(double) * g.n);
    lay.off.push_back(lay.doubles);
    lay.doubles += six_cols(g.n).doubles;
}
template <class Spec>
static void six_fill(const Spec* s, const SixLayout& lay, double* hp) {
    for (int g = 0; g < s->n_groups; ++g) {
        const SixGroup o = six_group(s->groups[g]);
        hp[lay.off[g]] = o.nu;
        six_put(o.col, o.n, six_cols(o.n), hp + lay.off[g]);
    }
}

static int sky_scan(const vag_sky_fit_spec* sky, SkyLayout& lay) {
    if (sky->n_groups < 0 || (sky->n_groups > 0 && !sky->groups)) return set_err(VAG_E_INVALID, "bad centroid group list");
    for (double v : {sky->pa_fixed, sky->east0_fixed, sky->north0_fixed})
        if (!std::isfinite(v)) return set_err(VAG_E_INVALID, "fixed sky placement values must be finite");
    six_begin(lay, sky->n_groups);
    for (int g = 0; g < sky->n_groups; ++g) {
        const vag_centroid_obs& o = sky->groups[g];
        if (o.n <= 0) return set_err(VAG_E_INVALID, "centroid group %d has no observations", g);
        if (!o.t || !o.east || !o.north || !o.err_east || !o.err_north || !o.weight) return set_err(VAG_E_INVALID, "centroid group %d: null array", g);
        six_push(lay, six_group(o), &o.n, 1);
    }
    return VAG_OK;
}

static int sky_rows(const vag_sky_fit_spec* sky) {
    for (int g = 0; g < sky->n_groups; ++g) {
        const vag_centroid_obs& o = sky->groups[g];
        if (!(o.nu > 0) || !std::isfinite(o.nu)) return set_err(VAG_E_INVALID, "centroid group %d: frequency must be positive", g);
        for (int i = 0; i < o.n; ++i) {
            if (!(o.t[i] > 0) || !std::isfinite(o.t[i]) || (i > 0 && o.t[i] < o.t[i - 1]))
                return set_err(VAG_E_INVALID, "centroid group %d: times must be positive and ascending", g);
            if (!std::isfinite(o.east[i]) || !std::isfinite(o.north[i]) || !std::isfinite(o.weight[i]))
                return set_err(VAG_E_INVALID, "centroid group %d: positions and weights must be finite", g);
            if (!(o.err_east[i] > 0) || !(o.err_north[i] > 0) || !std::isfinite(o.err_east[i]) || !std::isfinite(o.err_north[i]))
                return set_err(VAG_E_INVALID, "centroid group %d: errors must be positive and finite", g);
        }
    }
    return VAG_OK;
}

static int pol_scan(const vag_pol_fit_spec* pol, PolLayout& lay) {
    if (pol->n_groups < 0 || !pol->groups) return set_err(VAG_E_INVALID, "bad polarization group list");
    if (pol->n_groups > VAG_POL_MAX_GROUPS) return set_err(VAG_E_INVALID, "at most %d polarization groups", VAG_POL_MAX_GROUPS);
    for (int e = 0; e < 2; ++e)
        if (std::isnan(pol->b_fixed[e]) || std::isnan(pol->pi_max_fixed[e]))
            return set_err(VAG_E_INVALID, "fixed polarization values must not be NaN");
    six_begin(lay, pol->n_groups);
    for (int g = 0; g < pol->n_groups; ++g) {
        const vag_polarization_obs& o = pol->groups[g];
        if (o.n < 1) return set_err(VAG_E_INVALID, "polarization group %d has no observations", g);
        if (o.n > VAG_VIS_MAX_EPOCHS) return set_err(VAG_E_INVALID, "polarization group %d: at most %d epochs", g, VAG_VIS_MAX_EPOCHS);
        if (o.kind != VAG_POL_QU && o.kind != VAG_POL_DEGREE) return set_err(VAG_E_INVALID, "polarization group %d: unknown kind %d", g, o.kind);
        if (!o.t || !o.q || !o.err_q || !o.weight || (o.kind == VAG_POL_QU && (!o.u || !o.err_u)))
            return set_err(VAG_E_INVALID, "polarization group %d: null array", g);
        const int head[3] = {o.n, o.n_az > 0 ? o.n_az : 256, o.kind};
        six_push(lay, six_group(o), head, 3);
    }
    return VAG_OK;
}

static int pol_rows(const vag_pol_fit_spec* pol) {
    for (int g = 0; g < pol->n_groups; ++g) {
        const vag_polarization_obs& o = pol->groups[g];
        const bool qu = o.kind == VAG_POL_QU;
        if (!(o.nu > 0) || !std::isfinite(o.nu)) return set_err(VAG_E_INVALID, "polarization group %d: frequency must be positive", g);
        for (int i = 0; i < o.n; ++i) {
            if (!(o.t[i] > 0) || !std::isfinite(o.t[i]) || (i > 0 && o.t[i] < o.t[i - 1]))
                return set_err(VAG_E_INVALID, "polarization group %d: times must be positive and ascending", g);
            if (!std::isfinite(o.q[i]) || (qu && !std::isfinite(o.u[i])) || !std::isfinite(o.weight[i]) || o.weight[i] < 0)
                return set_err(VAG_E_INVALID, "polarization group %d: measurements must be finite, weights finite and >= 0", g);
            if (!(o.err_q[i] > 0) || !std::isfinite(o.err_q[i]) || (qu && (!(o.err_u[i] > 0) || !std::isfinite(o.err_u[i]))))
                return set_err(VAG_E_INVALID, "polarization group %d: errors must be positive and finite", g);
        }
    }
    return VAG_OK;
}

// ---- visibility groups (vag_loglike_vis_batch): one device buffer.  Layout in doubles, per group: [nu | t | u | v | re | im | err |
//      weight] (1 + n_epochs + 6 n_vis), im of an AMPLITUDE group zeros; beside it, per group, the blocks of at most 64 visibilities of
//      one epoch as int32 [epoch, first visibility, visibilities] (d_visblk). ----
struct VisCols { size_t t, six, doubles; };  // t: the `+ 1` past nu; six: where [u | v | re | im | err | weight] (n_vis each) start
static VisCols vis_cols(const vag_visibility_obs& o) {
    const size_t six = 1 + (size_t)o.n_epochs;
    return {1, six, six_cols(o.n_vis, six).doubles};
}

struct VisLayout {               // of one group; made on a miss, from the validated first[]
    size_t obs_off;              // its data in the vis block [doubles]
    int blk_off;                 // its blocks in d_visblk [blocks of 3 ints]
    std::vector<int> epoch_blk;  // [n_epochs + 1]: first block of every epoch
};

static int vis_scan(const vag_vis_fit_spec* vis, BlockKey& key) {
    if (vis->n_groups < 0 || !vis->groups) return set_err(VAG_E_INVALID, "bad visibility group list");
    if (vis->n_groups > VAG_VIS_MAX_GROUPS) return set_err(VAG_E_INVALID, "at most %d visibility groups", VAG_VIS_MAX_GROUPS);
    key = {fnv1a(FNV_SEED, &vis->n_groups, sizeof vis->n_groups), 0};
    uint64_t& h = key.hash;
    for (int g = 0; g < vis->n_groups; ++g) {
        const vag_visibility_obs& o = vis->groups[g];
        if (o.n_epochs < 1 || o.n_vis < 1) return set_err(VAG_E_INVALID, "visibility group %d has no observations", g);
        if (o.n_epochs > VAG_VIS_MAX_EPOCHS) return set_err(VAG_E_INVALID, "visibility group %d: at most %d epochs", g, VAG_VIS_MAX_EPOCHS);
        if (o.kind != VAG_VIS_COMPLEX && o.kind != VAG_VIS_AMPLITUDE) return set_err(VAG_E_INVALID, "visibility group %d: unknown kind %d", g, o.kind);
        if (!o.t || !o.first || !o.u || !o.v || !o.re || !o.err || !o.weight || (o.kind == VAG_VIS_COMPLEX && !o.im))
            return set_err(VAG_E_INVALID, "visibility group %d: null array", g);
        const int head[4] = {o.n_epochs, o.n_vis, o.n_az > 0 ? o.n_az : 1024, o.kind};
        h = fnv1a(h, &o.nu, sizeof o.nu);
        h = fnv1a(h, head, sizeof head);
        h = fnv1a(h, o.t, sizeof(double) * o.n_epochs);
        h = fnv1a(h, o.first, sizeof(int32_t) * ((size_t)o.n_epochs + 1));
        for (const double* arr : {o.u, o.v, o.re, o.kind == VAG_VIS_COMPLEX ? o.im : nullptr, o.err, o.weight})
            if (arr) h = fnv1a(h, arr, sizeof(double) * o.n_vis);
        key.doubles += vis_cols(o).doubles;
    }
    return VAG_OK;
}

// Validates the groups' rows; lays the groups out in layout and cuts their epochs into blocks.
static int vis_rows(const vag_vis_fit_spec* vis, std::vector<VisLayout>& layout, std::vector<int>& blocks) {
    layout.assign(vis->n_groups, VisLayout{});
    blocks.clear();
    size_t off = 0;
    for (int g = 0; g < vis->n_groups; ++g) {
        const vag_visibility_obs& o = vis->groups[g];
        if (!(o.nu > 0) || !std::isfinite(o.nu)) return set_err(VAG_E_INVALID, "visibility group %d: frequency must be positive", g);
        if (o.first[0] != 0 || o.first[o.n_epochs] != o.n_vis)
            return set_err(VAG_E_INVALID, "visibility group %d: first[0] must be 0 and first[n_epochs] n_vis", g);
        VisLayout& lay = layout[g];
        lay.obs_off = off;
        lay.blk_off = (int)(blocks.size() / 3);
        off += vis_cols(o).doubles;
        for (int e = 0; e < o.n_epochs; ++e) {
            if (!(o.t[e] > 0) || !std::isfinite(o.t[e]) || (e > 0 && !(o.t[e] > o.t[e - 1])))
                return set_err(VAG_E_INVALID, "visibility group %d: times must be positive and strictly ascending", g);
            const int k0 = o.first[e], k1 = o.first[e + 1];
            if (k0 < 0 || k1 > o.n_vis || k1 <= k0) return set_err(VAG_E_INVALID, "visibility group %d: epoch %d is empty or first[] is not ascending", g, e);
            if (k1 - k0 > VAG_VIS_MAX_PER_EPOCH)
                return set_err(VAG_E_INVALID, "visibility group %d: at most %d visibilities per epoch", g, VAG_VIS_MAX_PER_EPOCH);
            lay.epoch_blk.push_back((int)(blocks.size() / 3) - lay.blk_off);
            for (int k = k0; k < k1; k += 64) blocks.insert(blocks.end(), {e, k, std::min(64, k1 - k)});
        }
        lay.epoch_blk.push_back((int)(blocks.size() / 3) - lay.blk_off);
        for (int k = 0; k < o.n_vis; ++k) {
            if (!std::isfinite(o.u[k]) || !std::isfinite(o.v[k]) || !std::isfinite(o.re[k]) || (o.kind == VAG_VIS_COMPLEX && !std::isfinite(o.im[k])))
                return set_err(VAG_E_INVALID, "visibility group %d: baselines and visibilities must be finite", g);
            if (!(o.err[k] > 0) || !std::isfinite(o.err[k])) return set_err(VAG_E_INVALID, "visibility group %d: errors must be positive and finite", g);
            if (!(o.weight[k] >= 0) || !std::isfinite(o.weight[k])) return set_err(VAG_E_INVALID, "visibility group %d: weights must be finite and >= 0", g);
        }
    }
    return VAG_OK;
}

static void vis_fill(const vag_vis_fit_spec* vis, const std::vector<VisLayout>& layout, double* hp) {
    for (int g = 0; g < vis->n_groups; ++g) {
        const vag_visibility_obs& o = vis->groups[g];
        const double* col[6] = {o.u, o.v, o.re, o.kind == VAG_VIS_COMPLEX ? o.im : nullptr, o.err, o.weight};
        const VisCols k = vis_cols(o);
        double* dst = hp + layout[g].obs_off;
        dst[0] = o.nu;
        put_doubles(dst + k.t, o.t, o.n_epochs);
        six_put(col, o.n_vis, six_cols(o.n_vis, k.six), dst);
    }
}

// ---- one likelihood request.  Every vag_loglike_*_batch entry point fills a FitRequest from its arguments (a spec it does not take
//      stays null) and calls loglike_dev or loglike_host; a request whose optional blocks are null or empty is therefore the narrower
//      entry point's request, statement for statement. ----
namespace {
struct FitRequest {
    const vag_fit_spec* spec = nullptr;
    const vag_sky_fit_spec* sky = nullptr;      // after fit_request_prepare: null when nothing reads the placement
    const vag_vis_fit_spec* vis = nullptr;      // after fit_request_prepare: null when it has no group; so pol, counts, index, fold
    const vag_pol_fit_spec* pol = nullptr;
    const vag_limit_fit_spec* lim = nullptr;    // after fit_request_prepare: null when no row is a limit (llay.any)
    const vag_noise_fit_spec* noise = nullptr;  // after fit_request_prepare: null when no row is grouped (nlay.any)
    const vag_counts_fit_spec* counts = nullptr;
    const vag_index_fit_spec* index = nullptr;
    const vag_fold_fit_spec* fold = nullptr;
    const vag_template_fit_spec* tmpl = nullptr;  // after fit_request_prepare: null when no row is touched (tlay.any)
    const vag_cov_fit_spec* cov = nullptr;        // after fit_request_prepare: null when it has no group
    const vag_robust_fit_spec* robust = nullptr;  // after fit_request_prepare: null when no detection row lies in a robust group (rlay.any)
    int ndim = 0;                                 // of the call: fit_scan holds the spec's against it
    FitLayout fit;                                // the four blocks hashed in place (fit, sky, vis, pol): scanned in the upload sequence
    SkyLayout slay;
    BlockKey vkey;
    PolLayout play;
    std::vector<VisLayout> vis_groups;  // what vis_rows made on a miss, with vis_blocks: the context keeps them beside the block
    std::vector<int> vis_blocks;
    LimLayout llay;
    NoiseLayout nlay;
    CountsLayout clay;
    IndexLayout ilay;
    FoldLayout flay;
    TmplLayout tlay;
    CovLayout vlay;
    RobustLayout rlay;
    std::vector<double> lstage, nstage, cstage, istage, fstage, tstage, vstage, rstage;  // what the scans lay out: one resident block each
    bool placed = false;                                 // some group reads east0 / north0
    bool prepared = false;                               // fit_request_prepare has run
};
}  // namespace

// Normalises the request and scans its host-side blocks, once per call (host work only: no context is touched).  spec is not null.
static int fit_request_prepare(FitRequest& r) {
    if (r.prepared) return VAG_OK;
    if (r.vis && r.vis->n_groups == 0) r.vis = nullptr;
    if (r.counts && r.counts->n_groups == 0) r.counts = nullptr;
    if (r.index && r.index->n_groups == 0) r.index = nullptr;
    if (r.fold && r.fold->n_groups == 0) r.fold = nullptr;
    if (r.cov && r.cov->n_groups == 0) r.cov = nullptr;
    int rc = VAG_OK;
    if (r.cov && (rc = cov_scan(r.cov, r.vstage, r.vlay))) return rc;
    if (r.tmpl && (rc = tmpl_scan(r.spec, r.tmpl, r.tstage, r.tlay))) return rc;
    if (r.fold && (rc = fold_scan(r.spec, r.fold, r.fstage, r.flay))) return rc;
    if (r.index && (rc = index_scan(r.index, r.istage, r.ilay))) return rc;
    if (r.counts && (rc = counts_scan(r.counts, r.cstage, r.clay))) return rc;
    if (r.noise && (rc = noise_scan(r.spec, r.noise, r.nstage, r.nlay))) return rc;
    if (r.lim && (rc = lim_scan(r.spec, r.pol, r.lim, r.lstage, r.llay))) return rc;  // (pol as given: an empty list checks n_pol_groups)
    if (r.robust && (rc = robust_scan(r.spec, r.noise, r.lim, r.robust, r.rstage, r.rlay))) return rc;  // (noise and lim as given, and accepted)
    if (!r.rlay.any) r.robust = nullptr;  // (rlay.mask stays: the outlier slots of the spec's robust groups are accepted)
    if (!r.nlay.any) r.noise = nullptr;
    if (!r.llay.any) r.lim = nullptr;
    if (!r.tlay.any) r.tmpl = nullptr;  // (tlay.n_templates stays: the amplitude slots of the spec's templates are accepted)
    if (r.pol && r.pol->n_groups == 0) r.pol = nullptr;
    r.placed = (r.sky && r.sky->n_groups > 0) || r.vis;
    // (east0 / north0 place centroid and visibility groups only: without such a group they are refused as free parameters)
    if (!r.pol && !r.placed) r.sky = nullptr;  // nothing reads the placement
    r.prepared = true;
    return VAG_OK;
}

// The passes of a prepared request, in the order they run: the point rows, then every group of each list.  Each adds one chi^2 term
// per walker; position 0 is the call's first pass (FitPass::first), the final position its last, which writes the call's output.
enum class PassKind { Point, Band, Centroid, Vis, Pol, Counts, Index, Fold, Cov };
struct PassItem { PassKind kind; int group; };
static std::vector<PassItem> fit_pass_list(const FitRequest& r) {
    std::vector<PassItem> list;
    if (r.spec->n_data > 0) list.push_back({PassKind::Point, 0});
    const struct { PassKind kind; int n; } lists[8] = {
        {PassKind::Band, r.spec->n_bands},   {PassKind::Centroid, r.sky ? r.sky->n_groups : 0}, {PassKind::Vis, r.vis ? r.vis->n_groups : 0},
        {PassKind::Pol, r.pol ? r.pol->n_groups : 0}, {PassKind::Counts, r.counts ? r.counts->n_groups : 0},
        {PassKind::Index, r.index ? r.index->n_groups : 0}, {PassKind::Fold, r.fold ? r.fold->n_groups : 0},
        {PassKind::Cov, r.cov ? r.cov->n_groups : 0}};
    for (const auto& l : lists)
        for (int g = 0; g < l.n; ++g) list.push_back({l.kind, g});
    return list;
}

// The frequencies of the np points of an index or fold group on the host (point i at nu[i % K], as its scan lays them out), for the
// shared-node test of a short series: written to nu_pts [max_points] and handed back, or null for a series above max_points.
static const double* short_series_nu(const double* nu, size_t K, size_t np, size_t max_points, double* nu_pts) {
    if (np > max_points) return nullptr;
    for (size_t i = 0; i < np; ++i) nu_pts[i] = nu[i % K];
    return nu_pts;
}

static FitAccepts fit_accepts(const FitRequest& r) {
    return {r.placed, r.pol != nullptr, r.fold && r.flay.any_sigma, r.counts || r.index || r.fold || r.cov,
            r.noise ? r.nlay.n_groups : 0, r.tlay.n_templates, r.noise ? r.rlay.mask : 0u};
}

static FitRequest fit_request(const vag_fit_spec* spec, const vag_sky_fit_spec* sky = nullptr, const vag_vis_fit_spec* vis = nullptr,
                              const vag_pol_fit_spec* pol = nullptr, const vag_limit_fit_spec* lim = nullptr, const vag_noise_fit_spec* noise = nullptr,
                              const vag_counts_fit_spec* counts = nullptr, const vag_index_fit_spec* index = nullptr,
                              const vag_fold_fit_spec* fold = nullptr, const vag_template_fit_spec* tmpl = nullptr, const vag_cov_fit_spec* cov = nullptr,
                              const vag_robust_fit_spec* robust = nullptr) {
    return FitRequest{spec, sky, vis, pol, lim, noise, counts, index, fold, tmpl, cov, robust};
}
