// vag_sky_moments.h -- exact flux-weighted moments of one sky term spread uniformly over its azimuthal bin (vag_sky_centroid_kernel,
// DESIGN §4k).  Plain math on doubles: compiled for the host too (VAG_HOST_DEBUG) by the tests.
//
// A term of weight w sits at X = a - b cos phi, Y = c sin phi with phi uniform over its bin [left, left + width].  With phi_m the
// bin midpoint, h = width / 2, s1 = sin h / h and s2 = sin(2h) / (2h):
//   <cos> = cos phi_m s1, <sin> = sin phi_m s1,
//   Var(cos) = A - sin^2 phi_m D,  Var(sin) = A - cos^2 phi_m D,  Cov(sin, cos) = sin phi_m cos phi_m D,
//   A = (1 + s2 - 2 s1^2) / 2 >= 0,  D = s2 - s1^2 <= 0
// (the same as 1/2 (1 - s1^2) +- 1/2 cos 2phi_m D, written so that every variance is a sum of non-negative terms).  A and D
// cancel to O(h^4) and O(h^2) in that form, so below h = 1 they come from their Taylor series.  A mirrored bin puts half of the
// weight at -phi: Ybar = 0, Mxy = 0 and Myy = w c^2 <sin^2>.  This is the n_az -> infinity limit of vag_sky_moments_kernel.
#pragma once
#include "vag_device.h"

namespace vag {

// The azimuthal bin of a row's phi node (the bin whose width enters its solid angle) and its number of parts.
struct SkyBin {
    double left, width;
    int S;
    bool mirrored;
};

// weight, centroid and central second moments (sums, not yet divided by w) of a set of sky points
struct SkyMom {
    double w, x, y, mxx, myy, mxy;
};

// Taylor coefficients of A and D in h^2 (h < 1: the 14th terms are below the last bit)
struct SkySeries {
    static constexpr int N = 14;
    double a[N + 1], d[N + 1];
};
constexpr SkySeries sky_series() {
    SkySeries s{};
    for (int j = 1; j <= SkySeries::N; ++j) {
        double f = 1, p4 = 1;  // (2j + 2)!, 4^j
        for (int k = 2; k <= 2 * j + 2; ++k) f *= k;
        for (int k = 0; k < j; ++k) p4 *= 4;
        const double sg = (j & 1) ? -1.0 : 1.0;
        s.a[j] = sg * p4 * (j - 1) / f;
        s.d[j] = sg * p4 * (2 * j) / f;
    }
    return s;
}

// A(h), D(h) and s1 of the header comment
VAG_DEV void sky_bin_ad(double h, double& A, double& D, double& s1) {
    if (h >= C_PI) {  // the whole circle (on-axis rows): exactly Var(cos) = Var(sin) = 1/2
        s1 = 0.0;
        A = 0.5;
        D = 0.0;
        return;
    }
    if (h < 1.0) {
        // A = sum_{j>=2} (-1)^j 4^j (j - 1) / (2j + 2)! h^2j,  D = sum_{j>=1} (-1)^j 4^j 2j / (2j + 2)! h^2j
        const double x = h * h;
        constexpr SkySeries S = sky_series();
        double a = 0, d = 0;
#pragma unroll
        for (int j = SkySeries::N; j >= 1; --j) {
            a = fma(a, x, S.a[j]);
            d = fma(d, x, S.d[j]);
        }
        A = a * x;  // (the j = 1 coefficient of A is zero)
        D = d * x;
        s1 = (h > 0) ? sin(h) / h : 1.0;
        return;
    }
    s1 = sin(h) / h;
    const double s2 = sin(2 * h) / (2 * h);
    A = 0.5 * (1 + s2 - 2 * s1 * s1);
    D = s2 - s1 * s1;
}

// the moments of one term (w, a, b, c) spread over its bin
VAG_DEV SkyMom sky_term_moments(double w, double a, double b, double c, const SkyBin& bin) {
    const double h = 0.5 * bin.width, pm = bin.left + h;
    double A, D, s1;
    sky_bin_ad(h, A, D, s1);
    double sn, cs;
    sincos(pm, &sn, &cs);
    if (h >= C_PI) sn = 0.0, cs = 0.0;  // (the whole circle: the mean is 0 whatever the midpoint)
    const double var_c = A - (sn * sn) * D, var_s = A - (cs * cs) * D;
    SkyMom m;
    m.w = w;
    m.x = a - b * (cs * s1);
    m.mxx = w * (b * b) * var_c;
    if (bin.mirrored) {
        const double ms = sn * s1;
        m.y = 0.0;
        m.myy = w * (c * c) * (var_s + ms * ms);
        m.mxy = 0.0;
    } else {
        m.y = c * (sn * s1);
        m.myy = w * (c * c) * var_s;
        m.mxy = -w * (b * c) * ((sn * cs) * D);
    }
    return m;
}

// Chan's pairwise update: the moments of the union of two point sets (p first).  Either weight may be zero.
VAG_DEV SkyMom sky_mom_merge(const SkyMom& p, const SkyMom& q) {
    if (!(q.w != 0)) return q.w == q.w ? p : q;  // (a NaN weight stays visible)
    if (p.w == 0) return q;
    SkyMom r;
    r.w = p.w + q.w;
    const double fq = q.w / r.w, pw_fq = p.w * fq;
    const double dx = q.x - p.x, dy = q.y - p.y;
    r.x = fma(dx, fq, p.x);
    r.y = fma(dy, fq, p.y);
    r.mxx = (p.mxx + q.mxx) + (dx * dx) * pw_fq;
    r.myy = (p.myy + q.myy) + (dy * dy) * pw_fq;
    r.mxy = (p.mxy + q.mxy) + (dx * dy) * pw_fq;
    return r;
}

}  // namespace vag
