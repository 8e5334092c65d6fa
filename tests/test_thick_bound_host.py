"""CPU test of the evaluator's thick-term bound (log2_I_nu_fast<true>, vag_device.h), compiled for the host (VAG_HOST_DEBUG):
with the switch on, the optically thick branch's softplus term is left out where SAB (thin - th) < -20 and SAB > 0, th being the
branch without that term.  The result must have the bits of the switch-off evaluation everywhere.

Cells come from syn_photons_build over a sweep of electron Lorentz factors and fields (slow and fast cooling, absorption break
below, between and above the others); frequencies run from 2^-36 to 2^9 times each cell's nu_m, the scale of the far cut, in
steps of 2^1.25.  The program classes every point with the evaluator's own expressions: beyond log2_x_far (no thick term
in either form), skipped by the bound, thick term computed.  Each class must hold >= 5 % of the points, so that equality is not
vacuous.  Added to the sweep: for every cell the frequencies where SAB (thin - th) lies within +-1 of -20, on both sides of the
threshold (above it the full path, below it the skip: the comparison is `< -20`), and NaN inputs (a NaN frequency, a NaN thick
norm), whose comparison is false: they must be classed as the full path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not os.path.exists(HIPCC):
    HIPCC = shutil.which("hipcc") or HIPCC

SRC = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
using std::isfinite;  // syn_freq's unqualified call, on the host
__host__ inline int __double2loint(double x) {  // host overload of the device intrinsic sp_fast reads its node index with
    std::uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return (int)(std::uint32_t)b;
}
#include "vag_device.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vag;

// sp_fast's table (vag_capi.hip: build_softplus_table): degree-5 interpolants of log2(1 + 2^-a) at Chebyshev nodes per interval
static std::vector<double> softplus_table() {
    const int n = SP_NCOEF;
    const long double PI = 3.141592653589793238462643383279502884L;
    std::vector<double> tab((size_t)SP_INTERVALS * n, 0.0);
    long double T[SP_NCOEF][SP_NCOEF] = {};
    T[0][0] = 1, T[1][1] = 1;
    for (int k = 2; k < n; ++k)
        for (int q = 0; q < n; ++q) T[k][q] = (q > 0 ? 2 * T[k - 1][q - 1] : 0) - T[k - 2][q];
    for (int i = 0; i < SP_INTERVALS; ++i) {
        const long double ac = (long double)i / SP_PER_UNIT, h = 1.0L / SP_PER_UNIT;
        long double f[SP_NCOEF], c[SP_NCOEF], mono[SP_NCOEF] = {};
        for (int j = 0; j < n; ++j) f[j] = log2l(1 + exp2l(-(ac + h / 2 * cosl(PI * (2 * j + 1) / (2 * n)))));
        for (int k = 0; k < n; ++k) {
            long double s = 0;
            for (int j = 0; j < n; ++j) s += f[j] * cosl(k * PI * (2 * j + 1) / (2 * n));
            c[k] = (k ? 2 : 1) * s / n;
        }
        for (int k = 0; k < n; ++k)
            for (int q = 0; q < n; ++q) mono[q] += c[k] * T[k][q];
        long double sc = 1;
        for (int q = 0; q < n; ++q, sc *= 2) tab[(size_t)i * n + q] = (double)(mono[q] * sc);
    }
    return tab;
}

static std::vector<double> g_tab;
static long n_far, n_skip, n_full, n_bad, near_above, near_below, nan_full, nan_other;

// SAB (thin - th) and the far cut with log2_I_nu_fast's expressions
static double blend_arg(const double* c, double x) {
    const double* sp = g_tab.data();
    const double l_lo = c[VP_LG2_LO];
    const double thin = (x - l_lo) * (1.0 / 3.0) - sp_fast(c[VP_DLO] * (x - l_lo), sp) * c[VP_INV_SLO] -
                        sp_fast(fma(c[VP_DHI], x, c[VP_BHI]), sp) * c[VP_INV_SHI];
    return c[VP_SAB] * (thin - fma(2.5, x, c[VP_TB]));
}
enum { FAR, SKIP, FULL };
static int point(const double* c, const SpecConst& sc, double x) {
    const double off = log2_I_nu_fast(c, 1, sc, x, g_tab.data()), on = log2_I_nu_fast<true>(c, 1, sc, x, g_tab.data());
    if (std::memcmp(&off, &on, sizeof off) != 0 && !(std::isnan(off) && std::isnan(on))) ++n_bad;
    if (x - c[VP_LG2_NUM] > sc.log2_x_far) return ++n_far, FAR;
    if (blend_arg(c, x) < -20.0 && c[VP_SAB] > 0) return ++n_skip, SKIP;
    return ++n_full, FULL;
}

int main() {
    g_tab = softplus_table();
    long cells = 0;
    for (double p : {2.05, 2.3, 2.9})
        for (double B = 1e-4; B < 30; B *= 7)
            for (double gm = 3; gm < 3e5; gm *= 6)
                for (double gc = 10; gc < 1e8; gc *= 20)
                    for (double ga = 2; ga < 2e4; ga *= 5) {
                        CellOut o;
                        syn_photons_build(o, gm, gc, ga, 1e8, 1e20, 1e50, B, p, 10.0, 1e17, 1e5);
                        SpecConst sc;
                        sc.init(p);
                        ++cells;
                        for (double dx = -36; dx <= 9; dx += 1.25) point(o.par, sc, o.par[VP_LG2_NUM] + dx);
                        // the frequency where SAB (thin - th) crosses -20 (it falls with frequency: slopes <= 1/3 against 2.5)
                        double lo = o.par[VP_LG2_NUM] - 60, hi = sc.log2_x_far + o.par[VP_LG2_NUM];
                        const bool crosses = blend_arg(o.par, lo) > -20.0 && blend_arg(o.par, hi) < -20.0;  // else: beyond the far cut
                        for (int it = 0; crosses && it < 60; ++it) {
                            const double mid = 0.5 * (lo + hi);
                            (blend_arg(o.par, mid) < -20.0 ? hi : lo) = mid;
                        }
                        for (double d = -0.4; crosses && d <= 0.4; d += 0.05) {
                            const double x = lo + d, v = blend_arg(o.par, x);
                            if (!(std::fabs(v + 20.0) <= 1.0)) continue;
                            const int cls = point(o.par, sc, x);
                            if (v < -20.0) near_below += cls == SKIP || cls == FAR;
                            else near_above += cls == FULL;
                        }
                        // NaN: the comparison is false, the full path runs
                        (point(o.par, sc, std::nan("")) == FULL ? nan_full : nan_other)++;
                        CellOut q = o;
                        q.par[VP_TB] = std::nan("");
                        (point(q.par, sc, o.par[VP_LG2_NUM] - 1.0) == FULL ? nan_full : nan_other)++;
                    }
    printf("thick %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", cells, n_far + n_skip + n_full, n_far, n_skip, n_full, n_bad, near_above, near_below,
           nan_full, nan_other);
}
"""


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the host build of the device math needs it")
    d = tmp_path_factory.mktemp("thick_bound_host")
    src, exe = d / "t.cpp", d / "t"
    src.write_text('#define VAG_HOST_DEBUG 1\n' + SRC)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "vegasafterglow_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    names = "cells points far skip full bad near_above near_below nan_full nan_other".split()
    line = [l for l in out.split("\n") if l.startswith("thick ")][0]
    return dict(zip(names, map(int, line.split()[1:])))


def test_bound_on_gives_the_bits_of_bound_off(counts):
    assert counts["points"] > 100000
    assert counts["bad"] == 0, counts


def test_every_class_is_exercised(counts):
    for k in ("far", "skip", "full"):
        assert counts[k] >= 0.05 * counts["points"], counts


def test_threshold_and_nan_points(counts):
    assert counts["near_above"] > 1000 and counts["near_below"] > 1000, counts
    assert counts["nan_full"] == 2 * counts["cells"] and counts["nan_other"] == 0, counts
