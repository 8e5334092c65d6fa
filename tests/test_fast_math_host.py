"""CPU tests of two pieces of the device math, compiled for the host (VAG_HOST_DEBUG) with hipcc:

1. exp2_or_zero, the interpolation's exp2 with the non-finite select folded into one clamp, against exp2 on a dense sweep of its
   whole finite range (<= 2.5e-16 relative), and its saturation: 0 for NaN / -inf / very negative x, inf for x >= 1024;
2. the boundary-spectrum evaluator on the folded cell block (vag_common.h: VP_BHI, VP_TB, VP_LG2_I_SLO) against the formula on the
   unfolded members it replaces, over the argument ranges the cells produce."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not os.path.exists(HIPCC):
    HIPCC = shutil.which("hipcc") or HIPCC

SRC = r"""
#include "vag_device.h"
#include <cmath>
#include <cstdio>
#include <random>
using namespace vag;

// the evaluator as it read the unfolded members (log2_nu_hi_, log2_thick_norm_, log2_I_nu_max)
static double unfolded(const double* c, double l_hi, double tnorm, double l_I, const SpecConst& sc, double x) {
    const double l_lo = c[VP_LG2_LO];
    const double thin = (x - l_lo) / 3.0 - log2_softplus(c[VP_DLO] * (x - l_lo)) * c[VP_INV_SLO] -
                        log2_softplus(c[VP_DHI] * (x - l_hi)) * c[VP_INV_SHI];
    const double lx = x - c[VP_LG2_NUM];
    double thick = 2.5 * lx;
    if (!(lx > sc.log2_x_far)) thick += log2_softplus(-0.5 * lx + -sc.smooth_thick * exp2(2. / 3 * lx));
    const double lb = thick + tnorm;
    const double smooth_one = thin - log2_softplus(c[VP_SAB] * (thin - lb)) * c[VP_INV_SAB];
    const double spec = l_I + (c[VP_INV_SLO] + smooth_one);
    if (x - c[VP_LG2_NUMAX] < -20) return spec;
    return spec - c[VP_INV_NUMAX] * exp2(x);
}

int main() {
    double e_worst = 0;
    const long n = 20000000;
    for (long i = 0; i <= n; ++i) {  // every normal result of exp2
        const double x = -1022.0 + i * (2045.99 / n);
        const double r = std::fabs(exp2_or_zero(x) - std::exp2(x)) / std::exp2(x);
        if (r > e_worst) e_worst = r;
    }
    int sat_ok = 1;
    for (double x : {-HUGE_VAL, std::nan(""), -2000.0, -1100.0, -1075.5}) sat_ok &= exp2_or_zero(x) == 0.0;
    for (double x : {1024.0, 1100.0, 2000.0}) sat_ok &= std::isinf(exp2_or_zero(x)) && exp2_or_zero(x) > 0;
    printf("exp2 %.6g %d\n", e_worst, sat_ok);

    std::mt19937_64 rng(7);
    auto u = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    double s_worst = 0;
    long evals = 0;
    for (int cell = 0; cell < 20000; ++cell) {
        SpecConst sc;
        sc.init(u(1.8, 3.2));
        double c[VAG_NPAR] = {};
        const double l_m = u(20, 60), l_c = u(20, 70), l_a = u(10, 50);
        const double l_lo = std::fmin(l_m, l_c), l_hi = std::fmax(l_m, l_c), l_I = u(-120, 10), tnorm = u(-40, 40);
        const double smooth_lo = u(0.3, 3), smooth_hi = u(0.3, 3);
        c[VP_LG2_LO] = l_lo;
        c[VP_DLO] = smooth_lo * u(0.1, 1.5);
        c[VP_DHI] = smooth_hi * u(0.1, 1.8);
        c[VP_INV_SLO] = 1.0 / smooth_lo;
        c[VP_INV_SHI] = 1.0 / smooth_hi;
        c[VP_LG2_NUM] = l_m;
        c[VP_SAB] = u(0.5, 2);
        c[VP_INV_SAB] = 1.0 / c[VP_SAB];
        c[VP_LG2_NUMAX] = u(40, 90);
        c[VP_INV_NUMAX] = LOG2E / exp2(c[VP_LG2_NUMAX]);
        // the folds of syn_photons_build
        c[VP_BHI] = -(c[VP_DHI] * l_hi);
        c[VP_TB] = tnorm - 2.5 * l_m;
        c[VP_LG2_I_SLO] = l_I + c[VP_INV_SLO];
        (void)l_a;
        for (int k = 0; k < 50; ++k) {
            const double x = u(20, 100);
            const double a = log2_I_nu(c, 1, sc, x), b = unfolded(c, l_hi, tnorm, l_I, sc, x);
            // log2 units, against the value's own size: a spectrum thousands of octaves down carries an absolute error of its ulp
            const double d = std::fabs(a - b) / std::fmax(1.0, std::fabs(b));
            if (std::isfinite(b) && d > s_worst) s_worst = d;
            ++evals;
        }
    }
    printf("spec %.6g %ld\n", s_worst, evals);
}
"""


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the host build of the device math needs it")
    d = tmp_path_factory.mktemp("fast_math_host")
    src, exe = d / "t.cpp", d / "t"
    src.write_text('#define VAG_HOST_DEBUG 1\n' + SRC)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "vegasafterglow_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_exp2_or_zero_matches_exp2_and_saturates_like_it(results):
    worst, sat_ok = float(results["exp2"][0]), int(results["exp2"][1])
    assert worst <= 2.5e-16, worst
    assert sat_ok == 1


def test_folded_cell_block_gives_the_unfolded_spectrum(results):
    worst, evals = float(results["spec"][0]), int(results["spec"][1])
    assert evals == 1000000
    assert worst < 5e-14, worst  # the folded terms (2.5 log2 nu, diff_hi_ log2 nu_hi_) reach ~250: their ulp is 2.8e-14
