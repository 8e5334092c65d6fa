"""CPU test of the two forms of sp_fast (vag_device.h) against each other, compiled for the host (VAG_HOST_DEBUG) the way
tests/test_sp_pair_host.py builds the evaluator.

The RELU_FIRST form, which the split flux kernel's boundary team uses, holds r = max(z, 0) for every lane ahead of the table side.
Both forms end that side in fma(0.5, z + |z|, p).  Ending the RELU_FIRST form in r + p, an instruction fewer, was measured and not
kept for its time (profiles/flux_boundary_ab.txt, part 4); it has the same bits -- for |z| <= 20, z + |z| is exactly 2 z or +0, half
of it is exact, and the FMA rounds z + p (or 0 + p) once, as the add does -- and this test held it to the plain form.  It stays as
the check of the two forms, whichever way the table side ends: the same bits for every z, and a NaN both ways.  Points: a grid of
step 2^-14 over [-21, 21] (the table side and both shortcuts), the same grid moved off the dyadic points by an irrational fraction of
a step, 200 000 doubles drawn log-uniformly in magnitude from 1e-320 (subnormal) to 21 with both signs, +-0, +-20 and the doubles
next to them, +-1e-300, the subnormal ends, +-inf and NaN."""
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
#include <limits>
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

int main() {
    const std::vector<double> tab = softplus_table();
    const double* sp = tab.data();
    long n = 0, n_table = 0, n_hi = 0, n_lo = 0, n_nan = 0, bad = 0, nan_bad = 0;
    auto point = [&](double z) {
        const double plain = sp_fast(z, sp), relu = sp_fast<true>(z, sp);
        ++n;
        if (std::isnan(z)) {
            ++n_nan;
            if (!(std::isnan(plain) && std::isnan(relu))) ++nan_bad;
            return;
        }
        if (z > 20) ++n_hi; else if (z < -20) ++n_lo; else ++n_table;
        if (std::memcmp(&plain, &relu, sizeof plain) != 0) {
            if (++bad <= 10) printf("differs at z = %a: plain %a relu-first %a\n", z, plain, relu);
        }
    };
    const double step = 1.0 / 16384;
    for (long i = -21 * 16384; i <= 21 * 16384; ++i) {
        point((double)i * step);
        point(((double)i + 0.41421356237309503) * step);  // off the dyadic points: full mantissas
    }
    std::uint64_t s = 0x9E3779B97F4A7C15ull;  // log-uniform magnitudes, both signs (splitmix64)
    auto next = [&]() {
        std::uint64_t x = (s += 0x9E3779B97F4A7C15ull);
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull, x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return (double)((x ^ (x >> 31)) >> 11) / 9007199254740992.0;
    };
    const double l_lo = std::log(1e-320), l_hi = std::log(21.0);
    for (int i = 0; i < 200000; ++i) {
        const double m = std::exp(l_lo + (l_hi - l_lo) * next());
        point(next() < 0.5 ? m : -m);
    }
    const double inf = std::numeric_limits<double>::infinity(), tiny = std::numeric_limits<double>::denorm_min();
    for (double e : {20.0, -20.0, 0.0, -0.0}) point(e), point(std::nextafter(e, inf)), point(std::nextafter(e, -inf));
    for (double e : {1e-300, tiny, std::numeric_limits<double>::min()}) point(e), point(-e);
    point(inf), point(-inf), point(std::nan("")), point(-std::nan(""));
    printf("points %ld table %ld above %ld below %ld nan %ld bad %ld nan_bad %ld\n", n, n_table, n_hi, n_lo, n_nan, bad, nan_bad);
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the host build of the device math needs it")
    d = tmp_path_factory.mktemp("sp_relu_add_host")
    src, exe = d / "t.cpp", d / "t"
    src.write_text('#define VAG_HOST_DEBUG 1\n' + SRC)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "vegasafterglow_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    w = out.strip().split("\n")[-1].split()
    assert w[0] == "points", out
    return {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}, out


def test_both_forms_give_the_same_bits(report):
    rep, out = report
    assert rep["table"] > 1500000 and rep["above"] > 10000 and rep["below"] > 10000, rep
    assert rep["bad"] == 0, out


def test_nan_stays_nan_in_both_forms(report):
    rep, out = report
    assert rep["nan"] >= 2 and rep["nan_bad"] == 0, out
