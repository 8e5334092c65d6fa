"""CPU tests of the count-spectrum groups of the likelihood (vag_loglike_fold_batch, Fitter.add_count_spectrum), and the
pure-numpy statement of the term (fitting.fold_expected) that tests/test_fold.py holds the device to:

0. the ctypes layouts of vag_fold_obs / vag_fold_fit_spec and the new constants against the C header; the new symbols in _lib.EXPORTS
   and in the library built for gfx950; vag_abi_version() stays 13;
1. every boundary error of add_count_spectrum, which leaves the Fitter unchanged;
2. the host arithmetic: nodes, the matrix A, the merged sample times and const2, against their direct formulas;
3. the quadrature: for a power law the folded value over the exact one is x / sinh x;
4. every refusal of the host scan, through both C entry points with no context (the scan runs before the device is touched);
5. the parameter N_H needs a group with absorption, in validate_parameters, build_spec and the C-ABI;
6. a NULL or empty fold spec forwards to vag_loglike_index_batch;
7. sharded likelihood calls refuse a fitter with count spectra."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from vegasafterglow_amd import _lib, fitting, units
from vegasafterglow_amd.fitting import fold_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
P = fitting.ParamDef
THETA_V = P("theta_v", 0.0, 0.8)
H = units._PLANCK_ERG_S


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def bins(J, lo=0.3, hi=10.0):
    e = np.geomspace(lo, hi, J + 1)
    return e[:-1].copy(), e[1:].copy()


def ok_args(J=4, nC=3, n=2, **kw):
    lo, hi = bins(J)
    rng = np.random.default_rng(1)
    a = dict(energy_lo=lo, energy_hi=hi, response=rng.uniform(10.0, 100.0, (nC, J)), t_start=np.array([1e5, 3e5])[:n],
             exposure=np.array([2e4, 5e4])[:n], counts=rng.integers(0, 50, (n, nC)).astype(float))
    a.update(kw)
    return a


# ---------------------------------------------------------------- 0. layout, symbols
LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define O(f) offsetof(vag_fold_obs, f)
#define S(f) offsetof(vag_fold_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_fold_obs), O(J), O(C), O(n), O(m), O(n_samples),
           O(pad), O(nu), O(A), O(sigma), O(t_sample), O(sample_idx), O(exposure_over_m), O(counts), O(background), O(weight));
    printf("%zu %zu %zu %zu %zu\n", sizeof(vag_fold_fit_spec), S(n_groups), S(pad), S(groups), S(n_h_fixed));
    printf("%d %d %d %d %d\n", VAG_ABI_VERSION, VAG_P_N_H, VAG_FOLD_MAX_BINS, VAG_FOLD_MAX_CHANNELS, VAG_P_NOISE_SYS0 + VAG_NOISE_MAX_GROUPS);
    return 0;
}
"""


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "c.c", tmp_path / "c"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    O = _lib.FoldObs
    assert [int(x) for x in lines[0].split()] == [C.sizeof(O)] + [getattr(O, n).offset for n in (
        "J", "C", "n", "m", "n_samples", "pad", "nu", "A", "sigma", "t_sample", "sample_idx", "exposure_over_m", "counts", "background",
        "weight")]
    S = _lib.FoldFitSpec
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S), S.n_groups.offset, S.pad.offset, S.groups.offset, S.n_h_fixed.offset]
    assert [int(x) for x in lines[2].split()] == [13, _lib.P_N_H, _lib.FOLD_MAX_BINS, _lib.FOLD_MAX_CHANNELS, _lib.P_N_H]
    assert _lib.P_N_H == 1016 and (_lib.FOLD_MAX_BINS, _lib.FOLD_MAX_CHANNELS) == (64, 256)  # the slot behind the last noise group's


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_fold_batch", "vag_loglike_fold_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


# ---------------------------------------------------------------- 1. boundary errors
def test_add_count_spectrum_boundary_errors_leave_the_fitter_unchanged():
    f = _fitter()
    ok = ok_args()
    lo, hi = ok["energy_lo"], ok["energy_hi"]
    big_lo, big_hi = bins(65)

    def ch(a, at, v):
        b = np.array(a, dtype=float)
        b[at] = v
        return b
    bad = [
        (dict(energy_lo=[]), "energy_lo"), (dict(energy_lo=lo[:3]), "energy_lo"), (dict(energy_lo=[lo], energy_hi=[hi]), "energy_lo"),
        (dict(energy_lo=big_lo, energy_hi=big_hi, response=np.ones((3, 65))), "energy_lo"),
        (dict(energy_lo=ch(lo, 0, 0.0)), "energy_lo"), (dict(energy_lo=ch(lo, 0, -1.0)), "energy_lo"),
        (dict(energy_lo=ch(lo, 1, np.nan)), "energy_lo"), (dict(energy_hi=ch(hi, 3, np.inf)), "energy_hi"),
        (dict(energy_hi=ch(hi, 1, lo[1])), "energy_hi"), (dict(energy_hi=ch(hi, 0, 1.5 * hi[0])), "overlap"),
        (dict(energy_lo=lo[::-1].copy(), energy_hi=hi[::-1].copy()), "ascending"),
        (dict(response=np.ones(4)), "response"), (dict(response=np.ones((3, 5))), "response"), (dict(response=np.ones((0, 4))), "response"),
        (dict(response=np.ones((257, 4)), counts=np.zeros((2, 257))), "response"), (dict(response=ch(ok["response"], (1, 2), -1.0)), "response"),
        (dict(response=ch(ok["response"], (0, 0), np.nan)), "response"), (dict(response=ch(ok["response"], (2, 3), np.inf)), "response"),
        (dict(response=ch(ok["response"], (2, 3), 1e300), energy_lo=ch(lo, 0, 1e-300)), "response"),
        (dict(num_exposure_points=0), "num_exposure_points"), (dict(num_exposure_points=2.5), "num_exposure_points"),
        (dict(t_start=[]), "t_start"), (dict(t_start=[[1e5, 3e5]]), "t_start"), (dict(t_start=[1e5]), "exposure"),
        (dict(t_start=[0.0, 3e5]), "t_start"), (dict(t_start=[-1.0, 3e5]), "t_start"), (dict(t_start=[np.nan, 3e5]), "t_start"),
        (dict(t_start=[np.inf, 3e5]), "t_start"), (dict(exposure=[0.0, 5e4]), "exposure"), (dict(exposure=[-1.0, 5e4]), "exposure"),
        (dict(exposure=[np.nan, 5e4]), "exposure"), (dict(exposure=[np.inf, 5e4]), "exposure"), (dict(exposure=[1e4]), "exposure"),
        (dict(exposure=[1e308, 1e308], t_start=[1.7e308, 1.7e308]), "t_start"),
        (dict(counts=np.zeros(3)), "counts"), (dict(counts=np.zeros((3, 2))), "counts"), (dict(counts=ch(ok["counts"], (0, 1), -1.0)), "counts"),
        (dict(counts=ch(ok["counts"], (0, 1), 2.5)), "counts"), (dict(counts=ch(ok["counts"], (1, 1), np.nan)), "counts"),
        (dict(counts=ch(ok["counts"], (1, 0), np.inf)), "counts"), (dict(counts=ch(ok["counts"], (1, 0), 2.0 ** 54)), "counts"),
        (dict(background=-1.0), "background"), (dict(background=np.nan), "background"), (dict(background=[1.0, 2.0]), "background"),
        (dict(background=np.ones((3, 2))), "background"), (dict(background=[1.0, np.inf, 0.0]), "background"),
        (dict(weights=-1.0), "weights"), (dict(weights=[1.0, 2.0]), "weights"), (dict(weights=[1.0, np.nan, 1.0]), "weights"),
        (dict(weights=np.full((2, 3), np.inf)), "weights"), (dict(weights=np.ones((2, 4))), "weights"),
        (dict(absorption=[1e-22] * 3), "absorption"), (dict(absorption=[1e-22, -1e-22, 0.0, 0.0]), "absorption"),
        (dict(absorption=[np.nan, 0.0, 0.0, 0.0]), "absorption"), (dict(absorption=[np.inf, 0.0, 0.0, 0.0]), "absorption"),
        (dict(absorption=1e-22), "absorption"),
    ]
    for change, word in bad:
        with pytest.raises(ValueError, match="add_count_spectrum") as e:
            f.add_count_spectrum(**{**ok, **change})
        assert word in str(e.value), (change, str(e.value))
        assert not f.has_count_spectra and not f._fold_obs, change
    with pytest.raises(ValueError, match="add_count_spectrum"):
        f.build_spec([THETA_V])  # the "no data" message names the new method
    for n_h in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="n_h"):
            _fitter(n_h=n_h)
    f.add_count_spectrum(**ok)
    assert f.has_count_spectra and not f._point_t and not f._band_obs and not f._counts_obs and not f._index_obs
    spec, _, _ = f.build_spec([THETA_V])  # a fit with nothing but a fold group
    assert spec.n_data == 0 and spec.n_bands == 0 and spec._fold.n_groups == 1 and spec._index is None and spec._counts is None
    assert spec._fold.n_h_fixed == 0.0 and not spec._fold.groups[0].sigma


# ---------------------------------------------------------------- 2. the host arithmetic
def test_nodes_matrix_samples_and_const2():
    f = _fitter(n_h=3e21)
    J, nC = 5, 7
    lo, hi = bins(J)
    hi[2] *= 0.9  # a gap behind bin 2
    rng = np.random.default_rng(2)
    R = rng.uniform(0.0, 200.0, (nC, J))
    R[3, 1] = 0.0
    t0, ex = np.array([3e5, 1e5, 1.5e5]), np.array([5e4, 5e4, 5e4])  # rows are kept in the order given; 1e5..1.5e5 and 1.5e5..2e5 touch
    N = rng.integers(0, 40, (3, nC)).astype(float)
    N[0, 0], N[1, 1], N[2, 2] = 0.0, 1e6, 17.0
    w = rng.uniform(0.5, 2.0, (3, nC))
    w[1, 4] = 0.0
    sig = rng.uniform(1e-24, 1e-22, J)
    f.add_count_spectrum(lo, hi, R, t0, ex, N, background=[0.5] * nC, num_exposure_points=3, weights=w, absorption=sig)
    f.add_count_spectrum(lo, hi, R, t0, ex, N, background=2.0)
    g, g1 = f._fold_obs
    # nodes and matrix, entry by entry from the formulas
    for j in range(J):
        assert g["nu"][j] == math.sqrt(lo[j] * hi[j]) * units.keV
        assert abs(g["nu"][j] * H / 1.602176634e-9 / math.sqrt(lo[j] * hi[j]) - 1) < 4e-16  # keV / h, h the project's constant
        for c in range(nC):
            assert g["A"][j, c] == R[c, j] * (math.log(hi[j] / lo[j]) / H)
    assert g["A"].shape == (J, nC) and g["A"].flags["C_CONTIGUOUS"] and np.array_equal(g["sigma"], sig) and g1["sigma"] is None
    # samples: m = 3 takes both ends and the middle; the shared end point 1.5e5 is evaluated once
    want_t = np.array([1e5, 1.25e5, 1.5e5, 1.75e5, 2e5, 3e5, 3.25e5, 3.5e5])
    assert np.array_equal(g["t_sample"], want_t) and g["m"] == 3
    assert np.array_equal(g["sample_idx"], [[5, 6, 7], [0, 1, 2], [2, 3, 4]]) and g["sample_idx"].dtype == np.int32
    assert np.array_equal(g["exposure_over_m"], ex / 3.0)
    assert np.array_equal(g1["t_sample"], [1.25e5, 1.75e5, 3.25e5]) and np.array_equal(g1["sample_idx"], [[2], [0], [1]])  # m = 1: midpoints
    assert np.array_equal(g1["exposure_over_m"], ex)
    # broadcasting
    assert g["background"].shape == (3, nC) and np.all(g["background"] == 0.5) and np.all(g1["background"] == 2.0)
    assert np.array_equal(g["weights"], w) and np.all(g1["weights"] == 1.0) and np.array_equal(g["counts"], N)
    # const2 = -2 sum w (N ln N - N - ln N!) over the channels with w > 0, with lgamma
    want = 0.0
    for i in range(3):
        for c in range(nC):
            if w[i, c] > 0 and N[i, c] > 0:
                n = N[i, c]
                want += w[i, c] * (n * math.log(n) - n - math.lgamma(n + 1.0))
    assert abs(g["const2"] - (-2.0 * want)) <= 1e-9 * abs(want)  # (lgamma's difference of large numbers at N = 1e6: ~1e-10 absolute)
    small = N < 1e3
    direct = sum(w[i, c] * (N[i, c] * math.log(N[i, c]) - N[i, c] - math.lgamma(N[i, c] + 1.0))
                 for i in range(3) for c in range(nC) if small[i, c] and N[i, c] > 0 and w[i, c] > 0)
    ours = float(np.sum(np.where((w > 0) & small, w * fitting._poisson_const(N), 0.0)))
    assert abs(ours - direct) <= 1e-13 * abs(direct)
    # the spec carries the arrays, the shapes and the fixed column
    spec, _, _ = f.build_spec([THETA_V])
    o = spec._fold.groups[0]
    assert (o.J, o.C, o.n, o.m, o.n_samples) == (J, nC, 3, 3, 8) and spec._fold.n_h_fixed == 3e21
    assert o.A[:J * nC] == list(g["A"].ravel()) and o.sigma[:J] == list(sig) and o.sample_idx[:9] == [5, 6, 7, 0, 1, 2, 2, 3, 4]
    assert o.counts[:3 * nC] == list(N.ravel()) and o.weight[:3 * nC] == list(w.ravel()) and o.exposure_over_m[:3] == list(ex / 3.0)
    assert not spec._fold.groups[1].sigma
    spec2, _, _ = f.build_spec([THETA_V, P("N_H", 1e22, 1e22, fitting.Scale.fixed)])
    assert spec2._fold.n_h_fixed == 1e22  # a fixed ParamDef overrides the keyword
    spec3, _, _ = f.build_spec([THETA_V, P("N_H", 1e20, 1e23, fitting.Scale.log)])
    assert spec3.ndim == 2 and spec3.slot[1] == _lib.P_N_H and spec3.is_log[1] == 1


def test_fold_expected_is_the_statement():
    """fold_expected against plain loops: the sample sum in s order, times exposure / m, times T; the j sum from 0, B added last."""
    f = _fitter()
    J, nC = 3, 4
    lo, hi = bins(J)
    rng = np.random.default_rng(3)
    sig = np.array([2e-22, 5e-23, 1e-23])
    f.add_count_spectrum(lo, hi, rng.uniform(1.0, 9.0, (nC, J)), [1e5, 1.2e5], [2e4, 2e4], np.zeros((2, nC)), background=rng.uniform(0, 3, (2, nC)),
                         num_exposure_points=2, absorption=sig)
    g = f._fold_obs[0]
    ns = g["t_sample"].size
    assert ns == 3  # the windows share 1.2e5
    F = rng.uniform(1e-30, 1e-28, (5, ns * J))
    n_h = rng.uniform(0, 2e22, 5)
    got = fold_expected(F, g, n_h)
    assert got.shape == (5, 2, nC)
    for b in range(5):
        for i in range(2):
            G = []
            for j in range(J):
                tot = 0.0
                for s in range(2):
                    tot = tot + F[b, g["sample_idx"][i, s] * J + j]
                G.append(math.exp(-(n_h[b] * sig[j])) * (g["exposure_over_m"][i] * tot))
            for c in range(nC):
                acc = 0.0
                for j in range(J):
                    acc = acc + g["A"][j, c] * G[j]
                # (np.exp and math.exp may differ by an ulp, 2^-52 of T; it reaches mu through the same operations, each rounding once more)
                assert abs(got[b, i, c] - (g["background"][i, c] + acc)) <= 4 * 2.0 ** -52 * got[b, i, c]
    assert np.array_equal(fold_expected(F[2], g, n_h[2]), got[2])  # one model: the same bits
    assert np.array_equal(fold_expected(F, g, 0.0), fold_expected(F, dict(g, sigma=None)))  # N_H = 0: T = 1 exactly
    with pytest.raises(ValueError, match="fold_expected"):
        fold_expected(F[:, :-1], g)


# ---------------------------------------------------------------- 3. quadrature
@pytest.mark.parametrize("ratio", [1.05, 2.0])
@pytest.mark.parametrize("beta", [0.0, 1.0, 2.5])
def test_the_fold_of_a_power_law_is_x_over_sinh_x_of_the_exact_integral(beta, ratio):
    """F_nu = nu^-beta through a diagonal response: mu_j / (R_j exposure int_bin N_E dE) = x / sinh x with x = beta ln(E_hi / E_lo) / 2,
    to 1e-12, the exact integral in closed form at 40 digits.  With the arithmetic mean as the node the ratio is off by 5e-4 (ratio 2, beta 1)."""
    import mpmath as mp
    J = 6
    lo = 0.3 * ratio ** np.arange(J)
    hi = lo * ratio
    hi[-1] = lo[-1] * ratio
    lo[1:] = hi[:-1]  # contiguous to the bit
    Rdiag = np.linspace(50.0, 300.0, J)
    f = _fitter()
    f.add_count_spectrum(lo, hi, np.diag(Rdiag), [1e5], [3e4], np.zeros((1, J)))
    g = f._fold_obs[0]
    F = g["nu"] ** -beta
    mu = fold_expected(F, g)[0]
    with mp.workdps(40):
        kev_h = mp.mpf(1.602176634e-9) / mp.mpf(H)
        for j in range(J):
            a, b = mp.mpf(float(lo[j])), mp.mpf(float(hi[j]))
            # int_bin N_E dE = int (F_nu / h) d ln E, nu = E keV / h: (keV / h)^-beta (a^-beta - b^-beta) / beta, ln(b / a) at beta = 0
            # (the closed form: mp.quad stops at an absolute tolerance that these integrands, 1e-43 and below, never reach)
            be = mp.mpf(beta)
            integral = kev_h ** -be * ((a ** -be - b ** -be) / be if beta else mp.log(b / a)) / mp.mpf(H)
            exact = mp.mpf(float(Rdiag[j])) * mp.mpf(3e4) * integral
            x = mp.mpf(beta) * mp.log(b / a) / 2
            want = x / mp.sinh(x) if beta else mp.mpf(1)
            got = mp.mpf(float(mu[j])) / exact
            assert abs(got / want - 1) < 1e-12, (j, float(got), float(want))
            if beta == 1.0 and ratio == 2.0:  # the arithmetic-mean node misses by far more than the bound
                wrong = (mp.mpf(0.5) * (a + b) * kev_h) ** -1 * mp.log(b / a) / mp.mpf(H) / integral
                assert abs(wrong / want - 1) > 1e-4


# ---------------------------------------------------------------- 4. the host scan
def _call(name, spec, fold, ctx=None, index_call=False):
    """The host-pointer or _dev entry point with four walkers and no context: whatever the host scan refuses is refused before
    the context is looked at."""
    lib = _lib.load()
    th, out = np.full((4, spec.ndim), 0.3), np.empty(4)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    args = [ctx, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise), ref(spec._counts),
            ref(spec._index)]
    if not index_call:
        args.append(fold)
    if name.endswith("_dev"):
        rc = getattr(lib, name)(*args, th.ctypes.data, 4, spec.ndim, out.ctypes.data)
    else:
        rc = getattr(lib, name)(*args, th.ctypes.data_as(dp), 4, spec.ndim, out.ctypes.data_as(dp))
    return rc, lib.vag_last_error().decode()


NAMES = ("vag_loglike_fold_batch", "vag_loglike_fold_batch_dev")


def test_the_host_scan_refuses_bad_groups_without_a_device():
    f = _fitter()
    f.add_count_spectrum(**ok_args())
    f.add_count_spectrum(**ok_args(J=5, nC=4, num_exposure_points=2, absorption=[1e-22, 5e-23, 2e-23, 1e-23, 0.0], background=1.0))
    spec, _, _ = f.build_spec([THETA_V])
    fs = spec._fold
    for name in NAMES:
        rc, msg = _call(name, spec, C.byref(fs))
        assert rc == _lib.VAG_E_INVALID and msg == "null context", (rc, msg)  # a valid spec reaches the context check

    def refused(*words):
        for name in NAMES:
            rc, msg = _call(name, spec, C.byref(fs))
            assert rc == _lib.VAG_E_INVALID and all(w in msg for w in words), (name, rc, msg, words)
    g0, g1 = f._fold_obs
    per_channel = [("counts", -1.0, "counts"), ("counts", 2.5, "counts"), ("counts", np.nan, "counts"), ("counts", np.inf, "counts"),
                   ("counts", 2.0 ** 54, "2^53"), ("background", -1.0, "background"), ("background", np.nan, "background"),
                   ("background", np.inf, "background"), ("weights", -1.0, "weight"), ("weights", np.nan, "weight"),
                   ("weights", np.inf, "weight")]
    for key, value, word in per_channel:
        keep = g1[key][1, 2]
        g1[key][1, 2] = value
        refused("fold group 1", "row 1", "channel 2", word)
        g1[key][1, 2] = keep
    for value in (-1.0, np.nan, np.inf):
        keep = g1["A"][3, 1]
        g1["A"][3, 1] = value
        refused("fold group 1", "bin 3", "channel 1", "response")
        g1["A"][3, 1] = keep
        keep = g1["sigma"][2]
        g1["sigma"][2] = value
        refused("fold group 1", "bin 2", "cross-section")
        g1["sigma"][2] = keep
    for k, value in ((0, 0.0), (0, -1e17), (2, np.nan), (4, np.inf), (1, g1["nu"][0]), (3, g1["nu"][1])):
        keep = g1["nu"][k]
        g1["nu"][k] = value
        refused("fold group 1", "frequenc", "strictly ascending")
        g1["nu"][k] = keep
    for k, value in ((0, 0.0), (0, -1.0), (1, np.nan), (2, np.inf), (1, g1["t_sample"][0])):
        keep = g1["t_sample"][k]
        g1["t_sample"][k] = value
        refused("fold group 1", f"sample {k}", "strictly ascending")
        g1["t_sample"][k] = keep
    for value in (-1, g1["t_sample"].size):
        keep = g1["sample_idx"][1, 0]
        g1["sample_idx"][1, 0] = value
        refused("fold group 1", "row 1", "sample index")
        g1["sample_idx"][1, 0] = keep
    for value in (0.0, -1.0, np.nan, np.inf):
        keep = g1["exposure_over_m"][1]
        g1["exposure_over_m"][1] = value
        refused("fold group 1", "row 1", "exposure_over_m")
        g1["exposure_over_m"][1] = keep
    o = fs.groups[0]
    for field, value, word in (("J", 0, "J (energy bins)"), ("J", 65, "J (energy bins)"), ("J", -1, "J (energy bins)"), ("C", 0, "C (channels)"),
                               ("C", 257, "C (channels)"), ("n", 0, "no rows"), ("n", -3, "no rows"), ("m", 0, "m (samples per row)"),
                               ("n_samples", 0, "no sample times")):
        keep = getattr(o, field)
        setattr(o, field, value)
        refused("fold group 0", word)
        setattr(o, field, keep)
    for name in ("nu", "A", "t_sample", "exposure_over_m", "counts", "background", "weight"):
        setattr(o, name, None)
        refused("fold group 0", "null array")
        setattr(o, name, g0["weights" if name == "weight" else name].ctypes.data_as(dp))
    addr = C.cast(o.sample_idx, C.c_void_p).value
    o.sample_idx = None
    refused("fold group 0", "null array")
    o.sample_idx = C.cast(addr, C.POINTER(C.c_int32))
    for value in (-1.0, np.nan, np.inf):
        fs.n_h_fixed = value
        refused("n_h_fixed")
    fs.n_h_fixed = 0.0
    fs.n_groups = -1
    refused("n_groups")
    fs.n_groups = 2
    addr = C.cast(fs.groups, C.c_void_p).value  # (a pointer read from the struct is a view of the field: keep the address)
    fs.groups = None
    refused("n_groups")
    fs.groups = C.cast(addr, C.POINTER(_lib.FoldObs))
    for name in NAMES:
        assert _call(name, spec, C.byref(fs)) == (_lib.VAG_E_INVALID, "null context")  # everything restored: valid again


# ---------------------------------------------------------------- 5. N_H
def test_n_h_needs_a_group_with_absorption():
    nh_free, nh_fixed = P("N_H", 1e20, 1e23, fitting.Scale.log), P("N_H", 1e21, 1e21, fitting.Scale.fixed)
    f = _fitter()
    f.add_flux_density(3e9, np.array([1e6, 2e6]), np.array([1e-27, 2e-27]), np.array([1e-28, 2e-28]))
    for nh in (nh_free, nh_fixed):  # no fold group at all
        with pytest.raises(ValueError, match="N_H"):
            f.validate_parameters([THETA_V, nh])
        with pytest.raises(ValueError, match="N_H"):
            f.build_spec([THETA_V, nh])
    f.add_count_spectrum(**ok_args())  # a group, but without a cross-section
    for nh in (nh_free, nh_fixed):
        with pytest.raises(ValueError, match="add_count_spectrum") as e:
            f.validate_parameters([THETA_V, nh])
        assert "absorption" in str(e.value)
        with pytest.raises(ValueError, match="absorption"):
            f.build_spec([THETA_V, nh])
    # the C-ABI: the slot with fold groups none of which has a sigma is refused by the scan, before the device is touched
    spec, _, _ = f.build_spec([THETA_V, P("theta_c", 0.02, 0.3)])
    spec.slot[1] = _lib.P_N_H
    for name in NAMES:
        assert _call(name, spec, C.byref(spec._fold)) == (_lib.VAG_E_INVALID, "bad parameter slot")
    spec.slot[1] = _lib.PARAM_SLOTS["theta_c"]
    for name in NAMES:
        assert _call(name, spec, C.byref(spec._fold)) == (_lib.VAG_E_INVALID, "null context")
    f.add_count_spectrum(**ok_args(absorption=[1e-22, 5e-23, 2e-23, 1e-23]))  # one group with a sigma serves
    f.validate_parameters([THETA_V, nh_free])
    f.validate_parameters([THETA_V, nh_fixed])
    spec, _, _ = f.build_spec([THETA_V, nh_free])
    assert spec.slot[1] == _lib.P_N_H
    for name in NAMES:
        assert _call(name, spec, C.byref(spec._fold)) == (_lib.VAG_E_INVALID, "null context")
    assert f.build_spec([THETA_V, nh_fixed])[0]._fold.n_h_fixed == 1e21
    for bad in (P("N_H", -1.0, 1e22), P("N_H", -1.0, -1.0, fitting.Scale.fixed), P("N_H", np.nan, np.nan, fitting.Scale.fixed)):
        with pytest.raises(ValueError, match="N_H"):
            f.validate_parameters([THETA_V, bad])
    f.validate_parameters([THETA_V, P("N_H", 0.0, 1e23)])  # linear from 0 is fine


# ---------------------------------------------------------------- 6. forwarding
def test_null_or_empty_fold_spec_forwards_to_the_index_call():
    f = _fitter()
    f.add_flux_density(3e9, np.array([1e6, 2e6]), np.array([1e-27, 2e-27]), np.array([1e-28, 2e-28]), noise="radio")
    f.add_counts((7.25e16, 2.42e18), [1e6, 2e6], [1e4, 2e4], [5, 0], 2e11)
    f.add_spectral_index((7.25e16, 2.42e18), [1e5, 2e5], [1.9, 2.0], [0.1, 0.1], convention="photon")
    spec, _, _ = f.build_spec([THETA_V])
    assert spec._fold is None and spec._index is not None
    empty = _lib.FoldFitSpec()
    for name in NAMES:
        want = _call(name.replace("fold", "index"), spec, None, index_call=True)
        assert want == (_lib.VAG_E_INVALID, "null context")
        for fs in (None, C.byref(empty)):
            assert _call(name, spec, fs) == want  # the same error code and message with a null context
    f._index_obs[0]["err"][1] = 0.0  # what the index call refuses, the forwarded call refuses in its words
    for name in NAMES:
        want = _call(name.replace("fold", "index"), spec, None, index_call=True)
        assert want[0] == _lib.VAG_E_INVALID and "index group 0, row 1" in want[1]
        for fs in (None, C.byref(empty)):
            assert _call(name, spec, fs) == want
    f._index_obs[0]["err"][1] = 0.1
    f._counts_obs[0]["counts"][0] = 2.5
    for name in NAMES:
        want = _call(name.replace("fold", "index"), spec, None, index_call=True)
        assert want[0] == _lib.VAG_E_INVALID and "counts group 0, row 0" in want[1]
        for fs in (None, C.byref(empty)):
            assert _call(name, spec, fs) == want
    # with fold groups present the other groups are still scanned, after the fold groups
    f.add_count_spectrum(**ok_args())
    spec, _, _ = f.build_spec([THETA_V])
    for name in NAMES:
        rc, msg = _call(name, spec, C.byref(spec._fold))
        assert rc == _lib.VAG_E_INVALID and "counts group 0, row 0" in msg
    f._counts_obs[0]["counts"][0] = 5.0
    for name in NAMES:
        assert _call(name, spec, C.byref(spec._fold)) == (_lib.VAG_E_INVALID, "null context")
    # the slot N_H with no fold spec at all is not one the index call knows: it needs a context to say so, like every slot check
    assert spec.ndim == 1


# ---------------------------------------------------------------- 7. sharding
def test_sharded_calls_refuse_count_spectra():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_count_spectra = True
    with pytest.raises(NotImplementedError, match="add_count_spectrum"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_count_spectrum(**ok_args())
    with pytest.raises(NotImplementedError, match="add_count_spectrum"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
