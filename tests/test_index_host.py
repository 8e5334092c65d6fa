"""CPU tests of the spectral-index groups of the likelihood (vag_loglike_index_batch, Fitter.add_spectral_index), and the sweep and
pure-numpy statement of the term (fitting.index_slope) that tests/test_index.py holds the device to:

1. the ctypes layouts of vag_index_obs / vag_index_fit_spec against the C header; VAG_MATH_LOG_SLOPE is 24, the earlier ids unchanged;
2. the new symbols in _lib.EXPORTS and in the library built for gfx950; vag_abi_version() stays 13;
3. index_slope against mpmath at 40 digits over K x band ratio x slope x flux scale; a plain sum of logs fails the same cap; scaling
   a row's fluxes by a power of two keeps the bits;
4. the least-squares coefficients;
5. the three conventions, and every boundary error of add_spectral_index, which leaves the Fitter unchanged;
6. every refusal of the host scan, through the C entry point with no context (the scan runs before the device is touched);
7. a NULL or empty index spec forwards to vag_loglike_counts_batch;
8. sharded likelihood calls refuse a fitter with spectral-index groups."""
import ctypes as C
import os

import numpy as np
import pytest

from vegasafterglow_amd import _lib, fitting
from vegasafterglow_amd.fitting import index_coefficients, index_from_slope, index_slope

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
U = 2.0 ** -52  # the unit of the error measures: errors are stated in U * slope_scale(F, coef)


# ---------------------------------------------------------------- the sweep both test files use
SWEEP_K = (2, 3, 5, 8)
SWEEP_RATIO = (1.05, 2.0, 33.4, 1e3, 1e6)
SWEEP_SLOPE = (-3.0, -1.25, -0.5, 1.0 / 3.0, 2.5)
SWEEP_SCALE = (1e-250, 1e-26, 1.0, 1e250)


def slope_sweep():
    """(F [N, 8], coef [N, 8], K [N]): spectra nu^slope with a curvature term (so that the least-squares slope is not the slope of
    any one pair) at K nodes over a band of the given ratio, in every flux unit of SWEEP_SCALE; entries from K on are 1 and 0."""
    F, Cf, Ks = [], [], []
    for K in SWEEP_K:
        for ratio in SWEEP_RATIO:
            nu = np.logspace(np.log10(4.84e14), np.log10(4.84e14 * ratio), K)
            nu[-1] = 4.84e14 * ratio
            c = index_coefficients(nu)
            x = np.log(nu / nu[0])
            for slope in SWEEP_SLOPE:
                shape = np.exp(slope * x - 0.07 * x * x / max(1.0, x[-1]))
                for scale in SWEEP_SCALE:
                    row, crow = np.ones(8), np.zeros(8)
                    row[:K], crow[:K] = scale * shape, c
                    F.append(row), Cf.append(crow), Ks.append(K)
    return np.array(F), np.array(Cf), np.array(Ks)


def slope_reference(F, coef, K):
    """sum_{k = 1 .. K-1} c_k ln(F_k / F_0) of one row at 40 digits (an mpf), and the row's scale sum_{k >= 1} |c_k| (1 + |ln(F_k / F_0)|)
    (a float)."""
    import mpmath as mp
    with mp.workdps(40):
        logs = [mp.log(mp.mpf(float(F[k])) / mp.mpf(float(F[0]))) for k in range(1, K)]
        ref = mp.fsum(mp.mpf(float(coef[k + 1])) * logs[k] for k in range(K - 1))
        scale = float(mp.fsum(abs(mp.mpf(float(coef[k + 1]))) * (1 + abs(logs[k])) for k in range(K - 1)))
    return ref, scale


def slope_errors(got, F, coef, K):
    """|got - 40 digits| / (2^-52 * scale) per row of the sweep."""
    import mpmath as mp
    out = np.empty(len(K))
    with mp.workdps(40):
        for i in range(len(K)):
            ref, scale = slope_reference(F[i], coef[i], int(K[i]))
            out[i] = float(abs(mp.mpf(float(got[i])) - ref)) / (U * scale)
    return out


# ---------------------------------------------------------------- 1. layout, ids
LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define O(f) offsetof(vag_index_obs, f)
#define S(f) offsetof(vag_index_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_index_obs), O(n), O(k), O(nu), O(coef), O(ext_slope), O(t), O(value),
           O(err), O(weight));
    printf("%zu %zu %zu %zu\n", sizeof(vag_index_fit_spec), S(n_groups), S(pad), S(groups));
    printf("%d %d %d %d %d %d\n", VAG_ABI_VERSION, (int)VAG_MATH_LOG_SLOPE, (int)VAG_MATH_POISSON_DEVIANCE, (int)VAG_MATH_LOG_NDTR,
           (int)VAG_MATH_COUNT, VAG_INDEX_MAX_NODES);
    return 0;
}
"""


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "c.c", tmp_path / "c"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    O = _lib.IndexObs
    assert [int(x) for x in lines[0].split()] == [C.sizeof(O)] + [getattr(O, n).offset for n in (
        "n", "k", "nu", "coef", "ext_slope", "t", "value", "err", "weight")]
    S = _lib.IndexFitSpec
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S), S.n_groups.offset, S.pad.offset, S.groups.offset]
    assert [int(x) for x in lines[2].split()] == [13, _lib.MATH_MORE["log_slope"], _lib.MATH_MORE["poisson_deviance"],
                                                  _lib.MATH["log_ndtr"], len(_lib.MATH) + len(_lib.MATH_MORE), _lib.INDEX_MAX_NODES]
    assert _lib.MATH_MORE["log_slope"] == 24  # appended: the earlier ids keep their values
    assert _lib.MATH_MORE["poisson_deviance"] == 23 and _lib.MATH["log_ndtr"] == 22 and _lib.MATH["exp2_fast"] == 0
    assert not set(_lib.MATH) & set(_lib.MATH_MORE) and not set(_lib.MATH.values()) & set(_lib.MATH_MORE.values())


# ---------------------------------------------------------------- 2. symbols
def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_index_batch", "vag_loglike_index_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


# ---------------------------------------------------------------- 3. the numpy statement
def test_the_numpy_statement_against_40_digits():
    """index_slope against mpmath at 40 digits over the sweep: every row within 2 units of 2^-52 sum_{k >= 1} |c_k| (1 + |ln(F_k / F_0)|)
    (0.92 was measured when the form was chosen).  The plain sum_k c_k ln F_k on the same rows exceeds that cap: the cap pins the
    pivot form."""
    F, coef, K = slope_sweep()
    assert len(K) == len(SWEEP_K) * len(SWEEP_RATIO) * len(SWEEP_SLOPE) * len(SWEEP_SCALE)
    got = np.array([index_slope(F[i, :K[i]], coef[i, :K[i]]) for i in range(len(K))])
    assert np.all(np.isfinite(got))
    err = slope_errors(got, F, coef, K)
    with np.errstate(all="ignore"):
        plain = np.array([np.sum(coef[i, :K[i]] * np.log(F[i, :K[i]])) for i in range(len(K))])
    err_plain = slope_errors(plain, F, coef, K)
    print("index_slope vs 40 digits [2^-52 S]: pivot form", err.max(), "plain sum of logs", err_plain.max())
    assert err.max() <= 2.0
    assert err_plain.max() > 2.0


def test_power_of_two_flux_units_keep_the_bits():
    F, coef, K = slope_sweep()
    unit = np.isin(F[:, 0], [1.0, 1e-26])
    assert unit.sum() == len(K) // 2
    for i in np.flatnonzero(unit):
        row, c = F[i, :K[i]], coef[i, :K[i]]
        want = index_slope(row, c)
        for e in (-300, -37, 1, 64, 500):
            assert index_slope(np.ldexp(row, e), c).tobytes() == want.tobytes(), (i, e)


def test_the_numpy_statement_shapes_and_edges():
    c = np.array([9.0, 0.5, -2.0])  # c_0 is not read
    F = np.array([[[1.0, np.e, 1.0]], [[2.0, 2.0, 2.0 * np.e ** 2]]])  # [2, 1, 3]
    got = index_slope(F, c)
    assert got.shape == (2, 1)
    np.testing.assert_allclose(got[:, 0], [0.5, -4.0], rtol=1e-15)
    for bad in (0.0, -1.0, np.nan, np.inf):
        for k in range(3):
            row = np.array([1.0, 2.0, 3.0])
            row[k] = bad
            assert np.isnan(index_slope(row, c)), (bad, k)


# ---------------------------------------------------------------- 4. coefficients
def test_coefficients():
    for K in range(2, 9):
        for ratio in (1.05, 33.4, 1e6):
            nu = np.logspace(np.log10(7.25e16), np.log10(7.25e16 * ratio), K)
            c, x = index_coefficients(nu), np.log(nu)
            size = np.sum(np.abs(c) * np.abs(x))
            assert abs(np.sum(c * x) - 1.0) <= 8 * U * size, (K, ratio)
            assert abs(np.sum(c)) <= 8 * U * np.sum(np.abs(c)), (K, ratio)
            for s in (-2.2, 0.0, 0.5):  # a pure power law returns its slope
                assert abs(index_slope(1e-27 * (nu / nu[0]) ** s, c) - s) <= 16 * U * np.sum(np.abs(c) * (1 + np.abs(s * (x - x[0])))), (K, s)
    nu = np.array([7.25e16, 2.42e18])
    c = index_coefficients(nu)
    np.testing.assert_allclose(c, np.array([-1.0, 1.0]) / np.log(nu[1] / nu[0]), rtol=2 * U)
    F = np.array([3e-30, 4e-31])
    np.testing.assert_allclose(index_slope(F, c), np.log(F[1] / F[0]) / np.log(nu[1] / nu[0]), rtol=2 * U)


# ---------------------------------------------------------------- 5. conventions, boundary errors
P = fitting.ParamDef
THETA_V = P("theta_v", 0.0, 0.8)
BAND = (7.25e16, 2.42e18)


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def test_conventions_nodes_and_order():
    f = _fitter()
    assert not f.has_spectral_indices
    t, idx, err = np.array([3e5, 1e5, 2e5]), np.array([1.9, 2.1, 1.75]), np.array([0.1, 0.2, 0.3])
    f.add_spectral_index(BAND, t, idx, err, convention="photon", weights=[1.0, 0.0, 2.0])
    f.add_spectral_index((3.3e14, 5e14), t, idx, err, num_points=5, convention="beta")
    f.add_spectral_index((3.3e14, 5e14), t, idx, err, num_points=8)
    assert f.has_spectral_indices and len(f._index_obs) == 3
    g0, g1, g2 = f._index_obs
    assert np.array_equal(g0["t"], [1e5, 2e5, 3e5]) and np.array_equal(g0["err"], [0.2, 0.3, 0.1])  # sorted by t, the error unchanged
    assert np.array_equal(g0["weights"], [0.0, 2.0, 1.0])
    assert np.array_equal(g0["value"], 1.0 - np.array([2.1, 1.75, 1.9]))  # photon: s = 1 - Gamma
    assert np.array_equal(g1["value"], -np.array([2.1, 1.75, 1.9]))       # beta: s = -beta
    assert np.array_equal(g2["value"], [2.1, 1.75, 1.9]) and np.array_equal(g2["weights"], [1.0, 1.0, 1.0])
    assert g0["nu"].size == 2 and g0["nu"][-1] == BAND[1] and g0["nu"][0] == 10.0 ** np.log10(BAND[0])
    assert abs(g0["nu"][0] / BAND[0] - 1) < 2 * U * np.log(BAND[0])  # (10^log10 x: the rounding of log10 x ~ 17, times ln 10)
    want = np.logspace(np.log10(3.3e14), np.log10(5e14), 5)
    assert g1["nu"][-1] == 5e14 and np.array_equal(g1["nu"][:-1], want[:-1]) and g2["nu"].size == 8
    for g in f._index_obs:
        assert np.array_equal(g["coef"], index_coefficients(g["nu"]))
    for conv in fitting.INDEX_CONVENTIONS:  # the map is its own inverse
        assert np.array_equal(index_from_slope(index_from_slope(idx, conv), conv), idx) or conv == "photon"
    np.testing.assert_allclose(index_from_slope(index_from_slope(idx, "photon"), "photon"), idx, rtol=2 * U)
    spec, _, _ = f.build_spec([THETA_V])  # a fit with nothing but index groups
    assert spec.n_data == 0 and spec.n_bands == 0 and spec._index.n_groups == 3 and spec._counts is None
    o = spec._index.groups[1]
    assert (o.n, o.k, o.ext_slope) == (3, 5, 0.0) and o.nu[:5] == list(g1["nu"]) and o.coef[:5] == list(g1["coef"])
    assert o.t[:3] == [1e5, 2e5, 3e5] and o.value[:3] == list(g1["value"]) and o.err[:3] == [0.2, 0.3, 0.1] and o.weight[:3] == [1.0] * 3


def test_ext_slope_is_the_reddening_of_the_law_over_the_nodes():
    from vegasafterglow_amd import extinction
    f = _fitter(extinction="smc")
    f.add_spectral_index((3.3e14, 5e14), [1e5], [-0.8], [0.1], num_points=8)
    spec, _, _ = f.build_spec([THETA_V, P("A_V", 0.0, 2.0)])
    g = f._index_obs[0]
    kappa = 0.4 * np.log(10.0) * np.asarray(f._k_lambda((2.99792458e10 / g["nu"]) / (1.0 + f.z)), dtype=np.float64)
    want = 0.0
    for k in range(1, 8):
        want = want + g["coef"][k] * (kappa[k] - kappa[0])
    assert spec._index.groups[0].ext_slope == want and want > 0  # (kappa rises to the blue: extinction steepens... reddens the slope)
    assert extinction is not None
    spec2, _, _ = f.build_spec([THETA_V, P("A_V", 0.0, 2.0), P("z", 0.5, 0.5, fitting.Scale.fixed, initial=0.5)])
    assert spec2._index.groups[0].ext_slope != want  # the law's rest-frame wavelengths follow a fixed z


def test_add_spectral_index_boundary_errors_leave_the_fitter_unchanged():
    f = _fitter()
    ok = dict(band=BAND, t=np.array([1e5, 2e5]), index=np.array([1.9, 2.0]), err=np.array([0.1, 0.2]))
    bad = [dict(band=1e17), dict(band=(1e18, 1e17)), dict(band=(0.0, 1e17)), dict(band=(1e17, np.inf)), dict(band=(np.nan, 1e18)),
           dict(band=(1e17, 1e17)), dict(band=(1e17, 1e17 * (1 + 2 * U)), num_points=8), dict(num_points=1), dict(num_points=9),
           dict(num_points=2.5), dict(t=[]), dict(t=[[1e5, 2e5]]), dict(t=[1e5]), dict(t=[0.0, 2e5]), dict(t=[-1.0, 2e5]),
           dict(t=[np.nan, 2e5]), dict(t=[np.inf, 2e5]), dict(index=[np.nan, 2.0]), dict(index=[np.inf, 2.0]), dict(index=[1.0, 2.0, 3.0]),
           dict(err=[0.0, 0.1]), dict(err=[-0.1, 0.1]), dict(err=[np.nan, 0.1]), dict(err=[np.inf, 0.1]), dict(err=[0.1]),
           dict(weights=[1.0]), dict(weights=[1.0, -1.0]), dict(weights=[np.nan, 1.0]), dict(weights=[np.inf, 1.0]),
           dict(convention="gamma"), dict(convention=None)]
    for change in bad:
        with pytest.raises(ValueError, match="add_spectral_index"):
            f.add_spectral_index(**{**ok, **change})
        assert not f.has_spectral_indices and not f._index_obs, change
    with pytest.raises(ValueError, match="add_spectral_index"):
        f.build_spec([THETA_V])  # the "no data" message names the new method
    f.add_spectral_index(**ok)
    assert f.has_spectral_indices and not f._point_t and not f._band_obs and not f._counts_obs
    spec, _, _ = f.build_spec([THETA_V])
    assert spec._index.n_groups == 1


# ---------------------------------------------------------------- 6. the host scan
def _call(name, spec, index, ctx=None, counts_call=False):
    """The host-pointer or _dev entry point with four walkers and no context: whatever the host scan refuses is refused before
    the context is looked at."""
    lib = _lib.load()
    th, out = np.full((4, spec.ndim), 0.3), np.empty(4)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    args = [ctx, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise), ref(spec._counts)]
    if not counts_call:
        args.append(index)
    if name.endswith("_dev"):
        rc = getattr(lib, name)(*args, th.ctypes.data, 4, spec.ndim, out.ctypes.data)
    else:
        rc = getattr(lib, name)(*args, th.ctypes.data_as(dp), 4, spec.ndim, out.ctypes.data_as(dp))
    return rc, lib.vag_last_error().decode()


NAMES = ("vag_loglike_index_batch", "vag_loglike_index_batch_dev")


def test_the_host_scan_refuses_bad_groups_without_a_device():
    f = _fitter()
    f.add_spectral_index(BAND, [1e5, 2e5, 2e5, 3e5], [1.9, 2.0, 2.1, 1.8], [0.1, 0.2, 0.1, 0.3], convention="photon")
    f.add_spectral_index((3.3e14, 5e14), [1e5, 4e5], [0.8, 0.7], [0.1, 0.1], num_points=5, convention="beta", weights=[1.0, 0.0])
    spec, _, _ = f.build_spec([THETA_V])
    isp = spec._index
    for name in NAMES:
        rc, msg = _call(name, spec, C.byref(isp))
        assert rc == _lib.VAG_E_INVALID and msg == "null context", (rc, msg)  # a valid spec (equal times included) reaches the context check

    def refused(*words):
        for name in NAMES:
            rc, msg = _call(name, spec, C.byref(isp))
            assert rc == _lib.VAG_E_INVALID and all(w in msg for w in words), (name, rc, msg, words)
    g0, g1 = f._index_obs
    rows = [("value", 1, np.nan, "index"), ("value", 0, np.inf, "index"), ("err", 1, 0.0, "error"), ("err", 0, -0.1, "error"),
            ("err", 1, np.nan, "error"), ("err", 0, np.inf, "error"), ("weights", 1, -1.0, "weight"), ("weights", 0, np.nan, "weight"),
            ("weights", 1, np.inf, "weight"), ("t", 0, 0.0, "times"), ("t", 0, -1.0, "times"), ("t", 1, np.nan, "times"),
            ("t", 1, np.inf, "times"), ("t", 1, 0.5e5, "times")]
    for key, row, value, word in rows:
        keep = g1[key][row]
        g1[key][row] = value
        refused("index group 1", f"row {row}", word)
        g1[key][row] = keep
    for k, value in ((0, 0.0), (0, -1e14), (2, np.nan), (4, np.inf), (1, g1["nu"][0]), (3, g1["nu"][1])):
        keep = g1["nu"][k]
        g1["nu"][k] = value
        refused("index group 1", "frequenc", "strictly ascending")
        g1["nu"][k] = keep
    for k, value in ((0, np.nan), (3, np.inf)):  # (c_0 is carried: it is checked like the others)
        keep = g1["coef"][k]
        g1["coef"][k] = value
        refused("index group 1", f"coefficient {k}")
        g1["coef"][k] = keep
    o = isp.groups[0]
    for field, value, word in (("k", 1, "k (frequencies)"), ("k", 9, "k (frequencies)"), ("k", -2, "k (frequencies)"), ("n", 0, "no rows"),
                               ("n", -4, "no rows"), ("ext_slope", np.nan, "ext_slope"), ("ext_slope", np.inf, "ext_slope")):
        keep = getattr(o, field)
        setattr(o, field, value)
        refused("index group 0", word)
        setattr(o, field, keep)
    for name in ("nu", "coef", "t", "value", "err", "weight"):
        setattr(o, name, None)
        refused("index group 0", "null array")
        setattr(o, name, g0["weights" if name == "weight" else name].ctypes.data_as(dp))
    isp.n_groups = -1
    refused("n_groups")
    isp.n_groups = 2
    addr = C.cast(isp.groups, C.c_void_p).value  # (a pointer read from the struct is a view of the field: keep the address)
    isp.groups = None
    refused("n_groups")
    isp.groups = C.cast(addr, C.POINTER(_lib.IndexObs))
    for name in NAMES:
        assert _call(name, spec, C.byref(isp)) == (_lib.VAG_E_INVALID, "null context")  # everything restored: valid again


# ---------------------------------------------------------------- 7. forwarding
def test_null_or_empty_index_spec_forwards_to_the_counts_call():
    f = _fitter()
    f.add_flux_density(3e9, np.array([1e6, 2e6]), np.array([1e-27, 2e-27]), np.array([1e-28, 2e-28]), noise="radio")
    f.add_counts(BAND, [1e6, 2e6], [1e4, 2e4], [5, 0], 2e11)
    spec, _, _ = f.build_spec([THETA_V])
    assert spec._index is None
    empty = _lib.IndexFitSpec()
    for name in NAMES:
        want = _call(name.replace("index", "counts"), spec, None, counts_call=True)
        assert want == (_lib.VAG_E_INVALID, "null context")
        for isp in (None, C.byref(empty)):
            assert _call(name, spec, isp) == want  # the same error code and message with a null context
    f._counts_obs[0]["counts"][0] = 2.5  # what the counts call refuses, the forwarded call refuses in its words
    for name in NAMES:
        want = _call(name.replace("index", "counts"), spec, None, counts_call=True)
        assert want[0] == _lib.VAG_E_INVALID and "counts group 0, row 0" in want[1]
        for isp in (None, C.byref(empty)):
            assert _call(name, spec, isp) == want
    # with index groups present the counts groups are still scanned, after the index groups
    f.add_spectral_index(BAND, [1e5], [1.9], [0.1], convention="photon")
    spec, _, _ = f.build_spec([THETA_V])
    for name in NAMES:
        rc, msg = _call(name, spec, C.byref(spec._index))
        assert rc == _lib.VAG_E_INVALID and "counts group 0, row 0" in msg
    f._counts_obs[0]["counts"][0] = 5.0
    for name in NAMES:
        assert _call(name, spec, C.byref(spec._index)) == (_lib.VAG_E_INVALID, "null context")


# ---------------------------------------------------------------- 8. sharding
def test_sharded_calls_refuse_spectral_indices():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_spectral_indices = True
    with pytest.raises(NotImplementedError, match="add_spectral_index"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_spectral_index(BAND, [1e5], [1.9], [0.1], convention="photon")
    with pytest.raises(NotImplementedError, match="add_spectral_index"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
