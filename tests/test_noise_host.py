"""CPU tests of the noise groups of the likelihood (vag_loglike_noise_batch, the ``noise`` / ``calibration`` keywords of the Fitter's
add_flux_density / add_spectrum / add_flux and the parameters ``sys_<label>``), and the pure-numpy statement of the term that
tests/test_noise.py holds the device to:

1. the ctypes layout of vag_noise_fit_spec and the new constants against the C header; the new symbols in _lib.EXPORTS and in the
   library built for gfx950; vag_abi_version() stays 13;
2. the term stated twice in numpy -- the closed form (noise_lnl) and a dense covariance (dense_chi2) -- and its algebra;
3. every argument error raises;
4. build_spec of data given in shuffled time order: the group ids follow the sort, limit rows keep theirs, the weights do not change;
5. sharded likelihood calls refuse a fitter with noise groups."""
import ctypes as C
import os

import numpy as np
import pytest

import test_limits_host as th_
from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noise_sums(r, ln_err, weight, s):
    """A, B, P, N of one group: r [..., n] residuals in ln F, s a scalar or [...] (one systematic per walker)."""
    r, sig, w = np.asarray(r, float), np.asarray(ln_err, float), np.asarray(weight, float)
    s2 = np.asarray(s, float)[..., None] ** 2
    p = w / (sig ** 2 + s2)
    return (np.sum(p * r * r, axis=-1), np.sum(p * r, axis=-1), np.sum(p * np.ones_like(r), axis=-1),
            np.sum(w * np.log1p(s2 / sig ** 2) * np.ones_like(r), axis=-1))


def noise_chi2(r, ln_err, weight, s, c):
    """chi^2_g = A - c^2 B^2 / (1 + c^2 P) + N + log1p(c^2 P), the closed form."""
    A, B, P, N = noise_sums(r, ln_err, weight, s)
    c2 = float(c) ** 2
    return A - c2 * B * B / (1.0 + c2 * P) + N + np.log1p(c2 * P)


def noise_lnl(ln_flux, model, ln_err, weight, s, c):
    """What the detection rows of one noise group add to ln L, -chi^2_g / 2, on model values [..., n] (clamped at 1e-300 like the
    plain detection term); s: the fractional systematic, a scalar or one per walker; c: the calibration fraction."""
    r = np.asarray(ln_flux, float) - np.log(np.maximum(np.asarray(model, float), 1e-300))
    return -0.5 * noise_chi2(r, ln_err, weight, s, c)


def dense_chi2(r, ln_err, weight, s, c):
    """The same from a dense covariance, for one walker: over the rows with w > 0, C = diag(v / w) + c^2 1 1^T with v = sigma^2 + s^2;
    r^T C^-1 r by a linear solve, ln det C by slogdet, measured from ln det diag(v / w) (what remains is the calibration's share), and
    the systematic's normalisation sum w ln(v / sigma^2) with a plain log."""
    r, sig, w = (np.asarray(a, float) for a in (r, ln_err, weight))
    keep = w > 0
    r, sig, w = r[keep], sig[keep], w[keep]
    v = sig ** 2 + float(s) ** 2
    Cm = np.diag(v / w) + float(c) ** 2 * np.ones((r.size, r.size))
    sign, logdet = np.linalg.slogdet(Cm)
    assert sign > 0
    return r @ np.linalg.solve(Cm, r) + (logdet - np.sum(np.log(v / w))) + np.sum(w * np.log(v / sig ** 2))


LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define S(f) offsetof(vag_noise_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_noise_fit_spec), S(n_groups), S(n_bands), S(point_group), S(band_group),
           S(sys_fixed), S(calib));
    printf("%d %d %d %d\n", VAG_P_NOISE_SYS0, VAG_NOISE_MAX_GROUPS, VAG_ABI_VERSION, VAG_P_POL_PI_MAX_RVS);
    printf("%zu %zu\n", sizeof(vag_model_params), sizeof(((vag_noise_fit_spec*)0)->calib) / sizeof(double));
    return 0;
}
"""


def test_ctypes_layout_matches_header(tmp_path):
    src, exe = tmp_path / "n.c", tmp_path / "n"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    S = _lib.NoiseFitSpec
    assert [int(x) for x in lines[0].split()] == [C.sizeof(S)] + [getattr(S, n).offset for n in (
        "n_groups", "n_bands", "point_group", "band_group", "sys_fixed", "calib")]
    assert [int(x) for x in lines[1].split()] == [_lib.P_NOISE_SYS0, _lib.NOISE_MAX_GROUPS, 13, _lib.POL_SLOTS["pol_pi_max_rvs"]]
    assert _lib.P_NOISE_SYS0 == 1008 and _lib.NOISE_MAX_GROUPS == 8
    assert [int(x) for x in lines[2].split()] == [272, 8] and C.sizeof(_lib.ModelParams) == 272


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_noise_batch", "vag_loglike_noise_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


# ---------------------------------------------------------------- 2. the term
def _case(rng):
    n = int(rng.integers(1, 80))
    sig = rng.uniform(0.03, 0.3, n)
    w = rng.uniform(0.5, 2.0, n)
    w[rng.integers(0, n)] = 0.0  # one zero weight (a 1-row case has no row left: chi^2 = 0)
    r = rng.uniform(-30.0, 30.0) + sig * rng.standard_normal(n)
    return r, sig, w


def test_closed_form_agrees_with_the_dense_covariance():
    """2000 random cases (100 draws x s in {0, .01, .1, 1} x c in {0, .02, .1, .5, 3}): n in [1, 80), sigma in [0.03, 0.3], w in
    [0.5, 2] with one zero weight, a common offset of r up to 30.  The two forms must agree to 1e-9 of max(1, |value|): they differ
    by rounding only (measured on a CPU: at most 3.1e-11, at c = 3 and the largest offsets, where r^T C^-1 r cancels ~1e6-fold)."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(100):
        r, sig, w = _case(rng)
        for s in (0.0, 0.01, 0.1, 1.0):
            for c in (0.0, 0.02, 0.1, 0.5, 3.0):
                a, b = float(noise_chi2(r, sig, w, s, c)), dense_chi2(r, sig, w, s, c)
                worst = max(worst, abs(a - b) / max(1.0, abs(b)))
    print("closed form vs dense covariance: worst", worst)
    assert worst <= 1e-9


def test_the_term_reduces_and_profiles():
    rng = np.random.default_rng(11)
    for _ in range(20):
        r, sig, w = _case(rng)
        lnf = rng.uniform(-60.0, -50.0, r.size)
        model = np.exp(lnf - r)
        # s = c = 0: today's detection term
        a, b = noise_lnl(lnf, model, sig, w, 0.0, 0.0), th_.detection_lnl(lnf, model, sig, w)
        assert a == pytest.approx(b, rel=1e-13, abs=1e-300)
        # all weights 1: the exact Gaussian, ln det C - ln det diag(sigma^2) in one piece
        ones = np.ones_like(w)
        Cm = np.diag(sig ** 2 + 0.1 ** 2) + 0.5 ** 2
        want = r @ np.linalg.solve(Cm, r) + np.linalg.slogdet(Cm)[1] - np.sum(np.log(sig ** 2))
        got = float(noise_chi2(r, sig, ones, 0.1, 0.5))
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want))
        # c -> infinity: A - B^2 / P + N + log1p(c^2 P), the profile over a free offset delta = B / P
        A, B, P, N = noise_sums(r, sig, w, 0.1)
        if P == 0:
            continue
        big = 1e6
        prof = np.sum(w / (sig ** 2 + 0.01) * (r - B / P) ** 2)
        assert A - B * B / P == pytest.approx(prof, rel=1e-6, abs=1e-6)  # (the left side cancels; the right is the stable form)
        got = float(noise_chi2(r, sig, w, 0.1, big)) - np.log1p(big ** 2 * P) - N
        assert got == pytest.approx(prof, rel=1e-6, abs=1e-6)
    # the model clamp, and one s per walker
    two = noise_lnl([0.0, 1.0], [[0.0, np.e], [1.0, np.e]], [0.1, 0.2], [1.0, 1.0], [0.0, 0.3], 0.0)
    assert two[0] == pytest.approx(-0.5 * (np.log(1e-300) / 0.1) ** 2, rel=1e-14)
    assert two[1] == pytest.approx(-0.5 * (np.log1p(0.09 / 0.01) + np.log1p(0.09 / 0.04)), rel=1e-14)


# ---------------------------------------------------------------- 3. argument errors
T = np.array([3e6, 1e6, 2e6, 4e6])
F = np.array([3e-27, 1e-27, 2e-27, 4e-27])
E = 0.1 * F
P = fitting.ParamDef
THETA_V = P("theta_v", 0.0, 0.8)


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def test_noise_argument_errors():
    f = _fitter()
    adders = (lambda **kw: f.add_flux_density(3e9, T, F, E, **kw), lambda **kw: f.add_spectrum(1e6, T * 1e3, F, E, **kw),
              lambda **kw: f.add_flux((1e17, 1e18), T, F * 1e10, E * 1e10, **kw))
    for add in adders:
        for label in ("", "a b", "a-b", "radio!", 3, b"a", ["a"]):
            with pytest.raises(ValueError, match="noise must be a label"):
                add(noise=label)
        with pytest.raises(ValueError, match="calibration needs noise"):
            add(calibration=0.05)
        for c in (-0.01, np.nan, np.inf, -np.inf, "much"):
            with pytest.raises(ValueError, match="calibration must be"):
                add(noise="a", calibration=c)
    assert not f.has_noise_groups and not f._point_t and not f._band_obs  # a refused call records nothing
    for k in range(8):
        adders[k % 3](noise=f"g{k}")
    assert f.has_noise_groups and f._noise_labels == [f"g{k}" for k in range(8)]  # numbered in order of first mention
    with pytest.raises(ValueError, match="at most 8 noise groups"):
        f.add_flux_density(3e9, T, F, E, noise="g8")
    f.add_flux_density(3e9, T, F, E, noise="g3")  # a known label is not a ninth
    assert len(f._noise_labels) == 8

    g = _fitter()
    g.add_flux_density(3e9, T, F, E, noise="radio", calibration=0.05)
    with pytest.raises(ValueError, match="calibration=0.05 from an earlier call"):
        g.add_spectrum(1e6, T * 1e3, F, E, noise="radio", calibration=0.1)
    g.add_spectrum(1e6, T * 1e3, F, E, noise="radio", calibration=0.05)  # the same value, and none, agree
    g.add_flux_density(6e9, T, F, E, noise="radio")
    assert g._noise_calib == {"radio": 0.05}
    for check in (g.validate_parameters, g.build_spec):
        with pytest.raises(ValueError, match="needs data added with noise='x'"):
            check([THETA_V, P("sys_x", 0.0, 1.0)])
        with pytest.raises(ValueError, match="needs data added with noise='x'"):
            check([THETA_V, P("sys_x", 0.1, 0.1, fitting.Scale.fixed)])
        with pytest.raises(ValueError, match="fixed sys_radio must be finite and >= 0"):
            check([THETA_V, P("sys_radio", -0.1, -0.1, fitting.Scale.fixed)])
        with pytest.raises(ValueError, match="fixed sys_radio must be finite and >= 0"):
            check([THETA_V, P("sys_radio", 0.0, 1.0, fitting.Scale.fixed, initial=np.nan)])
        with pytest.raises(ValueError, match="lower >= 0"):
            check([THETA_V, P("sys_radio", -0.1, 1.0)])
        with pytest.raises(ValueError):  # (validate_parameters names the log scale first, build_spec the systematic)
            check([THETA_V, P("sys_radio", 0.0, 1.0, fitting.Scale.log)])
        check([THETA_V, P("sys_radio", 0.0, 1.0)])
        check([THETA_V, P("sys_radio", 1e-3, 1.0, fitting.Scale.log)])
        check([THETA_V, P("sys_radio", 0.0, 0.0, fitting.Scale.fixed)])
    with pytest.raises(ValueError, match="sys_radio"):  # no noise group at all
        _fitter_with_points().build_spec([THETA_V, P("sys_radio", 0.0, 1.0)])


def _fitter_with_points():
    f = _fitter()
    f.add_flux_density(3e9, T, F, E)
    return f


def test_a_calibrated_group_must_lie_in_one_pass():
    band = ((1e17, 1e18), T, F * 1e10, E * 1e10)
    f = _fitter()  # point rows and a band group
    f.add_flux_density(3e9, T, F, E, noise="x", calibration=0.05)
    f.add_flux(*band, noise="x")
    with pytest.raises(ValueError, match="noise group 'x' has calibration=0.05 and rows in 2 passes"):
        f.build_spec([THETA_V])
    f = _fitter()  # two band groups
    f.add_flux(*band, noise="x")
    f.add_flux((2e17, 2e18), T, F * 1e10, E * 1e10, noise="x", calibration=0.05)
    with pytest.raises(ValueError, match="rows in 2 passes"):
        f.build_spec([THETA_V])
    f = _fitter()  # without a calibration the group may span passes; with one, several point calls are one pass
    f.add_flux_density(3e9, T, F, E, noise="x")
    f.add_flux(*band, noise="x")
    f.add_flux((2e17, 2e18), T, F * 1e10, E * 1e10, noise="x")
    f.add_flux_density(6e9, T, F, E, noise="y", calibration=0.05)
    f.add_spectrum(1e6, T * 1e3, F, E, noise="y")
    f.add_flux((3e17, 3e18), T, F * 1e10, E * 1e10, noise="z", calibration=0.2)
    spec, _, _ = f.build_spec([THETA_V])
    nz = spec._noise
    assert nz.n_groups == 3 and nz.n_bands == 3 and nz.band_group[:3] == [0, 0, 2]
    assert nz.calib[:3] == [0.0, 0.05, 0.2] and nz.sys_fixed[:8] == [0.0] * 8


# ---------------------------------------------------------------- 4. build_spec
def test_build_spec_of_shuffled_input_times():
    rng = np.random.default_rng(5)
    t1, t2, t3 = rng.permutation(np.linspace(1e5, 2e6, 9)), rng.permutation(np.linspace(1.5e5, 3e6, 7)), rng.permutation(
        np.linspace(2.5e5, 1e6, 5))
    w1, w2, w3 = rng.uniform(0.5, 2.0, 9), rng.uniform(0.5, 2.0, 7), rng.uniform(0.5, 2.0, 5)
    lim1 = np.arange(9) % 4 == 1
    fl = lambda t: 1e-27 * (t / 1e6) ** -0.7  # noqa: E731

    def build(with_noise):
        kw = (lambda **k: k) if with_noise else (lambda **k: {})
        f = _fitter()
        f.add_flux_density(3e9, t1, fl(t1), 0.1 * fl(t1), weights=w1, upper_limit=lim1, **kw(noise="radio", calibration=0.05))
        f.add_flux_density(5e14, t2, fl(t2), 0.2 * fl(t2), weights=w2)
        f.add_flux_density(np.full(5, 2e17), t3, fl(t3), 0.3 * fl(t3), weights=w3, **kw(noise="xray"))
        f.add_spectrum(5e5, [1e9, 2e9, 4e9], fl(np.full(3, 5e5)), 0.1 * fl(np.full(3, 5e5)), **kw(noise="radio", calibration=0.05))
        f.add_flux((1e17, 1e18), t3, fl(t3) * 1e10, fl(t3) * 1e9, **kw(noise="xray"))
        f.add_flux((1e15, 1e16), t2, fl(t2) * 1e10, fl(t2) * 1e9)
        return f, f.build_spec([THETA_V, P("sys_radio", 0.0, 1.0), P("sys_xray", 0.2, 0.2, fitting.Scale.fixed)] if with_noise
                               else [THETA_V])[0]
    f, spec = build(True)
    g, plain = build(False)
    n = spec.n_data
    assert n == 24 and f.has_noise_groups and not g.has_noise_groups and plain._noise is None
    nz = spec._noise
    assert nz.n_groups == 2 and nz.n_bands == 2 and nz.band_group[:2] == [1, -1]
    assert nz.sys_fixed[:2] == [0.0, 0.2] and nz.calib[:2] == [0.05, 0.0]
    assert spec.slot[1] == _lib.P_NOISE_SYS0 and spec.ndim == 2  # sys_radio is group 0; sys_xray is fixed
    t, nu, grp = np.array(spec.t[:n]), np.array(spec.nu[:n]), np.array(nz.point_group[:n])
    assert np.all(np.diff(t) >= 0)
    want = np.where(nu < 1e10, 0, np.where(nu == 2e17, 1, -1))  # the group ids follow the sort: a row's frequency names its call
    assert np.array_equal(grp, want) and (grp == 0).sum() == 12 and (grp == 1).sum() == 5 and (grp == -1).sum() == 7
    kind = np.array(spec._lim.point.kind[:n])
    assert kind.sum() == lim1.sum() == 2 and np.all(grp[kind == 1] == 0)  # limit rows keep their group id, flagged as limits
    assert sorted(t[kind == 1]) == sorted(t1[lim1])
    for name in ("t", "nu", "ln_flux", "ln_err", "weight"):  # nothing else changes: the rows and weights without noise=, bit for bit
        assert np.array_equal(np.array(getattr(spec, name)[:n]), np.array(getattr(plain, name)[:n])), name
    assert np.sum(np.array(spec.weight[:n])[kind == 0]) == pytest.approx(22.0, rel=1e-15)
    for b in range(2):
        assert spec.bands[b].weight[:spec.bands[b].n] == plain.bands[b].weight[:plain.bands[b].n]
    assert f._params_at([0.3, 0.5], [THETA_V, P("sys_radio", 0.0, 1.0)])[0].theta_obs == 0.3  # the systematic is no Model field


# ---------------------------------------------------------------- 5. sharding
def test_sharded_calls_refuse_noise_groups():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_noise_groups = True
    with pytest.raises(NotImplementedError, match="noise="):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_flux_density(3e9, T, F, E, noise="radio")
    with pytest.raises(NotImplementedError, match="noise="):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
