"""CPU tests of the upper-limit rows of the likelihood (vag_loglike_lim_batch, the ``upper_limit`` keyword of the Fitter's add_*
methods), and the pure-numpy statement of the limit term that tests/test_limits.py holds the device to:

1. the ctypes layouts of vag_limit_rows / vag_limit_fit_spec and the VAG_OBS_* constants against the C header; the new symbols in
   _lib.EXPORTS and in the library built for gfx950; vag_abi_version() stays 13;
2. every argument error of the keyword raises;
3. build_spec of a mixed data set yields the sorted rows with the right kind / limit / sigma, and the weights of the detections are
   those of the same fitter without the limit rows;
4. sharded likelihood calls refuse a fitter with limits."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.special import log_ndtr

from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def limit_lnl(limit, model, sigma, weight):
    """What the limit rows add to ln L: sum_i w_i ln Phi((L_i - M_i) / sigma_i) (chi^2 gains -2 of it); summed over the last axis."""
    z = (np.asarray(limit, float) - np.asarray(model, float)) / np.asarray(sigma, float)
    return np.sum(np.asarray(weight, float) * log_ndtr(z), axis=-1)


def detection_lnl(ln_flux, model, ln_err, weight):
    """The detection rows' -chi^2 / 2 (Fitter._chi2_sum: residuals in ln F, the model clamped at 1e-300); summed over the last axis."""
    q = (np.asarray(ln_flux, float) - np.log(np.maximum(np.asarray(model, float), 1e-300))) / np.asarray(ln_err, float)
    return -0.5 * np.sum(np.asarray(weight, float) * q * q, axis=-1)


def mixed_lnl(kind, ln_flux, ln_err, limit, sigma, weight, model):
    """ln L of rows of both kinds on model values [..., n]: detections where kind == 0, limits where kind == 1."""
    lim = np.asarray(kind) == _lib.OBS_UPPER_LIMIT
    model = np.asarray(model, float)
    return detection_lnl(ln_flux[~lim], model[..., ~lim], ln_err[~lim], weight[~lim]) + \
        limit_lnl(limit[lim], model[..., lim], sigma[lim], weight[lim])


def inverse_mills(z):
    """The inverse Mills ratio m(z) = phi(z) / Phi(z) = d ln Phi(z) / dz (positive, decreasing; -> -z in the lower tail)."""
    z = np.asarray(z, float)
    return np.exp(-0.5 * z * z - 0.5 * np.log(2 * np.pi) - log_ndtr(z))


LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define R(f) offsetof(vag_limit_rows, f)
#define S(f) offsetof(vag_limit_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(vag_limit_rows), R(kind), R(limit), R(sigma));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_limit_fit_spec), S(point), S(n_bands), S(pad), S(bands), S(n_pol_groups),
           S(pad2), S(pol_kind));
    printf("%d %d %d %d\n", VAG_OBS_DETECTION, VAG_OBS_UPPER_LIMIT, VAG_ABI_VERSION, (int)VAG_MATH_LOG_NDTR);
    return 0;
}
"""


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    R = _lib.LimitRows
    assert [int(x) for x in lines[0].split()] == [C.sizeof(R), R.kind.offset, R.limit.offset, R.sigma.offset]
    S = _lib.LimitFitSpec
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S)] + [getattr(S, n).offset for n in (
        "point", "n_bands", "pad", "bands", "n_pol_groups", "pad2", "pol_kind")]
    assert [int(x) for x in lines[2].split()] == [_lib.OBS_DETECTION, _lib.OBS_UPPER_LIMIT, 13, _lib.MATH["log_ndtr"]]
    assert _lib.MATH["log_ndtr"] == len(_lib.MATH) - 1  # appended: the earlier ids keep their values
    assert _lib.MATH["lds_add"] == 21


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_lim_batch", "vag_loglike_lim_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


def test_the_numpy_term():
    assert limit_lnl([1.0], [1.0], [0.5], [2.0]) == pytest.approx(2.0 * np.log(0.5), rel=1e-15)
    assert limit_lnl([3.0], [0.0], [1.0], [1.0]) == pytest.approx(np.log(0.9986501019683699), rel=1e-13)  # a 3 sigma limit, no flux
    far = limit_lnl([1.0], [1e6 + 1.0], [1.0], [1.0])
    assert np.isfinite(far) and far == pytest.approx(-0.5e12 - np.log(1e6) - 0.5 * np.log(2 * np.pi), rel=1e-12)
    assert inverse_mills(0.0) == pytest.approx(np.sqrt(2 / np.pi), rel=1e-15)
    assert inverse_mills(-30.0) == pytest.approx(30.0, rel=2e-3)  # m(z) -> -z in the tail


T = np.array([3e6, 1e6, 2e6, 4e6])
F = np.array([3e-27, 1e-27, 2e-27, 4e-27])
E = 0.1 * F


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def test_upper_limit_argument_errors():
    f = _fitter()
    mask = np.array([True, False, False, True])
    bad = [np.array([True, False]), np.array([1, 0, 0, 1]), np.array([1.0, 0.0, 0.0, 1.0]), "yes", 1, mask.reshape(2, 2),
           np.array(["a", "b", "c", "d"])]
    for m in bad:
        with pytest.raises(ValueError, match="upper_limit"):
            f.add_flux_density(3e9, T, F, E, upper_limit=m)
        with pytest.raises(ValueError, match="upper_limit"):
            f.add_spectrum(1e6, T * 1e3, F, E, upper_limit=m)
        with pytest.raises(ValueError, match="upper_limit"):
            f.add_flux((1e17, 1e18), T, F * 1e10, E * 1e10, upper_limit=m)
        with pytest.raises(ValueError, match="upper_limit"):
            f.add_polarization(3e9, np.sort(T), np.full(4, 0.1), err_q=np.full(4, 0.02), kind="degree", upper_limit=m)
    neg = F * np.array([-1.0, 1.0, 1.0, 1.0])
    for call in (lambda: f.add_flux_density(3e9, T, neg, E, upper_limit=mask),
                 lambda: f.add_spectrum(1e6, T * 1e3, neg, E, upper_limit=True),
                 lambda: f.add_flux((1e17, 1e18), T, neg, E, upper_limit=mask)):
        with pytest.raises(ValueError, match="upper limit must be >= 0"):
            call()
    with pytest.raises(ValueError, match="err must be finite and > 0"):  # sigma > 0 on a limit row like an error on a detection
        f.add_flux_density(3e9, T, F, E * np.array([0.0, 1, 1, 1]), upper_limit=mask)
    with pytest.raises(ValueError, match="non-finite"):
        f.add_flux_density(3e9, T, F * np.array([np.inf, 1, 1, 1]), E, upper_limit=mask)
    with pytest.raises(ValueError, match="strictly positive"):  # a zero flux is a valid limit, not a valid detection
        f.add_flux((1e17, 1e18), T, F * np.array([1.0, 0.0, 1, 1]), E, upper_limit=mask)
    for m in (True, mask):
        with pytest.raises(ValueError, match="kind='degree'"):
            f.add_polarization(3e9, np.sort(T), np.full(4, 0.1), np.zeros(4), np.full(4, 0.02), np.full(4, 0.02), upper_limit=m)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        f.add_polarization(3e9, np.sort(T), np.array([0.1, 0.1, 1.2, 0.1]), err_q=np.full(4, 0.02), kind="degree", upper_limit=True)
    assert not f._point_t and not f._band_obs and not f._pol_obs and not f.has_limits
    f.add_flux((1e17, 1e18), T, F * np.array([0.0, 1, 1, 1]), E, upper_limit=mask)  # L = 0 is a valid limit
    f.add_polarization(3e9, np.sort(T), np.full(4, 0.1), np.zeros(4), np.full(4, 0.02), np.full(4, 0.02), upper_limit=False)
    assert f.has_limits and f._pol_obs[0]["lim"] is None
    f.add_flux_density(3e9, T, F * np.array([0.0, 1, 1, 1]), E)  # a zero detection is refused when the data are consolidated
    with pytest.raises(ValueError, match="strictly positive"):
        f.build_spec([fitting.ParamDef("theta_v", 0.0, 0.8)])


def test_build_spec_of_a_mixed_data_set():
    defs = [fitting.ParamDef("theta_v", 0.0, 0.8)]
    mask = np.array([False, True, False, True])  # (in the order given: t = 3e6, 1e6, 2e6, 4e6)
    w = np.array([1.0, 0.25, 3.0, 0.5])
    t2, f2, e2 = np.array([2.5e6, 5e5]), np.array([5e-27, 0.0]), np.array([1e-27, 2e-27])
    f = _fitter()
    assert not f.has_limits
    f.add_flux_density(3e9, T, F, E, weights=w, upper_limit=mask)
    f.add_spectrum(2.5e6, [1e9, 2e9], f2[::-1] + 1e-27, e2)  # two detections at one epoch
    f.add_flux_density(6e9, t2, f2, e2, upper_limit=np.array([False, True]))  # L = 0 at t = 5e5
    assert f.has_limits
    spec, _, _ = f.build_spec(defs)
    n = spec.n_data
    assert n == 8 and spec._lim is not None and spec._lim.n_bands == 0 and spec._lim.n_pol_groups == 0
    t = np.array(spec.t[:n])
    assert np.all(np.diff(t) >= 0)
    kind = np.array(spec._lim.point.kind[:n])
    limit, sigma = np.array(spec._lim.point.limit[:n]), np.array(spec._lim.point.sigma[:n])
    want_kind = {5e5: 1, 1e6: 1, 2e6: 0, 3e6: 0, 4e6: 1}
    for i in range(n):
        if t[i] == 2.5e6:
            assert kind[i] == 0
        else:
            assert kind[i] == want_kind[t[i]], (i, t[i])
    assert limit[kind == 1].tolist() == [0.0, F[1], F[3]] and sigma[kind == 1].tolist() == [2e-27, E[1], E[3]]
    assert np.all(limit[kind == 0] == 0) and np.all(sigma[kind == 0] == 1)
    lnf, lne, wt = np.array(spec.ln_flux[:n]), np.array(spec.ln_err[:n]), np.array(spec.weight[:n])
    assert np.all(lnf[kind == 1] == 0) and np.all(lne[kind == 1] == 1)  # not read on a limit row
    assert wt[kind == 1].tolist() == [1.0, 0.25, 0.5]  # limit rows keep their weights (default 1)
    # the same fitter without the limit rows: the detections' rows, bit for bit
    g = _fitter()
    g.add_flux_density(3e9, T[~mask], F[~mask], E[~mask], weights=w[~mask])
    g.add_spectrum(2.5e6, [1e9, 2e9], f2[::-1] + 1e-27, e2)
    g.add_flux_density(6e9, t2[:1], f2[:1], e2[:1])
    plain, _, _ = g.build_spec(defs)
    assert plain._lim is None and not g.has_limits and plain.n_data == 5
    for name, got in (("t", t), ("ln_flux", lnf), ("ln_err", lne), ("weight", wt), ("nu", np.array(spec.nu[:n]))):
        assert np.array_equal(got[kind == 0], np.array(getattr(plain, name)[:5])), name
    assert np.sum(wt[kind == 0]) == pytest.approx(5.0, rel=1e-15)


def test_build_spec_of_band_and_polarization_limits():
    defs = [fitting.ParamDef("theta_v", 0.0, 0.8)]
    f = _fitter()
    f.add_flux((1e17, 1e18), T, F, E)  # no limit row
    f.add_flux((2e17, 2e18), T, F * np.array([1, 0, 1, 1.0]), E, weights=[1.0, 2.0, 3.0, 4.0], upper_limit=np.array([False, True, True, False]))
    tp = np.sort(T)
    f.add_polarization(3e9, tp, np.full(4, 0.1), np.zeros(4), np.full(4, 0.02), np.full(4, 0.02))
    f.add_polarization(3e9, tp, np.array([0.12, 0.05, 0.2, 1.0]), err_q=np.array([0.04, 0.01, 0.01, 0.3]), kind="degree",
                       upper_limit=np.array([True, False, False, True]))
    spec, _, _ = f.build_spec(defs)
    lim = spec._lim
    assert not lim.point.kind and lim.n_bands == 2 and lim.n_pol_groups == 2
    assert not lim.bands[0].kind and not lim.pol_kind[0]
    b = lim.bands[1]  # sorted by t: 1e6 (limit, L = 0), 2e6 (limit), 3e6, 4e6
    assert b.kind[:4] == [1, 1, 0, 0] and b.limit[:4] == [0.0, F[2], 0.0, 0.0] and b.sigma[:4] == [E[1], E[2], 1.0, 1.0]
    bd = spec.bands[1]
    assert bd.ln_flux[:2] == [0.0, 0.0] and bd.ln_err[:2] == [1.0, 1.0] and bd.weight[:4] == [2.0, 3.0, 1.0, 4.0]
    assert bd.ln_flux[2] == np.log(3e-27) and bd.ln_err[3] == pytest.approx(0.1)
    assert lim.pol_kind[1][:4] == [1, 0, 0, 1]
    assert spec._pol.groups[1].q[0] == 0.12 and spec._pol.groups[1].err_q[0] == 0.04  # L and sigma of a degree limit
    only_pol = _fitter()
    only_pol.add_polarization(3e9, tp, np.full(4, 0.1), err_q=np.full(4, 0.02), kind="degree", upper_limit=True)
    spec, _, _ = only_pol.build_spec(defs)
    assert spec.n_data == 0 and spec._lim.n_pol_groups == 1 and spec._lim.pol_kind[0][:4] == [1, 1, 1, 1]


def test_sharded_calls_refuse_limits():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_limits = True
    with pytest.raises(NotImplementedError, match="upper limits"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_flux_density(3e9, T, F, E, upper_limit=np.array([True, False, False, False]))
    with pytest.raises(NotImplementedError, match="upper limits"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
