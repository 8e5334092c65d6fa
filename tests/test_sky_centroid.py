"""Exact sky moments on the device (vag_sky_centroid_batch, Model.sky_moments(exact=True)) and the centroid term of the walker
likelihood (vag_loglike_sky_batch[_dev], Fitter.add_centroid): agreement with the CPU checker and convergence of the azimuthal-part
moments towards them, flux conservation, bits, the GW170817-like centroid motion, the likelihood against host arithmetic, calls
without centroid data, invalid walkers, and the theta_obs / theta_c degeneracy that centroid data break."""
import ctypes as C

import numpy as np
import pytest

import _abi
import _skycheck as sk
import configs
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, units

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
# the sky-image models, a spreading jet (c_spread_3d) and an SSC model (d_c3_fwd_ssc) among them
NAMES = ["a_c1a", "b_c2", "c_spread_3d", "d_c3_fwd_ssc", "e_rs_tophat", "f_c4"]


def model(name):
    return va.Model.from_params(sk.params(name))


def mom_array(sm):
    return np.stack([getattr(sm, n) for n in va.SkyMoments.names], axis=-1)


def batch_centroid(params, t, nu):
    lib = _lib.load()
    h, lock = va.get_context(0)
    t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(np.atleast_1d(nu), float)
    nb = len(params)
    arr = (_lib.ModelParams * nb)(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in params])
    out = np.empty((nb, nu.size, t.size, 6))
    with lock:
        _lib.check(lib.vag_sky_centroid_batch(h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                              out.ctypes.data_as(dp)))
    return out


@pytest.fixture(scope="module")
def exact():
    return {n: mom_array(model(n).sky_moments(sk.T, sk.NU, exact=True)) for n in NAMES}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return sk.build_checker(tmp_path_factory.mktemp("sky_checker"))


def _live(ref):
    return np.isfinite(ref[..., 1]) & (ref[..., 0] > 1e-10 * ref[..., 0].max())


@pytest.mark.parametrize("name", NAMES)
def test_against_the_checker(name, exact, checker):
    """The checker's parts at n_az = 65536 and 32768, one Richardson step: their midpoint error ~(dphi / S)^2 / 24 is ~1e-7 on varY
    of the off-axis jets, whose emission spans a narrow range of phi.  What is left is the per-term difference between the device
    and the oracle (~4e-8 on varX of the on-axis a_c1a, whose full-circle part sums are exact)."""
    p = sk.params(name)
    fine, coarse = checker.moments(p, sk.T, sk.NU, 65536), checker.moments(p, sk.T, sk.NU, 32768)
    want = fine.copy()
    want[..., 1:] = (4 * fine[..., 1:] - coarse[..., 1:]) / 3
    got = exact[name]
    ok = _live(fine)
    err_x = np.abs(got[..., 1] - want[..., 1])[ok] / np.abs(want[..., 1][ok]).clip(min=np.sqrt(want[..., 3] + want[..., 4])[ok])
    err_v = [np.abs(got[..., q] - want[..., q])[ok] / want[..., q][ok] for q in (3, 4)]
    print(name, "Xbar", err_x.max(), "varX", err_v[0].max(), "varY", err_v[1].max())
    assert err_x.max() <= 1e-8
    assert err_v[0].max() <= 1e-7 and err_v[1].max() <= 1e-7


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d", "f_c4"])
def test_parts_converge_to_the_exact_moments(name, exact):
    m = model(name)
    ex = exact[name]
    ok = _live(ex)
    s = np.sqrt(ex[..., 3] + ex[..., 4])[ok]
    gaps = []
    for n_az in (2048, 4096, 8192):
        mo = mom_array(m.sky_moments(sk.T, sk.NU, n_az=n_az))
        gaps.append(max(np.max(np.abs(mo[..., 1] - ex[..., 1])[ok] / s),
                        max(np.max(np.abs(mo[..., q] - ex[..., q])[ok] / s ** 2) for q in (3, 4, 5))))
    print(name, gaps)
    for a, b in zip(gaps, gaps[1:]):
        assert 3.0 <= a / b <= 5.5, gaps


@pytest.mark.parametrize("name", NAMES)
def test_flux_is_conserved(name, exact):
    ref = model(name).flux_density_grid(sk.T, sk.NU).total
    live = sk.live_bins(ref)
    assert np.max(np.abs(exact[name][..., 0] - ref)[live] / ref[live]) <= 1e-13


def test_bitwise_reproducible_and_independent_of_the_batch(exact):
    for n in ("b_c2", "d_c3_fwd_ssc"):
        again = mom_array(model(n).sky_moments(sk.T, sk.NU, exact=True))
        assert np.array_equal(again, exact[n], equal_nan=True), n
    mixed = batch_centroid([sk.params(n) for n in NAMES], sk.T, sk.NU)  # mixed flags: SSC, reverse shock, spreading
    for q, n in enumerate(NAMES):
        assert np.array_equal(mixed[q], exact[n], equal_nan=True), n
    same = batch_centroid([sk.params("b_c2")] * 3 + [sk.params("f_c4")], sk.T, sk.NU)
    assert np.array_equal(same[0], same[2], equal_nan=True) and np.array_equal(same[1], exact["b_c2"], equal_nan=True)


def test_t_chunked_path_is_bitwise_equal(exact):
    import os
    lib = _lib.load()
    os.environ["VAG_SKY_CHUNK_T"] = "2"
    lib.vag_reload_env_hooks()
    try:
        cut = mom_array(model("b_c2").sky_moments(sk.T, sk.NU, exact=True))
    finally:
        del os.environ["VAG_SKY_CHUNK_T"]
        lib.vag_reload_env_hooks()
    assert np.array_equal(cut, exact["b_c2"], equal_nan=True)


def test_c4_centroid_moves_out_and_stays_on_the_axis(exact):
    t = np.geomspace(20, 1000, 10) * units.day
    sm = model("f_c4").sky_moments(t, 3e9, exact=True)
    assert np.all(sm.F > 0) and np.all(np.diff(sm.Xbar) > 0) and sm.Xbar[0] > 0
    assert np.all(sm.Ybar == 0)  # mirrored grid: exactly
    for n in sk.AXISYMMETRIC:
        ok = np.isfinite(exact[n][..., 2])
        assert np.all(exact[n][..., 2][ok] == 0), n
    shift = (model("f_c4").sky_moments(np.array([75.0, 230.0]) * units.day, 3e9, exact=True).Xbar @ [-1, 1]) / units.mas
    assert 1.0 <= shift <= 6.0, shift


# ---- the likelihood ----
C4_LC_T = np.geomspace(10, 300, 8) * units.day
C4_LC_NU = 3e9
C4_CEN_T = np.array([75.0, 160.0, 230.0]) * units.day
C4_CEN_NU = 8e9


def _c4_fitter(with_centroid, pa_true=0.3, east0_true=2e-10, flux_err=0.3, pos_err=0.2 * units.mas):
    tr = configs.C4_TRUTH
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    truth = va.Model.from_params(_abi.make_params(**tr))
    fl = truth.flux_density_grid(C4_LC_T, C4_LC_NU).total[0]
    f.add_flux_density(C4_LC_NU, C4_LC_T, fl, flux_err * fl)
    if with_centroid:
        sm = truth.sky_moments(C4_CEN_T, C4_CEN_NU, exact=True)
        east = east0_true + sm.Xbar * np.sin(pa_true) + sm.Ybar * np.cos(pa_true)
        north = sm.Xbar * np.cos(pa_true) - sm.Ybar * np.sin(pa_true)
        err = np.full(C4_CEN_T.size, pos_err)
        f.add_centroid(C4_CEN_NU, C4_CEN_T, east, north, err, 1.5 * err, weights=[1.0, 0.5, 2.0])
    return f


def _c4_fixed(skip=()):
    tr = configs.C4_TRUTH
    vals = dict(E_iso=tr["E_iso"], Gamma0=tr["Gamma0"], theta_c=tr["theta_c"], theta_v=tr["theta_obs"], n_ism=tr["n_ism"],
                eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"])
    return [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in vals.items() if k not in skip]


def _walkers(nb, seed=5):
    rng = np.random.default_rng(seed)
    tr = configs.C4_TRUTH
    th = np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nb), tr["theta_obs"] * rng.uniform(0.85, 1.15, nb),
                          np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nb)])
    sky = np.column_stack([rng.uniform(0.0, 0.6, nb), rng.uniform(-1e-9, 1e-9, nb)])
    return th, sky


FLUX_DEFS = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
             fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)]
SKY_DEFS = [fitting.ParamDef("pa", -1.0, 1.0), fitting.ParamDef("east0", -2e-9, 2e-9)]


def _host_centroid_chi2(f_sky, defs, samples):
    params = [f_sky._params_at(s, defs)[0] for s in samples]
    mo = batch_centroid(params, C4_CEN_T, C4_CEN_NU)[:, 0]
    cd = f_sky._centroid_obs[0]
    pa, e0 = samples[:, 3:4], samples[:, 4:5]
    east = e0 + mo[..., 1] * np.sin(pa) + mo[..., 2] * np.cos(pa)
    north = mo[..., 1] * np.cos(pa) - mo[..., 2] * np.sin(pa)
    return (cd["weights"] * (((cd["east"] - east) / cd["err_east"]) ** 2 + ((cd["north"] - north) / cd["err_north"]) ** 2)).sum(1)


def test_likelihood_matches_host_arithmetic():
    import torch
    th, sky = _walkers(64)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    fixed = _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    f_flux, f_sky = _c4_fitter(False), _c4_fitter(True)
    defs_flux, defs_sky = FLUX_DEFS + fixed, FLUX_DEFS + SKY_DEFS + fixed
    ll_flux = f_flux.loglike_batch(th, defs_flux)
    chi2_c = _host_centroid_chi2(f_sky, defs_sky, samples)
    want = ll_flux - 0.5 * chi2_c
    assert np.all(np.isfinite(want)) and np.all(chi2_c > 0)
    got = f_sky.loglike_batch(samples, defs_sky)
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-10
    # device-pointer form
    ev = f_sky.device_evaluator(defs_sky)
    vals, _ = ev(torch.from_numpy(samples).to("cuda:0"))
    torch.cuda.synchronize()
    assert np.max(np.abs(vals.cpu().numpy() - want) / np.abs(want)) <= 1e-10
    # with priors: the flux fit's ln prior plus the sky parameters' Uniform(lower, upper)
    lp_flux = f_flux.log_prob_batch(th, defs_flux)
    lp_sky = -np.log(2.0) - np.log(4e-9)
    want_p = lp_flux - 0.5 * chi2_c + lp_sky
    got_p = f_sky.log_prob_batch(samples, defs_sky)
    assert np.max(np.abs(got_p - want_p) / np.abs(want_p)) <= 1e-10
    ev_p = f_sky.device_evaluator(defs_sky, use_priors=True)
    vals_p, _ = ev_p(torch.from_numpy(samples).to("cuda:0"))
    torch.cuda.synchronize()
    assert np.max(np.abs(vals_p.cpu().numpy() - want_p) / np.abs(want_p)) <= 1e-10


def test_no_centroid_groups_is_bitwise_the_flux_call():
    th, _ = _walkers(64, seed=9)
    f = _c4_fitter(False)
    defs = FLUX_DEFS + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    spec, _, _ = f.build_spec(defs)
    th = np.ascontiguousarray(th)
    lib = _lib.load()
    h, lock = va.get_context(0)
    a, b = np.empty(th.shape[0]), np.empty(th.shape[0])
    none = _lib.SkyFitSpec()
    with lock:
        _lib.check(lib.vag_loglike_batch(h, C.byref(spec), th.ctypes.data_as(dp), th.shape[0], spec.ndim, a.ctypes.data_as(dp)))
        _lib.check(lib.vag_loglike_sky_batch(h, C.byref(spec), C.byref(none), th.ctypes.data_as(dp), th.shape[0], spec.ndim,
                                             b.ctypes.data_as(dp)))
    assert np.array_equal(a, b)
    assert np.array_equal(f.loglike_batch(th, defs), a)


def test_walkers_with_no_flux_at_an_epoch_score_minus_inf():
    th, sky = _walkers(16, seed=3)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    defs = FLUX_DEFS + SKY_DEFS + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    f = _c4_fitter(True)
    assert np.all(np.isfinite(f.loglike_batch(samples, defs)))
    cd = f._centroid_obs[0]
    f.add_centroid(1e30, cd["t"], cd["east"], cd["north"], cd["err_east"], cd["err_north"])  # far above the synchrotron cut-off
    params = [f._params_at(s, defs)[0] for s in samples]
    assert np.all(batch_centroid(params, cd["t"], 1e30)[..., 0] == 0)
    out = f.loglike_batch(samples, defs)
    assert np.all(out == -np.inf)
    assert f.last_plan.n_walkers_rejected == samples.shape[0]


def test_centroid_data_break_the_angle_degeneracy():
    tr = configs.C4_TRUTH
    ratio = tr["theta_c"] / tr["theta_obs"]
    scan = tr["theta_obs"] * np.array([0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3])
    samples = np.column_stack([scan * ratio, scan])
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("pa", 0.3, 0.3, fitting.Scale.fixed), fitting.ParamDef("east0", 2e-10, 2e-10, fitting.Scale.fixed)]
    defs += _c4_fixed(skip=("theta_c", "theta_v"))
    ll_with = _c4_fitter(True).loglike_batch(samples, defs)
    ll_without = _c4_fitter(False).loglike_batch(samples, defs[:2] + defs[4:])
    print("with", ll_with, "without", ll_without)
    assert np.argmax(ll_with) == 3
    drop_with = ll_with[3] - np.delete(ll_with, 3)
    drop_without = ll_without[3] - np.delete(ll_without, 3)
    assert np.all(drop_with > drop_without), (drop_with, drop_without)  # flatter without the centroid data
    assert np.ptp(ll_with) > np.ptp(ll_without)
    cen = ll_with - ll_without  # the centroid term alone: zero at the truth, negative on either side
    assert cen[3] == 0 and np.all(np.delete(cen, 3) < 0) and cen[0] < -1.0
