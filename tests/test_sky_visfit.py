"""Visibility groups of the walker likelihood (vag_loglike_vis_batch[_dev], Fitter.add_visibilities) on the device: against host
arithmetic on vag_sky_visibility_batch, against the independent CPU checker, other emitters / passes / phi bins, a model with no flux,
calls without visibility groups, centroid and visibility groups together, bits (twice, alone / in a batch / reversed, evaluation order,
t-chunks), invalid walkers, Fitter.visibilities, and the theta_obs / theta_c degeneracy that visibilities break.

The set-up is test_sky_centroid.py's GW170817-like truth and light curve, with one visibility group at 8 GHz: three epochs of 70, 5
and 130 visibilities (more than one block of 64, less than one, an odd remainder) on baselines out to 2 pi |b| rho = 10."""
import ctypes as C
import os

import numpy as np
import pytest

import _abi
import _skycheck as sk
import _vischeck as vk
import configs
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, units

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

C4_LC_T = np.geomspace(10, 300, 8) * units.day
C4_LC_NU = 3e9
C4_CEN_T = np.array([75.0, 160.0, 230.0]) * units.day
C4_CEN_NU = 8e9
VIS_T = np.array([75.0, 160.0, 230.0]) * units.day
VIS_NU = 8e9
VIS_COUNTS = (70, 5, 130)
PA_TRUE, EAST0_TRUE = 0.3, 2e-10

FLUX_DEFS = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
             fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)]
SKY_DEFS = [fitting.ParamDef("pa", -1.0, 1.0), fitting.ParamDef("east0", -2e-9, 2e-9)]


def mom_array(sm):
    return np.stack([getattr(sm, n) for n in va.SkyMoments.names], axis=-1)


def batch_vis(params, t, nu, u, v, pa=0.0, n_az=0):
    lib = _lib.load()
    h, lock = va.get_context(0)
    nb = len(params)
    t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(np.atleast_1d(nu), float)
    arr = (_lib.ModelParams * nb)(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in params])
    u, v = np.ascontiguousarray(u, float), np.ascontiguousarray(v, float)
    out = np.empty((nb, nu.size, t.size, u.shape[-1], 2))
    with lock:
        _lib.check(lib.vag_sky_visibility_batch(h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                u.ctypes.data_as(dp), v.ctypes.data_as(dp), u.shape[-1], pa, n_az,
                                                out.ctypes.data_as(dp)))
    return out[..., 0] + 1j * out[..., 1]


def _c4_truth():
    return va.Model.from_params(_abi.make_params(**configs.C4_TRUTH))


def _c4_fitter(with_centroid=False, pa_true=PA_TRUE, east0_true=EAST0_TRUE, flux_err=0.3, pos_err=0.2 * units.mas):
    tr = configs.C4_TRUTH
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    truth = _c4_truth()
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


def make_group(model, t, nu, counts, pa, east0, seed=1, noise=0.05, sigma=0.05):
    """Data of one visibility group from `model`: baselines of _vischeck.baselines (the last counts[e] of 130 at epoch e), the
    model's own visibilities at n_az 1024 placed by pa / east0 on the host, complex Gaussian noise of `noise` F per component and
    errors of `sigma` F.  Returns flat arrays (t, u, v, vis, err) and the epoch fluxes F."""
    t = np.asarray(t, float)
    mo = mom_array(model.sky_moments(t, np.array([nu]), n_az=1024))  # (1, nt, 6)
    u, v = vk.baselines(mo, 10.0, 130, seed=1)
    V = model.sky_visibilities(t, np.array([nu]), u, v, pa=pa, n_az=1024)[0]
    F = mo[0, :, 0]
    rng = np.random.default_rng(seed)
    ts, us, vs, vis, err = [], [], [], [], []
    for e, n in enumerate(counts):
        ue, ve = u[0, e, -n:], v[0, e, -n:]
        Ve = V[e, -n:] * np.exp(-2j * np.pi * ue * east0)
        Ve = Ve + noise * F[e] * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        ts.append(np.full(n, t[e])), us.append(ue), vs.append(ve), vis.append(Ve), err.append(np.full(n, sigma * F[e]))
    return tuple(np.concatenate(a) for a in (ts, us, vs, vis, err)) + (F,)


@pytest.fixture(scope="module")
def data():
    return make_group(_c4_truth(), VIS_T, VIS_NU, VIS_COUNTS, PA_TRUE, EAST0_TRUE)


@pytest.fixture(scope="module")
def clean():
    return make_group(_c4_truth(), VIS_T, VIS_NU, VIS_COUNTS, PA_TRUE, EAST0_TRUE, noise=0.0)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return vk.build_checker(tmp_path_factory.mktemp("sky_visfit_checker"))


def add_group(f, d, nu=VIS_NU, **kw):
    t, u, v, vis, err = d[:5]
    if kw.get("kind") == "amplitude":
        vis = np.abs(vis)
    f.add_visibilities(nu, t, u, v, vis, err, **kw)
    return f


def _rect(vd):
    """The group's ragged baselines padded with zeros to [1][n_epochs][max per epoch]."""
    first, ne = vd["first"], vd["t"].size
    nbl = int(np.diff(first).max())
    u, v = np.zeros((1, ne, nbl)), np.zeros((1, ne, nbl))
    for e in range(ne):
        n = first[e + 1] - first[e]
        u[0, e, :n], v[0, e, :n] = vd["u"][first[e]:first[e + 1]], vd["v"][first[e]:first[e + 1]]
    return u, v


def host_model_vis(f, defs, sample, vd, pa, east0, vis_fn=None):
    """V_mod of one walker at the group's data, flat: vag_sky_visibility_batch (nb = 1) on the padded rectangle, times the east0 phase."""
    p = f._params_at(sample, defs)[0]
    u, v = _rect(vd)
    if vis_fn is None:
        rect = batch_vis([p], vd["t"], vd["nu"], u, v, pa=float(pa), n_az=vd["n_az"] or 0)[0, 0]
    else:
        rect = vis_fn(_abi.ModelParams.from_buffer_copy(bytes(p)), vd["t"], np.array([vd["nu"]]), u, v, float(pa), vd["n_az"] or 1024)[0]
    first = vd["first"]
    flat = np.concatenate([rect[e, :first[e + 1] - first[e]] for e in range(vd["t"].size)])
    return flat * np.exp(-2j * np.pi * vd["u"] * east0)


def host_chi2(f, defs, samples, g=0, pa_col=3, e0_col=4, vis_fn=None, parts=False):
    vd = f._vis_obs[g]
    out, res = [], []
    for s in samples:
        pa = s[pa_col] if pa_col is not None else PA_TRUE
        e0 = s[e0_col] if e0_col is not None else EAST0_TRUE
        V = host_model_vis(f, defs, s, vd, pa, e0, vis_fn)
        r = np.abs(vd["re"] - np.abs(V)) if vd["kind"] == "amplitude" else np.abs(vd["re"] + 1j * vd["im"] - V)
        out.append(np.sum(vd["weights"] * r ** 2 / vd["err"] ** 2))
        res.append(r)
    return (np.array(out), np.array(res)) if parts else np.array(out)


def _defs():
    fixed = _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    return FLUX_DEFS + fixed, FLUX_DEFS + SKY_DEFS + fixed


def _rel(got, want):
    return np.max(np.abs(got - want) / np.abs(want))


def test_likelihood_matches_host_arithmetic(data):
    """The tolerance is the centroid likelihood test's, 1e-10 relative: V agrees with vag_sky_visibility_batch to summation order
    (~1e-13 F), which moves a datum's chi^2 term by about 2 |r| / sigma 1e-13 F / sigma ~ 4e-12 at sigma = 0.05 F."""
    import torch
    th, sky = _walkers(64)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    defs_flux, defs_sky = _defs()
    f_flux = _c4_fitter()
    w = np.random.default_rng(2).uniform(0.5, 2.0, data[0].size)
    f_vis = add_group(_c4_fitter(), data, weights=w)
    assert f_vis.has_visibilities and not f_flux.has_visibilities
    ll_flux = f_flux.loglike_batch(th, defs_flux)
    chi2 = host_chi2(f_vis, defs_sky, samples)
    want = ll_flux - 0.5 * chi2
    assert np.all(np.isfinite(want)) and np.all(chi2 > 0)
    got = f_vis.loglike_batch(samples, defs_sky)
    print("complex, 64 walkers: rel", _rel(got, want), "chi2", chi2.min(), chi2.max())
    assert np.all(np.isfinite(got))
    assert _rel(got, want) <= 1e-10
    ev = f_vis.device_evaluator(defs_sky)  # device-pointer form
    vals, _ = ev(torch.from_numpy(samples).to("cuda:0"))
    torch.cuda.synchronize()
    assert _rel(vals.cpu().numpy(), want) <= 1e-10
    lp_flux = f_flux.log_prob_batch(th, defs_flux)  # with priors: the flux fit's ln prior plus the sky parameters' Uniform
    want_p = lp_flux - 0.5 * chi2 - np.log(2.0) - np.log(4e-9)
    assert _rel(f_vis.log_prob_batch(samples, defs_sky), want_p) <= 1e-10
    ev_p = f_vis.device_evaluator(defs_sky, use_priors=True)
    vals_p, _ = ev_p(torch.from_numpy(samples).to("cuda:0"))
    torch.cuda.synchronize()
    assert _rel(vals_p.cpu().numpy(), want_p) <= 1e-10


def test_amplitude_kind_and_n_az_match_host_arithmetic(data):
    th, sky = _walkers(8, seed=6)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    defs_flux, defs_sky = _defs()
    ll_flux = _c4_fitter().loglike_batch(th, defs_flux)
    chi2 = {}
    for key, kw in (("amplitude", dict(kind="amplitude")), ("n_az 64", dict(n_az=64)), ("n_az 1024", dict())):
        f = add_group(_c4_fitter(), data, **kw)
        chi2[key] = host_chi2(f, defs_sky, samples)
        want = ll_flux - 0.5 * chi2[key]
        got = f.loglike_batch(samples, defs_sky)
        print(key, "rel", _rel(got, want), "chi2", chi2[key])
        assert np.all(np.isfinite(got)) and np.all(chi2[key] > 0)
        assert _rel(got, want) <= 1e-10
        if key == "amplitude":  # east0 drops out of an amplitude fit
            moved = samples.copy()
            moved[:, 4] += 3e-10
            assert np.array_equal(f.loglike_batch(moved, defs_sky), got)
        chi2[key + " device"] = -2.0 * (got - ll_flux)
    a, b = chi2["n_az 64 device"], chi2["n_az 1024 device"]
    print("n_az 64 against 1024, relative:", np.abs(a - b) / b)
    assert np.all(np.abs(a - b) / b > 1e-7)  # the knob is read


def test_against_the_cpu_checker(data, checker):
    """The device-vs-checker visibility test allows |dV| <= 1e-6 F; propagated: |d chi^2| <= sum w (2 |r| delta + delta^2) / sigma^2
    with delta = 1e-6 F of the epoch and r the checker's residuals."""
    th, sky = _walkers(4, seed=7)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    defs_flux, defs_sky = _defs()
    f = add_group(_c4_fitter(), data, n_az=256)
    vd = f._vis_obs[0]
    chi2_ref, res = host_chi2(f, defs_sky, samples, vis_fn=checker.visibility, parts=True)
    got = -2.0 * (f.loglike_batch(samples, defs_sky) - _c4_fitter().loglike_batch(th, defs_flux))
    for q, s in enumerate(samples):
        p = _abi.ModelParams.from_buffer_copy(bytes(f._params_at(s, defs_sky)[0]))
        F = checker.moments(p, vd["t"], np.array([vd["nu"]]), 256)[0, :, 0]
        delta = 1e-6 * np.repeat(F, np.diff(vd["first"]))
        bound = np.sum(vd["weights"] * (2 * res[q] * delta + delta ** 2) / vd["err"] ** 2)
        print("walker", q, "chi2 device", got[q], "checker", chi2_ref[q], "bound", bound)
        assert np.isfinite(got[q]) and abs(got[q] - chi2_ref[q]) <= bound


def _other_emitter_case(kind):
    if kind == "fwd_ssc":  # near configs.C3: forward SSC with Klein-Nishina on a power-law jet in a wind
        f = fitting.Fitter(z=1.0, lumi_dist=1e28, jet="powerlaw", medium="wind", fwd_ssc=True, kn=True, resolution=(0.29, 0.16, 10.0))
        fixed = dict(theta_c=0.1, Gamma0=300.0, k_e=2.0, k_g=2.0, tau=1.0, A_star=0.1, n_ism=0.0, eps_e=0.1, eps_B=0.01, p=2.3)
        free = [fitting.ParamDef("theta_v", 0.0, 0.8), fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)]
        truth = np.array([0.2, 52.0])
    else:  # near rs_thin_tophat: a reverse shock seen on axis (two emitters, the single full-circle phi bin)
        f = fitting.Fitter(z=1.0, lumi_dist=1e28, jet="tophat", medium="ism", rvs_shock=True)
        fixed = dict(theta_v=0.0, Gamma0=300.0, n_ism=1.0, eps_e=0.1, eps_B=0.01, p=2.3, eps_e_r=0.1, eps_B_r=0.01, p_r=2.3)
        free = [fitting.ParamDef("theta_c", 0.02, 0.5), fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)]
        truth = np.array([0.1, 52.0])
    fixed_defs = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in fixed.items()]
    return f, free, fixed_defs, truth


@pytest.mark.parametrize("kind", ["fwd_ssc", "rvs_on_axis"])
def test_other_emitters_passes_and_bins(kind):
    f, free, fixed_defs, truth = _other_emitter_case(kind)
    defs_flux, defs_sky = free + fixed_defs, free + SKY_DEFS + fixed_defs
    t_vis, nu = np.array([1e4, 1e5, 1e6]), 1e9  # inside _skycheck.T's range
    assert sk.T[0] <= t_vis[0] and t_vis[-1] <= sk.T[-1]
    helper = _other_emitter_case(kind)[0]  # (a Fitter makes a Model once it holds data)
    helper.add_flux_density(nu, [1e5], [1.0], [1.0])
    model = helper.model(truth, defs_flux)
    lc_t = np.geomspace(3e3, 3e6, 6)
    fl = model.flux_density_grid(lc_t, nu).total[0]
    assert np.all(fl > 0)
    f.add_flux_density(nu, lc_t, fl, 0.3 * fl)
    d = make_group(model, t_vis, nu, (70, 5, 33), PA_TRUE, EAST0_TRUE, seed=3)
    assert np.all(d[5] > 0)
    rng = np.random.default_rng(8)
    th = truth + np.column_stack([truth[0] * rng.uniform(-0.1, 0.1, 8) if truth[0] else np.zeros(8), rng.uniform(-0.2, 0.2, 8)])
    samples = np.ascontiguousarray(np.column_stack([th, rng.uniform(0.0, 0.6, 8), rng.uniform(-1e-9, 1e-9, 8)]))
    ll_flux = f.loglike_batch(th, defs_flux)
    add_group(f, d, nu=nu)
    chi2 = host_chi2(f, defs_sky, samples, pa_col=2, e0_col=3)
    want = ll_flux - 0.5 * chi2
    got = f.loglike_batch(samples, defs_sky)
    print(kind, "rel", _rel(got, want), "chi2", chi2)
    assert np.all(np.isfinite(got)) and np.all(chi2 > 0)
    assert _rel(got, want) <= 1e-10


def test_no_flux_is_not_invalid(data):
    th, sky = _walkers(16, seed=3)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    _, defs_sky = _defs()
    w = np.random.default_rng(4).uniform(0.5, 2.0, data[0].size)
    f = add_group(_c4_fitter(), data)
    first_only = f.loglike_batch(samples, defs_sky)
    add_group(f, data, nu=1e30, weights=w)  # far above the synchrotron cut-off
    vd = f._vis_obs[1]
    u, v = _rect(vd)
    params = [f._params_at(s, defs_sky)[0] for s in samples]
    assert np.all(batch_vis(params, vd["t"], 1e30, u, v, pa=0.3) == 0)
    both = f.loglike_batch(samples, defs_sky)
    assert np.all(np.isfinite(both)) and np.all(np.isfinite(first_only))
    assert f.last_plan.n_walkers_rejected == 0
    term = -0.5 * np.sum(w * (vd["re"] ** 2 + vd["im"] ** 2) / vd["err"] ** 2)
    print("no-flux group: term", term, "device", both - first_only)
    assert np.max(np.abs((both - first_only) - term) / np.abs(both)) <= 1e-10


@pytest.mark.parametrize("with_centroid", [False, True])
def test_no_visibility_groups_is_bitwise_the_sky_call(with_centroid):
    th, sky = _walkers(64, seed=9)
    f = _c4_fitter(with_centroid)
    defs_flux, defs_sky = _defs()
    defs, samples = (defs_sky, np.column_stack([th, sky])) if with_centroid else (defs_flux, th)
    samples = np.ascontiguousarray(samples)
    spec, _, _ = f.build_spec(defs)
    lib = _lib.load()
    h, lock = va.get_context(0)
    nb = samples.shape[0]
    a, b, c = np.empty(nb), np.empty(nb), np.empty(nb)
    sky_spec = spec._sky if spec._sky is not None else _lib.SkyFitSpec()
    none = _lib.VisFitSpec()
    args = (samples.ctypes.data_as(dp), nb, spec.ndim)
    with lock:
        _lib.check(lib.vag_loglike_sky_batch(h, C.byref(spec), C.byref(sky_spec), *args, a.ctypes.data_as(dp)))
        _lib.check(lib.vag_loglike_vis_batch(h, C.byref(spec), C.byref(sky_spec), None, *args, b.ctypes.data_as(dp)))
        _lib.check(lib.vag_loglike_vis_batch(h, C.byref(spec), C.byref(sky_spec), C.byref(none), *args, c.ctypes.data_as(dp)))
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(f.loglike_batch(samples, defs), a)


def test_centroid_and_visibility_groups_add(data):
    th, sky = _walkers(16, seed=11)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    defs_flux, defs_sky = _defs()
    ll_flux = _c4_fitter().loglike_batch(th, defs_flux)
    ll_cen = _c4_fitter(True).loglike_batch(samples, defs_sky)
    ll_vis = add_group(_c4_fitter(), data).loglike_batch(samples, defs_sky)
    ll_both = add_group(_c4_fitter(True), data).loglike_batch(samples, defs_sky)
    assert np.all(np.isfinite(ll_both))
    err = np.abs((ll_both - ll_flux) - ((ll_cen - ll_flux) + (ll_vis - ll_flux))) / np.abs(ll_both)
    print("centroid + visibility groups: additivity", err.max())
    assert err.max() <= 1e-10


def _with_hook(name, value, fn):
    lib = _lib.load()
    os.environ[name] = value
    lib.vag_reload_env_hooks()
    try:
        return fn()
    finally:
        del os.environ[name]
        lib.vag_reload_env_hooks()


def test_bits(data):
    th, sky = _walkers(64, seed=12)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    _, defs_sky = _defs()
    f = add_group(_c4_fitter(), data)
    a = f.loglike_batch(samples, defs_sky)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, f.loglike_batch(samples, defs_sky))  # run to run (and in the evaluation order the first call left)
    alone = f.loglike_batch(samples[5:6], defs_sky)
    assert alone[0] == a[5]
    rev = f.loglike_batch(np.ascontiguousarray(samples[::-1]), defs_sky)
    assert np.array_equal(rev[::-1], a)
    assert np.array_equal(_with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(samples, defs_sky)), a)
    assert np.array_equal(_with_hook("VAG_SKY_CHUNK_T", "1", lambda: f.loglike_batch(samples, defs_sky)), a)


def test_invalid_walkers(data):
    th, sky = _walkers(16, seed=13)
    samples = np.ascontiguousarray(np.column_stack([th, sky]))
    defs_flux, defs_sky = _defs()
    f = add_group(_c4_fitter(), data)
    good = f.loglike_batch(samples, defs_sky)
    assert np.all(np.isfinite(good)) and f.last_plan.n_walkers_rejected == 0
    bad = samples.copy()
    bad[3, 0] = -0.01  # theta_c <= 0 fails vag_params_validate
    assert _c4_fitter().loglike_batch(np.ascontiguousarray(bad[:, :3]), defs_flux)[3] == -np.inf
    out = f.loglike_batch(bad, defs_sky)
    assert out[3] == -np.inf
    assert np.array_equal(np.delete(out, 3), np.delete(good, 3))
    assert f.last_plan.n_walkers_rejected == 1


def test_fitter_visibilities(data):
    tr = configs.C4_TRUTH
    _, defs_sky = _defs()
    f = add_group(_c4_fitter(), data)
    add_group(f, data, n_az=64)
    best = np.array([tr["theta_c"], tr["theta_obs"], np.log10(tr["E_iso"]), PA_TRUE, EAST0_TRUE])
    got = f.visibilities(best, defs_sky)
    assert len(got) == 2 and all(g.shape == data[0].shape and g.dtype == np.complex128 for g in got)
    model = f.model(best, defs_sky)
    F = np.repeat(data[5], VIS_COUNTS)
    for g, n_az in zip(got, (None, 64)):
        vd = f._vis_obs[0]
        u, v = _rect(vd)
        rect = model.sky_visibilities(vd["t"], np.array([VIS_NU]), u, v, pa=PA_TRUE, n_az=n_az)[0]
        want = np.concatenate([rect[e, :n] for e, n in enumerate(VIS_COUNTS)]) * np.exp(-2j * np.pi * vd["u"] * EAST0_TRUE)
        assert np.max(np.abs(g - want) / F) <= 1e-14
    assert np.max(np.abs(got[0] - got[1]) / F) > 1e-7  # the group's own n_az


def test_visibilities_break_the_angle_degeneracy(clean):
    """The scan of test_centroid_data_break_the_angle_degeneracy on noise-free visibilities: the term is 0 at the truth to rounding
    (the data come from vag_sky_visibility_kernel, the fit from vag_sky_vis_chi2_kernel) and falls off on either side.  The CPU
    checker gives -8332, -4669, -1362, 0, -1053, -2930, -4166 at n_az 64 and unit weights."""
    tr = configs.C4_TRUTH
    ratio = tr["theta_c"] / tr["theta_obs"]
    scan = tr["theta_obs"] * np.array([0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3])
    samples = np.ascontiguousarray(np.column_stack([scan * ratio, scan]))
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("pa", PA_TRUE, PA_TRUE, fitting.Scale.fixed), fitting.ParamDef("east0", EAST0_TRUE, EAST0_TRUE, fitting.Scale.fixed)]
    defs += _c4_fixed(skip=("theta_c", "theta_v"))
    ll_with = add_group(_c4_fitter(), clean).loglike_batch(samples, defs)
    ll_without = _c4_fitter().loglike_batch(samples, defs[:2] + defs[4:])
    term = ll_with - ll_without
    print("visibility term over the scan:", term)
    assert np.argmax(term) == 3 and abs(term[3]) <= 1e-9
    assert np.all(term <= 0)
    assert np.all(np.diff(term[:4]) > 0) and np.all(np.diff(term[3:]) < 0)
    assert np.all(np.delete(term, 3) < -1.0)
