"""Polarization groups of the walker likelihood (vag_loglike_pol_batch[_dev], Fitter.add_polarization) on the device: against host
arithmetic on vag_sky_polarization_batch, against the independent CPU checker, other emitters, bits (twice, alone / in a batch /
reversed, evaluation order, t-chunks), calls without polarization groups, all three kinds of sky groups together, invalid walkers,
Fitter.polarization, and the scans over the field anisotropy and the viewing geometry that polarimetry constrains.

The set-up is test_sky_visfit.py's GW170817-like truth and light curve at 3 GHz, with one polarization group at 3 GHz, t = 75, 160,
230, 400 d, truth b = 0.5 and pa = 0.3, Gaussian noise of 0.01 on q and u with sigma = 0.01, and non-uniform weights."""
import ctypes as C

import numpy as np
import pytest

import _abi
import _polcheck as pk
import configs
import test_sky_visfit as tv
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, units

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

POL_T = np.array([75.0, 160.0, 230.0, 400.0]) * units.day
POL_NU = 3e9
B_TRUE, PA_TRUE, SIGMA = 0.5, 0.3, 0.01
DELTA = 2e-6  # the checker bound: test_sky_polarization.test_against_the_checker allows 1e-6 on |dQ| / I and on |dI| / I, |q| <= 1

FLUX_DEFS = tv.FLUX_DEFS
POL_DEFS = [fitting.ParamDef("pa", -1.0, 1.0), fitting.ParamDef("pol_b", 0.0, 3.0)]
_c4_fitter, _c4_fixed, _rel, _with_hook = tv._c4_fitter, tv._c4_fixed, tv._rel, tv._with_hook


def batch_pol(p, t, nu, spec, pa, n_az):
    """vag_sky_polarization_batch of one model: I, Q, U on the sky, each [nt]."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray([nu], float)
    arr = (_lib.ModelParams * 1)(_lib.ModelParams.from_buffer_copy(bytes(p)))
    sp = (_lib.PolSpec * 1)(_lib.PolSpec.from_buffer_copy(bytes(spec)))
    out = np.empty((1, 1, t.size, 3))
    with lock:
        _lib.check(lib.vag_sky_polarization_batch(h, arr, 1, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), 1, sp, float(pa),
                                                  int(n_az or 0), out.ctypes.data_as(dp)))
    return out[0, 0, :, 0], out[0, 0, :, 1], out[0, 0, :, 2]


def make_group(model, t=POL_T, nu=POL_NU, b=B_TRUE, pa=PA_TRUE, noise=SIGMA, seed=1, **kw):
    """Data of one polarization group from `model`: its own q, u (Model.sky_polarization) plus Gaussian noise, errors SIGMA."""
    r = model.sky_polarization(t, nu, b=b, pa=pa, **kw)
    assert np.all(r.I > 0)
    rng = np.random.default_rng(seed)
    q, u = r.Q / r.I + noise * rng.standard_normal(t.size), r.U / r.I + noise * rng.standard_normal(t.size)
    return dict(nu=nu, t=np.asarray(t, float), q=q, u=u, err=np.full(t.size, SIGMA))


def add_group(f, d, kind="qu", **kw):
    if kind == "degree":
        f.add_polarization(d["nu"], d["t"], np.hypot(d["q"], d["u"]), err_q=d["err"], kind="degree", **kw)
    else:
        f.add_polarization(d["nu"], d["t"], d["q"], d["u"], d["err"], 1.5 * d["err"], **kw)
    return f


@pytest.fixture(scope="module")
def data():
    return make_group(tv._c4_truth())


@pytest.fixture(scope="module")
def clean():
    return make_group(tv._c4_truth(), noise=0.0)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return pk.build_checker(tmp_path_factory.mktemp("sky_polfit_checker"))


def _field(s, cols, fixed):
    """pa and the keywords of _polcheck.spec of one walker: `cols` names the sample's columns, `fixed` the other values."""
    v = dict(pa=0.0, b=0.0, pi_max=None, b_rvs=None, pi_max_rvs=None)
    v.update(fixed)
    v.update({k: s[c] for k, c in cols.items()})
    return v.pop("pa"), v


def host_chi2(f, defs, samples, cols, fixed=None, g=0, stokes_fn=None, parts=False):
    """chi^2 of group g formed here from vag_sky_polarization_batch (nb = 1 per walker) or from stokes_fn(p, t, nu, n_az, pa, **spec);
    with parts also the absolute residuals [walker][2][epoch] (q, u; for a degree group the degree and zeros)."""
    pd = f._pol_obs[g]
    w, out, res = pd["weights"], [], []
    for s in samples:
        pa, kw = _field(s, cols, fixed or {})
        p = f._params_at(s, defs)[0]
        if stokes_fn is None:
            I, Q, U = batch_pol(p, pd["t"], pd["nu"], pk.spec(**kw), pa, pd["n_az"])
        else:
            I, Q, U = (a[0] for a in stokes_fn(_abi.ModelParams.from_buffer_copy(bytes(p)), pd["t"], np.array([pd["nu"]]),
                                                pd["n_az"] or 256, pa=float(pa), **kw))
        if pd["kind"] == "degree":
            rq, ru = np.abs(pd["q"] - np.hypot(Q, U) / I), np.zeros_like(I)
            out.append(np.sum(w * (rq / pd["err_q"]) ** 2))
        else:
            rq, ru = np.abs(pd["q"] - Q / I), np.abs(pd["u"] - U / I)
            out.append(np.sum(w * ((rq / pd["err_q"]) ** 2 + (ru / pd["err_u"]) ** 2)))
        res.append((rq, ru))
    return (np.array(out), np.array(res)) if parts else np.array(out)


def checker_bound(pd, res):
    """|d chi^2| <= sum w (2 |r| delta + delta^2) / sigma^2 over q and u, r the checker's residuals (a degree group: the degree)."""
    eu = pd["err_u"] if pd["err_u"] is not None else np.full_like(pd["err_q"], np.inf)
    return np.sum(pd["weights"] * ((2 * res[0] * DELTA + DELTA ** 2) / pd["err_q"] ** 2 + (2 * res[1] * DELTA + DELTA ** 2) / eu ** 2))


def _walkers(nb, seed=5):
    th, _ = tv._walkers(nb, seed)
    rng = np.random.default_rng(seed + 100)
    return th, np.column_stack([rng.uniform(0.0, 0.6, nb), rng.uniform(0.2, 0.8, nb)])


def _defs(extra=POL_DEFS, skip=()):
    fixed = _c4_fixed(skip=("theta_c", "theta_v", "E_iso") + tuple(skip))
    return FLUX_DEFS + fixed, FLUX_DEFS + list(extra) + fixed


COLS = dict(pa=3, b=4)


def test_likelihood_matches_host_arithmetic(data):
    """1e-10 relative, the tolerance of the centroid and visibility likelihood tests: the model I, Q, U are the bits of
    vag_sky_polarization_batch, so only the turn by 2 pa and the residual arithmetic differ (a few ulp of q)."""
    import torch
    th, pol = _walkers(64)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    defs_flux, defs_pol = _defs()
    f_flux = _c4_fitter()
    w = np.random.default_rng(2).uniform(0.5, 2.0, POL_T.size)
    f_pol = add_group(_c4_fitter(), data, weights=w)
    assert f_pol.has_polarization and not f_flux.has_polarization
    ll_flux = f_flux.loglike_batch(th, defs_flux)
    chi2 = host_chi2(f_pol, defs_pol, samples, COLS)
    want = ll_flux - 0.5 * chi2
    assert np.all(np.isfinite(want)) and np.all(chi2 > 0)
    got = f_pol.loglike_batch(samples, defs_pol)
    print("qu, 64 walkers: rel", _rel(got, want), "chi2", chi2.min(), chi2.max())
    assert np.all(np.isfinite(got)) and f_pol.last_plan.n_walkers_rejected == 0
    assert _rel(got, want) <= 1e-10
    ev = f_pol.device_evaluator(defs_pol)  # device-pointer form
    assert ev.has_polarization and not ev.has_visibilities and not ev.has_centroids
    vals, _ = ev(torch.from_numpy(samples).to("cuda:0"))
    torch.cuda.synchronize()
    assert _rel(vals.cpu().numpy(), want) <= 1e-10
    lp_flux = f_flux.log_prob_batch(th, defs_flux)  # with priors: the flux fit's ln prior plus Uniform(-1, 1) and Uniform(0, 3)
    want_p = lp_flux - 0.5 * chi2 - np.log(2.0) - np.log(3.0)
    assert _rel(f_pol.log_prob_batch(samples, defs_pol), want_p) <= 1e-10
    ev_p = f_pol.device_evaluator(defs_pol, use_priors=True)
    vals_p, _ = ev_p(torch.from_numpy(samples).to("cuda:0"))
    torch.cuda.synchronize()
    assert _rel(vals_p.cpu().numpy(), want_p) <= 1e-10


def test_degree_kind_and_n_az_match_host_arithmetic(data):
    th, pol = _walkers(8, seed=6)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    defs_flux, defs_pol = _defs()
    ll_flux = _c4_fitter().loglike_batch(th, defs_flux)
    w = np.array([1.0, 0.5, 2.0, 1.5])
    chi2 = {}
    for key, kw in (("degree", dict(kind="degree")), ("n_az 64", dict(n_az=64)), ("n_az 256", dict())):
        f = add_group(_c4_fitter(), data, weights=w, **kw)
        chi2[key] = host_chi2(f, defs_pol, samples, COLS)
        want = ll_flux - 0.5 * chi2[key]
        got = f.loglike_batch(samples, defs_pol)
        print(key, "rel", _rel(got, want), "chi2", chi2[key])
        assert np.all(np.isfinite(got)) and np.all(chi2[key] > 0)
        assert _rel(got, want) <= 1e-10
        if key == "degree":  # pa drops out of a degree fit
            moved = samples.copy()
            moved[:, 3] += 0.37
            assert np.array_equal(f.loglike_batch(moved, defs_pol), got)
        chi2[key + " device"] = -2.0 * (got - ll_flux)
    a, b = chi2["n_az 64 device"], chi2["n_az 256 device"]
    print("n_az 64 against 256, relative:", np.abs(a - b) / b)
    assert np.all(np.abs(a - b) / b > 1e-9)  # the knob is read


def test_free_p_moves_the_default_pi_max(data):
    """pol_pi_max not given: (p + 1) / (p + 7/3) with the walker's own p; fixed at 0.7 the same walkers give another value."""
    th, pol = _walkers(8, seed=7)
    rng = np.random.default_rng(17)
    p_col = configs.C4_TRUTH["p"] + rng.uniform(-0.1, 0.3, 8)
    extra = [fitting.ParamDef("p", 2.01, 2.9)] + POL_DEFS
    defs_flux, defs_pol = _defs(extra=extra, skip=("p",))
    defs_flux = defs_flux[:3] + [extra[0]] + defs_flux[3:]
    th_p = np.ascontiguousarray(np.column_stack([th, p_col]))
    samples = np.ascontiguousarray(np.column_stack([th_p, pol]))
    cols = dict(pa=4, b=5)
    ll_flux = _c4_fitter().loglike_batch(th_p, defs_flux)
    f = add_group(_c4_fitter(), data, weights=[1.0, 0.5, 2.0, 1.5])
    chi2 = host_chi2(f, defs_pol, samples, cols)  # pi_max = -1 in the spec: from the p of the walker's own parameters
    got = f.loglike_batch(samples, defs_pol)
    print("free p: rel", _rel(got, ll_flux - 0.5 * chi2))
    assert np.all(np.isfinite(got)) and _rel(got, ll_flux - 0.5 * chi2) <= 1e-10
    by_hand = np.array([host_chi2(f, defs_pol, s[None], cols, fixed=dict(pi_max=(s[3] + 1) / (s[3] + 7.0 / 3.0)))[0] for s in samples])
    assert _rel(by_hand, chi2) <= 1e-12  # the default is the walker's own (p + 1) / (p + 7/3)
    defs_07 = defs_pol + [fitting.ParamDef("pol_pi_max", 0.7, 0.7, fitting.Scale.fixed)]
    chi2_07 = host_chi2(f, defs_07, samples, cols, fixed=dict(pi_max=0.7))
    got_07 = f.loglike_batch(samples, defs_07)
    assert _rel(got_07, ll_flux - 0.5 * chi2_07) <= 1e-10
    assert np.all(np.abs(got_07 - got) > 1e-6 * np.abs(got))


def test_against_the_cpu_checker(data, checker):
    """|d chi^2| <= sum w (2 |r| delta + delta^2) / sigma^2 summed over q and u, with delta = 2e-6: the device-vs-checker test of
    Model.sky_polarization allows 1e-6 on |dQ| / I and 1e-6 on |dI| / I, and |q| <= 1; r are the checker's residuals."""
    th, pol = _walkers(4, seed=8)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    defs_flux, defs_pol = _defs()
    f = add_group(_c4_fitter(), data, weights=[1.0, 0.5, 2.0, 1.5])
    pd = f._pol_obs[0]
    chi2_ref, res = host_chi2(f, defs_pol, samples, COLS, stokes_fn=checker.polarization, parts=True)
    got = -2.0 * (f.loglike_batch(samples, defs_pol) - _c4_fitter().loglike_batch(th, defs_flux))
    for k in range(4):
        bound = checker_bound(pd, res[k])
        print("walker", k, "chi2 device", got[k], "checker", chi2_ref[k], "bound", bound)
        assert np.isfinite(got[k]) and abs(got[k] - chi2_ref[k]) <= bound


@pytest.mark.parametrize("kind", ["fwd_ssc", "rvs_off_axis"])
def test_other_emitters(kind):
    """test_sky_visfit's other emitters: forward SSC + KN on a power-law jet in a wind (an unpolarized pass), and a reverse shock,
    moved off axis (theta_v = 0.15, test_sky_polarization's h_rs_offaxis) so that q != 0, with its own free pol_b_rvs."""
    f, free, fixed_defs, truth = tv._other_emitter_case("fwd_ssc" if kind == "fwd_ssc" else "rvs_on_axis")
    helper = tv._other_emitter_case("fwd_ssc" if kind == "fwd_ssc" else "rvs_on_axis")[0]
    rvs = kind != "fwd_ssc"
    if rvs:
        fixed_defs = [fitting.ParamDef("theta_v", 0.15, 0.15, fitting.Scale.fixed) if d.name == "theta_v" else d for d in fixed_defs]
    pol_defs = POL_DEFS + ([fitting.ParamDef("pol_b_rvs", 0.0, 3.0)] if rvs else [])
    defs_flux, defs_pol = free + fixed_defs, free + pol_defs + fixed_defs
    t_pol, nu = np.array([1e4, 1e5, 1e6]), 1e9
    helper.add_flux_density(nu, [1e5], [1.0], [1.0])
    model = helper.model(truth, defs_flux)
    lc_t = np.geomspace(3e3, 3e6, 6)
    fl = model.flux_density_grid(lc_t, nu).total[0]
    assert np.all(fl > 0)
    f.add_flux_density(nu, lc_t, fl, 0.3 * fl)
    d = make_group(model, t_pol, nu, b=0.5, pa=PA_TRUE, seed=3, **(dict(b_rvs=1.7) if rvs else {}))
    truth_q = model.sky_polarization(t_pol, nu, b=0.5, pa=PA_TRUE, **(dict(b_rvs=1.7) if rvs else {}))
    assert np.any(np.abs(truth_q.Q / truth_q.I) > 1e-4)  # q != 0: there is polarization to fit
    rng = np.random.default_rng(8)
    th = truth + np.column_stack([truth[0] * rng.uniform(-0.1, 0.1, 8), rng.uniform(-0.2, 0.2, 8)])
    cols_v = [rng.uniform(0.0, 0.6, 8), rng.uniform(0.2, 0.8, 8)] + ([rng.uniform(1.2, 2.2, 8)] if rvs else [])
    samples = np.ascontiguousarray(np.column_stack([th] + cols_v))
    cols = dict(pa=2, b=3, **(dict(b_rvs=4) if rvs else {}))
    ll_flux = f.loglike_batch(th, defs_flux)
    add_group(f, d, weights=[1.0, 0.5, 2.0])
    chi2 = host_chi2(f, defs_pol, samples, cols)
    want = ll_flux - 0.5 * chi2
    got = f.loglike_batch(samples, defs_pol)
    print(kind, "rel", _rel(got, want), "chi2", chi2)
    assert np.all(np.isfinite(got)) and np.all(chi2 > 0)
    assert _rel(got, want) <= 1e-10
    if rvs:  # the reverse shock's own b is read: following the forward b gives another value
        follow = host_chi2(f, defs_pol, samples, dict(pa=2, b=3))
        assert np.all(np.abs(follow - chi2) > 1e-9 * chi2)


def test_bits(data):
    th, pol = _walkers(64, seed=12)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    _, defs_pol = _defs()
    f = add_group(_c4_fitter(), data)
    a = f.loglike_batch(samples, defs_pol)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, f.loglike_batch(samples, defs_pol))  # run to run (and in the evaluation order the first call left)
    alone = f.loglike_batch(samples[5:6], defs_pol)
    assert alone[0] == a[5]
    rev = f.loglike_batch(np.ascontiguousarray(samples[::-1]), defs_pol)
    assert np.array_equal(rev[::-1], a)
    assert np.array_equal(_with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(samples, defs_pol)), a)
    assert np.array_equal(_with_hook("VAG_SKY_CHUNK_T", "1", lambda: f.loglike_batch(samples, defs_pol)), a)


@pytest.mark.parametrize("with_centroid", [False, True])
def test_no_polarization_groups_is_bitwise_the_vis_call(with_centroid):
    th, sky = tv._walkers(64, seed=9)
    f = _c4_fitter(with_centroid)
    defs_flux, defs_sky = tv._defs()
    defs, samples = (defs_sky, np.column_stack([th, sky])) if with_centroid else (defs_flux, th)
    samples = np.ascontiguousarray(samples)
    spec, _, _ = f.build_spec(defs)
    lib = _lib.load()
    h, lock = va.get_context(0)
    nb = samples.shape[0]
    a, b, c = np.empty(nb), np.empty(nb), np.empty(nb)
    sky_spec = spec._sky if spec._sky is not None else _lib.SkyFitSpec()
    none = _lib.PolFitSpec()
    args = (samples.ctypes.data_as(dp), nb, spec.ndim)
    with lock:
        _lib.check(lib.vag_loglike_vis_batch(h, C.byref(spec), C.byref(sky_spec), None, *args, a.ctypes.data_as(dp)))
        _lib.check(lib.vag_loglike_pol_batch(h, C.byref(spec), C.byref(sky_spec), None, None, *args, b.ctypes.data_as(dp)))
        _lib.check(lib.vag_loglike_pol_batch(h, C.byref(spec), C.byref(sky_spec), None, C.byref(none), *args, c.ctypes.data_as(dp)))
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(f.loglike_batch(samples, defs), a)


def test_centroid_visibility_and_polarization_groups_add(data):
    th, sky = tv._walkers(16, seed=11)
    pol_b = np.random.default_rng(21).uniform(0.2, 0.8, 16)
    samples = np.ascontiguousarray(np.column_stack([th, sky, pol_b]))  # theta_c, theta_v, E_iso, pa, east0, pol_b
    fixed = _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    defs_flux, defs_sky = tv._defs()
    defs_all = FLUX_DEFS + tv.SKY_DEFS + [POL_DEFS[1]] + fixed
    defs_pol = FLUX_DEFS + POL_DEFS + fixed
    vis = tv.make_group(tv._c4_truth(), tv.VIS_T, tv.VIS_NU, (70, 5, 33), tv.PA_TRUE, tv.EAST0_TRUE)
    sky_samples = np.ascontiguousarray(samples[:, :5])
    ll_flux = _c4_fitter().loglike_batch(th, defs_flux)
    ll_cen = _c4_fitter(True).loglike_batch(sky_samples, defs_sky)
    ll_vis = tv.add_group(_c4_fitter(), vis, n_az=64).loglike_batch(sky_samples, defs_sky)
    ll_pol = add_group(_c4_fitter(), data).loglike_batch(np.ascontiguousarray(samples[:, [0, 1, 2, 3, 5]]), defs_pol)
    ll_all = add_group(tv.add_group(_c4_fitter(True), vis, n_az=64), data).loglike_batch(samples, defs_all)
    assert np.all(np.isfinite(ll_all))
    err = np.abs((ll_all - ll_flux) - ((ll_cen - ll_flux) + (ll_vis - ll_flux) + (ll_pol - ll_flux))) / np.abs(ll_all)
    print("centroid + visibility + polarization groups: additivity", err.max())
    assert err.max() <= 1e-10


def test_invalid_walkers(data):
    th, pol = _walkers(16, seed=13)
    extra = POL_DEFS + [fitting.ParamDef("pol_pi_max", 0.1, 1.0)]
    samples = np.ascontiguousarray(np.column_stack([th, pol, np.full(16, 0.7)]))
    defs_flux, defs_pol = _defs(extra=extra)
    f = add_group(_c4_fitter(), data)
    good = f.loglike_batch(samples, defs_pol)
    assert np.all(np.isfinite(good)) and f.last_plan.n_walkers_rejected == 0
    bad = samples.copy()
    bad[2, 4] = -0.1   # pol_b < 0
    bad[7, 5] = 1.01   # a free pol_pi_max > 1
    bad[11, 0] = -0.01  # theta_c <= 0 fails vag_params_validate
    out = f.loglike_batch(bad, defs_pol)
    assert np.all(out[[2, 7, 11]] == -np.inf)
    assert np.array_equal(np.delete(out, [2, 7, 11]), np.delete(good, [2, 7, 11]))  # the other walkers keep their bits
    assert f.last_plan.n_walkers_rejected == 3


def test_no_flux_is_invalid(data):
    """A group far above the synchrotron cut-off: I = 0 at every epoch, q is undefined, every walker scores -inf -- the centroid
    groups' F <= 0 rule, unlike a visibility group, for which a model with no flux is valid (V = 0 is a prediction).  A walker scored
    -inf is a rejected walker (n_walkers_rejected counts the walkers scored -inf, as test_sky_centroid.py holds for F = 0)."""
    th, pol = _walkers(16, seed=3)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    _, defs_pol = _defs()
    f = add_group(_c4_fitter(), data)
    first_only = f.loglike_batch(samples, defs_pol)
    assert np.all(np.isfinite(first_only)) and f.last_plan.n_walkers_rejected == 0
    add_group(f, dict(data, nu=1e30))
    p = f._params_at(samples[0], defs_pol)[0]
    I, Q, U = batch_pol(p, POL_T, 1e30, pk.spec(b=0.5), 0.3, 0)
    assert np.all(I == 0) and np.all(Q == 0) and np.all(U == 0)
    out = f.loglike_batch(samples, defs_pol)
    assert np.all(out == -np.inf)
    assert f.last_plan.n_walkers_rejected == samples.shape[0]


def test_fitter_polarization(data):
    tr = configs.C4_TRUTH
    _, defs_pol = _defs()
    f = add_group(_c4_fitter(), data)
    add_group(f, data, n_az=64)
    best = np.array([tr["theta_c"], tr["theta_obs"], np.log10(tr["E_iso"]), PA_TRUE, B_TRUE])
    got = f.polarization(best, defs_pol)
    assert len(got) == 2 and all(isinstance(g, va.SkyPolarization) and g.I.shape == POL_T.shape for g in got)
    model = f.model(best, defs_pol)
    for g, n_az in zip(got, (None, 64)):
        want = model.sky_polarization(POL_T, POL_NU, b=B_TRUE, pa=PA_TRUE, n_az=n_az)
        for x in ("I", "Q", "U"):
            assert np.max(np.abs(getattr(g, x) - getattr(want, x)) / want.I) <= 1e-14
    assert np.max(np.abs(got[0].Q - got[1].Q) / got[0].I) > 1e-12  # the group's own n_az
    defs_fixed = FLUX_DEFS + [fitting.ParamDef("pa", 0.1, 0.1, fitting.Scale.fixed), fitting.ParamDef("pol_b", 2.0, 2.0, fitting.Scale.fixed),
                              fitting.ParamDef("pol_pi_max", 0.6, 0.6, fitting.Scale.fixed)] + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    got = f.polarization(best[:3], defs_fixed)[0]
    want = model.sky_polarization(POL_T, POL_NU, b=2.0, pi_max=0.6, pa=0.1)
    assert np.max(np.abs(got.Q - want.Q) / want.I) <= 1e-14 and np.max(np.abs(got.U - want.U) / want.I) <= 1e-14


# sum [(dq)^2 + (du)^2] / sigma^2 of the CPU checker against its own b = 0.5 truth (n_az 256, pa 0.3, sigma 0.01, unit weights)
CHECKER_B_SCAN = {0.2: 1033.5, 0.35: 212.4, 0.45: 20.93, 0.5: 0.0, 0.55: 18.71, 0.65: 151.4, 0.8: 522.1}
CHECKER_FACTOR_SCAN = {0.7: 186.5, 0.8: 82.71, 0.9: 18.34, 1.0: 0.0, 1.1: 10.60, 1.2: 31.81, 1.3: 54.14}


def _listed(value, listed):
    """`value` rounds to the figure as listed (four significant digits, at least one decimal)."""
    if listed == 0:
        return value == 0
    digits = max(1, 3 - int(np.floor(np.log10(listed))))
    return abs(value - listed) <= 0.5001 * 10.0 ** -digits


@pytest.mark.parametrize("scan", ["b", "factor"])
def test_polarization_constrains_the_field_and_the_geometry(scan, clean, checker):
    """Noise-free data of the truth (b = 0.5, pa 0.3 fixed, unit weights, sigma = 0.01): the polarization term ll_with - ll_without
    is 0 at the truth to 1e-9, negative elsewhere and strictly monotone on each side, over the anisotropy b and over a common
    factor on (theta_c, theta_v) -- the direction the light curve cannot tell.  The CPU checker's chi^2 against its own truth:

        b        0.2     0.35    0.45    0.5   0.55    0.65    0.8
        chi^2    1033.5  212.4   20.93   0     18.71   151.4   522.1
        factor   0.7     0.8     0.9     1.0   1.1     1.2     1.3
        chi^2    186.5   82.71   18.34   0     10.60   31.81   54.14

    Each device term is -1/2 of the checker's chi^2 within the bound of test_against_the_cpu_checker.  The checker's chi^2 is formed
    here in full precision (the listed figures are rounded to four digits, coarser than the bound) and must round to the list."""
    tr = configs.C4_TRUTH
    listed = CHECKER_B_SCAN if scan == "b" else CHECKER_FACTOR_SCAN
    x = np.array(list(listed))
    if scan == "b":
        samples = np.column_stack([np.full(7, tr["theta_c"]), np.full(7, tr["theta_obs"]), x])
    else:
        samples = np.column_stack([tr["theta_c"] * x, tr["theta_obs"] * x, np.full(7, B_TRUE)])
    samples = np.ascontiguousarray(samples)
    free = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8)]
    fixed = _c4_fixed(skip=("theta_c", "theta_v"))
    defs = free + [fitting.ParamDef("pol_b", 0.0, 3.0), fitting.ParamDef("pa", PA_TRUE, PA_TRUE, fitting.Scale.fixed)] + fixed
    f = _c4_fitter()
    f.add_polarization(POL_NU, POL_T, clean["q"], clean["u"], clean["err"], clean["err"])
    ll_with = f.loglike_batch(samples, defs)
    ll_without = _c4_fitter().loglike_batch(np.ascontiguousarray(samples[:, :2]), free + fixed)
    term = ll_with - ll_without
    print(scan, "scan, polarization term:", term)
    assert np.argmax(term) == 3 and abs(term[3]) <= 1e-9
    assert np.all(np.delete(term, 3) < 0)
    assert np.all(np.diff(term[:4]) > 0) and np.all(np.diff(term[3:]) < 0)
    # the checker against its own truth
    p_true = _abi.ModelParams.from_buffer_copy(bytes(f._params_at(samples[3], defs)[0]))
    I0, Q0, U0 = (a[0] for a in checker.polarization(p_true, POL_T, np.array([POL_NU]), 256, pa=PA_TRUE, b=B_TRUE))
    ref = _c4_fitter()
    ref.add_polarization(POL_NU, POL_T, Q0 / I0, U0 / I0, clean["err"], clean["err"])
    chi2_ref, res = host_chi2(ref, defs, samples, dict(b=2), fixed=dict(pa=PA_TRUE), stokes_fn=checker.polarization, parts=True)
    for k in range(7):
        bound = checker_bound(ref._pol_obs[0], res[k])
        print(scan, x[k], "device", -2 * term[k], "checker", chi2_ref[k], "listed", listed[x[k]], "bound", bound)
        assert _listed(chi2_ref[k], listed[x[k]])
        assert abs(-2 * term[k] - chi2_ref[k]) <= bound
