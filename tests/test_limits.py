"""Upper limits (non-detections) in the walker likelihood (vag_loglike_lim_batch[_dev], the ``upper_limit`` keyword of the Fitter's
add_* methods) on the device: the accuracy of vag::log_ndtr, the arithmetic against the formula on the device's own model values
(point rows, a band group, a polarization-degree group), the CPU checker, bits, behaviour at the edges, and a fit.

The point data are the C4 problem (3 bands x 20 epochs, configs.c4_mock_data): the device's own truth with 5 % Gaussian noise and
10 % errors.  LIMIT_ROWS (15 of the 60 rows, every fourth) become upper limits with sigma = 0.1 F_truth and L = F_truth + z sigma,
z from -6 to +4 at the truth, and random weights.  The numpy statement of the term is tests/test_limits_host.py's."""
import ctypes as C

import numpy as np
import pytest

import _abi
import _mathref as R
import _polcheck as pk
import configs
import test_limits_host as th_
import test_sky_polfit as tp
import test_sky_visfit as tv
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)

FLUX_DEFS, _c4_fixed, _rel = tv.FLUX_DEFS, tv._c4_fixed, tv._rel
LIMIT_ROWS = np.arange(1, 60, 4)  # 15 rows over all epochs and bands
Z_TRUE = np.linspace(-6.0, 4.0, LIMIT_ROWS.size)


def defs():
    return FLUX_DEFS + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))


def device_series(params, t, nu):
    """vag_flux_density_batch: the device's model fluxes of the (t, nu) series, [nb][n]."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    arr = (_lib.ModelParams * len(params))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in params])
    t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
    out = np.empty((len(params), t.size))
    with lock:
        _lib.check(lib.vag_flux_density_batch(h, arr, len(params), t.ctypes.data_as(dp), nu.ctypes.data_as(dp), t.size,
                                              out.ctypes.data_as(dp)))
    return out


@pytest.fixture(scope="module")
def c4():
    """t, nu (sorted), the device's truth, the noisy detections, errors, and the limit rows' L, sigma, weights."""
    t, nu = configs.c4_mock_data()
    truth = device_series([_abi.make_params(**configs.C4_TRUTH)], t, nu)[0]
    assert np.all(truth > 0)
    rng = np.random.default_rng(42)
    obs = truth * (1 + 0.05 * rng.standard_normal(t.size))
    err = 0.1 * truth
    lim = np.zeros(t.size, dtype=bool)
    lim[LIMIT_ROWS] = True
    L = np.where(lim, 0.0, obs)
    L[LIMIT_ROWS] = truth[LIMIT_ROWS] + Z_TRUE * err[LIMIT_ROWS]
    w = np.ones(t.size)
    w[LIMIT_ROWS] = rng.uniform(0.5, 2.0, LIMIT_ROWS.size)
    assert np.all(L >= 0)
    return dict(t=t, nu=nu, truth=truth, obs=obs, err=err, lim=lim, value=L, w=w)


def c4_fitter(c4, limits=True, rows=None, value=None, err=None, as_detections=False):
    """The C4 fitter: with its limit rows (limits=True), or the detections alone (limits=False: the 45 other rows); `rows` selects
    rows, `value` / `err` replace the data, as_detections adds every row (the limit rows' noisy data too) as a detection."""
    tr = configs.C4_TRUTH
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    value = c4["value"] if value is None else value
    err = c4["err"] if err is None else err
    keep = np.ones(60, dtype=bool) if rows is None else rows
    if as_detections:
        f.add_flux_density(c4["nu"], c4["t"], c4["obs"], err)
        return f
    if not limits:
        keep = keep & ~c4["lim"]
    f.add_flux_density(c4["nu"][keep], c4["t"][keep], value[keep], err[keep], weights=c4["w"][keep],
                       upper_limit=c4["lim"][keep] if limits else None)
    return f


def formula(f, F):
    """ln L of the fitter's consolidated point rows on model fluxes F [nb][n]."""
    f._consolidate_data()
    if f._all_lim is None:
        return th_.detection_lnl(f._all_log_flux, F, f._all_log_err, f._all_weights)
    return th_.mixed_lnl(f._all_lim["kind"], f._all_log_flux, f._all_log_err, f._all_lim["limit"], f._all_lim["sigma"],
                         f._all_weights, F)


def walker_fluxes(f, samples, d):
    f._consolidate_data()
    return device_series([f._params_at(s, d)[0] for s in samples], f._all_t, f._all_nu)


# ---------------------------------------------------------------- 1. log_ndtr
# measured on an MI355X: 1.293e-14 over the dense sweep (at z near 10, the z^2 amplification), 8.5e-15 over the +-k ulp points, 1.9e-16
# over the tail sweep; the gate is 4 x the maximum
LOG_NDTR_GATE = 5.2e-14


@pytest.fixture(scope="module")
def math_dev():
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def run(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.full(x.shape[0], np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, _lib.MATH["log_ndtr"], x.ctypes.data_as(dp), x.shape[0], out.ctypes.data_as(dp)))
        return out
    yield run
    lib.vag_ctx_destroy(ctx)


def log_ndtr_ref(z):
    """ln Phi(z) at 40 digits: log(erfc(-z / sqrt 2) / 2) (mpmath keeps erfc's full relative accuracy in the tail)."""
    mp = R.mpmath
    with mp.workdps(40):
        return np.array([mp.log(mp.erfc(-mp.mpf(float(v)) / mp.sqrt(2)) / 2) for v in z], dtype=object)


def log_ndtr_rel_err(got, z):
    mp = R.mpmath
    ref = log_ndtr_ref(z)
    with mp.workdps(40):
        return np.array([float(abs((mp.mpf(float(g)) - r) / r)) for g, r in zip(got, ref)])


def test_log_ndtr_accuracy(math_dev):
    """Relative error of ln Phi against mpmath at 40 digits over a dense sweep of z in [-40, 10] (20001 points), the points +-k ulp
    (k <= 4) around -38, -1, 0, 1 and 8.3, and a log sweep of -z from 40 to 1e150 (2001 points).  Expected from the form: the
    library's erfcx / erfc / log / log1p (a few ulp) and, for z > 0, z^2 x 1.6e-16 from the rounding of z / sqrt 2 (1.6e-14 at
    z = 10).  Measured on an MI355X: 1.293e-14 (dense sweep; 8.5e-15 at the ulp points, 1.9e-16 in the tail); gate: 4 x that,
    5.2e-14 (LOG_NDTR_GATE; also in profiles/HISTORY.md).  A measured value above 1e-12 would mean the form is wrong.  The values
    must be finite everywhere and strictly increasing along both sweeps (the reference is, over the whole range); the +-k ulp
    neighbours are held to the accuracy gate only: their true values differ by less than the result's rounding."""
    dense = np.linspace(-40.0, 10.0, 20001)
    near = np.array([np_nudge(c, k) for c in (-38.0, -1.0, 0.0, 1.0, 8.3) for k in range(-4, 5)])
    tail = -np.geomspace(40.0, 1e150, 2001)
    worst = {}
    for name, z in (("dense", dense), ("ulp", near), ("tail", tail)):
        y = math_dev(z)
        assert np.all(np.isfinite(y)), name
        assert not np.any((z < 0) & (y >= 0)), name  # never +0 (or NaN) for a negative z
        nz = y != 0  # (ln Phi(0 +- k denormals) = ln 1/2; no zero result in these inputs)
        assert np.all(nz), name
        worst[name] = float(np.max(log_ndtr_rel_err(y, z)))
        if name == "dense":
            assert np.all(np.diff(y) > 0), "not strictly increasing along the dense sweep"
        if name == "tail":
            assert np.all(np.diff(y) < 0), "not strictly decreasing as -z grows"
    measured = max(worst.values())
    print("\n[device math] routine                     measured      gate   metric")
    print(f"[device math] {'log_ndtr':<26} {measured:10.3e} {LOG_NDTR_GATE:9.2e}   relative, ln Phi  {worst}")
    assert measured <= 1e-12, "the form is wrong"
    assert measured <= LOG_NDTR_GATE, measured
    special = math_dev(np.array([np.nan, -np.inf, np.inf, 40.0, -1e155]))
    assert np.isnan(special[0]) and special[1] == -np.inf and special[2] == 0 and special[3] == 0 and special[4] == -np.inf


def np_nudge(x, k):
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


# ---------------------------------------------------------------- 2. arithmetic
def test_likelihood_matches_the_formula_on_device_fluxes(c4):
    """64 walkers.  ln L of the mixed fitter against the formula (detections in ln F, limits w ln Phi((L - F) / sigma)) on the
    device's own fluxes of the same merged series (vag_flux_density_batch).  The tolerance is measured here: `base` is how well the
    detection-only fitter (the same 60 rows, all detections: existing behaviour) agrees with its own formula on those fluxes, as
    max |got - want| / |want|; the mixed fitter is allowed 2 x base.  Measured on an MI355X: base 8.3e-15; mixed 4.1e-15 (host and
    device pointers, with and without priors), the limit rows' z between -98 and +11 over the walkers."""
    import torch
    th, _ = tv._walkers(64)
    d = defs()
    f_det = c4_fitter(c4, as_detections=True)
    f_mix = c4_fitter(c4)
    assert f_mix.has_limits and not f_det.has_limits
    F = walker_fluxes(f_mix, th, d)
    assert np.array_equal(F, walker_fluxes(f_det, th, d))  # the same merged series
    base = _rel(f_det.loglike_batch(th, d), formula(f_det, F))
    want = formula(f_mix, F)
    got = f_mix.loglike_batch(th, d)
    z = (f_mix._all_lim["limit"] - F) / f_mix._all_lim["sigma"]
    z = z[:, f_mix._all_lim["kind"] == 1]
    print("detection-only rel (base)", base, "mixed rel", _rel(got, want), "z of the limit rows", z.min(), z.max())
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and f_mix.last_plan.n_walkers_rejected == 0
    zt = (c4["value"][c4["lim"]] - c4["truth"][c4["lim"]]) / c4["err"][c4["lim"]]
    assert abs(zt.min() + 6) < 1e-9 and abs(zt.max() - 4) < 1e-9  # z at the truth spans -6 ... +4
    assert base > 0
    assert _rel(got, want) <= 2 * base
    dev = torch.from_numpy(np.ascontiguousarray(th)).to("cuda:0")
    ev = f_mix.device_evaluator(d)  # device-pointer form
    assert ev.has_limits
    vals, _ = ev(dev)
    torch.cuda.synchronize()
    assert _rel(vals.cpu().numpy(), want) <= 2 * base
    ln_prior = -np.log(0.3 - 0.02) - np.log(0.8) - np.log(4.0)  # Uniform over the three boxes (E_iso in log10)
    got_p = f_mix.log_prob_batch(th, d)
    print("with priors rel", _rel(got_p, want + ln_prior))
    assert _rel(got_p, want + ln_prior) <= 2 * base
    vals_p, _ = f_mix.device_evaluator(d, use_priors=True)(dev)
    torch.cuda.synchronize()
    assert _rel(vals_p.cpu().numpy(), want + ln_prior) <= 2 * base


# ---------------------------------------------------------------- 3. the CPU checker
def test_limit_term_against_the_cpu_checker(c4, oracle):
    """The limit rows' contribution -2 (ln L_mixed - ln L_detections), both on the device (the 45 detections carry the same
    weights in both fitters), against -2 sum w ln Phi((L - F) / sigma) on the CPU checker's fluxes (oracle.flux_density), for every
    one of the 64 walkers.  Allowed per walker: sum_i w_i 2 m(z_i - delta_i / sigma_i) delta_i / sigma_i, with m = phi / Phi (it
    falls with z, so the lower end of the interval bounds the slope of ln Phi) and delta_i the flux difference that
    test_gpu_parity.assert_close grants: 2e-6 F_i above 1e-12 of the peak, 2e-6 of the peak below."""
    th, _ = tv._walkers(64)
    d = defs()
    f_mix, f_det = c4_fitter(c4), c4_fitter(c4, limits=False)
    f_mix._consolidate_data()
    f_det._consolidate_data()
    kind = f_mix._all_lim["kind"] == 1
    assert np.array_equal(f_mix._all_weights[~kind], f_det._all_weights)
    got = -2.0 * (f_mix.loglike_batch(th, d) - f_det.loglike_batch(th, d))
    L, sig, w = f_mix._all_lim["limit"][kind], f_mix._all_lim["sigma"][kind], f_mix._all_weights[kind]
    for k, s in enumerate(th):
        p = _abi.ModelParams.from_buffer_copy(bytes(f_mix._params_at(s, d)[0]))
        F = oracle.flux_density(p, f_mix._all_t, f_mix._all_nu)
        delta = 2e-6 * np.where(F > 1e-12 * F.max(), F, F.max())[kind]
        z = (L - F[kind]) / sig
        ref = -2.0 * th_.limit_lnl(L, F[kind], sig, w)
        bound = np.sum(w * 2.0 * th_.inverse_mills(z - delta / sig) * delta / sig)
        print("walker", k, "device", got[k], "checker", ref, "bound", bound, "z", z.min(), z.max())
        assert np.isfinite(got[k]) and abs(got[k] - ref) <= bound


# ---------------------------------------------------------------- 4. band groups and degree groups
BAND = (2.41e17 * 0.3, 2.41e17 * 10.0)
BAND_T = configs.C4_EPOCHS[2::3]  # 6 epochs
POINT_ROWS = np.arange(60) % 3 == 0  # a third of the point rows (their detections) go with the group tests


def test_band_group_with_limit_rows(c4):
    """A band group (Model.flux on the device) with two limit rows of six: ln L against the point rows' own ln L plus the formula on
    Model.flux of every walker.  Tolerance as in the point-row test: 2 x what the same group as detections gives."""
    th, _ = tv._walkers(16, seed=6)
    d = defs()
    rows = POINT_ROWS & ~c4["lim"]
    truth = tv._c4_truth().flux(BAND_T, BAND[0], BAND[1], 7).total
    assert np.all(truth > 0)
    rng = np.random.default_rng(3)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(6)), 0.1 * truth
    lim = np.array([True, False, False, True, False, False])
    value = np.where(lim, truth + np.array([2.0, 0, 0, -3.0, 0, 0]) * err, obs)
    w = rng.uniform(0.5, 2.0, 6)
    f_pts = c4_fitter(c4, limits=False, rows=rows)
    ll_pts = f_pts.loglike_batch(th, d)
    bands = np.array([f_pts.model(s, d).flux(BAND_T, BAND[0], BAND[1], 7).total for s in th])
    res = {}
    for name, kw in (("detections", dict(flux=obs)), ("mixed", dict(flux=value, upper_limit=lim))):
        f = c4_fitter(c4, limits=False, rows=rows)
        f.add_flux(BAND, BAND_T, kw.pop("flux"), err, num_points=7, weights=w, **kw)
        bd = f._band_obs[0]
        if name == "mixed":
            want = ll_pts + th_.mixed_lnl(bd["lim"], bd["ln_flux"], bd["ln_err"], bd["limit"], bd["sigma"], bd["weights"], bands)
        else:
            want = ll_pts + th_.detection_lnl(bd["ln_flux"], bands, bd["ln_err"], bd["weights"])
        got = f.loglike_batch(th, d)
        assert np.all(np.isfinite(got)) and f.last_plan.n_walkers_rejected == 0
        res[name] = _rel(got, want)
        assert f.has_limits == (name == "mixed")
    print("band group: detections rel (base)", res["detections"], "mixed rel", res["mixed"])
    assert res["detections"] > 0 and res["mixed"] <= 2 * res["detections"]


def test_degree_group_with_limit_rows(c4):
    """A polarization-degree group with two limit epochs of four ("Pi < L"): ln L against the flux fit's own ln L plus the formula
    on hypot(Q, U) / I of vag_sky_polarization_batch.  Tolerance: 2 x what the same group as detections gives (measured on an
    MI355X: 6.6e-16 as detections, 1.0e-15 mixed)."""
    th, pol = tp._walkers(8, seed=6)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    defs_flux, defs_pol = tp._defs()
    data = tp.make_group(tv._c4_truth())
    degree = np.hypot(data["q"], data["u"])
    ll_flux = tp._c4_fitter().loglike_batch(th, defs_flux)
    w = np.array([1.0, 0.5, 2.0, 1.5])
    lim = np.array([True, False, True, False])
    value = np.where(lim, degree + np.array([0.02, 0, -0.01, 0]), degree)
    res = {}
    for name, kw in (("detections", dict(q=degree)), ("mixed", dict(q=value, upper_limit=lim))):
        f = tp._c4_fitter()
        f.add_polarization(data["nu"], data["t"], kw.pop("q"), err_q=data["err"], kind="degree", weights=w, **kw)
        pd = f._pol_obs[0]
        terms = []
        for s in samples:
            pa, spec_kw = tp._field(s, tp.COLS, {})
            I, Q, U = tp.batch_pol(f._params_at(s, defs_pol)[0], pd["t"], pd["nu"], pk.spec(**spec_kw), pa, pd["n_az"])
            r = (pd["q"] - np.hypot(Q, U) / I) / pd["err_q"]
            lnl = -0.5 * w * r * r
            if name == "mixed":
                lnl = np.where(lim, w * th_.log_ndtr(r), lnl)
            terms.append(np.sum(lnl))
        want = ll_flux + np.array(terms)
        got = f.loglike_batch(samples, defs_pol)
        assert np.all(np.isfinite(got)) and f.last_plan.n_walkers_rejected == 0
        res[name] = _rel(got, want)
    print("degree group: detections rel (base)", res["detections"], "mixed rel", res["mixed"])
    assert res["detections"] > 0 and res["mixed"] <= 2 * res["detections"]


def _call(spec, lim, samples, dev_out=None):
    lib = _lib.load()
    h, lock = va.get_context(0)
    out = np.empty(samples.shape[0])
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    with lock:
        rc = lib.vag_loglike_lim_batch(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(lim),
                                       samples.ctypes.data_as(dp), samples.shape[0], spec.ndim, out.ctypes.data_as(dp))
    return rc, out


def test_a_qu_group_refuses_limit_rows():
    th, pol = tp._walkers(4, seed=6)
    samples = np.ascontiguousarray(np.column_stack([th, pol]))
    _, defs_pol = tp._defs()
    f = tp.add_group(tp._c4_fitter(), tp.make_group(tv._c4_truth()))  # kind "qu"
    spec, _, _ = f.build_spec(defs_pol)
    kind = np.array([0, 1, 0, 0], dtype=np.int32)
    lim = _lib.LimitFitSpec()
    kinds = (ip * 1)(kind.ctypes.data_as(ip))
    lim.n_pol_groups, lim.pol_kind = 1, kinds
    rc, _ = _call(spec, lim, samples)
    assert rc == -1 and "VAG_POL_DEGREE" in _lib.load().vag_last_error().decode()
    kind[:] = 0  # no limit row: the polarization call
    rc, out = _call(spec, lim, samples)
    assert rc == 0 and np.array_equal(out, f.loglike_batch(samples, defs_pol))


# ---------------------------------------------------------------- 5. bits
@pytest.mark.parametrize("groups", ["none", "centroid", "centroid+visibility+polarization"])
def test_no_limit_row_is_bitwise_the_pol_call(c4, groups):
    th, sky = tv._walkers(64, seed=9)
    fixed = _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    f = tv._c4_fitter(groups != "none")
    d, samples = FLUX_DEFS + fixed, th
    if groups != "none":
        d, samples = FLUX_DEFS + tv.SKY_DEFS + fixed, np.column_stack([th, sky])
    if groups.endswith("polarization"):
        vis = tv.make_group(tv._c4_truth(), tv.VIS_T, tv.VIS_NU, (70, 5, 33), tv.PA_TRUE, tv.EAST0_TRUE)
        tv.add_group(f, vis, n_az=64)
        tp.add_group(f, tp.make_group(tv._c4_truth()), kind="degree")
        d = FLUX_DEFS + tv.SKY_DEFS + [tp.POL_DEFS[1]] + fixed
        samples = np.column_stack([samples, np.random.default_rng(21).uniform(0.2, 0.8, 64)])
    samples = np.ascontiguousarray(samples)
    spec, _, _ = f.build_spec(d)
    assert spec._lim is None
    lib = _lib.load()
    h, lock = va.get_context(0)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    a = np.empty(64)
    with lock:
        _lib.check(lib.vag_loglike_pol_batch(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol),
                                             samples.ctypes.data_as(dp), 64, spec.ndim, a.ctypes.data_as(dp)))
    assert np.all(np.isfinite(a))
    zeros = np.zeros(spec.n_data, dtype=np.int32)
    with_kind = _lib.LimitFitSpec()
    with_kind.point.kind = zeros.ctypes.data_as(ip)  # all detections; limit / sigma stay NULL: they are not read
    if spec._pol is not None:
        pz = np.zeros(spec._pol.groups[0].n, dtype=np.int32)
        kinds = (ip * 1)(pz.ctypes.data_as(ip))
        with_kind.n_pol_groups, with_kind.pol_kind = 1, kinds
    for lim in (None, _lib.LimitFitSpec(), with_kind):
        rc, b = _call(spec, lim, samples)
        assert rc == 0 and np.array_equal(a, b)
    assert np.array_equal(f.loglike_batch(samples, d), a)


def test_bits_with_limits(c4):
    th, _ = tv._walkers(64, seed=12)
    th = np.ascontiguousarray(th)
    d = defs()
    f = c4_fitter(c4)
    a = f.loglike_batch(th, d)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
    assert f.loglike_batch(th[5:6], d)[0] == a[5]  # alone
    assert np.array_equal(f.loglike_batch(np.ascontiguousarray(th[::-1]), d)[::-1], a)
    assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
    other = c4_fitter(c4, value=c4["value"] * np.where(c4["lim"], 1.5, 1.0))  # other limits, same shapes: the resident copy must follow
    b = other.loglike_batch(th, d)
    assert np.all(b != a) and np.array_equal(f.loglike_batch(th, d), a)


# ---------------------------------------------------------------- 6. behaviour
def test_more_energy_makes_the_limit_term_more_negative(c4):
    tr = configs.C4_TRUTH
    e = np.log10(tr["E_iso"]) + np.linspace(-0.5, 0.5, 9)
    th = np.ascontiguousarray(np.column_stack([np.full(9, tr["theta_c"]), np.full(9, tr["theta_obs"]), e]))
    d = defs()
    term = c4_fitter(c4).loglike_batch(th, d) - c4_fitter(c4, limits=False).loglike_batch(th, d)
    print("limit term over E_iso:", term)
    assert np.all(np.isfinite(term)) and np.all(term < 0) and np.all(np.diff(term) < 0)


def test_edges(c4):
    """A model 1e6 sigma above a limit: finite and very negative.  No flux at a limit row: valid.  A limit so far below the model
    that z^2 / 2 overflows, and a NaN parameter: -inf, counted."""
    tr = configs.C4_TRUTH
    th = np.ascontiguousarray(np.column_stack([tr["theta_c"] * np.array([1.0, 1.02, 0.98, 1.01]), np.full(4, tr["theta_obs"]),
                                               np.full(4, np.log10(tr["E_iso"]))]))
    d = defs()
    i = LIMIT_ROWS[7]
    base = c4_fitter(c4, rows=np.arange(60) != i)
    ll0 = base.loglike_batch(th, d)
    value, err = c4["value"].copy(), c4["err"].copy()
    value[i], err[i] = 0.0, c4["truth"][i] * 1e-6
    f = c4_fitter(c4, value=value, err=err)
    far = f.loglike_batch(th, d)
    want = formula(f, walker_fluxes(f, th, d))
    print("1e6 sigma above a limit:", far, "want", want, "without the row", ll0)
    assert np.all(np.isfinite(far)) and np.all(far < -1e11) and np.all(ll0 > -1e6) and f.last_plan.n_walkers_rejected == 0
    assert _rel(far, want) <= 1e-10  # (the sibling likelihood tests' tolerance against host arithmetic)
    # no flux: a limit row far above the synchrotron cut-off
    g = c4_fitter(c4)
    g.add_flux_density(1e30, [c4["t"][30]], [1e-28], [2e-29], weights=[0.7], upper_limit=True)
    assert np.all(device_series([g._params_at(s, d)[0] for s in th], [c4["t"][30]], [1e30]) == 0)
    got = g.loglike_batch(th, d)
    want = c4_fitter(c4).loglike_batch(th, d) + 0.7 * th_.log_ndtr(5.0)  # z = L / sigma = 5
    assert np.all(np.isfinite(got)) and g.last_plan.n_walkers_rejected == 0 and _rel(got, want) <= 1e-10
    # -inf through the limit term itself, and a NaN parameter
    err[i] = 1e-190
    h = c4_fitter(c4, value=value, err=err)
    out = h.loglike_batch(th, d)
    assert np.all(out == -np.inf) and h.last_plan.n_walkers_rejected == 4
    bad = th.copy()
    bad[2, 0] = np.nan
    f2 = c4_fitter(c4)
    good = f2.loglike_batch(th, d)
    out = f2.loglike_batch(bad, d)
    assert out[2] == -np.inf and np.array_equal(np.delete(out, 2), np.delete(good, 2)) and f2.last_plan.n_walkers_rejected == 1


def test_invalid_limit_arrays(c4):
    th, _ = tv._walkers(4)
    th = np.ascontiguousarray(th)
    d = defs()
    f = c4_fitter(c4)
    f.add_flux(BAND, BAND_T, np.full(6, 1e-13), np.full(6, 1e-14), upper_limit=np.array([True] + [False] * 5))
    f.add_polarization(3e9, tp.POL_T, np.full(4, 0.1), err_q=np.full(4, 0.02), kind="degree", upper_limit=np.array([True, False, False, False]))
    d_pol = FLUX_DEFS + tp.POL_DEFS + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))
    samples = np.ascontiguousarray(np.column_stack([th, np.full(4, 0.3), np.full(4, 0.5)]))
    spec, _, _ = f.build_spec(d_pol)
    rc, out = _call(spec, spec._lim, samples)
    assert rc == 0 and np.all(np.isfinite(out))
    lim = f._all_lim

    def refused(word):
        rc, _ = _call(spec, spec._lim, samples)
        msg = _lib.load().vag_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def poke(arr, i, v, word):
        old = arr[i]
        arr[i] = v
        refused(word)
        arr[i] = old
    r, det = int(np.flatnonzero(lim["kind"] == 1)[3]), int(np.flatnonzero(lim["kind"] == 0)[0])
    poke(lim["kind"], 0, 2, "row 0")
    poke(lim["kind"], 5, -1, "row 5")
    poke(lim["limit"], r, np.nan, f"row {r}")
    poke(lim["limit"], r, np.inf, f"row {r}")
    poke(lim["limit"], r, -1e-30, f"row {r}")
    poke(lim["sigma"], r, 0.0, f"row {r}")
    poke(lim["sigma"], r, -1.0, f"row {r}")
    poke(lim["sigma"], r, np.inf, f"row {r}")
    poke(lim["sigma"], r, np.nan, f"row {r}")
    poke(f._band_obs[0]["limit"], 0, -1.0, "band group 0, row 0")
    poke(f._band_obs[0]["lim"], 3, 7, "band group 0, row 3")
    poke(f._pol_obs[0]["q"], 0, 1.5, "polarization group 0, epoch 0")
    poke(f._pol_obs[0]["lim"], 2, 3, "polarization group 0, epoch 2")
    lim["limit"][det] = np.nan  # a detection row: not read
    rc, again = _call(spec, spec._lim, samples)
    assert rc == 0 and np.array_equal(again, out)
    lim["limit"][det] = 0.0
    for field, n in (("n_bands", 2), ("n_pol_groups", 3)):
        old = getattr(spec._lim, field)
        setattr(spec._lim, field, n)
        refused(field)
        setattr(spec._lim, field, old)
    rc, again = _call(spec, spec._lim, samples)
    assert rc == 0 and np.array_equal(again, out)


# ---------------------------------------------------------------- 7. a fit
def test_a_fit_with_limits(c4):
    """The C4 mock with its first two epochs (6 rows) replaced by 3 sigma limits placed above the truth (L = 1.5 F_truth, sigma =
    L / 3): sampling.fit with 32 walkers and 40 steps from a ball around the truth.  Every walker ends with a finite
    log-probability, and the best sample's is at or above the truth's."""
    tr = configs.C4_TRUTH
    lim = np.arange(60) < 6
    value = np.where(lim, 1.5 * c4["truth"], c4["obs"])
    err = np.where(lim, value / 3.0, c4["err"])
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    f.add_flux_density(c4["nu"], c4["t"], value, err, upper_limit=lim)
    d = defs()
    truth = np.array([tr["theta_c"], tr["theta_obs"], np.log10(tr["E_iso"])])
    lp_truth = f.log_prob_batch(truth[None], d)[0]
    nwalkers, nsteps = 32, 40
    res = sampling.fit(f, d, nwalkers=nwalkers, nsteps=nsteps, seed=4, center=truth, spread=0.02)
    last = res["log_prob"][-nwalkers:]
    print("fit with limits: truth", lp_truth, "best", res["log_prob"].max(), "at", res["best"], "last step", last.min(), last.max())
    assert np.isfinite(lp_truth) and np.all(np.isfinite(last))
    assert res["log_prob"].max() >= lp_truth
