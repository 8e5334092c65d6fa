"""Outlier groups in the walker likelihood (vag_loglike_robust_batch[_dev]; the ``outliers`` keyword of the Fitter's add_flux_density
/ add_spectrum / add_flux and the parameters ``out_frac_<label>``, ``out_scale_<label>``, ``out_shift_<label>``) on the device: the
arithmetic against the numpy statement of the term (fitting.outlier_terms, tests/test_outliers_host.py) on the device's own model
values, reductions, bits, edges, invalid walkers, refusals, a likelihood profile, the device sampler and the CPU checker.

The problem is that of tests/test_outliers_host.py built from the device's own truth: the rows of tests/test_noise.py (70 point rows,
so the kernel's lane loop wraps past 64; every seventh row an upper limit; random weights), group "a" robust and without calibration,
group "b" a plain noise group, group "c" with its calibration, three band groups (c, b and the robust a), six planted flares among
the point rows of group "a" and one in its band group.  Free: FLUX_DEFS, sys_a, out_frac_a (linear; walker 0 exactly 0), out_scale_a
(log) and out_shift_a."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_limits as tl
import test_outliers_host as oh
import test_sky_visfit as tv
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
defs, make_fitter, formula = oh.defs, oh.make_fitter, oh.formula


@pytest.fixture(scope="module")
def prob():
    t, nu = oh.point_rows()
    at_truth = [_abi.make_params(**configs.C4_TRUTH)]
    truth = np.concatenate([tl.device_series(at_truth, t[:60], nu[:60])[0], tl.device_series(at_truth, t[60:], nu[60:])[0]])
    model = tv._c4_truth()
    band_truth = {key: model.flux(bt, band[0], band[1], 7).total for key, (band, bt) in oh.BANDS.items()}
    return oh.problem(truth, band_truth)


def walkers(nb, seed=5):
    """[theta_c, theta_v, log10 E_iso, sys_a, out_frac_a, log10 out_scale_a, out_shift_a]; walker 0 has out_frac_a = 0 exactly."""
    th, _ = tv._walkers(nb, seed=seed)
    rng = np.random.default_rng(seed + 200)
    frac = rng.uniform(0.01, 0.5, nb)
    frac[0] = 0.0
    return np.ascontiguousarray(np.column_stack([th, rng.uniform(0.0, 0.3, nb), frac, rng.uniform(-1.0, 0.7, nb),
                                                 rng.uniform(-0.5, 2.0, nb)]))


def device_band(params, bd):
    """vag_flux_batch: the device's band-integrated fluxes of one band group, [nb][n]."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    arr = (_lib.ModelParams * len(params))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in params])
    t = np.ascontiguousarray(bd["t"], float)
    out = np.empty((len(params), t.size))
    with lock:
        _lib.check(lib.vag_flux_batch(h, arr, len(params), t.ctypes.data_as(dp), t.size, bd["nu_min"], bd["nu_max"], bd["num_points"],
                                      out.ctypes.data_as(dp)))
    return out


def model_values(f, samples, d):
    """The device's own model values at the fitter's rows: the point rows from vag_flux_density_batch, the band groups from
    vag_flux_batch, one call each for all walkers."""
    f._consolidate_data()
    params = [f._params_at(s, d)[0] for s in samples]
    return tl.device_series(params, f._all_t, f._all_nu), [device_band(params, bd) for bd in f._band_obs]


def rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@pytest.fixture(scope="module")
def ref64(prob):
    """The 64 walkers of the arithmetic, reduction and bit tests, the full fitter and the device's model values at them (once)."""
    f, d, th = make_fitter(prob), defs(), walkers(64)
    F, bands = model_values(f, th, d)
    return dict(f=f, d=d, th=th, F=F, bands=bands)


# ---------------------------------------------------------------- 1. arithmetic
# measured on an MI355X: the largest |got - want| / max(1, |want|) over the 64 walkers is MEASURED_ARITH = 4.9e-15 (4.877e-15; host
# entry; the device-pointer entry returns the same bits, test_bits); the gate is 4 x that, 1.96e-14.  Anything above 1e-9, the cap of
# tests/test_noise.py, would be an algebra error, not rounding.
MEASURED_ARITH = 4.9e-15
ARITH_CAP = 1e-9


def gate(measured):
    assert measured <= ARITH_CAP
    return 4 * measured


def test_likelihood_matches_the_statement_on_device_fluxes(prob, ref64):
    f, d, th, F, bands = (ref64[k] for k in ("f", "d", "th", "F", "bands"))
    assert f.has_outlier_groups and f.has_noise_groups and f.has_limits and f._noise_labels == ["a", "b", "c"]
    assert f._noise_robust == {"a": True} and f._noise_calib == {"c": 0.1} and th[0, 4] == 0.0 and np.all(th[1:, 4] > 0)
    f._consolidate_data()
    assert f._all_t.size == 70 and (f._all_grp == 0).sum() == 30 and (f._all_grp == 1).sum() == 20 and f._all_lim["kind"].sum() == 10
    assert [bd["noise"] for bd in f._band_obs] == [2, 1, 0] and prob["planted"].sum() == 6
    want = formula(f, d, th, F, bands)
    got = f.loglike_batch(th, d)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and f.last_plan.n_walkers_rejected == 0
    # against the same rows with group "a" a plain noise group: every walker with P > 0 differs; walker 0 (P = 0) is that fitter's
    # value (test_zero_fraction_is_the_noise_group holds it to its gate).  Against the rows without noise=: every walker differs.
    noise = make_fitter(prob, outliers=False).loglike_batch(np.ascontiguousarray(th[:, :4]), defs(outliers=False))
    plain = make_fitter(prob, groups=False).loglike_batch(np.ascontiguousarray(th[:, :3]), oh.FLUX_DEFS + oh.c4_fixed(
        skip=("theta_c", "theta_v", "E_iso")))
    measured = rel(got, want)
    print("outlier groups: rel to the statement", measured, "ln L range", want.min(), want.max(), "change against the plain group",
          np.abs(got - noise)[1:].min(), np.abs(got - noise).max(), "walker 0", abs(got[0] - noise[0]), "against no groups",
          np.abs(got - plain).min())
    assert np.all(np.abs(got - noise)[1:] > 1e-3) and np.all(np.abs(got - plain) > 1e-3)
    assert abs(got[0] - noise[0]) <= 1e-9 * abs(noise[0])
    assert measured <= ARITH_CAP, "an algebra error, not rounding"
    assert measured <= gate(MEASURED_ARITH)


# ---------------------------------------------------------------- 2. out_frac fixed at 0
# measured on an MI355X in the same way, against the fitter without outliers= (not bit for bit: the robust kernel sums w l per row, the
# noise kernel A and N apart): MEASURED_ZERO = 4.1e-16 (4.009e-16); the gate is 4 x that, 1.64e-15.
MEASURED_ZERO = 4.1e-16


def test_zero_fraction_is_the_noise_group(prob, ref64):
    th = ref64["th"]
    d0 = defs(out_frac_a=0.0)  # free: FLUX_DEFS, sys_a, out_scale_a, out_shift_a -- the last two change nothing at P = 0
    a = make_fitter(prob).loglike_batch(np.ascontiguousarray(th[:, [0, 1, 2, 3, 5, 6]]), d0)
    b = make_fitter(prob, outliers=False).loglike_batch(np.ascontiguousarray(th[:, :4]), defs(outliers=False))
    measured = rel(a, b)
    print("out_frac = 0 against the plain noise group: rel", measured)
    assert np.all(np.isfinite(b)) and measured <= ARITH_CAP
    assert measured <= gate(MEASURED_ZERO)
    # 0 when not given: out_frac_a left out is out_frac_a fixed at 0, to the bit
    d_none = [pd for pd in d0 if pd.name != "out_frac_a"]
    assert np.array_equal(make_fitter(prob).loglike_batch(np.ascontiguousarray(th[:, [0, 1, 2, 3, 5, 6]]), d_none), a)


# ---------------------------------------------------------------- 3. no effect without robust rows
def _ref(x):
    return C.byref(x) if x is not None else None


def call_cov(spec, samples):
    lib = _lib.load()
    h, lock = va.get_context(0)
    out = np.empty(samples.shape[0])
    with lock:
        rc = lib.vag_loglike_cov_batch(h, C.byref(spec), _ref(spec._sky), _ref(spec._vis), _ref(spec._pol), _ref(spec._lim),
                                       _ref(spec._noise), _ref(spec._counts), _ref(spec._index), _ref(spec._fold), _ref(spec._tmpl),
                                       _ref(spec._cov), samples.ctypes.data_as(dp), samples.shape[0], spec.ndim, out.ctypes.data_as(dp))
    return rc, out


def call_robust(spec, samples, robust="spec", noise="spec"):
    """vag_loglike_robust_batch on the request of the spec, with the robust / noise member replaced where given (None: null)."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    out = np.empty(samples.shape[0])
    req = fitting.loglike_request(spec)
    if robust != "spec":
        req.robust = C.pointer(robust) if robust is not None else None
    if noise != "spec":
        req.noise = C.pointer(noise) if noise is not None else None
    with lock:
        rc = lib.vag_loglike_robust_batch(h, C.byref(req), samples.ctypes.data_as(dp), samples.shape[0], spec.ndim, out.ctypes.data_as(dp))
    return rc, out


def test_without_a_robust_row_it_is_bitwise_the_cov_call(prob, ref64):
    th = np.ascontiguousarray(ref64["th"][:, :4])
    f = make_fitter(prob, outliers=False)
    spec, _, _ = f.build_spec(defs(outliers=False))
    assert spec._robust is None and spec._noise is not None
    rc, a = call_cov(spec, th)
    assert rc == 0 and np.all(np.isfinite(a))
    rc, b = call_robust(spec, th)  # a null robust block
    assert rc == 0 and np.array_equal(a, b)
    none = _lib.RobustFitSpec()  # no group is robust
    none.n_groups = 3
    rc, b = call_robust(spec, th, robust=none)
    assert rc == 0 and np.array_equal(a, b)
    # a robust group without a row: the noise spec gains an empty fourth group, which the mask names
    spec._noise.n_groups = 4
    rc, a4 = call_cov(spec, th)
    empty = _lib.RobustFitSpec()
    empty.n_groups, empty.mask = 4, 1 << 3
    empty.frac_fixed[3], empty.scale_fixed[3] = 0.3, 2.0
    rc2, b = call_robust(spec, th, robust=empty)
    assert rc == 0 and rc2 == 0 and np.array_equal(a4, a) and np.array_equal(b, a)
    spec._noise.n_groups = 3
    assert np.array_equal(f.loglike_batch(th, defs(outliers=False)), a)


# ---------------------------------------------------------------- 4. bits
def test_bits(ref64):
    import torch
    f, d, th = ref64["f"], ref64["d"], ref64["th"]
    a = f.loglike_batch(th, d)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
    assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
    perm = np.random.default_rng(1).permutation(64)
    assert np.array_equal(f.loglike_batch(np.ascontiguousarray(th[perm]), d), a[perm])  # a permuted batch
    assert f.loglike_batch(th[7:8], d)[0] == a[7] and f.loglike_batch(th[0:1], d)[0] == a[0]  # alone
    ev = f.device_evaluator(d)
    assert ev.has_noise_groups and ev.has_limits
    vals, _ = ev(torch.from_numpy(th).to("cuda:0"))  # the device-pointer entry
    torch.cuda.synchronize()
    assert np.array_equal(vals.cpu().numpy(), a)
    with pytest.raises(NotImplementedError, match="noise="):
        ev.native.shard(None, 64, 0, 1, None)
    spec, _, _ = f.build_spec(d)
    rc, direct = call_robust(spec, th)  # the entry itself
    assert rc == 0 and np.array_equal(direct, a)


# ---------------------------------------------------------------- 5. edges through the likelihood
def test_edges(prob):
    """Each edge on 8 walkers, finite and in agreement with the statement on the device's own model values (1e-9: an algebra error or
    an overflow shows far above it; the rounding is that of test 1)."""
    th = walkers(8, seed=3)

    def check(name, f, d, samples, bands=True):
        F, B = model_values(f, samples, d)
        got, want = f.loglike_batch(samples, d), formula(f, d, samples, F, B if bands else [])
        print(name, "ln L", got.min(), got.max(), "rel", rel(got, want))
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and f.last_plan.n_walkers_rejected == 0, name
        assert rel(got, want) <= ARITH_CAP, name
        return got
    f = make_fitter(prob)
    near1 = th.copy()
    near1[:, 4] = 1.0 - 1e-12
    check("P = 1 - 1e-12", f, defs(), near1)
    tiny = th.copy()
    tiny[:, 4] = -12.0
    check("P = 1e-12 on log scale", f, defs(out_frac_a="log"), tiny)
    same = check("b = 0 with mu = 0", f, defs(out_scale_a=0.0, out_shift_a=0.0), np.ascontiguousarray(th[:, :5]))
    noise = make_fitter(prob, outliers=False).loglike_batch(np.ascontiguousarray(th[:, :4]), defs(outliers=False))
    assert rel(same, noise) <= ARITH_CAP  # both components are one Gaussian: the plain noise group, whatever P
    # no model flux at a detection row of the robust group (far above the synchrotron cut-off): the 1e-300 clamp
    t_mid = prob["t"][30]
    g = make_fitter(prob, bands=False, extra=(1e30, t_mid, 1e-28, 2e-29, 0.7))
    dg = defs(bands=False)
    Fg, _ = model_values(g, th, dg)
    assert np.all(Fg[:, g._all_nu == 1e30] == 0)
    clamped = check("a clamped row", g, dg, th, bands=False)
    assert np.all(clamped < make_fitter(prob, bands=False).loglike_batch(th, dg) - 5)  # the row costs ln P - ln(1 - P) and more
    # a planted residual of 1e3 sigma: a datum e^100 above the truth with 10 % error
    k = int(np.flatnonzero((prob["nu"] == configs.C4_BANDS[0]) & (np.arange(70) < 60))[8])
    big = prob["truth"][k] * np.exp(100.0)
    check("a residual of 1e3 sigma", make_fitter(prob, bands=False, extra=(prob["nu"][k], prob["t"][k], big, 0.1 * big, 1.0)), dg, th,
          bands=False)


# ---------------------------------------------------------------- 6. invalid walkers
def test_invalid_walkers_score_minus_infinity_and_are_counted(prob):
    f, d = make_fitter(prob), defs(out_scale_a="linear")  # (a negative b needs the linear scale)
    th = walkers(12, seed=3)
    th[:, 5] = 10.0 ** th[:, 5]
    good = f.loglike_batch(th, d)
    assert np.all(np.isfinite(good)) and f.last_plan.n_walkers_rejected == 0
    bad = th.copy()
    bad[1, 4] = 1.0       # P = 1
    bad[2, 4] = -1e-3     # P < 0
    bad[3, 4] = np.nan    # P = NaN
    bad[4, 5] = -0.5      # b < 0
    bad[5, 6] = np.inf    # mu = inf
    bad[6, 0] = np.nan    # an invalid model parameter: no flux
    bad[7, 4] = np.inf
    bad[8, 5] = np.nan
    bad[9, 6] = np.nan
    ll = f.loglike_batch(bad, d)
    assert np.all(ll[1:10] == -np.inf) and f.last_plan.n_walkers_rejected == 9
    keep = [0, 10, 11]
    assert np.array_equal(ll[keep], good[keep])  # the others do not notice
    lp = f.log_prob_batch(bad[[0, 1, 2, 10]], d)  # under the bounds mask the box refuses them first
    assert np.isfinite(lp[0]) and lp[1] == -np.inf and lp[2] == -np.inf and np.isfinite(lp[3])


# ---------------------------------------------------------------- 7. refusals
def test_refusals_through_the_c_abi(prob):
    f, d = make_fitter(prob), defs()
    th = walkers(4, seed=3)
    spec, _, _ = f.build_spec(d)
    rb = spec._robust
    assert rb.n_groups == 3 and rb.mask == 1
    rc, out = call_robust(spec, th)
    assert rc == 0 and np.all(np.isfinite(out))

    def refused(word, **kw):
        rc, _ = call_robust(spec, th, **kw)
        msg = _lib.load().vag_last_error().decode()
        assert rc == _lib.VAG_E_INVALID and word in msg, (rc, msg, word)
    refused("need a noise block", noise=None)
    rb.n_groups = 2
    refused("n_groups must be the noise spec's 3")
    rb.n_groups = 3
    rb.mask = 1 | (1 << 3)
    refused("at or above n_groups")
    rb.mask = 1 | (1 << 2)  # group c has a calibration fraction
    refused("outlier group 2 has a calibration")
    rb.mask = 1
    for arr, values, word in ((rb.frac_fixed, (np.nan, np.inf, -0.1, 1.0), "outlier group 0: the outlier fraction"),
                              (rb.scale_fixed, (np.nan, np.inf, -1.0), "outlier group 0: the outlier scatter"),
                              (rb.shift_fixed, (np.nan, np.inf, -np.inf), "outlier group 0: the outlier offset")):
        for v in values:
            keep = arr[0]
            arr[0] = v
            refused(word)
            arr[0] = keep
    old = spec.slot[4]
    for slot in (_lib.P_ROBUST_FRAC0 + 1, _lib.P_ROBUST_SCALE0 + 2, _lib.P_ROBUST_SHIFT0 + 7):  # groups that are not robust
        spec.slot[4] = slot
        refused("bad parameter slot")
    spec.slot[4] = old
    rc, _ = call_cov(spec, th)  # the earlier entry points do not know the slots
    assert rc == _lib.VAG_E_INVALID and "bad parameter slot" in _lib.load().vag_last_error().decode()
    lib = _lib.load()
    h, lock = va.get_context(0)
    with lock:
        rc = lib.vag_loglike_robust_batch(h, None, th.ctypes.data_as(dp), 4, spec.ndim, out.ctypes.data_as(dp))
    assert rc == _lib.VAG_E_INVALID and "null request" in lib.vag_last_error().decode()
    rc, again = call_robust(spec, th)  # nothing is left changed
    assert rc == 0 and np.array_equal(again, out)
    assert np.array_equal(f.loglike_batch(th, d), out)


# ---------------------------------------------------------------- 8. a profile
def test_profile_over_the_energy(prob):
    """Nine values of log10 E_iso around the truth, all else at the truth (sys_a = 0.02, out_frac = 0.15, out_scale = 1.5, out_shift =
    0).  With outliers= the maximum is at the truth; without it the seven flares pull it to a higher energy.  The rows' outlier
    probabilities at the truth satisfy the 0.9 / 0.1 condition of the host test."""
    tr = configs.C4_TRUTH
    grid = np.log10(tr["E_iso"]) + 0.05 * np.arange(-4, 5)
    th = np.ascontiguousarray(np.column_stack([np.full(9, tr["theta_c"]), np.full(9, tr["theta_obs"]), grid]))
    f, d = make_fitter(prob), defs(sys_a=0.02, out_frac_a=oh.FRAC_TRUE, out_scale_a=oh.SCALE_TRUE, out_shift_a=0.0)
    robust = f.loglike_batch(th, d)
    plain = make_fitter(prob, outliers=False).loglike_batch(th, defs(outliers=False, sys_a=0.02))
    print("profile over log10 E_iso: with outliers=", robust - robust.max(), "argmax", int(np.argmax(robust)), "without",
          plain - plain.max(), "argmax", int(np.argmax(plain)))
    assert np.all(np.isfinite(robust)) and np.all(np.isfinite(plain))
    assert int(np.argmax(robust)) == 4 and int(np.argmax(plain)) > 4
    groups = f.outlier_probabilities(th[4], d)
    oh.check_flare_probabilities(f, prob, groups)
    g = groups[0]
    assert np.array_equal(g["band"][:30], np.full(30, -1)) and np.array_equal(g["band"][30:], np.full(4, 2)) and g["t"].size == 34
    assert np.all(np.diff(g["t"][:30]) >= 0) and np.all(np.isnan(g["nu"][30:])) and np.array_equal(g["t"][30:], oh.BANDS["a"][1])
    assert make_fitter(prob, outliers=False).outlier_probabilities(th[4], defs(outliers=False, sys_a=0.02)) == []


# ---------------------------------------------------------------- 9. the device sampler
def test_the_block_reaches_the_device_sampler(prob):
    """fit(sampler="device"), 32 walkers and 8 steps: bit for bit the chain of the host statement of the move driven by
    log_prob_batch, which test 1 holds to the outlier term."""
    f, d = make_fitter(prob), defs()
    _, lo, hi = f.build_spec(d)
    center = oh.truth_sample(d, sys_a=0.05, out_frac_a=oh.FRAC_TRUE, out_scale_a=oh.SCALE_TRUE, out_shift_a=0.0)
    res = f.fit(d, nwalkers=32, nsteps=8, seed=3, sampler="device", center=center, spread=0.02)
    pos0 = sampling.initial_positions(lo, hi, 32, np.random.default_rng(3), center=center, spread=0.02)
    chain, logp, acc = sampling.run_stretch_move_philox(lambda x: f.log_prob_batch(x, d), pos0, 8, seed=3)
    assert res["chain"].shape == (8, 32, 7) and np.all(np.isfinite(logp))
    assert np.array_equal(res["chain"], chain) and np.array_equal(res["log_prob"], logp.reshape(-1))
    assert np.array_equal(res["acceptance"], acc) and 0 < acc.sum()
    assert np.any(chain[-1] != pos0)


# ---------------------------------------------------------------- 10. the CPU checker
def test_against_the_cpu_checker(prob, oracle):
    """The fitter without its band groups on 16 draws of the prior box (one with theta_c < 0: the checker raises, the device scores
    -inf): ln L against the statement on the CPU checker's fluxes, at the rtol / atol of tests/test_noise.py's test of the same name;
    -inf on the same walkers."""
    f, d = make_fitter(prob, bands=False), defs(bands=False)
    _, lo, hi = f.build_spec(d)
    rng = np.random.default_rng(0)
    samples = lo + (hi - lo) * rng.random((16, len(lo)))
    samples[:, 3] = rng.uniform(0.0, 0.5, 16)   # sys_a: the lower part of its box
    samples[:, 4] = rng.uniform(0.0, 0.5, 16)   # out_frac_a
    samples[:, 5] = rng.uniform(-1.0, 0.7, 16)  # log10 out_scale_a
    samples[:, 6] = rng.uniform(-1.0, 2.0, 16)  # out_shift_a
    samples[5, 0] = -0.5
    samples = np.ascontiguousarray(samples)
    got = f.loglike_batch(samples, d)
    want = np.empty(16)
    for i, s in enumerate(samples):
        try:
            p = _abi.ModelParams.from_buffer_copy(bytes(f._params_at(s, d)[0]))
            Fo = oracle.flux_density(p, f._all_t, f._all_nu)
            v = formula(f, d, samples[i:i + 1], Fo[None, :], [])[0]
            want[i] = v if np.isfinite(v) else -np.inf
        except ValueError:
            want[i] = -np.inf
    ok = np.isfinite(want)
    print("CPU checker: finite", ok.sum(), "largest rel", np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])))
    assert got[5] == -np.inf and want[5] == -np.inf
    assert ok.sum() >= 14 and np.array_equal(np.isfinite(got), ok)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-5, atol=1e-6)
