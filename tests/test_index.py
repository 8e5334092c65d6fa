"""Spectral indices on the device (vag_loglike_index_batch[_dev], Fitter.add_spectral_index, Fitter.spectral_indices): the log-slope
routine against 40 digits, the arithmetic against the numpy statement of the term (fitting.index_slope, held to 40 digits by
tests/test_index_host.py) on the device's own model values, a mixed fit, bits, edges, memory, the read-back and a fit.

The problem is C4 (configs.C4_TRUTH, default resolutions) with the 64 prior draws plus the truth of tests/test_counts.py.  Observed
indices are the device's own slope at the truth plus Gaussian noise of sigma = 0.05 .. 0.3, drawn once with a fixed seed."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_counts as tc
import test_index_host as ih
import test_limits as tl
import test_noise as tn
import test_sky_visfit as tv
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, sampling
from vegasafterglow_amd.fitting import index_from_slope, index_slope

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

P = fitting.ParamDef
defs, prior_draws, TRUTH, EPOCHS, DAY = tc.defs, tc.prior_draws, tc.TRUTH, tc.EPOCHS, tc.DAY
X_BAND, O_BAND = (7.25e16, 2.42e18), (3.3e14, 5e14)
A_V_TRUE = 0.3
A_V_DEF = [P("A_V", 0.0, 1.0)]


def new_fitter(**kw):
    tr = configs.C4_TRUTH
    return fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism", **kw)


def series_flux(params, t, nu):
    """tl.device_series (vag_flux_density_batch), [nb][n]: the request an index pass makes at its n K points.  A batch that holds a
    model the engine rejects raises; its walkers are then evaluated one by one and the rejected ones are rows of NaN."""
    def rejected(e):  # (grid capacity or an ODE row without an acceptable step: what scores -inf in a fit; anything else is an error)
        return "capacity" in str(e) or "ODE" in str(e)
    try:
        return tl.device_series(params, t, nu)
    except (ValueError, RuntimeError) as e:
        if not rejected(e):
            raise
    rows = []
    for p in params:
        try:
            rows.append(tl.device_series([p], t, nu)[0])
        except (ValueError, RuntimeError) as e:
            if not rejected(e):
                raise
            rows.append(np.full(np.size(t), np.nan))
    return np.array(rows)


def points(gd):
    """The n K points (t_i, nu_k) of a group, i outer."""
    return np.repeat(gd["t"], gd["nu"].size), np.tile(gd["nu"], gd["t"].size)


def group_slopes(f, gd, samples, d):
    """S [nb][n] of one group in numpy (index_slope, minus A_V ext_slope) on the device's series fluxes at the group's points; NaN
    rows for walkers the engine rejects."""
    pa = [f._params_at(s, d) for s in samples]
    ts, nus = points(gd)
    F = series_flux([p for p, _ in pa], ts, nus).reshape(len(pa), gd["t"].size, gd["nu"].size)
    ext = np.array([f._index_ext_slope(gd, float(p.z)) for p, _ in pa])
    return index_slope(F, gd["coef"]) - (np.array([a for _, a in pa]) * ext)[:, None]


def reference(f, samples, d, groups=None):
    """ln L of the fitter's index groups in numpy: -1/2 sum_i w_i ((S_i - s_i) / sigma_i)^2, rows with w = 0 left out; a walker the
    engine rejects, or whose value is not finite, is -inf."""
    total = np.zeros(len(samples))
    for gd in (f._index_obs if groups is None else groups):
        q = (group_slopes(f, gd, samples, d) - gd["value"]) / gd["err"]
        with np.errstate(invalid="ignore"):
            total = total - 0.5 * np.sum(np.where(gd["weights"] > 0, gd["weights"] * (q * q), 0.0), axis=-1)
    return np.where(np.isfinite(total), total, -np.inf)


def make_group(band, t, K, convention, seed, weights=None, truth=TRUTH, d=None, **fitter_kw):
    """The arguments of one add_spectral_index call: the device's own index at `truth` in the convention, plus Gaussian noise of
    sigma drawn from 0.05 .. 0.3, once, with a fixed seed."""
    t = np.asarray(t, float)
    probe = new_fitter(**fitter_kw)
    probe.add_spectral_index(band, t, np.zeros(t.size), np.ones(t.size), num_points=K, convention=convention)
    gd = probe._index_obs[0]
    S = group_slopes(probe, gd, [truth], defs() if d is None else d)[0]
    assert np.all(np.isfinite(S))
    back = np.empty(t.size)
    back[np.argsort(t, kind="stable")] = index_from_slope(S, convention)  # (the group's rows are sorted by t; the arguments need not be)
    rng = np.random.default_rng(seed)
    err = rng.uniform(0.05, 0.3, t.size)
    return dict(band=band, t=t, index=back + err * rng.standard_normal(t.size), err=err, num_points=K, convention=convention,
                weights=weights)


def index_fitter(groups, **kw):
    f = new_fitter(**kw)
    for g in groups:
        f.add_spectral_index(**g)
    return f


def case(name):
    """(groups, fitter keywords, parameter list, samples) of the arithmetic cases."""
    rng = np.random.default_rng(5)
    th, d, kw = prior_draws(), defs(), {}
    if name == "a":
        g = [make_group(X_BAND, EPOCHS, 2, "photon", seed=31)]
    elif name == "b":
        g = [make_group(X_BAND, EPOCHS[7:8], 2, "slope", seed=32)]
    elif name == "c":
        g = [make_group(X_BAND, np.geomspace(9 * DAY, 1000 * DAY, 70)[rng.permutation(70)], 5, "slope", seed=33,
                        weights=rng.uniform(0.5, 2.0, 70))]
    elif name == "d":
        kw, d = dict(extinction="smc"), defs(A_V_DEF)
        th = np.ascontiguousarray(np.column_stack([th, np.append(np.random.default_rng(6).uniform(0.0, 1.0, 64), A_V_TRUE)]))
        g = [make_group(O_BAND, EPOCHS, 8, "slope", seed=34, truth=th[-1], d=d, **kw)]
    elif name == "e":
        t = np.repeat(EPOCHS[::2], 2)  # pairs of equal times
        w = np.where(np.arange(20) % 4 == 1, 0.0, rng.uniform(0.5, 2.0, 20))
        g = [make_group(X_BAND, t, 3, "beta", seed=35, weights=w)]
    else:
        raise KeyError(name)
    return g, kw, d, th


@pytest.fixture(scope="module")
def group_a():
    return case("a")[0]


# ---------------------------------------------------------------- 1. the device routine
# measured on an MI355X: 0.447 units over the sweep (at K = 3, band ratio 2, slope 2.5, flux unit 1e-250; the numpy statement's
# own maximum over the sweep is 0.56); the gate is 4 x the maximum, 1.79.  A value above 8 would mean the pivot form is not what runs (the division
# is correctly rounded and the log good to about an ulp; the plain sum of logs is at hundreds of units).
MEASURED_SLOPE = 0.447
SLOPE_GATE = 4 * MEASURED_SLOPE


@pytest.fixture(scope="module")
def math_dev():
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def run(F, coef, K):
        x = np.ascontiguousarray(np.column_stack([F, coef, np.asarray(K, float)]), dtype=np.float64)
        assert x.shape[1] == 17
        out = np.full(x.shape[0], 7.0)
        _lib.check(lib.vag_debug_device_math(ctx, _lib.MATH_MORE["log_slope"], x.ctypes.data_as(dp), x.shape[0], out.ctypes.data_as(dp)))
        return out
    yield run
    lib.vag_ctx_destroy(ctx)


def test_log_slope_accuracy(math_dev):
    """vag::log_slope against mpmath at 40 digits over the sweep of tests/test_index_host.py (K in {2, 3, 5, 8}, band ratios
    1.05 .. 1e6, slopes -3 .. 2.5, flux units 1e-250 .. 1e250), the error in units of 2^-52 sum_{k >= 1} |c_k| (1 + |ln(F_k / F_0)|).
    Cap 8; gate SLOPE_GATE = 4 x the maximum measured on an MI355X.  A NaN, zero, negative or infinite F_k among the K returns NaN;
    entries from K on are not read."""
    F, coef, K = ih.slope_sweep()
    got = math_dev(F, coef, K)
    assert np.all(np.isfinite(got))
    err = ih.slope_errors(got, F, coef, K)
    k = int(np.argmax(err))
    measured = float(err[k])
    print("\n[device math] routine                     measured      gate   metric")
    print(f"[device math] {'log_slope':<26} {measured:10.3e} {SLOPE_GATE:9.2e}   units of 2^-52 S, at K = {K[k]}, F_0 = {F[k, 0]:.3e}, "
          f"F_K-1 / F_0 = {F[k, K[k] - 1] / F[k, 0]:.3e}")
    assert measured <= 8.0, "the pivot form is not what runs"
    assert MEASURED_SLOPE <= 8.0
    assert measured <= SLOPE_GATE, measured
    rows, want_nan = [], []
    base, c = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]), np.linspace(-1.0, 1.0, 8)
    for Kq in (2, 5, 8):
        for bad in (np.nan, 0.0, -1.0, np.inf, -0.0):
            for pos in range(8):
                row = base.copy()
                row[pos] = bad
                rows.append((row, c, Kq))
                want_nan.append(pos < Kq)
    out = math_dev(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), [r[2] for r in rows])
    assert np.array_equal(np.isnan(out), want_nan)
    assert np.all(np.isfinite(out[~np.array(want_nan)]))


# ---------------------------------------------------------------- 2. arithmetic
# measured on an MI355X, the largest |got - want| / max(1, |want|) over the 65 walkers: (a) 1.2e-15, (b) 5.9e-15, (c) 6.6e-16,
# (d) 7.0e-15, (e) 1.0e-15; the gate is 4 x the maximum over the cases, 2.8e-14.  All 65 walkers are finite in every case, (d)
# included (ln L from -237 to -4.6 there).
MEASURED_INDEX_ARITH = 7.0e-15
INDEX_ARITH_GATE = 4 * MEASURED_INDEX_ARITH


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_likelihood_matches_the_formula_on_device_fluxes(name):
    """64 prior draws plus the truth; ln L of an index-only fitter against the numpy statement on tl.device_series at the group's
    n K points, with tn.rel.  Cap 1e-9 (above it: an algebra error); gate INDEX_ARITH_GATE = 4 x the maximum measured on an MI355X
    -- the flux of a series request may follow the batch in its last bits, and those reach S multiplied by sum |c_k| / sigma, so the
    gate is measured here and not borrowed from the other groups.  (a) n = 20, K = 2, the X-ray band, photon indices; (b) n = 1;
    (c) n = 70, K = 5: a lane carries two rows; (d) K = 8 on 3.3e14 - 5e14 Hz under an SMC law with a free A_V; (e) beta, pairs of
    equal times, some rows with w = 0."""
    groups, kw, d, th = case(name)
    f = index_fitter(groups, **kw)
    gd = f._index_obs[0]
    if name == "c":
        assert gd["t"].size == 70 and gd["nu"].size == 5 and np.all(np.diff(gd["t"]) > 0)
    if name == "e":
        assert np.all(gd["t"][::2] == gd["t"][1::2]) and (gd["weights"] == 0).sum() == 5
    want = reference(f, th, d)
    got = f.loglike_batch(th, d)
    ok = np.isfinite(want)
    measured = tn.rel(got[ok], want[ok])
    print(f"index case ({name}): rel to the formula", measured, "finite", ok.sum(), "of", th.shape[0], "ln L range", want[ok].min(),
          want[ok].max(), "rejected", f.last_plan.n_walkers_rejected, "truth", got[-1])
    if name == "d":
        spec, _, _ = f.build_spec(d)
        ext = spec._index.groups[0].ext_slope
        assert ext != 0.0 and ext == f._index_ext_slope(gd, configs.C4_TRUTH["z"])
        zero = th.copy()
        zero[:, 3] = np.where(th[:, 3] > 0.5, 0.0, 1.0)
        other = f.loglike_batch(zero, d)
        print("index case (d): ext_slope", ext, "smallest change of ln L when A_V changes", np.abs(other - got)[ok].min())
        assert np.all(other[ok] != got[ok])  # A_V changes every walker's value
    assert np.isfinite(got[-1]) and ok.sum() >= 48  # the truth, and most of the box
    assert np.array_equal(np.isfinite(got), ok) and np.all(got[~ok] == -np.inf)
    assert f.last_plan.n_walkers_rejected == (~ok).sum()
    assert measured <= 1e-9, "an algebra error, not rounding"
    assert MEASURED_INDEX_ARITH <= 1e-9
    assert measured <= INDEX_ARITH_GATE, measured


# ---------------------------------------------------------------- 3. a mixed fit
SYS_A = tc.SYS_A


@pytest.fixture(scope="module")
def mixed(group_a):
    """Point data (60 C4 rows; band 0 in the noise group "a" with a fixed systematic, one limit row) + one add_flux group + one
    counts group + two index groups; each part as a fitter of its own; and the whole without its index groups."""
    c4t, c4nu = configs.c4_mock_data()
    truth = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], c4t, c4nu)[0]
    rng = np.random.default_rng(8)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(60)), 0.1 * truth
    lim = np.arange(60) == 17
    value = np.where(lim, 1.3 * truth, obs)
    radio = c4nu == configs.C4_BANDS[0]
    bt = EPOCHS[2::3]
    bflux = tc.device_flux([_abi.make_params(**configs.C4_TRUTH)], bt, tl.BAND, 7)[0] * (1 + 0.05 * rng.standard_normal(bt.size))
    counts = tc.case_args("a")[0]
    second = make_group(O_BAND, EPOCHS[1::2], 4, "beta", seed=36)

    def pts(f):
        f.add_flux_density(c4nu[radio], c4t[radio], value[radio], err[radio], upper_limit=lim[radio], noise="a", calibration=0.05)
        f.add_flux_density(c4nu[~radio], c4t[~radio], value[~radio], err[~radio], upper_limit=lim[~radio])

    builds = (pts, lambda f: f.add_flux(tl.BAND, bt, bflux, 0.1 * bflux, num_points=7), lambda f: f.add_counts(**counts),
              lambda f: f.add_spectral_index(**group_a[0]), lambda f: f.add_spectral_index(**second))
    parts = []
    for build in builds:
        f = new_fitter()
        build(f)
        parts.append(f)
    whole, rest = new_fitter(), new_fitter()
    for build in builds:
        build(whole)
    for build in builds[:3]:
        build(rest)
    return whole, parts, rest


def test_a_mixed_fit_is_the_sum_of_its_parts(mixed):
    """ln L of the whole against the sum of each part's own fit (no priors: nothing is counted twice) to INDEX_ARITH_GATE, and the
    index parts against the formula.  The whole without its index groups returns, through the new entry point with a NULL or empty
    index spec, the bits vag_loglike_counts_batch returns."""
    whole, parts, rest = mixed
    th = prior_draws()
    assert whole.has_spectral_indices and whole.has_counts and whole.has_limits and whole.has_noise_groups and len(whole._index_obs) == 2
    got = whole.loglike_batch(th, defs(SYS_A))
    each = [parts[0].loglike_batch(th, defs(SYS_A))] + [p.loglike_batch(th, defs()) for p in parts[1:]]
    want = np.sum(each, axis=0)
    ok = np.isfinite(want)
    print("mixed fit: rel to the sum of its parts", tn.rel(got[ok], want[ok]), "finite", ok.sum(), "parts at the truth", [e[-1] for e in each])
    assert ok[-1] and ok.sum() >= 48 and np.array_equal(np.isfinite(got), ok)
    assert tn.rel(got[ok], want[ok]) <= INDEX_ARITH_GATE
    index_part = reference(whole, th, defs(SYS_A))
    assert tn.rel((each[3] + each[4])[ok], index_part[ok]) <= INDEX_ARITH_GATE
    spec, _, _ = rest.build_spec(defs(SYS_A))
    assert spec._index is None and spec._counts is not None and spec._noise is not None
    rc, base = tc._raw("vag_loglike_counts_batch", spec, th, C.byref(spec._counts))
    assert rc == 0 and np.isfinite(base).sum() >= 48
    empty = _lib.IndexFitSpec()
    for isp in (None, C.byref(empty)):
        rc, out = tc._raw("vag_loglike_index_batch", spec, th, C.byref(spec._counts), isp)
        assert rc == 0 and np.array_equal(out, base)
    assert np.array_equal(rest.loglike_batch(th, defs(SYS_A)), base)


# ---------------------------------------------------------------- 4. bits
def test_bits(mixed, group_a):
    """The host entry and the device-pointer entry return the same bits, and so do two calls, a call in the identity evaluation
    order and the reversed batch (the same models, so the same launch choices).  A walker alone goes through a series request
    whose launch shape follows the batch, so its flux may differ from the batch's in the last bits: the term's independence of
    the other walkers is held to INDEX_ARITH_GATE.  Observed on an MI355X: every sixth walker alone returned the
    bits it returned among the 67, for the index-only fitter and for the mixed one."""
    import torch
    th = np.ascontiguousarray(np.vstack([tv._walkers(66, seed=12)[0], TRUTH]))
    th[40, 0] = np.nan  # one invalid walker
    for f, d in ((index_fitter(group_a + case("c")[0]), defs()), (mixed[0], defs(SYS_A))):
        a = f.loglike_batch(th, d)
        assert th.shape[0] == 67 and a[40] == -np.inf and np.all(np.isfinite(np.delete(a, 40))) and f.last_plan.n_walkers_rejected == 1
        assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
        assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
        ev = f.device_evaluator(d)
        assert ev.has_spectral_indices
        vals, _ = ev(torch.from_numpy(th).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(vals.cpu().numpy(), a)
        with pytest.raises(NotImplementedError, match="add_spectral_index"):
            ev.native.shard(None, 67, 0, 1, None)
        keep = np.arange(67) != 40
        rev = f.loglike_batch(np.ascontiguousarray(th[::-1]), d)[::-1]
        alone = np.array([f.loglike_batch(th[i:i + 1], d)[0] for i in range(0, 67, 6)])
        print("bits: reversed batch equal", np.array_equal(rev, a), "rel", tn.rel(rev[keep], a[keep]), "; alone equal",
              np.array_equal(alone, a[::6]), "rel", tn.rel(alone, a[::6]))
        assert np.array_equal(rev, a)
        assert tn.rel(alone, a[::6]) <= INDEX_ARITH_GATE


# ---------------------------------------------------------------- 5. edges
def test_edges(group_a):
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    d = defs()
    # no flux (far above the synchrotron cut-off): the slope is undefined, every walker scores -inf and is counted
    far = (1e29, 1e30)
    F = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], np.repeat(EPOCHS[:4], 2), np.tile([1e29, 1e30], 4))[0]
    assert np.all(F == 0)
    g = dict(band=far, t=EPOCHS[:4], index=[2.0, 2.1, 1.9, 2.0], err=[0.1, 0.1, 0.2, 0.1], convention="photon")
    base = index_fitter(group_a).loglike_batch(th, d)
    assert np.all(np.isfinite(base))
    h = index_fitter(group_a + [g])
    out = h.loglike_batch(th, d)
    assert np.all(out == -np.inf) and h.last_plan.n_walkers_rejected == 8
    # the same group with all weights 0 changes nothing
    h = index_fitter(group_a + [dict(g, weights=np.zeros(4))])
    out = h.loglike_batch(th, d)
    assert np.array_equal(out, base) and h.last_plan.n_walkers_rejected == 0
    # one weighted row among them is enough
    h = index_fitter(group_a + [dict(g, weights=[0.0, 0.0, 1e-3, 0.0])])
    assert np.all(h.loglike_batch(th, d) == -np.inf) and h.last_plan.n_walkers_rejected == 8
    # a walker the pass rejects is counted, and the context stays usable
    bad = th.copy()
    bad[2, 0] = -0.05  # theta_c < 0
    k = index_fitter(group_a)
    out = k.loglike_batch(bad, d)
    assert out[2] == -np.inf and np.array_equal(np.delete(out, 2), np.delete(base, 2)) and k.last_plan.n_walkers_rejected == 1
    assert np.array_equal(k.loglike_batch(th, d), base) and k.last_plan.n_walkers_rejected == 0


# ---------------------------------------------------------------- 6. memory, bad input
def test_device_memory_returns_after_destroy(group_a):
    lib = _lib.load()
    f = index_fitter(group_a + case("c")[0])
    d = defs()
    spec, _, _ = f.build_spec(d)
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    want = f.loglike_batch(th, d)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    out = np.empty(8)
    for _ in range(2):  # (the second call finds the groups resident)
        _lib.check(lib.vag_loglike_index_batch(ctx, C.byref(spec), None, None, None, None, None, None, C.byref(spec._index),
                                               th.ctypes.data_as(dp), 8, spec.ndim, out.ctypes.data_as(dp)))
        assert np.array_equal(out, want)
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before


def test_invalid_groups_through_the_c_abi_leave_the_context_usable(group_a):
    f, d = index_fitter(group_a), defs()
    th = np.ascontiguousarray(tv._walkers(4, seed=3)[0])
    spec, _, _ = f.build_spec(d)
    rc, good = tc._raw("vag_loglike_index_batch", spec, th, None, C.byref(spec._index))
    assert rc == 0 and np.all(np.isfinite(good))
    gd = f._index_obs[0]
    for key, i, v, word in (("value", 3, np.nan, "row 3"), ("err", 19, 0.0, "row 19"), ("t", 5, -1.0, "row 5"), ("nu", 1, 1e16, "frequency 1")):
        keep = gd[key][i]
        gd[key][i] = v
        rc, _ = tc._raw("vag_loglike_index_batch", spec, th, None, C.byref(spec._index))
        msg = tc.lib_error()
        assert rc == _lib.VAG_E_INVALID and "index group 0" in msg and word in msg, (rc, msg)
        gd[key][i] = keep
    rc, again = tc._raw("vag_loglike_index_batch", spec, th, None, C.byref(spec._index))
    assert rc == 0 and np.array_equal(again, good)
    other = dict(group_a[0], index=np.asarray(group_a[0]["index"]) + 0.5)  # other indices, same shapes: the resident copy must follow
    b = index_fitter([other]).loglike_batch(th, d)
    assert np.all(b != good) and np.array_equal(f.loglike_batch(th, d), good)


# ---------------------------------------------------------------- 7. the read-back
def test_fitter_spectral_indices_is_the_statement_on_the_groups_own_request():
    """Fitter.spectral_indices at the truth against index_slope on vag_flux_density_batch at each group's points, minus
    A_V ext_slope, mapped to the group's convention: to the bits (the same request of one model, the same numpy arithmetic)."""
    d = defs(A_V_DEF)
    truth = np.append(TRUTH, A_V_TRUE)
    f = new_fitter(extinction="smc")
    f.add_spectral_index(X_BAND, EPOCHS[::3], np.full(7, 2.0), np.full(7, 0.1), convention="photon")
    f.add_spectral_index(O_BAND, EPOCHS[::-4], np.full(5, 0.7), np.full(5, 0.1), num_points=8, convention="beta")
    f.add_spectral_index(O_BAND, EPOCHS[:3], np.full(3, -0.7), np.full(3, 0.1), num_points=3)
    got = f.spectral_indices(truth, d)
    assert len(got) == 3
    p = f._params_at(truth, d)[0]
    slopes = []
    for gd, g in zip(f._index_obs, got):
        ts, nus = points(gd)
        F = tl.device_series([p], ts, nus)[0].reshape(gd["t"].size, gd["nu"].size)
        S = index_slope(F, gd["coef"]) - A_V_TRUE * f._index_ext_slope(gd, configs.C4_TRUTH["z"])
        slopes.append(S)
        assert g.shape == gd["t"].shape and np.array_equal(g, index_from_slope(S, gd["convention"]))
    assert np.array_equal(got[0], 1.0 - slopes[0]) and np.array_equal(got[1], -slopes[1]) and np.array_equal(got[2], slopes[2])
    assert f._index_ext_slope(f._index_obs[1], configs.C4_TRUTH["z"]) > 0 and np.all(got[1] > 0)  # a red optical spectrum, reddened further
    plain = new_fitter()
    plain.add_spectral_index(O_BAND, EPOCHS[::-4], np.full(5, 0.7), np.full(5, 0.1), num_points=8, convention="beta")
    assert np.all(plain.spectral_indices(TRUTH, defs())[0] < got[1])  # without the law the spectrum is bluer


# ---------------------------------------------------------------- 8. a fit
FIT_MARGIN = 0.1


def test_a_fit_on_indices_and_three_flux_rows():
    """Photon indices at the 20 epochs (sigma 0.05 .. 0.3) and three X-ray flux rows to fix the normalisation, p free on 2.05 .. 2.8
    and everything else at the truth: 32 walkers x 60 steps from a ball around the prior centre (p = 2.425; the truth is 2.15).
    The median of the second half of the chain is closer to the truth than to the prior centre, and the chain's best ln L is at
    least ln L at the truth minus FIT_MARGIN = 0.1.  The maximum of ln L is never below its value at the truth; the margin is what
    the chain's best sample may miss the maximum by (0.1 is a sample 0.45 posterior standard deviations from it).  First run on
    an MI355X: ln L at the truth -5.998, best -5.854 (0.144 above the truth's) at p = 2.144; second-half median 2.149, standard
    deviation 0.020, from a start at 2.42; acceptance 0.62."""
    tr = configs.C4_TRUTH
    d = [P("p", 2.05, 2.8)] + _fixed_but_p()
    truth = np.array([tr["p"]])
    g = make_group(X_BAND, EPOCHS, 2, "photon", seed=37, truth=truth, d=d)
    f = index_fitter([g])
    t3 = EPOCHS[[2, 9, 16]]
    F3 = tl.device_series([_abi.make_params(**tr)], t3, np.full(3, 2.41e17))[0]
    f.add_flux_density(np.full(3, 2.41e17), t3, F3 * (1 + 0.05 * np.random.default_rng(38).standard_normal(3)), 0.1 * F3)
    lp_truth = f.log_prob_batch(truth[None], d)[0]
    centre = np.array([0.5 * (2.05 + 2.8)])
    nwalkers, nsteps = 32, 60
    res = sampling.fit(f, d, nwalkers=nwalkers, nsteps=nsteps, seed=4, center=centre, spread=0.02)
    tail = res["chain"][nsteps // 2:].reshape(-1)
    median = float(np.median(tail))
    print("fit on indices: truth", lp_truth, "best", res["log_prob"].max(), "at", res["best"], "second half median", median, "std",
          tail.std(), "start", np.median(res["chain"][0]), "acceptance", res["acceptance"].mean())
    assert np.isfinite(lp_truth) and np.all(np.isfinite(res["log_prob"][-nwalkers:]))
    assert abs(median - truth[0]) < abs(median - centre[0])
    assert res["log_prob"].max() >= lp_truth - FIT_MARGIN


def _fixed_but_p():
    tr = configs.C4_TRUTH
    vals = dict(E_iso=tr["E_iso"], Gamma0=tr["Gamma0"], theta_c=tr["theta_c"], theta_v=tr["theta_obs"], n_ism=tr["n_ism"],
                eps_e=tr["eps_e"], eps_B=tr["eps_B"])
    return [P(k, v, v, fitting.Scale.fixed) for k, v in vals.items()]
