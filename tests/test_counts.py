"""Photon counts with a Poisson likelihood on the device (vag_loglike_counts_batch[_dev], Fitter.add_counts, Fitter.counts): the
deviance routine against 40 digits, the arithmetic against the numpy statement of the term (tests/test_counts_host.py) on the
device's own model values, bits, edges, a fit and the expected counts.

The problem is C4 (configs.C4_TRUTH, default resolutions), band 7.25e16 - 2.42e18 Hz with 5 Boole nodes.  Every group's conversions
are chosen so that mu at the truth runs over 1e-2 .. 1e6 along its rows (with a background on every third row), and its counts are
drawn once, with a fixed seed, from the device's own truth: N = 0 rows, single counts and large N all occur."""
import ctypes as C
import math

import numpy as np
import pytest

import _abi
import _mathref as R
import configs
import test_counts_host as ch
import test_limits as tl
import test_noise as tn
import test_sky_visfit as tv
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

P = fitting.ParamDef
FLUX_DEFS, _c4_fixed = tv.FLUX_DEFS, tv._c4_fixed
BAND, NUM_POINTS = (7.25e16, 2.42e18), 5
DAY = 86400.0
TRUTH = np.array([configs.C4_TRUTH["theta_c"], configs.C4_TRUTH["theta_obs"], np.log10(configs.C4_TRUTH["E_iso"])])


def defs(extra=()):
    return FLUX_DEFS + list(extra) + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))


def new_fitter():
    tr = configs.C4_TRUTH
    return fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")


def device_flux(params, t, band=BAND, num_points=NUM_POINTS):
    """vag_flux_batch: the device's band fluxes at times t, [nb][nt] -- the request a counts pass makes on its merged sample times.
    A batch that holds a model the engine rejects raises; its walkers are then evaluated one by one (a walker's value does not
    depend on the batch) and the rejected ones are rows of NaN."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    t = np.ascontiguousarray(t, float)

    def run(ps):
        arr = (_lib.ModelParams * len(ps))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in ps])
        out = np.empty((len(ps), t.size))
        with lock:
            _lib.check(lib.vag_flux_batch(h, arr, len(ps), t.ctypes.data_as(dp), t.size, band[0], band[1], num_points,
                                          out.ctypes.data_as(dp)))
        return out

    def rejected(e):  # (grid capacity or an ODE row without an acceptable step: what scores -inf in a fit; anything else is an error)
        return "capacity" in str(e) or "ODE" in str(e)
    try:
        return run(params)
    except (ValueError, RuntimeError) as e:
        if not rejected(e):
            raise
    rows = []
    for p in params:
        try:
            rows.append(run([p])[0])
        except (ValueError, RuntimeError) as e:
            if not rejected(e):
                raise
            rows.append(np.full(t.size, np.nan))
    return np.array(rows)


def make_group(t_start, exposure, m, seed, weights=None, band=BAND, num_points=NUM_POINTS):
    """The arguments of one add_counts call whose mu at the truth is geomspace(1e-2, 1e6) along the rows in a shuffled order, with a
    background of 30 % of mu on every third row; N ~ Poisson(mu) once, with a fixed seed."""
    t_start, exposure = np.asarray(t_start, float), np.asarray(exposure, float)
    n = t_start.size
    probe = new_fitter()
    probe.add_counts(band, t_start, exposure, np.zeros(n), 1.0, num_points=num_points, num_exposure_points=m)
    cd = probe._counts_obs[0]
    F = device_flux([_abi.make_params(**configs.C4_TRUTH)], cd["t_sample"], band, num_points)[0]
    assert np.all(F > 0)
    rng = np.random.default_rng(seed)
    target = rng.permutation(np.geomspace(1e-2, 1e6, n)) if n > 1 else np.array([30.0])
    bkg = np.where(np.arange(n) % 3 == 1, 0.3 * target, 0.0)
    mean_flux = ch.counts_mu(0.0, 1.0 / m, cd["sample_idx"], F)
    conversion = (target - bkg) / (exposure * mean_flux)
    counts = rng.poisson(target).astype(float)
    return dict(band=band, t_start=t_start, exposure=exposure, counts=counts, conversion=conversion, background=bkg,
                num_points=num_points, num_exposure_points=m, weights=weights)


def reference(f, samples, d, groups=None):
    """ln L of the fitter's counts groups in numpy (ch.counts_lnl) on vag_flux_batch at each group's merged sample times; a walker
    the engine rejects, or whose value is not finite, is -inf."""
    params = [f._params_at(s, d)[0] for s in samples]
    total = np.zeros(len(params))
    for cd in (f._counts_obs if groups is None else groups):
        F = device_flux(params, cd["t_sample"], (cd["nu_min"], cd["nu_max"]), cd["num_points"])
        total = total + ch.counts_lnl(cd["counts"], cd["background"], cd["scale"], cd["sample_idx"], cd["weights"], F)
    return np.where(np.isfinite(total), total, -np.inf)


def prior_draws(nb=64, seed=21):
    """nb draws of the boxes of FLUX_DEFS (theta_c, theta_v, log10 E_iso), then the truth."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([0.02, 0.0, 50.0]), np.array([0.3, 0.8, 54.0])
    return np.ascontiguousarray(np.vstack([lo + (hi - lo) * rng.random((nb, 3)), TRUTH]))


EPOCHS = configs.C4_EPOCHS
EDGES = np.round(np.geomspace(9 * DAY, 1000 * DAY, 21) / 2000.0) * 2000.0  # contiguous bins whose ends and midpoints are exact


def case_args(name):
    rng = np.random.default_rng(3)
    if name == "a":
        return [make_group(EPOCHS, np.full(20, 5e4), 1, seed=11, weights=rng.uniform(0.5, 2.0, 20))]
    if name == "b":
        return [make_group(EPOCHS[7:8], [3e4], 1, seed=12)]
    if name == "c":
        return [make_group(np.geomspace(9 * DAY, 1000 * DAY, 70)[rng.permutation(70)], np.full(70, 2e4), 1, seed=13)]
    if name == "d":
        return [make_group(EDGES[:-1], np.diff(EDGES), 3, seed=14)]
    if name == "e":
        return [make_group(EPOCHS, 0.8 * EPOCHS, 3, seed=15, weights=rng.uniform(0.5, 2.0, 20))]
    raise KeyError(name)


def counts_fitter(groups):
    f = new_fitter()
    for g in groups:
        f.add_counts(**g)
    return f


@pytest.fixture(scope="module")
def group_a():
    return case_args("a")


# ---------------------------------------------------------------- 1. the deviance routine
# measured on an MI355X: 7.916e-16 over the sweep and the switch points (at N = 10, mu = 1.5 N, the first point of the direct branch;
# 4.5e-16 in the series branch); the gate is 4 x the maximum, 3.17e-15.  A value above 1e-13 would mean the routine is not doing its
# job (the naive x - log1p(x) is at 2e-13 already for |x| > 1e-3).
MEASURED_DEVIANCE = 7.916e-16
DEVIANCE_GATE = 4 * MEASURED_DEVIANCE


@pytest.fixture(scope="module")
def math_dev():
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def run(N, mu):
        x = np.ascontiguousarray(np.column_stack([N, mu]), dtype=np.float64)
        out = np.full(x.shape[0], np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, _lib.MATH_MORE["poisson_deviance"], x.ctypes.data_as(dp), x.shape[0], out.ctypes.data_as(dp)))
        return out
    yield run
    lib.vag_ctx_destroy(ctx)


def test_poisson_deviance_accuracy(math_dev):
    """D(N, mu) against mpmath at 40 digits: N in {1, 2, 3, 10, 1e3, 1e6, 1e9}, mu / N - 1 = +-10^u with u on 241 points of [-12, 0)
    and 121 of (0, 6] (the negative branch stops where mu would not be positive), and the points within 4 ulp of the switch
    |mu - N| = N / 2 on both sides.  Expected from the form: a few 1e-16 in the series branch, up to ~1e-15 just outside the switch
    (two terms of opposite sign, ten times the result).  Gate: DEVIANCE_GATE = 4 x the maximum measured on an MI355X; the measured
    maximum must be below 1e-13.  The exact results: D(N, N) = 0, D(0, mu) = mu, D(N > 0, 0) = +inf, NaN stays NaN."""
    mp = R.mpmath
    Ns = [1.0, 2.0, 3.0, 10.0, 1e3, 1e6, 1e9]
    us = np.concatenate([np.linspace(-12.0, 0.0, 241)[:-1], np.linspace(0.0, 6.0, 121)[1:]])
    N, mu = [], []
    for n in Ns:
        for sign in (1.0, -1.0):
            m = n * (1.0 + sign * 10.0 ** us)
            m = m[m > 0]
            N.append(np.full(m.size, n))
            mu.append(m)
        near = np.array([tl.np_nudge(c * n, k) for c in (0.5, 1.5) for k in range(-4, 5)])
        N.append(np.full(near.size, n))
        mu.append(near)
    N, mu = np.concatenate(N), np.concatenate(mu)
    got = math_dev(N, mu)
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    with mp.workdps(40):
        err = np.empty(N.size)
        for i, (n, m, g) in enumerate(zip(N, mu, got)):
            nm, mm = mp.mpf(float(n)), mp.mpf(float(m))
            ref = mm - nm - nm * mp.log(mm / nm)
            err[i] = float(abs(mp.mpf(float(g)) - ref) / ref) if ref != 0 else abs(g)
    k = int(np.argmax(err))
    measured = float(err[k])
    series = np.abs(mu - N) <= 0.5 * N
    print("\n[device math] routine                     measured      gate   metric")
    print(f"[device math] {'poisson_deviance':<26} {measured:10.3e} {DEVIANCE_GATE:9.2e}   relative, at N = {N[k]:g}, mu / N - 1 = "
          f"{mu[k] / N[k] - 1:.3e}; series branch {err[series].max():.3e}, direct branch {err[~series].max():.3e}")
    assert measured < 1e-13, "the routine is not doing its job"
    assert MEASURED_DEVIANCE < 1e-13
    assert measured <= DEVIANCE_GATE, measured
    exact = math_dev(np.array([5.0, 1e9, 0.0, 0.0, 3.0, 1e9, np.nan, 2.0, 0.0]),
                     np.array([5.0, 1e9, 2.5, 0.0, 0.0, 0.0, 1.0, np.nan, np.nan]))
    assert np.array_equal(exact[:4], [0.0, 0.0, 2.5, 0.0]) and exact[4] == np.inf and exact[5] == np.inf
    assert np.all(np.isnan(exact[6:]))


# ---------------------------------------------------------------- 2. arithmetic
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_likelihood_matches_the_formula_on_device_fluxes(name):
    """64 prior draws plus the truth; ln L of a counts-only fitter against ch.counts_lnl on vag_flux_batch at the group's merged
    sample times, to tn.ARITH_GATE with tn.rel (the tolerance of the noise groups' formula comparison).  (a) n = 20, m = 1;
    (b) n = 1; (c) n = 70: a lane carries two rows; (d) m = 3, contiguous bins; (e) m = 3, overlapping windows."""
    groups = case_args(name)
    f, d, th = counts_fitter(groups), defs(), prior_draws()
    cd = f._counts_obs[0]
    N = cd["counts"]
    if name in "ace":
        assert (N == 0).any() and ((N > 0) & (N <= 5)).any() and N.max() > 1e5, N
    if name == "c":
        assert N.size == 70
    if name == "d":
        assert cd["t_sample"].size == 41 and cd["m"] == 3  # 20 bins x 3 samples, the 19 shared ends once
    if name == "e":
        assert np.all(cd["sample_idx"][1:, 0] < cd["sample_idx"][:-1, 2])  # every window starts inside the one before it
    want = reference(f, th, d)
    got = f.loglike_batch(th, d)
    ok = np.isfinite(want)
    measured = tn.rel(got[ok], want[ok])
    print(f"counts case ({name}): rel to the formula", measured, "finite", ok.sum(), "of", th.shape[0], "ln L range", want[ok].min(),
          want[ok].max(), "rejected", f.last_plan.n_walkers_rejected)
    assert np.isfinite(got[-1]) and ok.sum() >= 48  # the truth, and most of the box
    assert np.array_equal(np.isfinite(got), ok) and np.all(got[~ok] == -np.inf)
    assert f.last_plan.n_walkers_rejected == (~ok).sum()
    assert measured <= tn.ARITH_GATE, measured


@pytest.fixture(scope="module")
def mixed(group_a):
    """(f) point data (60 C4 rows; band 0 in the noise group "a" with a fixed systematic, one limit row) + one add_flux group + two
    counts groups, and each part as a fitter of its own."""
    c4t, c4nu = configs.c4_mock_data()
    truth = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], c4t, c4nu)[0]
    rng = np.random.default_rng(8)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(60)), 0.1 * truth
    lim = np.arange(60) == 17
    value = np.where(lim, 1.3 * truth, obs)
    radio = c4nu == configs.C4_BANDS[0]
    bt = EPOCHS[2::3]
    bflux = device_flux([_abi.make_params(**configs.C4_TRUTH)], bt, tl.BAND, 7)[0] * (1 + 0.05 * rng.standard_normal(bt.size))
    second = make_group(EPOCHS[1::2], 0.5 * EPOCHS[1::2], 2, seed=16, band=(1e17, 1e18), num_points=7)

    def points(f):
        f.add_flux_density(c4nu[radio], c4t[radio], value[radio], err[radio], upper_limit=lim[radio], noise="a", calibration=0.05)
        f.add_flux_density(c4nu[~radio], c4t[~radio], value[~radio], err[~radio], upper_limit=lim[~radio])

    def band(f):
        f.add_flux(tl.BAND, bt, bflux, 0.1 * bflux, num_points=7)
    parts = []
    for build in (points, band, lambda f: f.add_counts(**group_a[0]), lambda f: f.add_counts(**second)):
        f = new_fitter()
        build(f)
        parts.append(f)
    whole = new_fitter()
    points(whole)
    band(whole)
    whole.add_counts(**group_a[0])
    whole.add_counts(**second)
    return whole, parts


SYS_A = [P("sys_a", 0.08, 0.08, fitting.Scale.fixed)]


def test_a_mixed_fit_is_the_sum_of_its_parts(mixed):
    """(f): ln L of the whole against the sum of each part's own fit (no priors: nothing is counted twice), and against the formula
    for its two counts groups.  The parts' chi^2 are the whole's pass by pass, so the sum differs by the rounding of three additions."""
    whole, parts = mixed
    th = prior_draws()
    assert whole.has_counts and whole.has_limits and whole.has_noise_groups and len(whole._counts_obs) == 2
    got = whole.loglike_batch(th, defs(SYS_A))
    each = [parts[0].loglike_batch(th, defs(SYS_A))] + [p.loglike_batch(th, defs()) for p in parts[1:]]
    want = np.sum(each, axis=0)
    ok = np.isfinite(want)
    print("mixed fit: rel to the sum of its parts", tn.rel(got[ok], want[ok]), "finite", ok.sum(), "parts at the truth", [e[-1] for e in each])
    assert ok[-1] and ok.sum() >= 48 and np.array_equal(np.isfinite(got), ok)
    assert tn.rel(got[ok], want[ok]) <= tn.ARITH_GATE
    counts_part = reference(whole, th, defs(SYS_A))
    assert tn.rel((each[2] + each[3])[ok], counts_part[ok]) <= tn.ARITH_GATE


# ---------------------------------------------------------------- 3. bits
def _raw(name, spec, samples, *extra):
    lib = _lib.load()
    h, lock = va.get_context(0)
    out = np.empty(samples.shape[0])
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    with lock:
        rc = getattr(lib, name)(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise),
                                *extra, samples.ctypes.data_as(dp), samples.shape[0], spec.ndim, out.ctypes.data_as(dp))
    return rc, out


def test_bits(mixed, group_a):
    import torch
    th = np.ascontiguousarray(np.vstack([tv._walkers(66, seed=12)[0], TRUTH]))
    th[40, 0] = np.nan  # one invalid walker
    for f, d in ((counts_fitter(group_a + case_args("d")), defs()), (mixed[0], defs(SYS_A))):
        a = f.loglike_batch(th, d)
        assert th.shape[0] == 67 and a[40] == -np.inf and np.all(np.isfinite(np.delete(a, 40))) and f.last_plan.n_walkers_rejected == 1
        assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
        assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
        assert np.array_equal(f.loglike_batch(np.ascontiguousarray(th[::-1]), d)[::-1], a)
        alone = np.array([f.loglike_batch(th[i:i + 1], d)[0] for i in range(67)])
        assert np.array_equal(alone, a)
        ev = f.device_evaluator(d)
        assert ev.has_counts
        vals, _ = ev(torch.from_numpy(th).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(vals.cpu().numpy(), a)
        with pytest.raises(NotImplementedError, match="add_counts"):
            ev.native.shard(None, 67, 0, 1, None)
    # a fit without counts groups through the new entry point is the noise call
    plain = mixed[1][0]
    spec, _, _ = plain.build_spec(defs(SYS_A))
    assert spec._counts is None and spec._noise is not None
    rc, want = _raw("vag_loglike_noise_batch", spec, th)
    assert rc == 0 and np.isfinite(want).sum() == 66
    empty = _lib.CountsFitSpec()
    for cs in (None, C.byref(empty)):
        rc, got = _raw("vag_loglike_counts_batch", spec, th, cs)
        assert rc == 0 and np.array_equal(got, want)


def test_bits_where_the_batch_would_choose_another_flux_kernel():
    """What a band request takes from the batch, and a counts pass must not.  (1) From 262144 (theta, phi) pairs on, a band of at
    most 4 nodes with at most 128 times goes to the row-per-lane kernel, which sums in another order: 560 walkers (about 500 pairs
    each) on a group with num_points = 4, every eighth walker alone and the first 100 as a batch of their own, to the bits.
    (2) The lane count of the workgroup kernel and its persistent form follow the batch's sizes: forced the other way by their
    hooks, the same bits, for that group and for a 5-node one."""
    narrow = counts_fitter([make_group(EPOCHS[::3], np.full(7, 4e4), 1, seed=17, num_points=4)])
    d = defs()
    th = np.ascontiguousarray(np.vstack([tv._walkers(559, seed=31)[0], TRUTH]))
    a = narrow.loglike_batch(th, d)
    cd = narrow._counts_obs[0]
    print("large narrow batch: total_pairs", narrow.last_plan.total_pairs, "pairs per block", narrow.last_plan.pairs_per_block)
    assert cd["num_points"] <= 4 and cd["t_sample"].size <= 128 and cd["t_sample"].size * cd["num_points"] <= 512
    assert narrow.last_plan.total_pairs >= 4096 * 64 and narrow.last_plan.total_pairs >= 128 * th.shape[0]
    assert np.all(np.isfinite(a)) and narrow.last_plan.n_walkers_rejected == 0
    assert np.array_equal(a, narrow.loglike_batch(th, d))
    alone = np.array([narrow.loglike_batch(th[i:i + 1], d)[0] for i in range(0, 560, 8)])
    assert np.array_equal(alone, a[::8])
    assert np.array_equal(narrow.loglike_batch(th[:100], d), a[:100])
    few = np.ascontiguousarray(th[-67:])
    for f in (narrow, counts_fitter(case_args("a"))):
        base = f.loglike_batch(few, d)
        assert np.all(np.isfinite(base))
        for hook, value in (("VAG_FLUX_WIDE", "1"), ("VAG_FLUX_PERSISTENT", "0"), ("VAG_FLUX_PERSISTENT", "2")):
            assert np.array_equal(tv._with_hook(hook, value, lambda: f.loglike_batch(few, d)), base), (hook, value)


# ---------------------------------------------------------------- 4. edges
def _lgamma_lnl(N, mu, w):
    return float(sum(wi * (n * math.log(m) - m - math.lgamma(n + 1)) for n, m, wi in zip(N, mu, w)))


def test_edges(group_a):
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    d = defs()
    # background only: a conversion so small that a F is lost in B.  The closed form with lgamma: three terms of at most 200 each,
    # so 1e-13 of the value (about -30) is more than its rounding
    N, B, w = np.array([0.0, 1.0, 4.0, 50.0, 17.0]), np.array([0.5, 2.0, 3.0, 40.0, 17.0]), np.array([1.0, 0.5, 2.0, 1.0, 1.5])
    f = new_fitter()
    f.add_counts(BAND, EPOCHS[:5], np.full(5, 1e4), N, 1e-200, background=B, weights=w)
    got = f.loglike_batch(th, d)
    want = _lgamma_lnl(N, B, w)
    print("background only:", got, "closed form", want)
    assert np.all(got == got[0]) and abs(got[0] - want) <= 1e-13 * abs(want) and f.last_plan.n_walkers_rejected == 0
    # the constant: mu = N on every row, so D = 0 and ln L = sum w S
    g = new_fitter()
    Nc = np.array([1.0, 2.0, 15.0, 16.0, 1e4, 1e9])
    wc = np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.25])
    g.add_counts(BAND, EPOCHS[:6], np.full(6, 1e4), Nc, 1e-200, background=Nc, weights=wc)
    got = g.loglike_batch(th, d)
    want = float(np.sum(wc * ch.poisson_const(Nc)))
    print("the constant:", got[0], "sum w S", want)
    assert np.all(got == got[0]) and abs(got[0] - want) <= tn.ARITH_GATE * max(1.0, abs(want))
    # no flux (far above the synchrotron cut-off): -inf when a row with N > 0 has no background, finite when all such rows have N = 0
    far = (1e29, 1e30)
    assert np.all(device_flux([f._params_at(s, d)[0] for s in th], EPOCHS[:4], far) == 0)
    h = new_fitter()
    h.add_counts(far, EPOCHS[:4], np.full(4, 1e4), [0, 3, 0, 2], 1e11, background=[0.0, 1.5, 0.0, 0.0])
    out = h.loglike_batch(th, d)
    assert np.all(out == -np.inf) and h.last_plan.n_walkers_rejected == 8
    h = new_fitter()
    h.add_counts(far, EPOCHS[:4], np.full(4, 1e4), [0, 3, 0, 2], 1e11, background=[0.0, 1.5, 0.0, 2.5])
    out = h.loglike_batch(th, d)
    want = _lgamma_lnl([3, 2], [1.5, 2.5], [1.0, 1.0])  # the N = 0 rows with mu = 0 add 0
    assert np.all(out == out[0]) and abs(out[0] - want) <= 1e-13 * abs(want) and h.last_plan.n_walkers_rejected == 0
    # rows with w = 0 change nothing, whatever they hold (same windows: the sample times, and so the request, are the same)
    a = group_a[0]
    base = counts_fitter([a]).loglike_batch(th, d)
    more = dict(a)
    for key, extra in (("t_start", a["t_start"][:6]), ("exposure", a["exposure"][:6]), ("counts", [0, 1, 7, 1e9, 3, 2.0 ** 53]),
                       ("conversion", a["conversion"][:6] * 1e30), ("background", [0.0, 5.0, 0.0, 0.0, 1e300, 0.0]),
                       ("weights", np.zeros(6))):
        more[key] = np.concatenate([a[key], extra])
    assert np.all(np.isfinite(base)) and np.array_equal(counts_fitter([more]).loglike_batch(th, d), base)
    # a walker the counts pass rejects is counted
    bad = th.copy()
    bad[2, 0] = np.nan
    k = counts_fitter([a])
    out = k.loglike_batch(bad, d)
    assert out[2] == -np.inf and np.array_equal(np.delete(out, 2), np.delete(base, 2)) and k.last_plan.n_walkers_rejected == 1


def test_device_memory_returns_after_destroy(group_a):
    lib = _lib.load()
    f = counts_fitter(group_a + case_args("d"))
    d = defs()
    spec, _, _ = f.build_spec(d)
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    want = f.loglike_batch(th, d)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    out = np.empty(8)
    for _ in range(2):  # (the second call finds the groups resident)
        _lib.check(lib.vag_loglike_counts_batch(ctx, C.byref(spec), None, None, None, None, None, C.byref(spec._counts),
                                                th.ctypes.data_as(dp), 8, spec.ndim, out.ctypes.data_as(dp)))
        assert np.array_equal(out, want)
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before


def test_invalid_counts_through_the_c_abi_leave_the_context_usable(group_a):
    f, d = counts_fitter(group_a), defs()
    th = np.ascontiguousarray(tv._walkers(4, seed=3)[0])
    spec, _, _ = f.build_spec(d)
    rc, good = _raw("vag_loglike_counts_batch", spec, th, C.byref(spec._counts))
    assert rc == 0 and np.all(np.isfinite(good))
    cd = f._counts_obs[0]
    for key, i, v, word in (("counts", 3, 0.5, "row 3"), ("scale", 19, 0.0, "row 19"), ("t_sample", 5, -1.0, "sample 5")):
        keep = cd[key][i]
        cd[key][i] = v
        rc, _ = _raw("vag_loglike_counts_batch", spec, th, C.byref(spec._counts))
        msg = lib_error()
        assert rc == _lib.VAG_E_INVALID and "counts group 0" in msg and word in msg, (rc, msg)
        cd[key][i] = keep
    rc, again = _raw("vag_loglike_counts_batch", spec, th, C.byref(spec._counts))
    assert rc == 0 and np.array_equal(again, good)
    other = dict(group_a[0], counts=group_a[0]["counts"] + 1.0)  # other counts, same shapes: the resident copy must follow
    b = counts_fitter([other]).loglike_batch(th, d)
    assert np.all(b != good) and np.array_equal(f.loglike_batch(th, d), good)


def lib_error():
    return _lib.load().vag_last_error().decode()


# ---------------------------------------------------------------- 5. a fit
def test_a_fit_on_counts_alone(group_a):
    """Counts-only data (case a), theta_v and E_iso free: sampling.fit with 32 walkers and 40 steps from a ball around the truth
    (the scale of test_limits.test_a_fit_with_limits).  Every walker ends with a finite log-probability, the best sample's is at or
    above the truth's, and the truth lies within 3 standard deviations of the second half of the chain from its mean, in both
    parameters."""
    tr = configs.C4_TRUTH
    f = counts_fitter(group_a)
    d = [P("theta_v", 0.0, 0.8), P("E_iso", 1e50, 1e54, fitting.Scale.log)] + _c4_fixed(skip=("theta_v", "E_iso"))
    truth = np.array([tr["theta_obs"], np.log10(tr["E_iso"])])
    lp_truth = f.log_prob_batch(truth[None], d)[0]
    nwalkers, nsteps = 32, 40
    res = sampling.fit(f, d, nwalkers=nwalkers, nsteps=nsteps, seed=4, center=truth, spread=0.02)
    last = res["log_prob"][-nwalkers:]
    tail = res["chain"][nsteps // 2:].reshape(-1, 2)
    mean, std = tail.mean(axis=0), tail.std(axis=0)
    print("fit on counts: truth", lp_truth, "best", res["log_prob"].max(), "at", res["best"], "second half mean", mean, "std", std,
          "truth", truth, "acceptance", res["acceptance"].mean())
    assert np.isfinite(lp_truth) and np.all(np.isfinite(last))
    assert res["log_prob"].max() >= lp_truth
    assert np.all(std > 0) and np.all(np.abs(mean - truth) <= 3 * std)


# ---------------------------------------------------------------- 6. the expected counts
def test_fitter_counts_is_mu_on_the_groups_own_flux_request(group_a):
    """Fitter.counts against B + a sum F with F from vag_flux_batch on the group's merged sample times, to the bits.  (The
    likelihood's own mu comes from the same request with a pinned workgroup size and may differ from it in the last bits; the
    arithmetic tests hold the likelihood to that F within their gate.)"""
    f = counts_fitter(group_a + case_args("e"))
    d = defs()
    mu = f.counts(TRUTH, d)
    assert len(mu) == 2
    for cd, got in zip(f._counts_obs, mu):
        F = device_flux([f._params_at(TRUTH, d)[0]], cd["t_sample"])[0]
        want = ch.counts_mu(cd["background"], cd["scale"], cd["sample_idx"], F)
        assert got.shape == cd["counts"].shape and np.array_equal(got, want)
    target = np.sort(mu[0])
    assert target[0] == pytest.approx(1e-2, rel=1e-12) and target[-1] == pytest.approx(1e6, rel=1e-12)  # as the conversions were chosen
