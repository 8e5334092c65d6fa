"""Count spectra through an instrument response on the device (vag_loglike_fold_batch[_dev], Fitter.add_count_spectrum,
Fitter.count_spectra): the arithmetic against the numpy statement of the term (fitting.fold_expected, held to its formulas by
tests/test_fold_host.py, with the Poisson statements of tests/test_counts_host.py) on the device's own model values, the rules, a
mixed fit, bits, the empty spec, bad input, memory, the read-back and a profile in N_H.

The problem is C4 (configs.C4_TRUTH, default resolutions) with the 64 prior draws plus the truth of tests/test_counts.py; energies
are 0.3 - 10 keV.  The response of every group is a smooth redistribution (a Gaussian in channel around each bin's own channel, times
an effective area that rises and falls), scaled so that mu at the truth has a stated mean; counts are drawn once, with a fixed seed,
from the numpy statement at the truth.  The reference is never the likelihood's own output."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_counts as tc
import test_counts_host as ch
import test_index as ti
import test_limits as tl
import test_noise as tn
import test_sky_visfit as tv
from test_index import group_a, mixed  # noqa: F401  (fixtures: the mixed fit of tests/test_index.py)
from vegasafterglow_amd import _lib, fitting
from vegasafterglow_amd.fitting import fold_expected

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

P = fitting.ParamDef
defs, prior_draws, TRUTH, EPOCHS, DAY = tc.defs, tc.prior_draws, tc.TRUTH, tc.EPOCHS, tc.DAY
new_fitter, series_flux = ti.new_fitter, ti.series_flux
N_H_DEF = [P("N_H", 1e20, 1e23, fitting.Scale.log)]
LOG_N_H_TRUE = 22.0


def bins(J, lo=0.3, hi=10.0):
    e = np.geomspace(lo, hi, J + 1)
    return e[:-1].copy(), e[1:].copy()


def cross_section(lo, hi):
    """A photoelectric-like cross-section [cm^2 per H atom] at the bins: 2e-22 (E / keV)^-2.5, tau = 2 at 1 keV for N_H = 1e22."""
    return 2e-22 * np.sqrt(lo * hi) ** -2.5


def response(J, nC, rng):
    """R [C][J]: bin j lands in channel (j + 1/2) C / J with a Gaussian spread of max(0.6, C / J) channels; the area rises and falls."""
    centre = (np.arange(J) + 0.5) * nC / J
    width = max(0.6, nC / J)
    red = np.exp(-0.5 * ((np.arange(nC)[:, None] + 0.5 - centre[None, :]) / width) ** 2)
    red /= red.sum(axis=0, keepdims=True)
    area = 100.0 * np.sin(np.pi * (np.arange(J) + 0.5) / J) ** 2 + 5.0 + rng.uniform(0.0, 1.0, J)
    return red * area[None, :]


def points(gd):
    """The n_samples J points (t_sample_s, nu_j) of a group, s outer."""
    return np.repeat(gd["t_sample"], gd["nu"].size), np.tile(gd["nu"], gd["t_sample"].size)


def n_h_of(f, samples, d):
    """N_H of every sample: the free parameter's value, else the fixed one."""
    spec, _, _ = f.build_spec(d)
    out = np.full(len(samples), spec._fold.n_h_fixed)
    for k in range(spec.ndim):
        if spec.slot[k] == _lib.P_N_H:
            v = np.asarray(samples)[:, k]
            out = 10.0 ** v if spec.is_log[k] else v.copy()
    return out


def group_mu(f, gd, samples, d):
    """mu [nb][n][C] of one group in numpy (fold_expected) on the device's series fluxes at the group's points; NaN for walkers the
    engine rejects."""
    params = [f._params_at(s, d)[0] for s in samples]
    ts, nus = points(gd)
    return fold_expected(series_flux(params, ts, nus), gd, n_h_of(f, samples, d))


def reference(f, samples, d, groups=None):
    """ln L of the fitter's fold groups in numpy: sum w [N ln mu - mu - ln N!] as -sum w D + sum w S (ch.poisson_deviance,
    ch.poisson_const), channels with w = 0 left out; a walker the engine rejects, or whose value is not finite, is -inf."""
    total = np.zeros(len(samples))
    for gd in (f._fold_obs if groups is None else groups):
        mu = group_mu(f, gd, samples, d)
        N, w = gd["counts"], gd["weights"]
        with np.errstate(invalid="ignore"):
            terms = np.where(w > 0, w * ch.poisson_deviance(N, mu), 0.0)
        total = total + (-np.sum(terms, axis=(-2, -1)) + np.sum(np.where(w > 0, w * ch.poisson_const(N), 0.0)))
    return np.where(np.isfinite(total), total, -np.inf)


def make_group(J, nC, t_start, exposure, m, seed, mean_mu=40.0, weights=None, absorption=False, background=0.0, truth=None, d=None,
               integer_counts=None):
    """The arguments of one add_count_spectrum call: the response scaled so that the model part of mu at `truth` has the mean
    mean_mu, counts ~ Poisson(mu) once with a fixed seed (integer_counts = "round": round(mu) instead)."""
    rng = np.random.default_rng(seed)
    lo, hi = bins(J)
    t_start, exposure = np.asarray(t_start, float), np.asarray(exposure, float)
    args = dict(energy_lo=lo, energy_hi=hi, response=response(J, nC, rng), t_start=t_start, exposure=exposure,
                counts=np.zeros((t_start.size, nC)), num_exposure_points=m, absorption=cross_section(lo, hi) if absorption else None)
    truth, d = (TRUTH if truth is None else truth), (defs() if d is None else d)
    probe = new_fitter()
    probe.add_count_spectrum(**args)
    mu0 = group_mu(probe, probe._fold_obs[0], [truth], d)[0]
    assert np.all(np.isfinite(mu0)) and np.all(mu0 >= 0) and mu0.mean() > 0
    args["response"] = args["response"] * (mean_mu / mu0.mean())
    mu = np.asarray(background, float) + mu0 * (mean_mu / mu0.mean())
    args["counts"] = np.round(mu) if integer_counts == "round" else rng.poisson(mu).astype(float)
    args.update(background=background, weights=weights)
    return args


def fold_fitter(groups, **kw):
    f = new_fitter(**kw)
    for g in groups:
        f.add_count_spectrum(**g)
    return f


def with_n_h(th, seed=6):
    """The walkers with a fourth column log10 N_H, drawn from 20 .. 23; the last row (the truth) at LOG_N_H_TRUE."""
    col = np.append(np.random.default_rng(seed).uniform(20.0, 23.0, th.shape[0] - 1), LOG_N_H_TRUE)
    return np.ascontiguousarray(np.column_stack([th, col]))


EDGES = np.array([60.0, 61.0, 63.0, 66.0]) * DAY  # contiguous windows whose ends and midpoints are exact


def case(name):
    """(groups, parameter list, samples) of the arithmetic cases."""
    rng = np.random.default_rng(7)
    th, d = prior_draws(), defs()
    if name == "a":
        g = [make_group(8, 16, EPOCHS[[6, 13]], [4e4, 9e4], 1, seed=41)]
    elif name == "b":
        g = [make_group(1, 1, EPOCHS[9:10], [5e4], 1, seed=42)]
    elif name == "c":
        w = np.where(rng.random((3, 130)) < 0.2, 0.0, rng.uniform(0.5, 2.0, (3, 130)))
        g = [make_group(64, 130, EDGES[:-1], np.diff(EDGES), 3, seed=43, mean_mu=1.5, weights=w, background=0.05)]
    elif name == "d":
        d, th = defs(N_H_DEF), with_n_h(th)
        g = [make_group(8, 16, EPOCHS[[6, 13]], [4e4, 9e4], 1, seed=44, absorption=True, truth=th[-1], d=d)]
    elif name == "e":
        g = [make_group(64, 4, EPOCHS[2:20:2], np.full(9, 3e4), 1, seed=45, weights=rng.uniform(0.5, 2.0, 4))]
    else:
        raise KeyError(name)
    return g, d, th


@pytest.fixture(scope="module")
def fold_a():
    return case("a")[0]


# ---------------------------------------------------------------- 1. arithmetic
# measured on an MI355X, the largest |got - want| / max(1, |want|) over the 65 walkers: (a) 1.83e-15, (b) 1.26e-15, (c) 1.60e-15,
# (d) 2.11e-15, (e) 1.85e-15; the gate is 4 x the maximum over the cases, 8.5e-15.  All 65 walkers are finite in every case (ln L from
# -9.5e6 to -2.8).  Every term of mu is non-negative, so the j sum is good to J 2^-53, and the values sit where that puts them: ln L
# is a sum of up to 390 terms of either sign (w [N ln mu - mu - ln N!] = -w D + w S), and a relative error of a few 2^-53 in each,
# against a total that is smaller than the terms' absolute sum, is 1e-15 to 2e-15 of the total.  Nothing here is far above J 2^-52.
MEASURED_FOLD_ARITH = 2.12e-15
FOLD_ARITH_GATE = 4 * MEASURED_FOLD_ARITH


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_likelihood_matches_the_formula_on_device_fluxes(name):
    """64 prior draws plus the truth; ln L of a fold-only fitter against the numpy statement on tl.device_series at the group's
    n_samples J points, with tn.rel over the walkers the reference finds finite.  Cap 1e-9 (above it: an algebra error); gate
    FOLD_ARITH_GATE = 4 x the maximum measured on an MI355X.  (a) J = 8, C = 16, n = 2, m = 1; (b) J = C = n = 1; (c) J = 64, C = 130,
    n = 3, m = 3: contiguous windows share their end points, a lane carries three channels, a fifth of the weights are 0 and mu is
    small enough that some N are 0; (d) as (a) with absorption and a free N_H on a log scale; (e) J = 64, n = 9, C = 4: 576 points,
    the series goes through in two chunks."""
    groups, d, th = case(name)
    f = fold_fitter(groups)
    gd = f._fold_obs[0]
    if name == "c":
        assert gd["t_sample"].size == 7 and gd["A"].shape == (64, 130) and (gd["weights"] == 0).mean() > 0.15
        assert ((gd["counts"] == 0) & (gd["weights"] > 0)).any() and (gd["counts"] > 0).any()
    if name == "e":
        assert gd["t_sample"].size * gd["nu"].size == 576
    want = reference(f, th, d)
    got = f.loglike_batch(th, d)
    ok = np.isfinite(want)
    measured = tn.rel(got[ok], want[ok])
    print(f"fold case ({name}): rel to the formula", measured, "finite", ok.sum(), "of", th.shape[0], "ln L range", want[ok].min(),
          want[ok].max(), "rejected", f.last_plan.n_walkers_rejected, "truth", got[-1])
    if name == "d":
        other = th.copy()
        other[:, 3] = np.where(th[:, 3] > 21.5, th[:, 3] - 1.0, th[:, 3] + 1.0)
        moved = f.loglike_batch(other, d)
        moved_rel = tn.rel(moved[ok], reference(f, other, d)[ok])
        print("fold case (d): smallest change of ln L when N_H changes", np.abs(moved - got)[ok].min(), "rel of the moved batch", moved_rel)
        assert np.all(moved[ok] != got[ok])  # N_H changes every finite walker's value
        assert moved_rel <= FOLD_ARITH_GATE, moved_rel
    assert np.isfinite(got[-1]) and ok[-1] and ok.sum() >= 48  # the truth, and most of the box
    assert np.array_equal(np.isfinite(got), ok) and np.all(got[~ok] == -np.inf)
    assert f.last_plan.n_walkers_rejected == (~ok).sum()
    assert measured <= 1e-9, "an algebra error, not rounding"
    assert MEASURED_FOLD_ARITH <= 1e-9
    assert measured <= FOLD_ARITH_GATE, measured


# ---------------------------------------------------------------- 2. the rules
def test_rules_of_a_channel_without_response(fold_a):
    """A channel whose response row is zero, with B = 0: N > 0 and w > 0 scores every walker -inf (mu = 0 cannot make counts);
    the same channel with w = 0, or with N = 0, leaves the value of the other channels unchanged to the bits."""
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    d = defs()
    g = dict(fold_a[0])
    R = g["response"].copy()
    R[5, :] = 0.0
    N = g["counts"].copy()
    N[:, 5] = [3.0, 1.0]
    off = np.ones((2, 16))
    off[:, 5] = 0.0
    base = fold_fitter([dict(g, weights=off)]).loglike_batch(th, d)  # the other channels alone (the response as it was)
    assert np.all(np.isfinite(base))
    h = fold_fitter([dict(g, response=R, counts=N)])
    out = h.loglike_batch(th, d)
    assert np.all(out == -np.inf) and h.last_plan.n_walkers_rejected == 8
    h = fold_fitter([dict(g, response=R, counts=N, weights=off)])
    assert np.array_equal(h.loglike_batch(th, d), base) and h.last_plan.n_walkers_rejected == 0
    N0 = N.copy()
    N0[:, 5] = 0.0
    h = fold_fitter([dict(g, response=R, counts=N0)])
    assert np.array_equal(h.loglike_batch(th, d), base) and h.last_plan.n_walkers_rejected == 0
    one = off.copy()
    one[1, 5] = 1e-3  # one weighted channel among them is enough
    h = fold_fitter([dict(g, response=R, counts=N, weights=one)])
    assert np.all(h.loglike_batch(th, d) == -np.inf)
    # a walker the pass rejects is counted, and the context stays usable
    bad = th.copy()
    bad[2, 0] = -0.05  # theta_c < 0
    k = fold_fitter(fold_a)
    full = k.loglike_batch(th, d)
    out = k.loglike_batch(bad, d)
    assert out[2] == -np.inf and np.array_equal(np.delete(out, 2), np.delete(full, 2)) and k.last_plan.n_walkers_rejected == 1
    assert np.array_equal(k.loglike_batch(th, d), full) and k.last_plan.n_walkers_rejected == 0


# ---------------------------------------------------------------- 3. a mixed fit
@pytest.fixture(scope="module")
def fold_mixed(fold_a, group_a):  # noqa: F811
    """Point rows (60 C4 rows) + a counts group + an index group + a fold group; each part as a fitter of its own."""
    c4t, c4nu = configs.c4_mock_data()
    truth = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], c4t, c4nu)[0]
    rng = np.random.default_rng(9)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(60)), 0.1 * truth
    counts = tc.case_args("a")[0]
    builds = (lambda f: f.add_flux_density(c4nu, c4t, obs, err), lambda f: f.add_counts(**counts),
              lambda f: f.add_spectral_index(**group_a[0]), lambda f: f.add_count_spectrum(**fold_a[0]))
    parts = []
    for build in builds:
        f = new_fitter()
        build(f)
        parts.append(f)
    whole = new_fitter()
    for build in builds:
        build(whole)
    return whole, parts


def test_a_mixed_fit_is_the_sum_of_its_parts(fold_mixed):
    """ln L of the whole against the sum of each part's own fit, added in pass order (no priors: nothing is counted twice), to the
    bits: -1/2 is exact, so the sum of the parts' ln L is the whole's chi^2 sum when every pass returns the bits it returns alone,
    and on an MI355X every pass of this mix does."""
    whole, parts = fold_mixed
    th, d = prior_draws(), defs()
    assert whole.has_count_spectra and whole.has_counts and whole.has_spectral_indices
    got = whole.loglike_batch(th, d)
    each = [p.loglike_batch(th, d) for p in parts]
    want = ((each[0] + each[1]) + each[2]) + each[3]
    ok = np.isfinite(want)
    print("mixed fit: equal to the sum of its parts", np.array_equal(got[ok], want[ok]), "rel", tn.rel(got[ok], want[ok]), "finite", ok.sum(),
          "parts at the truth", [e[-1] for e in each])
    assert ok[-1] and ok.sum() >= 48 and np.array_equal(np.isfinite(got), ok)
    assert np.array_equal(got[ok], want[ok])
    fold_part = reference(whole, th, d)
    assert tn.rel(each[3][ok], fold_part[ok]) <= FOLD_ARITH_GATE


# ---------------------------------------------------------------- 4. bits
def test_bits(fold_mixed, fold_a):
    """Two calls, a call under VAG_NO_ORDER, and the host-pointer and device-pointer entries return the same bits; one invalid
    walker (a NaN parameter) scores -inf and is counted.  A walker alone goes through a series request whose launch shape follows
    the batch, so its flux may differ from the batch's in the last bits: the term's independence of the other walkers is held to
    FOLD_ARITH_GATE.  Observed on an MI355X: every eleventh walker alone returned the bits it returned among the 67, for the
    fold-only fitter and for the mixed one; seven walkers do not show it for every batch, so bit equality is not asserted."""
    import torch
    th = np.ascontiguousarray(np.vstack([tv._walkers(66, seed=12)[0], TRUTH]))
    th[40, 0] = np.nan  # one invalid walker
    for f, d in ((fold_fitter(fold_a + case("e")[0]), defs()), (fold_mixed[0], defs())):
        a = f.loglike_batch(th, d)
        assert th.shape[0] == 67 and a[40] == -np.inf and np.all(np.isfinite(np.delete(a, 40))) and f.last_plan.n_walkers_rejected == 1
        assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
        assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
        ev = f.device_evaluator(d)
        assert ev.has_count_spectra
        vals, _ = ev(torch.from_numpy(th).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(vals.cpu().numpy(), a)
        with pytest.raises(NotImplementedError, match="add_count_spectrum"):
            ev.native.shard(None, 67, 0, 1, None)
        alone = np.array([f.loglike_batch(th[i:i + 1], d)[0] for i in range(0, 67, 11)])
        print("bits: alone equal", np.array_equal(alone, a[::11]), "rel", tn.rel(alone, a[::11]))
        assert tn.rel(alone, a[::11]) <= FOLD_ARITH_GATE


# ---------------------------------------------------------------- 5. the empty spec
def test_null_or_empty_fold_spec_is_the_index_call(mixed):  # noqa: F811
    """On the mixed fit of tests/test_index.py the new entry point with fold NULL or empty returns the bits of vag_loglike_index_batch,
    and Fitter.loglike_batch, which calls it, does too."""
    whole = mixed[0]
    th, d = prior_draws(), defs(ti.SYS_A)
    spec, _, _ = whole.build_spec(d)
    assert spec._fold is None and spec._index is not None and spec._counts is not None and spec._noise is not None
    rc, base = tc._raw("vag_loglike_index_batch", spec, th, C.byref(spec._counts), C.byref(spec._index))
    assert rc == 0 and np.isfinite(base).sum() >= 48
    empty = _lib.FoldFitSpec()
    for fs in (None, C.byref(empty)):
        rc, out = tc._raw("vag_loglike_fold_batch", spec, th, C.byref(spec._counts), C.byref(spec._index), fs)
        assert rc == 0 and np.array_equal(out, base)
    assert np.array_equal(whole.loglike_batch(th, d), base)


# ---------------------------------------------------------------- 6. bad input, memory
def test_invalid_groups_through_the_c_abi_leave_the_context_usable(fold_a):
    f, d = fold_fitter(fold_a), defs()
    th = np.ascontiguousarray(tv._walkers(4, seed=3)[0])
    spec, _, _ = f.build_spec(d)
    rc, good = tc._raw("vag_loglike_fold_batch", spec, th, None, None, C.byref(spec._fold))
    assert rc == 0 and np.all(np.isfinite(good))
    gd = f._fold_obs[0]
    for key, at, v, words in (("counts", (1, 3), 2.5, ("row 1", "channel 3")), ("background", (0, 15), -1.0, ("row 0", "channel 15")),
                              ("A", (7, 2), np.nan, ("bin 7", "channel 2")), ("nu", 1, 1e16, ("bin 1",)), ("t_sample", 0, -1.0, ("sample 0",)),
                              ("exposure_over_m", 1, 0.0, ("row 1",)), ("sample_idx", (1, 0), 2, ("row 1", "sample index"))):
        keep = gd[key][at]
        gd[key][at] = v
        rc, _ = tc._raw("vag_loglike_fold_batch", spec, th, None, None, C.byref(spec._fold))
        msg = tc.lib_error()
        assert rc == _lib.VAG_E_INVALID and "fold group 0" in msg and all(w in msg for w in words), (rc, msg)
        gd[key][at] = keep
    spec.slot[0] = _lib.P_N_H  # no group has a cross-section
    rc, _ = tc._raw("vag_loglike_fold_batch", spec, th, None, None, C.byref(spec._fold))
    assert rc == _lib.VAG_E_INVALID and tc.lib_error() == "bad parameter slot"
    spec.slot[0] = _lib.PARAM_SLOTS["theta_c"]
    rc, again = tc._raw("vag_loglike_fold_batch", spec, th, None, None, C.byref(spec._fold))
    assert rc == 0 and np.array_equal(again, good)
    other = dict(fold_a[0], counts=fold_a[0]["counts"] + 1.0)  # other counts, same shapes: the resident copy must follow
    b = fold_fitter([other]).loglike_batch(th, d)
    assert np.all(b != good) and np.array_equal(f.loglike_batch(th, d), good)


def test_device_memory_returns_after_destroy(fold_a):
    lib = _lib.load()
    f = fold_fitter(fold_a + case("e")[0])
    d = defs()
    spec, _, _ = f.build_spec(d)
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    want = f.loglike_batch(th, d)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    out = np.empty(8)
    for _ in range(2):  # (the second call finds the groups resident)
        _lib.check(lib.vag_loglike_fold_batch(ctx, C.byref(spec), None, None, None, None, None, None, None, C.byref(spec._fold),
                                              th.ctypes.data_as(dp), 8, spec.ndim, out.ctypes.data_as(dp)))
        assert np.array_equal(out, want)
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before


# ---------------------------------------------------------------- 7. the read-back
def test_fitter_count_spectra_is_the_statement_on_the_groups_own_request():
    """Fitter.count_spectra at the truth against fold_expected on vag_flux_density_batch at each group's points with the sample's
    N_H: to the bits (the same request of one model, the same numpy arithmetic)."""
    d = defs(N_H_DEF)
    truth = np.append(TRUTH, LOG_N_H_TRUE)
    lo, hi = bins(8)
    rng = np.random.default_rng(46)
    f = new_fitter()
    f.add_count_spectrum(lo, hi, response(8, 16, rng), EPOCHS[[6, 13]], [4e4, 9e4], np.zeros((2, 16)), background=0.5, absorption=cross_section(lo, hi))
    f.add_count_spectrum(lo, hi, response(8, 5, rng), EPOCHS[3:6], [1e4, 2e4, 3e4], np.zeros((3, 5)), num_exposure_points=3)
    got = f.count_spectra(truth, d)
    assert len(got) == 2 and got[0].shape == (2, 16) and got[1].shape == (3, 5)
    p = f._params_at(truth, d)[0]
    for gd, g in zip(f._fold_obs, got):
        ts, nus = points(gd)
        want = fold_expected(tl.device_series([p], ts, nus)[0], gd, 10.0 ** LOG_N_H_TRUE)
        assert np.array_equal(g, want) and np.all(g > 0)
    clear = f.count_spectra(np.append(TRUTH, 20.0), d)
    assert np.all(clear[0] > got[0]) and np.array_equal(clear[1], got[1])  # less absorption, more counts; no sigma, no change
    fixed = defs([P("N_H", 1e22, 1e22, fitting.Scale.fixed)])
    assert np.array_equal(f.count_spectra(TRUTH, fixed)[0], got[0])
    assert np.array_equal(f.count_spectra(TRUTH, defs())[0], fold_expected(tl.device_series([p], *points(f._fold_obs[0]))[0], f._fold_obs[0], 0.0))


# ---------------------------------------------------------------- 8. a profile in N_H
def test_the_profile_in_n_h_peaks_at_the_truth():
    """Counts round(mu) at the truth (N_H = 1e22), the response scaled so that channels hold 1e4 counts on average: ln L over 13 values
    of log10 N_H, 0.1 dex apart and centred on the truth, every other parameter at the truth, has its maximum at the truth and falls
    monotonically to both sides."""
    d = defs(N_H_DEF)
    truth = np.append(TRUTH, LOG_N_H_TRUE)
    g = make_group(8, 16, EPOCHS[[6, 13]], [4e4, 9e4], 1, seed=47, mean_mu=1e4, absorption=True, truth=truth, d=d, integer_counts="round")
    assert g["counts"].mean() > 5e3
    f = fold_fitter([g])
    th = np.tile(truth, (13, 1))
    th[:, 3] = LOG_N_H_TRUE + 0.1 * np.arange(-6, 7)
    assert th[6, 3] == LOG_N_H_TRUE
    lnl = f.loglike_batch(np.ascontiguousarray(th), d)
    print("N_H profile: ln L - max", lnl - lnl.max())
    assert np.all(np.isfinite(lnl)) and int(np.argmax(lnl)) == 6
    assert np.all(np.diff(lnl[:7]) > 0) and np.all(np.diff(lnl[6:]) < 0)
