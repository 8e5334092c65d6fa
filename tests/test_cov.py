"""Correlated groups on the device (vag_loglike_cov_batch[_dev], Fitter.add_correlated, Fitter.correlated): the term against its
definition in numpy.longdouble on the device's own model values, against the point rows (a diagonal covariance) and against the
calibration group of vag_loglike_noise_batch (diag + c^2 1 1^T), a mixed fit, the null spec, bits, edges, invalid specs, memory and
the read-back.

The problem is C4 (configs.C4_TRUTH, default resolutions) with the 64 prior draws plus the truth of tests/test_counts.py: 65
walkers, so that a batch straddles 64.  The groups are the cases of tests/test_cov_host.py -- n in {1, 2, 63, 64, 65, 130, 256} rows
at times 1e3 .. 1e7 s, sigma_ln from 0.03 .. 0.3, the families "gp" and "cal" -- at frequencies drawn from 1e9 .. 10^17.5 Hz ("gp":
more than 8 distinct ones from n = 63 on, the general series path) or from the three C4 bands ("cal": the shared-node path).
Observed fluxes are the device's own flux at the truth times exp(L z), L the Cholesky factor of C_ln, drawn once with a fixed seed.

The gate is the bound B of tests/test_cov_host.py (derived there, not measured on the code under test): chi^2 of the device
against the definition in longdouble on the same device fluxes within B, i.e. ln L within w B / 2; every case also has
B <= 1e-9 chi^2_ref, so that a loose bound cannot hide an algebra error.
Measured on an MI355X: the worst |chi^2_dev - chi^2_ref| / B over the 16 cases and their 65 walkers is 0.517 (n = 2, "cal"); per case
it falls from 0.14 .. 0.52 at n <= 2 to 0.003 .. 0.005 at n = 256 (the bound's first term grows with n, the error does not).  B / chi^2
is at most 7.6e-11 (n = 256, "cal": a walker far from the truth, whose common offset the family's C^-1 damps).  The same rows as point
rows: at most 0.021 of (B_cov + B_points) / 2; against the calibration group: at most 0.24 B; a mixed fit equals the sum of its parts
to the bits; one walker alone and in batches of 2, 64 and 65 returned the batch's bits for the correlated fitter, and differed by at
most 0.015 of the tolerance for the mixed one."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_counts as tc
import test_cov_host as ch
import test_index as ti
import test_limits as tl
import test_noise as tn
import test_sky_visfit as tv
from vegasafterglow_amd import _lib, fitting

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
LD = np.longdouble

P = fitting.ParamDef
defs, prior_draws, TRUTH, EPOCHS = tc.defs, tc.prior_draws, tc.TRUTH, tc.EPOCHS
new_fitter, series_flux = ti.new_fitter, ti.series_flux
A_V_TRUE, A_V_DEF = ti.A_V_TRUE, ti.A_V_DEF
Z = configs.C4_TRUTH["z"]
# the worst |chi^2_dev - chi^2_ref| / B over the cases of test_likelihood_matches_the_definition_on_device_fluxes, on an MI355X: a
# record, not a gate (the gate is B itself)
MEASURED_FRACTION = 0.517


def frequencies(n, kind):
    rng = np.random.default_rng(77 * n + ch.FAMILIES.index(kind))
    if kind == "gp":
        return 10 ** rng.uniform(9.0, 17.5, n)
    return configs.C4_BANDS[rng.integers(0, 3, n)]


_DATA = {}


def make_data(n, kind, truth=TRUTH, d=None, **fitter_kw):
    """The arguments (nu, t, f_nu, cov) of one add_correlated call, made once per case and shared: the device's own flux at `truth`
    (with the law's extinction when the fitter has one) times exp(L z)."""
    key = (n, kind, tuple(np.asarray(truth, dtype=float)), tuple(sorted(fitter_kw.items())))
    if key not in _DATA:
        t, _, c_ln, _ = ch.case(n, kind)
        nu = frequencies(n, kind)
        probe = new_fitter(**fitter_kw)
        probe.add_correlated(3e9, [1e5], [1.0], [[1.0]])  # (a fitter without data builds no spec)
        p, a_v = probe._params_at(truth, defs() if d is None else d)
        F = series_flux([p], t, nu)[0]
        assert np.all(F > 0) and np.all(np.isfinite(F))
        ext = probe._cov_ext(dict(nu=nu), Z)
        if ext is not None:
            F = F * np.exp(-a_v * ext)
        rng = np.random.default_rng(5000 + 13 * n + ch.FAMILIES.index(kind))
        f_obs = F * np.exp(np.linalg.cholesky(c_ln) @ rng.standard_normal(n))
        _DATA[key] = dict(nu=nu, t=np.array(t), f_nu=f_obs, cov=c_ln * np.outer(f_obs, f_obs))
    return _DATA[key]


def cov_fitter(groups, **kw):
    f = new_fitter(**kw)
    for g in groups:
        f.add_correlated(**g)
    return f


def reference(f, samples, d, groups=None):
    """(ln L, B, chi^2) [nb] of the fitter's correlated groups: the definition in numpy.longdouble on the device's series fluxes at each
    group's rows, and the bound of tests/test_cov_host.py summed over the groups with their weights.  A walker the engine rejects, or
    whose value is not finite, is -inf."""
    pa = [f._params_at(s, d) for s in samples]
    a_v = np.array([a for _, a in pa])
    chi2, B = np.zeros(len(pa), LD), np.zeros(len(pa))
    for gd in (f._cov_obs if groups is None else groups):
        F = series_flux([p for p, _ in pa], gd["t"], gd["nu"]).astype(LD)
        ext = f._cov_ext(gd, Z)
        av_ext = a_v[:, None] * ext[None, :] if ext is not None else np.zeros(F.shape)
        with np.errstate(all="ignore"):
            fl = F * np.exp(-av_ext.astype(LD))
            ln_f = np.log(np.where(np.isnan(fl), fl, np.maximum(fl, LD(1e-300))))
            r = gd["ln_flux"].astype(LD) - ln_f
            chi2 = chi2 + gd["weight"] * ch.chi2_longdouble(gd["whitener"], r)
            B = B + gd["weight"] * ch.bound(gd["whitener"], r.astype(np.float64), gd["ln_flux"], ln_f.astype(np.float64), av_ext)
    lnl = (-0.5 * chi2).astype(np.float64)
    return np.where(np.isfinite(lnl), lnl, -np.inf), B, chi2.astype(np.float64)


def case(name):
    """(groups, fitter keywords, parameter list, samples) of the formula cases: "<n>-<family>", "ext" (n = 65, "cal", an SMC law with a
    free A_V) and "w" (n = 65, "gp", weight 0.37)."""
    th, d, kw = prior_draws(), defs(), {}
    if name == "ext":
        kw, d = dict(extinction="smc"), defs(A_V_DEF)
        th = np.ascontiguousarray(np.column_stack([th, np.append(np.random.default_rng(6).uniform(0.0, 1.0, 64), A_V_TRUE)]))
        g = [make_data(65, "cal", truth=th[-1], d=d, **kw)]
    elif name == "w":
        g = [dict(make_data(65, "gp"), weight=0.37)]
    else:
        n, kind = name.split("-")
        g = [make_data(int(n), kind)]
    return g, kw, d, th


FORMULA_CASES = [f"{n}-{kind}" for n, kind in ch.CASES] + ["ext", "w"]
_WORST = {}


# ---------------------------------------------------------------- 1. the formula
@pytest.mark.parametrize("name", FORMULA_CASES)
def test_likelihood_matches_the_definition_on_device_fluxes(name):
    """A fitter that holds only the group: ln L against -1/2 w chi^2_ref (no prior) within w B / 2, for every n and both families,
    once under an SMC law with a free A_V and once with w = 0.37.  B is the bound of tests/test_cov_host.py, whose docstring derives
    it: 3 (n + 2) u sum a_i^2 for the dot products and the sum of squares, 2 sum a_i sum_j |W_ij| e_j for an ulp-level difference of
    log and exp between the device and numpy (and of the series flux between two requests)."""
    groups, kw, d, th = case(name)
    f = cov_fitter(groups, **kw)
    gd = f._cov_obs[0]
    assert th.shape[0] == 65 and f.has_correlated and not f._point_t and np.all(np.diff(gd["t"]) >= 0)
    want, B, chi2 = reference(f, th, d)
    got = f.loglike_batch(th, d)
    ok = np.isfinite(want)
    frac = np.abs(-2.0 * got[ok].astype(LD) - (-2.0 * want[ok].astype(LD))) / B[ok]
    _WORST[name] = float(frac.max())
    print(f"cov case ({name}): worst |chi2_dev - chi2_ref| / B {frac.max():.3e} (so far, all cases: {max(_WORST.values()):.3e}); "
          f"B / chi2 at most {np.max(B[ok] / chi2[ok]):.2e}; finite {ok.sum()} of 65; ln L range {want[ok].min():.6g} .. "
          f"{want[ok].max():.6g}; rejected {f.last_plan.n_walkers_rejected}; truth {got[-1]:.6g}")
    if name == "ext":
        spec, _, _ = f.build_spec(d)
        assert spec._cov.groups[0].ext and np.all(f._cov_ext(gd, Z)[gd["nu"] == configs.C4_BANDS[1]] > 0.5)
        zero = th.copy()
        zero[:, 3] = np.where(th[:, 3] > 0.5, 0.0, 1.0)
        assert np.all(f.loglike_batch(zero, d)[ok] != got[ok])  # A_V changes every walker's value
    if name == "w":
        assert gd["weight"] == 0.37
    assert np.isfinite(got[-1]) and ok.sum() >= 48  # the truth, and most of the box
    assert np.array_equal(np.isfinite(got), ok) and np.all(got[~ok] == -np.inf)
    assert f.last_plan.n_walkers_rejected == (~ok).sum()
    assert np.all(B[ok] > 0) and np.all(B[ok] <= 1e-9 * chi2[ok]), "a loose bound"
    assert np.all(np.abs(got[ok] - want[ok]) <= 0.5 * B[ok]), float(frac.max())


# ---------------------------------------------------------------- 2. a diagonal covariance
@pytest.mark.parametrize("n", [2, 65, 256])
def test_a_diagonal_covariance_is_the_point_rows(n):
    """cov = diag(err^2) against the same rows through add_flux_density (unit weights), within half the sum of the two bounds: B of
    the correlated group, and the same expression for the point rows' sum ((ln F_obs - ln f) / sigma_ln)^2, W = diag(1 / sigma_ln)."""
    g = make_data(n, "gp")
    err = np.sqrt(np.diag(g["cov"]))
    d, th = defs(), prior_draws()
    a = cov_fitter([dict(g, cov=np.diag(err ** 2))])
    b = new_fitter()
    b.add_flux_density(g["nu"], g["t"], g["f_nu"], err)
    la, lb = a.loglike_batch(th, d), b.loglike_batch(th, d)
    assert np.array_equal(b._all_weights, np.ones(n)) and np.array_equal(b._all_t, a._cov_obs[0]["t"])
    _, Ba, _ = reference(a, th, d)
    _, Bb, _ = reference(a, th, d, groups=[dict(a._cov_obs[0], whitener=np.diag(1.0 / b._all_log_err))])
    ok = np.isfinite(la)
    print(f"diagonal n={n}: worst |ln L_cov - ln L_points| / ((B_cov + B_points) / 2) {np.max(np.abs(la - lb)[ok] / (0.5 * (Ba + Bb)[ok])):.3e}")
    assert ok.sum() >= 48 and np.array_equal(np.isfinite(lb), ok)
    assert np.all(np.abs(la - lb)[ok] <= 0.5 * (Ba + Bb)[ok])


# ---------------------------------------------------------------- 3. the calibration group
@pytest.mark.parametrize("n", ch.NS)
def test_the_cal_family_is_the_calibration_group(n):
    """cov = diag(err^2) + 0.2^2 f f^T against the same rows in a noise group with calibration=0.2 and no systematic: the noise
    group carries the determinant's walker-dependent half, ln L_cov - ln L_noise = +1/2 log1p(c^2 sum 1 / sigma_ln^2), for every
    walker, within B.  vag_fit_back_noise_kernel forms r^T C^-1 r by the Sherman-Morrison formula: code built independently."""
    g = make_data(n, "cal")
    f_obs = g["f_nu"]
    sig = ch.case(n, "cal")[1]
    err = sig * f_obs
    d, th = defs(), prior_draws()
    a = cov_fitter([dict(g, cov=np.diag(err ** 2) + 0.2 ** 2 * np.outer(f_obs, f_obs))])
    b = new_fitter()
    b.add_flux_density(g["nu"], g["t"], f_obs, err, noise="zp", calibration=0.2)
    la, lb = a.loglike_batch(th, d), b.loglike_batch(th, d)
    assert np.array_equal(b._all_weights, np.ones(n))
    shift = 0.5 * np.log1p(0.2 ** 2 * np.sum(1.0 / b._all_log_err ** 2))
    _, B, _ = reference(a, th, d)
    ok = np.isfinite(la)
    print(f"calibration n={n}: shift {shift:.6g}; worst |ln L_cov - ln L_noise - shift| / B {np.max(np.abs(la - lb - shift)[ok] / B[ok]):.3e}")
    assert ok.sum() >= 48 and np.array_equal(np.isfinite(lb), ok)
    assert np.all(np.abs(la - lb - shift)[ok] <= B[ok])


# ---------------------------------------------------------------- 4. a mixed fit
@pytest.fixture(scope="module")
def mixed():
    """Point data (the 60 C4 rows) + one add_flux group + one index group + two correlated groups; each part as a fitter of its own;
    and the whole without its correlated groups."""
    c4t, c4nu = configs.c4_mock_data()
    truth = tl.device_series([_abi.make_params(**configs.C4_TRUTH)], c4t, c4nu)[0]
    rng = np.random.default_rng(8)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(60)), 0.1 * truth
    bt = EPOCHS[2::3]
    bflux = tc.device_flux([_abi.make_params(**configs.C4_TRUTH)], bt, tl.BAND, 7)[0] * (1 + 0.05 * rng.standard_normal(bt.size))
    index = ti.make_group(ti.X_BAND, EPOCHS, 2, "photon", seed=31)
    builds = (lambda f: f.add_flux_density(c4nu, c4t, obs, err), lambda f: f.add_flux(tl.BAND, bt, bflux, 0.1 * bflux, num_points=7),
              lambda f: f.add_spectral_index(**index), lambda f: f.add_correlated(**make_data(65, "gp")),
              lambda f: f.add_correlated(**make_data(130, "cal"), weight=0.37))
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
    """ln L of the whole against the sum of each part's own fit (no priors: nothing is counted twice), with the criterion of
    tests/test_index.py::test_a_mixed_fit_is_the_sum_of_its_parts: tn.rel <= ti.INDEX_ARITH_GATE."""
    whole, parts, _ = mixed
    th, d = prior_draws(), defs()
    assert whole.has_correlated and whole.has_spectral_indices and len(whole._cov_obs) == 2 and len(whole._band_obs) == 1
    got = whole.loglike_batch(th, d)
    each = [p.loglike_batch(th, d) for p in parts]
    want = np.sum(each, axis=0)
    ok = np.isfinite(want)
    print("mixed fit: rel to the sum of its parts", tn.rel(got[ok], want[ok]), "finite", ok.sum(), "parts at the truth", [e[-1] for e in each])
    assert ok[-1] and ok.sum() >= 48 and np.array_equal(np.isfinite(got), ok)
    assert tn.rel(got[ok], want[ok]) <= ti.INDEX_ARITH_GATE


# ---------------------------------------------------------------- 5. the null spec
def _raw(name, spec, samples, *trailing):
    """The entry point `name` with the spec's blocks up to the index groups, then `trailing`."""
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    return tc._raw(name, spec, samples, ref(spec._counts), ref(spec._index), *trailing)


def test_a_null_or_empty_spec_is_the_template_call(mixed):
    """cov NULL and n_groups = 0 return the bits of vag_loglike_tmpl_batch, and the Fitter's own path for a fit without correlated
    groups makes that call."""
    rest = mixed[2]
    th, d = prior_draws(), defs()
    spec, _, _ = rest.build_spec(d)
    assert spec._cov is None and spec._index is not None
    rc, base = _raw("vag_loglike_tmpl_batch", spec, th, None, None)
    assert rc == 0 and np.isfinite(base).sum() >= 48
    empty = _lib.CovFitSpec()
    for cs in (None, C.byref(empty)):
        rc, out = _raw("vag_loglike_cov_batch", spec, th, None, None, cs)
        assert rc == 0 and np.array_equal(out, base)
    assert np.array_equal(rest.loglike_batch(th, d), base)


# ---------------------------------------------------------------- 6. bits
def test_bits(mixed):
    """The host entry and the device-pointer entry return the same bits, and so do two calls, a call in the identity evaluation
    order and a permuted batch.  A walker alone or in a batch of 2, 64 or 65 goes through a series request whose launch shape follows
    the batch, so its flux may differ in the last bits (the condition the index groups state): the term's independence of the other
    walkers is held to the bound, w B / 2 for the correlated fitter, and to ti.INDEX_ARITH_GATE for the mixed one."""
    import torch
    th = np.ascontiguousarray(np.vstack([tv._walkers(64, seed=12)[0], TRUTH]))
    th[40, 0] = np.nan  # one invalid walker
    d = defs()
    keep = np.arange(65) != 40
    for f in (cov_fitter([make_data(65, "gp"), dict(make_data(256, "cal"), weight=0.37)]), mixed[0]):
        a = f.loglike_batch(th, d)
        assert th.shape[0] == 65 and a[40] == -np.inf and np.all(np.isfinite(a[keep])) and f.last_plan.n_walkers_rejected == 1
        assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
        assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
        ev = f.device_evaluator(d)
        assert ev.has_correlated
        vals, _ = ev(torch.from_numpy(th).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(vals.cpu().numpy(), a)
        with pytest.raises(NotImplementedError, match="add_correlated"):
            ev.native.shard(None, 65, 0, 1, None)
        perm = np.random.default_rng(4).permutation(65)
        shuffled = np.empty(65)
        shuffled[perm] = f.loglike_batch(np.ascontiguousarray(th[perm]), d)
        assert np.array_equal(shuffled, a)
        if f is mixed[0]:
            tol = ti.INDEX_ARITH_GATE * np.maximum(1.0, np.abs(a))
        else:
            tol = np.where(keep, 0.5 * reference(f, np.where(keep[:, None], th, TRUTH), d)[1], 0.0)
        for lo, hi in ((64, 65), (0, 1), (6, 8), (0, 64), (0, 65)):  # alone (twice), in batches of 2, 64 and 65
            part = f.loglike_batch(np.ascontiguousarray(th[lo:hi]), d)
            sel = keep[lo:hi]
            diff = np.where(sel, np.abs(np.where(sel, part, 0.0) - np.where(sel, a[lo:hi], 0.0)), 0.0)
            print(f"bits: walkers {lo}..{hi - 1} equal to the batch of 65: {np.array_equal(part, a[lo:hi])}; worst difference / tolerance "
                  f"{np.max(diff[sel] / tol[lo:hi][sel]):.3e}")
            assert np.array_equal(np.isfinite(part), sel)
            assert np.all(diff[sel] <= tol[lo:hi][sel])


# ---------------------------------------------------------------- 7. edges
def test_edges():
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    d = defs()
    g65 = make_data(65, "gp")
    f = cov_fitter([g65])
    base = f.loglike_batch(th, d)
    assert np.all(np.isfinite(base)) and f.last_plan.n_walkers_rejected == 0
    # a walker outside its prior scores -inf and is counted; the others add the (uniform) ln prior
    out_of_box = th.copy()
    out_of_box[3, 1] = 0.9  # theta_v above its upper bound 0.8
    lp = f.log_prob_batch(out_of_box, d)
    assert lp[3] == -np.inf and np.all(np.isfinite(np.delete(lp, 3))) and f.last_plan.n_walkers_rejected == 1
    ln_prior = -np.log(0.3 - 0.02) - np.log(0.8) - np.log(4.0)
    assert tn.rel(np.delete(lp, 3), np.delete(base, 3) + ln_prior) <= 1e-14
    # a walker the pass rejects scores -inf and is counted, and the context stays usable
    bad = th.copy()
    bad[2, 0] = -0.05  # theta_c < 0
    out = f.loglike_batch(bad, d)
    assert out[2] == -np.inf and np.array_equal(np.delete(out, 2), np.delete(base, 2)) and f.last_plan.n_walkers_rejected == 1
    assert np.array_equal(f.loglike_batch(th, d), base) and f.last_plan.n_walkers_rejected == 0
    # no flux (far above the synchrotron cut-off): the model value takes the 1e-300 clamp, the term stays finite
    t3, nu3 = EPOCHS[:3], np.array([1e29, 1e30, 1e29])
    assert np.all(tl.device_series([_abi.make_params(**configs.C4_TRUTH)], t3, nu3)[0] == 0)
    fo = np.array([1e-30, 2e-30, 3e-30])
    dark = dict(nu=nu3, t=t3, f_nu=fo, cov=np.outer(fo, fo) * (np.diag([0.04, 0.09, 0.01]) + 0.02))
    h = cov_fitter([dark])
    out = h.loglike_batch(th, d)
    gd = h._cov_obs[0]
    r = gd["ln_flux"] - np.log(1e-300)
    want = -0.5 * float(fitting.whitened_chi2(r, gd["whitener"]))
    B = float(ch.bound(gd["whitener"], r, gd["ln_flux"], np.full(3, np.log(1e-300))))
    assert np.all(np.isfinite(out)) and h.last_plan.n_walkers_rejected == 0 and np.all(np.abs(out - want) <= 0.5 * B)
    assert np.all(out == out[0])  # every walker has the same (clamped) model value
    # a group with w = 0 makes its request and adds 0; with a rejected walker it still scores -inf
    k = cov_fitter([g65, dict(dark, weight=0.0)])
    assert np.array_equal(k.loglike_batch(th, d), base) and k.last_plan.n_walkers_rejected == 0
    out = k.loglike_batch(bad, d)
    assert out[2] == -np.inf and np.array_equal(np.delete(out, 2), np.delete(base, 2)) and k.last_plan.n_walkers_rejected == 1
    # n = 1: -1/2 ((ln F_obs - ln F) / sigma_ln)^2; and a group at VAG_COV_MAX_ROWS
    g1 = make_data(1, "cal")
    one = cov_fitter([g1])
    out = one.loglike_batch(th, d)
    F = series_flux([one._params_at(s, d)[0] for s in th], g1["t"], g1["nu"])[:, 0]
    sig_ln = np.sqrt(g1["cov"][0, 0]) / g1["f_nu"][0]
    want = -0.5 * ((np.log(g1["f_nu"][0]) - np.log(F)) / sig_ln) ** 2
    assert one._cov_obs[0]["whitener"].shape == (1, 1) and np.all(np.abs(out - want) <= 0.5 * reference(one, th, d)[1] + 4 * ch.U * np.abs(want))
    cap = cov_fitter([make_data(_lib.COV_MAX_ROWS, "gp")])
    out = cap.loglike_batch(th, d)
    want, B, _ = reference(cap, th, d)
    assert cap._cov_obs[0]["t"].size == 256 and np.all(np.isfinite(out)) and np.all(np.abs(out - want) <= 0.5 * B)
    with pytest.raises(ValueError, match="at most 256 rows"):
        big = np.arange(1.0, 258.0)
        new_fitter().add_correlated(3e9, big * 1e3, big, np.diag(big))


# ---------------------------------------------------------------- 8. invalid specs
def test_invalid_groups_through_the_c_abi_leave_the_context_usable():
    f, d = cov_fitter([make_data(65, "gp"), make_data(2, "cal")]), defs()
    th = np.ascontiguousarray(tv._walkers(4, seed=3)[0])
    spec, _, _ = f.build_spec(d)
    rc, good = _raw("vag_loglike_cov_batch", spec, th, None, None, C.byref(spec._cov))
    assert rc == 0 and np.all(np.isfinite(good))
    gd = f._cov_obs[0]
    for key, at, v, words in (("ln_flux", 3, np.nan, ("row 3", "ln_flux")), ("t", 5, -1.0, ("row 5", "times")),
                              ("nu", 64, 0.0, ("row 64", "frequency")), ("whitener", (7, 7), 0.0, ("row 7", "diagonal")),
                              ("whitener", (9, 2), np.inf, ("row 9", "entry 2"))):
        keep = gd[key][at]
        gd[key][at] = v
        rc, _ = _raw("vag_loglike_cov_batch", spec, th, None, None, C.byref(spec._cov))
        msg = tc.lib_error()
        assert rc == _lib.VAG_E_INVALID and "correlated group 0" in msg and all(w in msg for w in words), (rc, msg)
        gd[key][at] = keep
    spec._cov.groups[1].n = 257
    rc, _ = _raw("vag_loglike_cov_batch", spec, th, None, None, C.byref(spec._cov))
    assert rc == _lib.VAG_E_INVALID and "correlated group 1" in tc.lib_error()
    spec._cov.groups[1].n = 2
    rc, again = _raw("vag_loglike_cov_batch", spec, th, None, None, C.byref(spec._cov))
    assert rc == 0 and np.array_equal(again, good)
    other = make_data(65, "gp")
    other = dict(other, f_nu=other["f_nu"] * 1.5, cov=other["cov"] * 2.25)  # other fluxes, same shapes: the resident copy must follow
    b = cov_fitter([other, make_data(2, "cal")]).loglike_batch(th, d)
    assert np.all(b != good) and np.array_equal(f.loglike_batch(th, d), good)


# ---------------------------------------------------------------- 9. memory
def test_device_memory_returns_after_destroy():
    lib = _lib.load()
    f = cov_fitter([make_data(65, "gp"), make_data(130, "cal")])
    d = defs()
    spec, _, _ = f.build_spec(d)
    th = np.ascontiguousarray(np.vstack([tv._walkers(7, seed=3)[0], TRUTH]))
    want = f.loglike_batch(th, d)
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    out = np.empty(8)
    for _ in range(2):  # (the second call finds the groups resident)
        _lib.check(lib.vag_loglike_cov_batch(ctx, C.byref(spec), None, None, None, None, None, None, None, None, None, C.byref(spec._cov),
                                             th.ctypes.data_as(dp), 8, spec.ndim, out.ctypes.data_as(dp)))
        assert np.array_equal(out, want)
    assert lib.vag_device_bytes_in_use() >= before + 8 * (4 * 65 + 65 * 65 + 4 * 130 + 130 * 130)  # (the groups' buffer among them)
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before


# ---------------------------------------------------------------- 10. the read-back
def test_fitter_correlated_is_the_statement_on_the_groups_own_request():
    """Fitter.correlated at one sample: model, residual and whitened values from vag_flux_density_batch at each group's rows with
    extinction applied, and chi2 against -2 (ln L - ln prior) of a fit that holds the group alone.  The tolerance is B plus what a
    1e-15-relative difference of the flux between the two requests (Fitter.counts documents it for an unpinned request) moves chi^2
    by: 2 w sum_i a_i sum_j |W_ij| 1e-15."""
    d = defs(A_V_DEF)
    truth = np.append(TRUTH, A_V_TRUE)
    kw = dict(extinction="smc")
    groups = [make_data(65, "cal", truth=truth, d=d, **kw), dict(make_data(63, "cal", truth=truth, d=d, **kw), weight=0.37)]
    f = cov_fitter(groups, **kw)
    got = f.correlated(truth, d)
    assert len(got) == 2
    p = f._params_at(truth, d)[0]
    for gd, res, g in zip(f._cov_obs, got, groups):
        n = gd["t"].size
        F = tl.device_series([p], gd["t"], gd["nu"])[0] * np.exp(-A_V_TRUE * f._cov_ext(gd, Z))
        assert set(res) == {"model", "residual", "whitened", "chi2"} and res["model"].shape == (n,)
        assert np.array_equal(res["model"], F) and np.array_equal(res["residual"], gd["ln_flux"] - np.log(F))
        assert np.allclose(res["whitened"], np.tril(gd["whitener"]) @ res["residual"], rtol=0, atol=1e-12 * np.abs(res["whitened"]).max())
        assert res["chi2"] == gd["weight"] * float(fitting.whitened_chi2(res["residual"], gd["whitener"]))
        alone = cov_fitter([g], **kw)
        lnl = alone.loglike_batch(truth[None], d)[0]  # (no priors: ln prior = 0)
        _, B, _ = reference(alone, truth[None], d)
        aW = np.abs(np.tril(gd["whitener"]))
        flux_term = 2 * gd["weight"] * np.sum((aW @ np.abs(res["residual"])) * (aW @ np.full(n, 1e-15)))
        print(f"correlated n={n}: chi2 {res['chi2']:.6g}, |chi2 + 2 ln L| / tolerance {abs(res['chi2'] + 2 * lnl) / (B[0] + flux_term):.3e}")
        assert abs(res["chi2"] + 2 * lnl) <= B[0] + flux_term
