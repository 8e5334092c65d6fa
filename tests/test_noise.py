"""Noise groups in the walker likelihood (vag_loglike_noise_batch[_dev]; the ``noise`` / ``calibration`` keywords of the Fitter's
add_flux_density / add_spectrum / add_flux and the parameters ``sys_<label>``) on the device: the arithmetic against the numpy
statement of the term (tests/test_noise_host.py) on the device's own model values, the CPU checker, the reductions, bits, edges and
a likelihood profile over a systematic.

The data are the C4 problem of tests/test_limits.py (3 bands x 20 epochs, the device's own truth with 5 % noise and 10 % errors)
plus a 10-row spectrum at a mid epoch: 70 point rows, so the kernel's lane loop wraps past 64.  Band 1 and the spectrum are noise
group "a" (calibration 0.05; interleaved in time with everything else), band 2 is group "b" (no calibration), band 3 has no
group.  Every seventh row is an upper limit; all rows carry random weights.  Two band groups: 5 epochs in group "c" (calibration
0.1, one limit row) and 3 epochs in group "b", so that sys_b spans two passes.  Free: FLUX_DEFS, sys_a (linear from 0) and sys_b
(log); sys_c is fixed."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import test_limits as tl
import test_limits_host as th_
import test_noise_host as nh
import test_sky_visfit as tv
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib, fitting

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

P = fitting.ParamDef
FLUX_DEFS, _c4_fixed = tv.FLUX_DEFS, tv._c4_fixed
SYS_C = 0.07
SPEC_T = configs.C4_EPOCHS[10]
SPEC_NU = np.geomspace(1e10, 1e17, 10)
BAND_C, BAND_C_T = tl.BAND, configs.C4_EPOCHS[3::4]  # 5 epochs
BAND_B, BAND_B_T = (5.06e14 * 0.5, 5.06e14 * 2.0), configs.C4_EPOCHS[5::6][:3]  # 3 epochs


def defs(sys_a=None, sys_b=None, sys_c=SYS_C, noise=True):
    """The parameter list: sys_a / sys_b free unless a value fixes them; sys_c=None leaves it out (a fitter without the band groups
    has no group c)."""
    fix = lambda name, v: P(name, v, v, fitting.Scale.fixed)  # noqa: E731
    d = list(FLUX_DEFS)
    if noise:
        d += [P("sys_a", 0.0, 2e3) if sys_a is None else fix("sys_a", sys_a),
              P("sys_b", 1e-3, 10.0, fitting.Scale.log) if sys_b is None else fix("sys_b", sys_b)]
        d += [fix("sys_c", sys_c)] if sys_c is not None else []
    return d + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))


@pytest.fixture(scope="module")
def prob():
    """The rows in the order they are added: 60 light-curve rows (band k = rows with nu == C4_BANDS[k]) and the 10 spectrum rows."""
    t, nu = configs.c4_mock_data()
    at_truth = [_abi.make_params(**configs.C4_TRUTH)]
    truth = np.concatenate([tl.device_series(at_truth, t, nu)[0], tl.device_series(at_truth, np.full(10, SPEC_T), SPEC_NU)[0]])
    t, nu = np.concatenate([t, np.full(10, SPEC_T)]), np.concatenate([nu, SPEC_NU])
    assert np.all(truth > 0)
    rng = np.random.default_rng(42)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(70)), 0.1 * truth
    lim = np.arange(70) % 7 == 3
    value = np.where(lim, truth + rng.uniform(-2.0, 4.0, 70) * err, obs)  # limits between 2 sigma below and 4 sigma above the truth
    w = rng.uniform(0.5, 2.0, 70)
    model = tv._c4_truth()
    bands = {}
    for key, band, bt in (("c", BAND_C, BAND_C_T), ("b", BAND_B, BAND_B_T)):
        tr = model.flux(bt, band[0], band[1], 7).total
        assert np.all(tr > 0)
        bands[key] = dict(t=bt, truth=tr, obs=tr * (1 + 0.05 * rng.standard_normal(bt.size)), err=0.1 * tr,
                          w=rng.uniform(0.5, 2.0, bt.size))
    bands["c"]["lim"] = np.array([False, False, True, False, False])
    bands["c"]["obs"][2] = bands["c"]["truth"][2] * 1.2
    return dict(t=t, nu=nu, truth=truth, value=value, err=err, lim=lim, w=w, bands=bands)


def make_fitter(prob, noise=True, calibration=True, bands=True, scatter_b=None):
    """noise=False: the same rows without noise=; calibration=False: groups without calibration fractions; scatter_b: factors that
    multiply the data of group b (its 20 point rows, then its 3 band rows)."""
    tr = configs.C4_TRUTH
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")

    def kw(label, cal=None):
        if not noise:
            return {}
        return dict(noise=label) if cal is None or not calibration else dict(noise=label, calibration=cal)
    value = prob["value"].copy()
    rows = [np.flatnonzero((prob["nu"] == b) & (np.arange(70) < 60)) for b in configs.C4_BANDS]
    if scatter_b is not None:
        value[rows[1]] = value[rows[1]] * scatter_b[:20]

    def add(sel, **k):
        f.add_flux_density(prob["nu"][sel], prob["t"][sel], value[sel], prob["err"][sel], weights=prob["w"][sel],
                           upper_limit=prob["lim"][sel], **k)
    add(rows[0], **kw("a", 0.05))
    add(rows[1], **kw("b"))
    add(rows[2])
    s = np.arange(60, 70)
    f.add_spectrum(SPEC_T, prob["nu"][s], value[s], prob["err"][s], weights=prob["w"][s], upper_limit=prob["lim"][s], **kw("a", 0.05))
    if bands:
        c, b = prob["bands"]["c"], prob["bands"]["b"]
        f.add_flux(BAND_C, c["t"], c["obs"], c["err"], num_points=7, weights=c["w"], upper_limit=c["lim"], **kw("c", 0.1))
        f.add_flux(BAND_B, b["t"], b["obs"] * (1.0 if scatter_b is None else scatter_b[20:]), b["err"], num_points=7, weights=b["w"],
                   **kw("b"))
    return f


def walkers(nb, seed=5):
    """[theta_c, theta_v, log10 E_iso, sys_a, log10 sys_b]; walker 0 has sys_a = 0 exactly, walker 1 sys_a = 1e3."""
    th, _ = tv._walkers(nb, seed=seed)
    rng = np.random.default_rng(seed + 100)
    sa = rng.uniform(0.0, 0.3, nb)
    sa[0], sa[1] = 0.0, 1e3
    return np.ascontiguousarray(np.column_stack([th, sa, rng.uniform(-3.0, 0.0, nb)]))


def model_values(f, samples, d, with_bands=True):
    """The device's own model values at the fitter's rows: the point rows from vag_flux_density_batch, the band groups from
    Model.flux."""
    f._consolidate_data()
    F = tl.device_series([f._params_at(s, d)[0] for s in samples], f._all_t, f._all_nu)
    bands = []
    if with_bands:
        for bd in f._band_obs:
            bands.append(np.array([f.model(s, d).flux(bd["t"], bd["nu_min"], bd["nu_max"], bd["num_points"]).total for s in samples]))
    return F, bands


def formula(f, d, samples, F, bands):
    """ln L of the fitter in numpy on model values F [nb][n] and bands[g] [nb][n_g]: ungrouped detections th_.detection_lnl, limit
    rows th_.limit_lnl whatever their group, and nh.noise_lnl for the detections of every (group, pass)."""
    f._consolidate_data()
    free = [pd for pd in d if pd.scale is not fitting.Scale.fixed]
    s_of = {}
    for g, label in enumerate(f._noise_labels):
        name = "sys_" + label
        col = [k for k, pd in enumerate(free) if pd.name == name]
        if col:
            v = samples[:, col[0]]
            s_of[g] = 10.0 ** v if free[col[0]].scale is fitting.Scale.log else v
        else:
            fixed = [pd for pd in d if pd.name == name]
            s_of[g] = np.full(samples.shape[0], fixed[0].lower if fixed else 0.0)
    cal = [f._noise_calib.get(label, 0.0) for label in f._noise_labels]

    def block(lnf, lne, w, model, grp, lim):
        kind = np.zeros(w.size, dtype=bool) if lim is None else np.asarray(lim["kind"]) == 1
        grp = np.full(w.size, -1) if grp is None else np.asarray(grp)
        plain = ~kind & (grp < 0)
        total = th_.detection_lnl(lnf[plain], model[:, plain], lne[plain], w[plain])
        if kind.any():
            total = total + th_.limit_lnl(lim["limit"][kind], model[:, kind], lim["sigma"][kind], w[kind])
        for g in sorted(set(grp[grp >= 0].tolist())):
            sel = ~kind & (grp == g)
            total = total + nh.noise_lnl(lnf[sel], model[:, sel], lne[sel], w[sel], s_of[g], cal[g])
        return total
    total = block(f._all_log_flux, f._all_log_err, f._all_weights, F, f._all_grp, f._all_lim)
    for bd, M in zip(f._band_obs, bands):
        lim = None if bd["lim"] is None else dict(kind=bd["lim"], limit=bd["limit"], sigma=bd["sigma"])
        total = total + block(bd["ln_flux"], bd["ln_err"], bd["weights"], M, np.full(bd["t"].size, bd["noise"]), lim)
    return total


def rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@pytest.fixture(scope="module")
def ref64(prob):
    """The 64 walkers of the arithmetic and reduction tests, the full fitter and the device's model values at them (computed once)."""
    f, d, th = make_fitter(prob), defs(), walkers(64)
    F, bands = model_values(f, th, d)
    return dict(f=f, d=d, th=th, F=F, bands=bands)


# ---------------------------------------------------------------- 1. arithmetic
# measured on an MI355X: the largest |got - want| / max(1, |want|) over the 64 walkers is MEASURED_ARITH = 4.3e-15 (host entry; the
# device-pointer entry returns the same bits, test_bits); the gate is 4 x that, 1.72e-14.  Anything above 1e-9, the cap of the host test, would be an algebra
# error, not rounding.
MEASURED_ARITH = 4.3e-15
ARITH_GATE = 4 * MEASURED_ARITH


def test_likelihood_matches_the_formula_on_device_fluxes(prob, ref64):
    f, d, th, F, bands = (ref64[k] for k in ("f", "d", "th", "F", "bands"))
    assert f.has_noise_groups and f.has_limits and f._noise_labels == ["a", "b", "c"]
    assert th[0, 3] == 0.0 and th[1, 3] == 1e3
    f._consolidate_data()
    assert f._all_t.size == 70 and (f._all_grp == 0).sum() == 30 and (f._all_grp == 1).sum() == 20 and f._all_lim["kind"].sum() == 10
    assert np.any(np.diff(f._all_grp[f._all_grp >= 0]) != 0)  # the groups interleave in time
    want = formula(f, d, th, F, bands)
    got = f.loglike_batch(th, d)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and f.last_plan.n_walkers_rejected == 0
    plain = make_fitter(prob, noise=False)
    diff = got - plain.loglike_batch(np.ascontiguousarray(th[:, :3]), defs(noise=False))
    measured = rel(got, want)
    print("noise groups: rel to the formula", measured, "ln L range", want.min(), want.max(), "change against no groups",
          np.abs(diff).min(), np.abs(diff).max())
    assert np.all(np.abs(diff) > 1e-3)  # the groups do change every walker's value
    assert measured <= 1e-9, "an algebra error, not rounding"
    assert MEASURED_ARITH <= 1e-9
    assert measured <= ARITH_GATE


# ---------------------------------------------------------------- 2. the CPU checker
def test_against_the_cpu_checker(prob, oracle):
    """The fitter without its band groups on 16 draws of the prior box (one with theta_c < 0: the checker raises, the device scores
    -inf): ln L against the formula on the CPU checker's fluxes, at the gate of
    test_gpu_parity.test_loglike_batch_matches_fitter_formula_on_oracle_fluxes; -inf on the same walkers."""
    f, d = make_fitter(prob, bands=False), defs(sys_c=None)
    _, lo, hi = f.build_spec(d)
    rng = np.random.default_rng(0)
    samples = lo + (hi - lo) * rng.random((16, len(lo)))
    samples[:, 3] = rng.uniform(0.0, 0.5, 16)  # sys_a: the lower part of its wide box
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


# ---------------------------------------------------------------- 3. reductions
def test_zero_systematics_without_calibration_is_the_plain_fitter(prob, ref64):
    """All sys fixed at 0 and no calibration: the fitter built without noise=, to rtol 1e-13 -- the terms are the same numbers summed
    in another order (70 positive terms x eps) and w / sigma^2 r^2 against w (r / sigma)^2 (a few ulp per term)."""
    th = np.ascontiguousarray(ref64["th"][:, :3])
    grouped, plain = make_fitter(prob, calibration=False), make_fitter(prob, noise=False)
    d0 = defs(sys_a=0.0, sys_b=0.0, sys_c=0.0)
    a = grouped.loglike_batch(th, d0)
    b = plain.loglike_batch(th, defs(noise=False))
    spec, _, _ = grouped.build_spec(d0)
    assert spec._noise is not None and plain.build_spec(defs(noise=False))[0]._noise is None
    print("s = c = 0 against no groups: rel", np.max(np.abs(a - b) / np.abs(b)))
    assert np.all(np.isfinite(b))
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)
    assert np.array_equal(a, grouped.loglike_batch(th, FLUX_DEFS + _c4_fixed(skip=("theta_c", "theta_v", "E_iso"))))  # 0 when not given


def _call(name, spec, samples, *extra):
    lib = _lib.load()
    h, lock = va.get_context(0)
    out = np.empty(samples.shape[0])
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    with lock:
        rc = getattr(lib, name)(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), *extra,
                                samples.ctypes.data_as(dp), samples.shape[0], spec.ndim, out.ctypes.data_as(dp))
    return rc, out


def test_null_noise_spec_is_bitwise_the_limit_call(prob, ref64):
    th = np.ascontiguousarray(ref64["th"][:, :3])
    f = make_fitter(prob, noise=False)
    spec, _, _ = f.build_spec(defs(noise=False))
    rc, a = _call("vag_loglike_lim_batch", spec, th)
    assert rc == 0 and np.all(np.isfinite(a))
    none = _lib.NoiseFitSpec()  # groups, but no grouped row
    none.n_groups, none.n_bands = 2, 2
    ids = np.full(2, -1, dtype=np.int32)
    none.band_group = ids.ctypes.data_as(C.POINTER(C.c_int32))
    for nz in (None, none):
        rc, b = _call("vag_loglike_noise_batch", spec, th, C.byref(nz) if nz is not None else None)
        assert rc == 0 and np.array_equal(a, b)
    assert np.array_equal(f.loglike_batch(th, defs(noise=False)), a)


# ---------------------------------------------------------------- 4. bits
def test_bits(ref64):
    import torch
    f, d, th = ref64["f"], ref64["d"], ref64["th"]
    a = f.loglike_batch(th, d)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, f.loglike_batch(th, d))  # run to run (and in the evaluation order the first call left)
    assert np.array_equal(tv._with_hook("VAG_NO_ORDER", "1", lambda: f.loglike_batch(th, d)), a)
    assert np.array_equal(f.loglike_batch(np.ascontiguousarray(th[::-1]), d)[::-1], a)
    assert f.loglike_batch(th[7:8], d)[0] == a[7]  # alone
    ev = f.device_evaluator(d)
    assert ev.has_noise_groups and ev.has_limits
    vals, _ = ev(torch.from_numpy(th).to("cuda:0"))
    torch.cuda.synchronize()
    assert np.array_equal(vals.cpu().numpy(), a)
    with pytest.raises(NotImplementedError, match="noise="):
        ev.native.shard(None, 64, 0, 1, None)


# ---------------------------------------------------------------- 5. edges
def test_edges(prob):
    f, d = make_fitter(prob), defs()
    th = walkers(8, seed=3)
    th[1, 3] = 0.2
    good = f.log_prob_batch(th, d)
    assert np.all(np.isfinite(good))
    out = th.copy()
    out[2, 3] = -1e-3  # sys_a below its lower bound 0
    out[3, 4] = 1.5    # sys_b above its upper bound 10
    lp = f.log_prob_batch(out, d)
    assert lp[2] == -np.inf and lp[3] == -np.inf and np.array_equal(np.delete(lp, [2, 3]), np.delete(good, [2, 3]))
    bad = th.copy()
    bad[4, 0] = np.nan  # an invalid model parameter
    ll = f.loglike_batch(bad, d)
    assert ll[4] == -np.inf and f.last_plan.n_walkers_rejected == 1
    assert np.array_equal(np.delete(ll, 4), np.delete(f.loglike_batch(th, d), 4))
    # no model flux at a grouped detection row (far above the synchrotron cut-off): the 1e-300 clamp, finite
    g, d = make_fitter(prob, bands=False), defs(sys_c=None)
    g.add_flux_density(1e30, [prob["t"][30]], [1e-28], [2e-29], weights=[0.7], noise="a", calibration=0.05)
    F, _ = model_values(g, th, d, with_bands=False)
    assert np.all(F[:, g._all_nu == 1e30] == 0)
    got = g.loglike_batch(th, d)
    want = formula(g, d, th, F, [])
    print("clamped row: ln L", got.min(), got.max(), "rel", rel(got, want))
    assert np.all(np.isfinite(got)) and g.last_plan.n_walkers_rejected == 0 and rel(got, want) <= 1e-9
    assert np.all(got < f.loglike_batch(th, d) - 1e3)  # the row dominates: (ln 1e-28 + 690.8)^2 / (0.2^2 + s^2)


def test_invalid_noise_specs_through_the_c_abi(prob):
    f, d = make_fitter(prob), defs()
    th = walkers(4, seed=3)
    spec, _, _ = f.build_spec(d)
    nz = spec._noise
    rc, out = _call("vag_loglike_noise_batch", spec, th, C.byref(nz))
    assert rc == 0 and np.all(np.isfinite(out))

    def refused(word):
        rc, _ = _call("vag_loglike_noise_batch", spec, th, C.byref(nz))
        msg = _lib.load().vag_last_error().decode()
        assert rc == _lib.VAG_E_INVALID and word in msg, (rc, msg)
    old = spec.slot[3]
    spec.slot[3] = _lib.P_NOISE_SYS0 + 5  # a systematic of a group the noise spec does not have
    refused("bad parameter slot")
    spec.slot[3] = old
    rc, _ = _call("vag_loglike_lim_batch", spec, th)  # the earlier entry points do not know the slots
    assert rc == _lib.VAG_E_INVALID and "bad parameter slot" in _lib.load().vag_last_error().decode()
    for i, v, word in ((0, 3, "point row 0"), (69, -2, "point row 69")):
        keep = f._all_grp[i]
        f._all_grp[i] = v
        refused(word)
        f._all_grp[i] = keep
    for arr, v, word in ((nz.sys_fixed, -0.1, "noise group 2"), (nz.sys_fixed, np.nan, "noise group 2"),
                         (nz.calib, -1.0, "noise group 2"), (nz.calib, np.inf, "noise group 2")):
        keep = arr[2]
        arr[2] = v
        refused(word)
        arr[2] = keep
    nz.n_bands = 1
    refused("n_bands")
    nz.n_bands = 2
    nz.n_groups = 9
    refused("n_groups")
    nz.n_groups = 3
    nz.band_group[1] = 2  # group c (calibration 0.1) in both band groups
    refused("2 passes")
    nz.band_group[1] = 3
    refused("band group 1")
    nz.band_group[1] = 1
    rc, again = _call("vag_loglike_noise_batch", spec, th, C.byref(nz))
    assert rc == 0 and np.array_equal(again, out)


# ---------------------------------------------------------------- 6. a profile
def test_profile_over_a_systematic(prob):
    """Model parameters at the truth, 20 % extra scatter (fixed seed) on the data of group b, one batch of 41 values of sys_b on a log
    grid: the device's ln L peaks at the grid point where the formula on the same fluxes does, strictly inside the grid."""
    rng = np.random.default_rng(17)
    f = make_fitter(prob, scatter_b=1.0 + 0.2 * rng.standard_normal(23))
    d = defs(sys_a=0.02)
    tr = configs.C4_TRUTH
    grid = np.linspace(-3.0, 1.0, 41)
    th = np.ascontiguousarray(np.column_stack([np.full(41, tr["theta_c"]), np.full(41, tr["theta_obs"]),
                                               np.full(41, np.log10(tr["E_iso"])), grid]))
    got = f.loglike_batch(th, d)
    F, bands = model_values(f, th[:1], d)
    want = formula(f, d, th, np.repeat(F, 41, axis=0), [np.repeat(b, 41, axis=0) for b in bands])
    k = int(np.argmax(got))
    print("profile over sys_b: argmax", k, "sys_b", 10.0 ** grid[k], "rel", rel(got, want))
    assert np.all(np.isfinite(got)) and k == int(np.argmax(want)) and 0 < k < 40
    assert rel(got, want) <= 1e-9
