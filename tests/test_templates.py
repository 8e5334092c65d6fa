"""Additive templates in the walker likelihood (vag_loglike_tmpl_batch[_dev]; the ``templates`` keyword of the Fitter's
add_flux_density / add_spectrum / add_flux, Fitter.add_template and the parameters ``amp_<name>``) on the device: the arithmetic
against the numpy statement of the term (fitting.template_terms, tests/test_templates_host.py) on the device's own model values,
the reduction to the fit without templates bit for bit, the CPU checker, bits, edges and a likelihood profile over an amplitude.

The data are the 70-row C4 problem of tests/test_noise.py through its helpers (3 bands x 20 epochs plus a 10-row spectrum, every
seventh row a limit, random weights, noise groups a, b, c and the two band groups), so the kernel's lane loop wraps past 64, with
    host1 = 1 on the rows of point band 1, host3 = 1 on point band 3 (plain: added behind the dust),
    sn    = a log-normal bump in t of unit peak on point band 2 and on the spectrum (extinguished),
    hostB = 1 on band group "c",
under Fitter(extinction="smc") with a fixed A_V = 0.3, so that the split into extinguished and plain templates matters.  Noise
group a spans templated rows of two kinds, group b templated point rows and an untemplated band group.  The truth amplitudes are the
truth flux of each data set's last epoch (the late rows about double); the data of tests/test_noise.py are scaled row by row to the
truth with templates, so they keep their 5 % noise, 10 % errors and limit offsets.  Free: FLUX_DEFS, amp_host1 (linear from 0),
amp_sn (log), sys_a, sys_b; amp_host3, amp_hostB and sys_c are fixed."""
import ctypes as C

import numpy as np
import pytest

import configs
import test_noise as tn
import test_sky_visfit as tv
import vegasafterglow_amd as va
from test_noise import prob  # noqa: F401  (the module-scoped fixture of the 70-row problem)
from vegasafterglow_amd import _lib, fitting

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)

P = fitting.ParamDef
A_V = 0.3
SN_PEAK, SN_WIDTH = 60.0 * 86400.0, 0.5


def sn_bump(t):
    return np.exp(-0.5 * (np.log(np.asarray(t, float) / SN_PEAK) / SN_WIDTH) ** 2)


def point_rows(prob):
    return [np.flatnonzero((prob["nu"] == b) & (np.arange(70) < 60)) for b in configs.C4_BANDS]


def truth_amps(prob):
    rows = point_rows(prob)
    last = lambda r: float(prob["truth"][r][np.argmax(prob["t"][r])])  # noqa: E731
    return dict(host1=last(rows[0]), sn=last(rows[1]), host3=last(rows[2]), hostB=float(prob["bands"]["c"]["truth"][-1]))


def ext_kernel(nu):
    """0.4 ln10 k(lambda_rest) of the SMC law at the C4 redshift, as the Fitter forms it for its point rows."""
    from vegasafterglow_amd.extinction import BUILTIN_LAWS
    lam = (2.99792458e10 / np.asarray(nu, float)) / (1.0 + configs.C4_TRUTH["z"])
    return 0.4 * np.log(10.0) * np.asarray(BUILTIN_LAWS["smc"](lam), dtype=np.float64)


def point_templates(prob):
    """T [4][70] in the order the rows are added, templates numbered sn, host1, host3, hostB."""
    rows = point_rows(prob)
    T = np.zeros((4, 70))
    T[0, rows[1]] = sn_bump(prob["t"][rows[1]])
    T[0, 60:] = sn_bump(tn.SPEC_T)
    T[1, rows[0]] = 1.0
    T[2, rows[2]] = 1.0
    return T


def truth_ratio(prob):
    """(truth with templates) / truth for the point rows and for band group c: what the data of tests/test_noise.py are scaled by."""
    a = truth_amps(prob)
    T = point_templates(prob)
    e, x = fitting.template_terms(T, [a["sn"], a["host1"], a["host3"], a["hostB"]], [1, 0, 0, 0])
    with_t = (prob["truth"] + x) * np.exp(-A_V * ext_kernel(prob["nu"])) + e
    c = prob["bands"]["c"]["truth"]
    return with_t / prob["truth"], (c + a["hostB"]) / c, with_t


def make_fitter(prob, templates=True, noise=True, limits=True, bands=True, exact=False):
    """templates=False: the same rows without templates=; noise / limits = False: no noise groups / every row a detection (the plain
    back kernel's path); exact: data = the truth with templates exactly (for the profile)."""
    tr = configs.C4_TRUTH
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism", extinction="smc")
    ratio, ratio_c, with_t = truth_ratio(prob)
    rows = point_rows(prob)
    lim = prob["lim"] if limits else np.zeros(70, dtype=bool)
    value, err = prob["value"] * ratio, prob["err"] * ratio
    if exact:
        value = np.where(lim, value, with_t)
    T = point_templates(prob)
    if templates:
        f.add_template("sn", extinguished=True)

    def kw(label, cal=None, **tm):
        k = {}
        if noise and label is not None:
            k.update(dict(noise=label) if cal is None else dict(noise=label, calibration=cal))
        if templates:
            k["templates"] = tm
        return k

    def add(sel, **k):
        f.add_flux_density(prob["nu"][sel], prob["t"][sel], value[sel], err[sel], weights=prob["w"][sel], upper_limit=lim[sel], **k)
    add(rows[0], **kw("a", 0.05, host1=1.0))
    add(rows[1], **kw("b", sn=T[0, rows[1]]))
    add(rows[2], **kw(None, host3=1.0))
    s = np.arange(60, 70)
    f.add_spectrum(tn.SPEC_T, prob["nu"][s], value[s], err[s], weights=prob["w"][s], upper_limit=lim[s], **kw("a", 0.05, sn=T[0, s]))
    if bands:
        c, b = prob["bands"]["c"], prob["bands"]["b"]
        obs_c = np.where(c["lim"] | (not exact), c["obs"], c["truth"]) * ratio_c
        f.add_flux(tn.BAND_C, c["t"], obs_c, c["err"] * ratio_c, num_points=7, weights=c["w"], upper_limit=c["lim"] if limits else None,
                   **kw("c", 0.1, hostB=1.0))
        f.add_flux(tn.BAND_B, b["t"], b["truth"] if exact else b["obs"], b["err"], num_points=7, weights=b["w"], **kw("b"))
    return f


def defs(prob, amp_host1=None, amp_sn=None, amp_host3="truth", amp_hostB="truth", sys_a=None, sys_b=None, noise=True, templates=True,
         bands=True):
    """The parameter list: amp_host1 / amp_sn / sys_a / sys_b free unless a value fixes them; amp_host3 / amp_hostB fixed at the truth
    unless a value is given.  bands=False leaves out sys_c and amp_hostB (a fitter without the band groups has neither)."""
    fix = lambda name, v: P(name, v, v, fitting.Scale.fixed)  # noqa: E731
    a = truth_amps(prob)
    d = list(tn.FLUX_DEFS)
    if templates:
        d += [P("amp_host1", 0.0, 10.0 * a["host1"]) if amp_host1 is None else fix("amp_host1", amp_host1),
              P("amp_sn", 1e-3 * a["sn"], 10.0 * a["sn"], fitting.Scale.log) if amp_sn is None else fix("amp_sn", amp_sn),
              fix("amp_host3", a["host3"] if amp_host3 == "truth" else amp_host3)]
        d += [fix("amp_hostB", a["hostB"] if amp_hostB == "truth" else amp_hostB)] if bands else []
    if noise:
        d += [P("sys_a", 0.0, 2e3) if sys_a is None else fix("sys_a", sys_a),
              P("sys_b", 1e-3, 10.0, fitting.Scale.log) if sys_b is None else fix("sys_b", sys_b)]
        d += [fix("sys_c", tn.SYS_C)] if bands else []
    return d + [fix("A_V", A_V)] + tn._c4_fixed(skip=("theta_c", "theta_v", "E_iso"))


def walkers(prob, nb, seed=5):
    """[theta_c, theta_v, log10 E_iso, amp_host1, log10 amp_sn, sys_a, log10 sys_b]; walker 0 has amp_host1 = 0 exactly."""
    th, _ = tv._walkers(nb, seed=seed)
    a = truth_amps(prob)
    rng = np.random.default_rng(seed + 200)
    h1 = a["host1"] * rng.uniform(0.3, 2.0, nb)
    h1[0] = 0.0
    sn = np.log10(a["sn"]) + rng.uniform(-1.0, 0.5, nb)
    return np.ascontiguousarray(np.column_stack([th, h1, sn, rng.uniform(0.0, 0.3, nb), rng.uniform(-3.0, 0.0, nb)]))


def with_templates(f, d, samples, F, bands):
    """The rows' model values f_i = (F_i + x_i) exp(-A_V k_i) + e_i on model fluxes F [nb][n] and bands[g] [nb][n_g], in numpy:
    template_terms on the spec's own template arrays and amplitudes (a pass without an extinction kernel: factor 1)."""
    spec, _, _ = f.build_spec(d)
    tp = spec._tmpl
    nt = tp.n_templates
    amp = np.tile(np.array(tp.amp_fixed[:nt]), (samples.shape[0], 1))
    for k in range(spec.ndim):
        c = spec.slot[k] - _lib.P_TMPL_AMP0
        if 0 <= c < nt:
            amp[:, c] = 10.0 ** samples[:, k] if spec.is_log[k] else samples[:, k]
    flags = list(tp.extinguished[:nt])
    n = spec.n_data
    e, x = fitting.template_terms(np.ctypeslib.as_array(tp.point, (nt, n)), amp, flags)
    out = (F + x) * np.exp(-A_V * f._ext_kernel) + e
    out_b = []
    for g, M in enumerate(bands):
        if tp.n_bands and tp.bands[g]:
            e, x = fitting.template_terms(np.ctypeslib.as_array(tp.bands[g], (nt, M.shape[1])), amp, flags)
            M = (M + x) + e
        out_b.append(M)
    return out, out_b


def formula(f, d, samples, F, bands):
    """ln L in numpy: the rows' model values with templates, then the pieces of tests/test_noise.py applied to them."""
    fi, fb = with_templates(f, d, samples, F, bands)
    return tn.formula(f, d, samples, fi, fb)


rel = tn.rel


@pytest.fixture(scope="module")
def ref64(prob):  # noqa: F811
    """The 64 walkers of the arithmetic, reduction and bits tests, the full fitter and the device's model values at them (once)."""
    f, d, th = make_fitter(prob), defs(prob), walkers(prob, 64)
    F, bands = tn.model_values(f, th, d)
    return dict(f=f, d=d, th=th, F=F, bands=bands)


# ---------------------------------------------------------------- 1. arithmetic
# measured on an MI355X: the largest |got - want| / max(1, |want|) over the 64 walkers is MEASURED_ARITH = 4.83e-15 (host entry; the
# device-pointer entry returns the same bits, test_bits); the gate is 4 x that, 1.93e-14.  Anything above 1e-9 would be an algebra
# error, not rounding.
MEASURED_ARITH = 4.83e-15
ARITH_GATE = 4 * MEASURED_ARITH


def test_likelihood_matches_the_formula_on_device_fluxes(prob, ref64):  # noqa: F811
    f, d, th, F, bands = (ref64[k] for k in ("f", "d", "th", "F", "bands"))
    assert f.has_templates and f.has_noise_groups and f.has_limits and f._tmpl_names == ["sn", "host1", "host3", "hostB"]
    assert f._tmpl_ext == [True, False, False, False] and th[0, 3] == 0.0
    spec, _, _ = f.build_spec(d)
    T = np.ctypeslib.as_array(spec._tmpl.point, (4, 70))
    assert spec.n_data == 70 and [(T[c] != 0).sum() for c in range(4)] == [30, 20, 20, 0] and f._all_lim["kind"].sum() == 10
    assert np.all(f._ext_kernel[f._all_nu == configs.C4_BANDS[1]] > 0.5)  # the optical rows are extinguished: x and e differ
    want = formula(f, d, th, F, bands)
    got = f.loglike_batch(th, d)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and f.last_plan.n_walkers_rejected == 0
    plain = make_fitter(prob, templates=False)
    diff = got - plain.loglike_batch(np.ascontiguousarray(th[:, [0, 1, 2, 5, 6]]), defs(prob, templates=False))
    measured = rel(got, want)
    print("templates: rel to the formula", measured, "ln L range", want.min(), want.max(), "change against no templates",
          np.abs(diff).min(), np.abs(diff).max())
    assert np.all(np.abs(diff) > 1e-3)  # the templates do change every walker's value (amp_sn, amp_host3, amp_hostB are never 0)
    assert measured <= 1e-9, "an algebra error, not rounding"
    assert MEASURED_ARITH <= 1e-9
    assert measured <= ARITH_GATE


# ---------------------------------------------------------------- 2. zero amplitudes
def _call(name, spec, samples, *extra):
    lib = _lib.load()
    h, lock = va.get_context(0)
    out = np.empty(samples.shape[0])
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    with lock:
        rc = getattr(lib, name)(h, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise),
                                ref(spec._counts), ref(spec._index), ref(spec._fold), *extra,
                                samples.ctypes.data_as(dp), samples.shape[0], spec.ndim, out.ctypes.data_as(dp))
    return rc, out


def test_zero_amplitudes_are_the_fit_without_templates_bit_for_bit(prob, ref64):  # noqa: F811
    """x + 0.0 and f + 0.0 are exact and the sums keep their order: with noise groups and limits (the noise kernel's path) and
    without either (the plain kernel's path), and with limits alone (the plain kernel's limit variant)."""
    th = ref64["th"]
    zero = dict(amp_host1=0.0, amp_sn=0.0, amp_host3=0.0, amp_hostB=0.0)
    for kw, cols in ((dict(), [0, 1, 2, 5, 6]), (dict(noise=False, limits=False), [0, 1, 2]), (dict(noise=False), [0, 1, 2])):
        t0 = np.ascontiguousarray(th[:, cols])
        with_t, without = make_fitter(prob, **kw), make_fitter(prob, templates=False, **kw)
        noise = kw.get("noise", True)
        a = with_t.loglike_batch(t0, defs(prob, noise=noise, **zero))
        b = without.loglike_batch(t0, defs(prob, noise=noise, templates=False))
        assert with_t.build_spec(defs(prob, noise=noise, **zero))[0]._tmpl is not None
        assert without.build_spec(defs(prob, noise=noise, templates=False))[0]._tmpl is None
        assert np.all(np.isfinite(b)) and np.array_equal(a, b), kw
        # the amplitudes not given at all are 0 too
        assert np.array_equal(with_t.loglike_batch(t0, defs(prob, noise=noise, templates=False)), b)


def test_null_or_untouched_template_spec_is_bitwise_the_fold_call(prob, ref64):  # noqa: F811
    th = np.ascontiguousarray(ref64["th"][:, [0, 1, 2, 5, 6]])
    f = make_fitter(prob, templates=False)
    d = defs(prob, templates=False)
    spec, _, _ = f.build_spec(d)
    rc, a = _call("vag_loglike_fold_batch", spec, th)
    assert rc == 0 and np.all(np.isfinite(a))
    none = _lib.TemplateFitSpec()  # templates, but no touched row
    none.n_templates, none.n_bands = 3, 2
    zp, zb = np.zeros((3, 70)), [np.zeros((3, 5)), np.zeros((3, 3))]
    none.point = zp.ctypes.data_as(dp)
    none.bands = (dp * 2)(*[z.ctypes.data_as(dp) for z in zb])
    none.amp_fixed[0], none.extinguished[1] = 1e-27, 1
    for tp in (None, none):
        rc, b = _call("vag_loglike_tmpl_batch", spec, th, C.byref(tp) if tp is not None else None)
        assert rc == 0 and np.array_equal(a, b)
    assert np.array_equal(f.loglike_batch(th, d), a)


# ---------------------------------------------------------------- 3. the CPU checker
def test_against_the_cpu_checker(prob, oracle):  # noqa: F811
    """The fitter without its band groups on 16 draws of the prior box (one with theta_c < 0: the checker raises, the device scores
    -inf): ln L against the formula on the CPU checker's fluxes, at the gate of tests/test_noise.py; -inf on the same walkers."""
    import _abi
    f, d = make_fitter(prob, bands=False), defs(prob, bands=False)
    _, lo, hi = f.build_spec(d)
    rng = np.random.default_rng(0)
    samples = lo + (hi - lo) * rng.random((16, len(lo)))
    samples[:, 5] = rng.uniform(0.0, 0.5, 16)  # sys_a: the lower part of its wide box
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
    assert ev.has_templates and ev.has_noise_groups and ev.has_limits
    vals, _ = ev(torch.from_numpy(th).to("cuda:0"))
    torch.cuda.synchronize()
    assert np.array_equal(vals.cpu().numpy(), a)
    with pytest.raises(NotImplementedError, match="templates="):
        ev.native.shard(None, 64, 0, 1, None)


# ---------------------------------------------------------------- 5. edges
def test_edges(prob):  # noqa: F811
    f, d = make_fitter(prob), defs(prob)
    a = truth_amps(prob)
    th = walkers(prob, 8, seed=3)
    th[0, 3] = 0.5 * a["host1"]
    good = f.log_prob_batch(th, d)
    assert np.all(np.isfinite(good))
    out = th.copy()
    out[2, 3] = -1e-3 * a["host1"]  # amp_host1 below its lower bound 0
    out[3, 4] = np.log10(a["sn"]) + 1.5  # amp_sn above its upper bound
    lp = f.log_prob_batch(out, d)
    assert lp[2] == -np.inf and lp[3] == -np.inf and np.array_equal(np.delete(lp, [2, 3]), np.delete(good, [2, 3]))
    base = f.loglike_batch(th, d)
    for col, v in ((3, -1e-3 * a["host1"]), (3, np.nan), (4, np.nan), (0, np.nan)):  # a negative / NaN amplitude, a NaN model parameter
        bad = th.copy()
        bad[4, col] = v
        ll = f.loglike_batch(bad, d)
        assert ll[4] == -np.inf and f.last_plan.n_walkers_rejected == 1, (col, v)
        assert np.array_equal(np.delete(ll, 4), np.delete(base, 4)), (col, v)
    # no model flux at a templated detection row (far above the synchrotron cut-off): f_i = e_i, no clamp, finite
    g, dg = make_fitter(prob, bands=False), defs(prob, bands=False)
    g.add_flux_density(1e30, [prob["t"][30]], [a["host1"]], [0.2 * a["host1"]], weights=[0.7], noise="a", calibration=0.05,
                       templates={"host1": 1.0})
    F, _ = tn.model_values(g, th, dg, with_bands=False)
    assert np.all(F[:, g._all_nu == 1e30] == 0)
    got = g.loglike_batch(th, dg)
    want = formula(g, dg, th, F, [])
    print("templated row without model flux: ln L", got.min(), got.max(), "rel", rel(got, want))
    assert np.all(np.isfinite(got)) and g.last_plan.n_walkers_rejected == 0 and rel(got, want) <= 1e-9
    assert np.all(got > -1e4)  # (no clamp: ln(1e-300) would cost ~1e6)
    # the same row with amplitude 0: the 1e-300 clamp, as without templates
    d0 = defs(prob, bands=False, amp_host1=0.0)
    t0 = np.ascontiguousarray(th[:, [0, 1, 2, 4, 5, 6]])
    got0 = g.loglike_batch(t0, d0)
    want0 = formula(g, d0, t0, F, [])
    print("the same row, amplitude 0: ln L", got0.min(), got0.max(), "rel", rel(got0, want0))
    assert np.all(np.isfinite(got0)) and g.last_plan.n_walkers_rejected == 0 and rel(got0, want0) <= 1e-9
    assert np.all(got0 < got - 1e3)  # the row dominates: (ln F_obs + 690.8)^2 / (0.2^2 + s^2)
    # a limit row under a template whose amplitude alone exceeds the limit by 10 sigma: finite and very negative
    A = 0.5 * a["host1"]
    h, dh = make_fitter(prob, bands=False), defs(prob, bands=False, amp_host1=A)
    before = h.loglike_batch(t0, dh)
    h.add_flux_density(3e9, [prob["t"][30]], [A * 3 / 13], [A / 13], weights=[1.0], upper_limit=True, templates={"host1": 1.0})
    after = h.loglike_batch(t0, dh)
    Fh, _ = tn.model_values(h, t0, dh, with_bands=False)
    print("limit row 10 sigma below a template: ln L change", (after - before).min(), (after - before).max())
    assert np.all(np.isfinite(after)) and h.last_plan.n_walkers_rejected == 0 and rel(after, formula(h, dh, t0, Fh, [])) <= 1e-9
    # ((L - f) / sigma <= -10 and ln Phi(-10) = -53.2; a limit row leaves the detections' weights as they were)
    assert np.all(after < before - 50.0)


def test_invalid_template_specs_through_the_c_abi(prob):  # noqa: F811
    f, d = make_fitter(prob), defs(prob)
    th = walkers(prob, 4, seed=3)
    spec, _, _ = f.build_spec(d)
    tp = spec._tmpl
    rc, out = _call("vag_loglike_tmpl_batch", spec, th, C.byref(tp))
    assert rc == 0 and np.all(np.isfinite(out))

    def refused(*words):
        rc, _ = _call("vag_loglike_tmpl_batch", spec, th, C.byref(tp))
        msg = _lib.load().vag_last_error().decode()
        assert rc == _lib.VAG_E_INVALID and all(w in msg for w in words), (rc, msg)
    old = spec.slot[3]
    spec.slot[3] = _lib.P_TMPL_AMP0 + 5  # an amplitude of a template the spec does not have
    refused("bad parameter slot")
    spec.slot[3] = old
    rc, _ = _call("vag_loglike_fold_batch", spec, th)  # the earlier entry points do not know the slots
    assert rc == _lib.VAG_E_INVALID and "bad parameter slot" in _lib.load().vag_last_error().decode()
    T = np.ctypeslib.as_array(tp.point, (4, 70))
    for c, i, v in ((0, 0, -1.0), (3, 69, np.nan), (1, 5, np.inf)):
        keep = T[c, i]
        T[c, i] = v
        refused(f"template {c}", f"point row {i}")
        T[c, i] = keep
    B = np.ctypeslib.as_array(tp.bands[0], (4, 5))
    B[3, 2] = -1e-300
    refused("template 3", "band group 0", "row 2")
    B[3, 2] = 1.0
    for arr, v, word in ((tp.amp_fixed, -1e-30, "template 2"), (tp.amp_fixed, np.nan, "template 2"), (tp.extinguished, 2, "template 2"),
                         (tp.extinguished, -1, "template 2")):
        keep = arr[2]
        arr[2] = v
        refused(word)
        arr[2] = keep
    tp.n_bands = 1
    refused("n_bands")
    tp.n_bands = 2
    tp.n_templates = 9
    refused("n_templates")
    tp.n_templates = 4
    rc, again = _call("vag_loglike_tmpl_batch", spec, th, C.byref(tp))
    assert rc == 0 and np.array_equal(again, out)


# ---------------------------------------------------------------- 6. a profile
def test_profile_over_an_amplitude(prob):  # noqa: F811
    """Noise-free data (the truth with templates exactly), the parameters at the truth, one batch of 9 values of amp_host1, the truth
    x 1.5^k for k = -4 .. 4: ln L peaks at k = 0 and falls monotonically on both sides."""
    f = make_fitter(prob, exact=True)
    a = truth_amps(prob)
    d = defs(prob, amp_sn=a["sn"], sys_a=0.02, sys_b=0.02)
    tr = configs.C4_TRUTH
    grid = a["host1"] * 1.5 ** np.arange(-4.0, 5.0)
    th = np.ascontiguousarray(np.column_stack([np.full(9, tr["theta_c"]), np.full(9, tr["theta_obs"]),
                                               np.full(9, np.log10(tr["E_iso"])), grid]))
    got = f.loglike_batch(th, d)
    print("profile over amp_host1: ln L", got)
    assert np.all(np.isfinite(got)) and int(np.argmax(got)) == 4
    assert np.all(np.diff(got[:5]) > 0) and np.all(np.diff(got[4:]) < 0)
