"""CPU tests of the outlier groups of the likelihood (vag_loglike_robust_batch, the ``outliers`` keyword of the Fitter's
add_flux_density / add_spectrum / add_flux and the parameters ``out_frac_<label>``, ``out_scale_<label>``, ``out_shift_<label>``),
and the problem and the numpy statement that tests/test_outliers.py holds the device to:

1. the ctypes layouts of vag_robust_fit_spec and the grown vag_loglike_request and the new constants against the C header; the new
   symbols in _lib.EXPORTS and in the library built for gfx950; vag_abi_version() stays 13;
2. tests/robust_check.cpp (robust_scan, the request's twelfth block, the slot acceptance, robust_row_lnl against long double) under
   the host sanitizers, built and run as tests/test_fit_request_host.py builds its program;
3. fitting.outlier_terms against extended precision (tests/_mathref.py) over the corners, its normalisation, p_out in [0, 1], and
   P = 0 against the noise statement of tests/test_noise_host.py;
4. every ValueError of the keyword and of the parameters; build_spec;
5. the planted flares of the problem on the CPU checker's model values: p_out > 0.9 on every planted row, < 0.1 on every clean one;
6. sharded likelihood calls refuse a fitter with outlier groups with the message of the noise groups.

The problem (problem(), make_fitter(), defs()) is that of tests/test_noise.py: the C4 light curves (3 bands x 20 epochs, the truth
with 5 % noise and 10 % errors) plus a 10-row spectrum, 70 point rows; every seventh row an upper limit; random weights.  Band 1 and
the spectrum are noise group "a", which loses its calibration and becomes robust; band 2 is group "b", a plain noise group; band 3
has no group.  Band groups: 5 epochs in group "c" (calibration 0.1, one limit row), 3 epochs in group "b" and 4 epochs in the robust
group "a".  Six detections of group "a" among the point rows are multiplied by 5 .. 10 and one row of the robust band group by 7.5,
with their errors: the planted flares."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _abi
import _mathref as mr
import configs
import test_limits_host as th_
import test_noise_host as nh
from test_fit_request_host import compile_cmd, run  # noqa: F401  (the fixture that finds a compiler which links the sanitizers)
from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = fitting.ParamDef
LOG, FIXED = fitting.Scale.log, fitting.Scale.fixed

# ---------------------------------------------------------------- the problem
FLUX_DEFS = [P("theta_c", 0.02, 0.3), P("theta_v", 0.0, 0.8), P("E_iso", 1e50, 1e54, LOG)]  # (tests/test_sky_visfit.py's)
SPEC_T = configs.C4_EPOCHS[10]
SPEC_NU = np.geomspace(1e10, 1e17, 10)
BANDS = dict(c=((2.41e17 * 0.3, 2.41e17 * 10.0), configs.C4_EPOCHS[3::4]),        # 5 epochs
             b=((5.06e14 * 0.5, 5.06e14 * 2.0), configs.C4_EPOCHS[5::6][:3]),     # 3 epochs
             a=((2.41e17 * 0.5, 2.41e17 * 2.0), configs.C4_EPOCHS[1::5]))         # 4 epochs, robust
FLARES = np.array([5.0, 6.0, 7.0, 8.0, 9.0, 10.0])
BAND_FLARE, BAND_FLARE_ROW = 7.5, 2
SYS_B, SYS_C = 0.05, 0.07
FRAC_TRUE, SCALE_TRUE = 0.15, 1.5


def point_rows():
    """(t, nu) of the 70 point rows in the order they are added: the 60 light-curve rows, then the 10 spectrum rows."""
    t, nu = configs.c4_mock_data()
    return np.concatenate([t, np.full(10, SPEC_T)]), np.concatenate([nu, SPEC_NU])


def c4_fixed(skip=()):
    tr = configs.C4_TRUTH
    vals = dict(E_iso=tr["E_iso"], Gamma0=tr["Gamma0"], theta_c=tr["theta_c"], theta_v=tr["theta_obs"], n_ism=tr["n_ism"],
                eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"])
    return [P(k, v, v, FIXED) for k, v in vals.items() if k not in skip]


def problem(truth, band_truth):
    """The data from the model's values at the truth: truth [70] at point_rows(), band_truth {"c", "b", "a"} at BANDS.  `planted`
    marks the flares among the point rows."""
    t, nu = point_rows()
    assert truth.shape == (70,) and np.all(truth > 0)
    rng = np.random.default_rng(42)
    obs, err = truth * (1 + 0.05 * rng.standard_normal(70)), 0.1 * truth
    lim = np.arange(70) % 7 == 3
    value = np.where(lim, truth + rng.uniform(-2.0, 4.0, 70) * err, obs)  # limits between 2 sigma below and 4 sigma above the truth
    w = rng.uniform(0.5, 2.0, 70)
    in_a = ((nu == configs.C4_BANDS[0]) & (np.arange(70) < 60)) | (np.arange(70) >= 60)
    det_a = np.flatnonzero(in_a & ~lim)
    assert det_a.size == 26
    rows = det_a[[1, 5, 9, 14, 19, 24]]  # light-curve and spectrum rows, early and late
    planted = np.zeros(70, dtype=bool)
    planted[rows] = True
    value[rows], err[rows] = value[rows] * FLARES, err[rows] * FLARES  # a flare is measured with the relative error of its neighbours
    bands = {}
    for key, (band, bt) in BANDS.items():
        tr = np.asarray(band_truth[key], dtype=np.float64)
        assert tr.shape == bt.shape and np.all(tr > 0)
        bands[key] = dict(t=bt, band=band, truth=tr, obs=tr * (1 + 0.05 * rng.standard_normal(bt.size)), err=0.1 * tr,
                          w=rng.uniform(0.5, 2.0, bt.size), lim=None)
    bands["c"]["lim"] = np.array([False, False, True, False, False])
    bands["c"]["obs"][2] = bands["c"]["truth"][2] * 1.2
    bands["a"]["obs"][BAND_FLARE_ROW] *= BAND_FLARE
    bands["a"]["err"][BAND_FLARE_ROW] *= BAND_FLARE
    return dict(t=t, nu=nu, truth=truth, value=value, err=err, lim=lim, w=w, bands=bands, planted=planted)


def make_fitter(prob, outliers=True, bands=True, extra=None, groups=True):
    """outliers=False: the same rows with group "a" a plain noise group; groups=False: the same rows without noise=.  extra: (nu, t,
    f_nu, err, weight) of one more detection of group "a"."""
    tr = configs.C4_TRUTH
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    ka = dict(noise="a", outliers=True) if outliers else dict(noise="a")
    kb, kc = dict(noise="b"), dict(noise="c", calibration=0.1)
    if not groups:
        ka = kb = kc = {}
    rows = [np.flatnonzero((prob["nu"] == b) & (np.arange(70) < 60)) for b in configs.C4_BANDS]

    def add(sel, **k):
        f.add_flux_density(prob["nu"][sel], prob["t"][sel], prob["value"][sel], prob["err"][sel], weights=prob["w"][sel],
                           upper_limit=prob["lim"][sel], **k)
    add(rows[0], **ka)
    add(rows[1], **kb)
    add(rows[2])
    s = np.arange(60, 70)
    f.add_spectrum(SPEC_T, prob["nu"][s], prob["value"][s], prob["err"][s], weights=prob["w"][s], upper_limit=prob["lim"][s], **ka)
    if extra is not None:
        f.add_flux_density(extra[0], [extra[1]], [extra[2]], [extra[3]], weights=[extra[4]], **({"noise": "a"} if groups else {}))
    if bands:
        for key, kw in (("c", kc), ("b", kb), ("a", {"noise": "a"} if groups else {})):
            b = prob["bands"][key]
            f.add_flux(b["band"], b["t"], b["obs"], b["err"], num_points=7, weights=b["w"], upper_limit=b["lim"], **kw)
    return f


def defs(outliers=True, bands=True, **fix):
    """The parameter list.  Free: FLUX_DEFS, sys_a, and with outliers out_frac_a (linear), out_scale_a (log), out_shift_a; a keyword
    (sys_a=0.02, out_frac_a=0.0, ...) fixes that parameter at the value, out_frac_a="log" frees it on log scale and
    out_scale_a="linear" on linear scale.  sys_b and sys_c are fixed."""
    free = [P("sys_a", 0.0, 1.0)]
    if outliers:
        free += [P("out_frac_a", 0.0, float(np.nextafter(1.0, 0.0))), P("out_scale_a", 1e-3, 1e2, LOG), P("out_shift_a", -5.0, 5.0)]
    d = list(FLUX_DEFS)
    for pd in free:
        v = fix.get(pd.name)
        if v == "log":
            d.append(P(pd.name, 1e-13, 0.5, LOG))
        elif v == "linear":
            d.append(P(pd.name, 0.0, 10.0))
        else:
            d.append(pd if v is None else P(pd.name, v, v, FIXED))
    d += [P("sys_b", SYS_B, SYS_B, FIXED)] + ([P("sys_c", SYS_C, SYS_C, FIXED)] if bands else [])
    return d + c4_fixed(skip=("theta_c", "theta_v", "E_iso"))


def truth_sample(d, **at):
    """The truth in sampler space for the free parameters of d; `at` gives the values of the parameters that are no Model fields."""
    tr = configs.C4_TRUTH
    known = dict(theta_c=tr["theta_c"], theta_v=tr["theta_obs"], E_iso=tr["E_iso"], **at)
    free = [pd for pd in d if pd.scale is not FIXED]
    return np.array([np.log10(known[pd.name]) if pd.scale is LOG else known[pd.name] for pd in free])


def group_values(f, d, samples, prefix, default=0.0):
    """{group id: the parameter ``<prefix><label>`` per walker} -- the free column (10^x on log scale), the fixed value, or default."""
    free = [pd for pd in d if pd.scale is not FIXED]
    out = {}
    for g, label in enumerate(f._noise_labels):
        col = [k for k, pd in enumerate(free) if pd.name == prefix + label]
        fixed = [pd for pd in d if pd.name == prefix + label and pd.scale is FIXED]
        if col:
            v = samples[:, col[0]]
            out[g] = 10.0 ** v if free[col[0]].scale is LOG else v
        else:
            out[g] = np.full(samples.shape[0], fixed[0].lower if fixed else default)
    return out


def formula(f, d, samples, F, bands):
    """ln L of the fitter in numpy on model values F [nb][n] and bands[g] [nb][n_g]: ungrouped detections th_.detection_lnl, limit
    rows th_.limit_lnl whatever their group, nh.noise_lnl for the detections of every plain (group, pass) and fitting.outlier_terms
    for those of every robust one."""
    f._consolidate_data()
    s_of = group_values(f, d, samples, "sys_")
    P_of, b_of, mu_of = (group_values(f, d, samples, q) for q in ("out_frac_", "out_scale_", "out_shift_"))
    cal = [f._noise_calib.get(label, 0.0) for label in f._noise_labels]
    robust = [f._noise_robust.get(label, False) for label in f._noise_labels]

    def block(lnf, lne, w, model, grp, lim):
        kind = np.zeros(w.size, dtype=bool) if lim is None else np.asarray(lim["kind"]) == 1
        grp = np.full(w.size, -1) if grp is None else np.asarray(grp)
        plain = ~kind & (grp < 0)
        total = th_.detection_lnl(lnf[plain], model[:, plain], lne[plain], w[plain])
        if kind.any():
            total = total + th_.limit_lnl(lim["limit"][kind], model[:, kind], lim["sigma"][kind], w[kind])
        for g in sorted(set(grp[grp >= 0].tolist())):
            sel = ~kind & (grp == g)
            if robust[g]:
                r = lnf[sel] - np.log(np.maximum(model[:, sel], 1e-300))
                total = total + fitting.outlier_terms(r, lne[sel], w[sel], s_of[g], P_of[g], b_of[g], mu_of[g])[0]
            else:
                total = total + nh.noise_lnl(lnf[sel], model[:, sel], lne[sel], w[sel], s_of[g], cal[g])
        return total
    total = block(f._all_log_flux, f._all_log_err, f._all_weights, F, f._all_grp, f._all_lim)
    for bd, M in zip(f._band_obs, bands):
        lim = None if bd["lim"] is None else dict(kind=bd["lim"], limit=bd["limit"], sigma=bd["sigma"])
        total = total + block(bd["ln_flux"], bd["ln_err"], bd["weights"], M, np.full(bd["t"].size, bd["noise"]), lim)
    return total


def planted_rows(f, prob):
    """The planted flag of the rows of group "a" in the order Fitter.outlier_probabilities lists them (point rows in ascending t, then
    the robust band group), and which of them are limits."""
    f._consolidate_data()
    by_key = {(t, nu): i for i, (t, nu) in enumerate(zip(prob["t"], prob["nu"]))}
    idx = np.array([by_key[(t, nu)] for t, nu in zip(f._all_t, f._all_nu)])
    sel = f._all_grp == 0
    band = np.zeros(BANDS["a"][1].size, dtype=bool)
    band[BAND_FLARE_ROW] = True
    return (np.concatenate([prob["planted"][idx][sel], band]),
            np.concatenate([prob["lim"][idx][sel], np.zeros(band.size, dtype=bool)]))


def check_flare_probabilities(f, prob, groups, with_band=True):
    """The 0.9 / 0.1 condition on the list Fitter.outlier_probabilities returned (or one assembled like it)."""
    assert [g["label"] for g in groups] == ["a"]
    g = groups[0]
    planted, lim = planted_rows(f, prob)
    if not with_band:
        planted, lim = planted[:-BANDS["a"][1].size], lim[:-BANDS["a"][1].size]
    p = g["p_out"]
    assert p.shape == planted.shape and np.all(np.isnan(p[lim])) and np.all(np.isnan(g["residual"][lim]))
    assert planted.sum() == (7 if with_band else 6) and not np.any(planted & lim)
    print("outlier probabilities: planted min", p[planted].min(), "clean max", np.nanmax(p[~planted & ~lim]))
    assert np.all((p[~lim] >= 0) & (p[~lim] <= 1))
    assert np.all(p[planted] > 0.9) and np.all(p[~planted & ~lim] < 0.1)


# ---------------------------------------------------------------- 1. layouts and symbols
LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define S(f) offsetof(vag_robust_fit_spec, f)
#define R(f) offsetof(vag_loglike_request, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(vag_robust_fit_spec), S(n_groups), S(mask), S(frac_fixed), S(scale_fixed), S(shift_fixed));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_loglike_request), R(spec), R(sky), R(vis), R(pol), R(lim),
           R(noise), R(counts), R(index), R(fold), R(tmpl), R(cov), R(robust));
    printf("%d %d %d %d %d %d %d\n", VAG_P_ROBUST_FRAC0, VAG_P_ROBUST_SCALE0, VAG_P_ROBUST_SHIFT0, VAG_P_TMPL_AMP0, VAG_TMPL_MAX,
           VAG_NOISE_MAX_GROUPS, VAG_ABI_VERSION);
    return 0;
}
"""
REQUEST_FIELDS = ("spec", "sky", "vis", "pol", "lim", "noise", "counts", "index", "fold", "tmpl", "cov", "robust")


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "r.c", tmp_path / "r"
    src.write_text(LAYOUT_SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    S, R = _lib.RobustFitSpec, _lib.LoglikeRequest
    assert [int(x) for x in lines[0].split()] == [C.sizeof(S)] + [getattr(S, n).offset for n in (
        "n_groups", "mask", "frac_fixed", "scale_fixed", "shift_fixed")]
    assert [int(x) for x in lines[1].split()] == [C.sizeof(R)] + [getattr(R, n).offset for n in REQUEST_FIELDS]
    assert [n for n, _ in R._fields_] == list(REQUEST_FIELDS) and C.sizeof(R) == 12 * C.sizeof(C.c_void_p)
    assert [int(x) for x in lines[2].split()] == [_lib.P_ROBUST_FRAC0, _lib.P_ROBUST_SCALE0, _lib.P_ROBUST_SHIFT0, _lib.P_TMPL_AMP0,
                                                  _lib.TMPL_MAX, _lib.NOISE_MAX_GROUPS, 13]
    assert (_lib.P_ROBUST_FRAC0, _lib.P_ROBUST_SCALE0, _lib.P_ROBUST_SHIFT0) == (1025, 1033, 1041)
    assert _lib.P_ROBUST_FRAC0 == _lib.P_TMPL_AMP0 + _lib.TMPL_MAX  # the first free slot behind the template amplitudes
    assert not _lib.LoglikeRequest().robust  # an unset member is null


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_robust_batch", "vag_loglike_robust_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


# ---------------------------------------------------------------- 2. the host program under the sanitizers
CASES = ["robust_scan layout", "robust_scan refusal", "fit_request_prepare robust block", "robust slots", "robust_row_lnl"]


def test_the_host_side_of_the_outlier_groups_under_asan_and_ubsan(compile_cmd, tmp_path):  # noqa: F811
    exe = tmp_path / "robust_check"
    built = run(compile_cmd + [os.path.join(ROOT, "tests", "robust_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = run([str(exe)])
    assert ran.returncode == 0, ran.stdout
    lines = ran.stdout.splitlines()
    for case in CASES:
        assert f"ok {case}" in lines, (case, ran.stdout)
    assert not any(ln.startswith("FAIL") for ln in lines), ran.stdout


# ---------------------------------------------------------------- 3. the term
def ref_terms(r, sig, s, P, b, mu, B=mr.DEFAULT):
    """(l, o) of one row in extended precision, from the definition: ln x = log2 x / log2 e, e^x = 2^(x log2 e)."""
    r, sig, s, P, b, mu = (B.arr(v) for v in (r, sig, s, P, b, mu))
    l2e = B.log2e()
    sig2, s2, b2 = sig * sig, s * s, b * b
    g = B.log1p(-P) - r * r / (2 * (sig2 + s2)) - B.log1p(s2 / sig2) / 2
    if float(P) == 0.0:
        return g, None
    o = B.log2(P) / l2e - (r - mu) * (r - mu) / (2 * (sig2 + s2 + b2)) - B.log1p((s2 + b2) / sig2) / 2
    hi, lo = (g, o) if g > o else (o, g)
    return hi + B.log1p(B.exp2((lo - hi) * l2e)), o


def test_outlier_terms_against_extended_precision():
    """The corners robust_check.cpp walks -- P = 0, tiny P, P near 1, b = 0, |r| up to 1e3 sigma -- one row at a time.  Every term of
    g and of o is <= 0, so neither sum cancels: a dozen roundings of at most an ulp of max(1, |l|) each, and numpy's log, log1p and
    exp below an ulp; the gate is 32 eps, as in the host program.  p_out = exp(o - l) carries the absolute error of o - l, eps |l|
    and eps |o| at most: it is held to 32 eps max(1, |o|) of its own value."""
    eps = np.finfo(float).eps
    sig, worst, worst_p, cases = 0.1, 0.0, 0.0, 0
    for P in (0.0, 1e-300, 1e-12, 0.15, 0.5, 1.0 - 1e-12, float(np.nextafter(1.0, 0.0))):
        for b in (0.0, 0.3, 1.5, 50.0):
            for s in (0.0, 0.05, 2.0):
                for mu in (0.0, 0.7, -3.0):
                    for k in (0.0, 1e-3, 0.5, 1.0, 3.0, 10.0, 37.0, 100.0, 1e3):
                        for sign in (1.0, -1.0):
                            r = sign * k * sig
                            lnl, p_out = fitting.outlier_terms([r], [sig], [1.0], s, P, b, mu)
                            want, o = ref_terms(r, sig, s, P, b, mu)
                            want = np.longdouble(mr.to_ld(want))
                            err = float(abs(np.longdouble(lnl) - want) / max(1.0, abs(want)))
                            worst, cases = max(worst, err), cases + 1
                            assert np.isfinite(lnl) and err <= 32 * eps, (P, b, s, mu, r, float(lnl), float(want))
                            assert 0.0 <= p_out[0] <= 1.0
                            if o is None:  # P = 0: the noise group's term of the row, and no outlier
                                noise = -0.5 * float(nh.noise_chi2(np.array([r]), [sig], [1.0], s, 0.0))
                                assert p_out[0] == 0.0 and abs(float(lnl) - noise) <= 4 * eps * max(1.0, abs(noise))
                                continue
                            o = np.longdouble(mr.to_ld(o))
                            want_p = float(np.exp(o - want))
                            if want_p > 1e-290:
                                worst_p = max(worst_p, abs(p_out[0] - want_p) / want_p / max(1.0, float(abs(o))))
    print("outlier_terms vs extended precision:", cases, "cases, worst", worst, "p_out worst (per max(1, |o|))", worst_p)
    assert worst_p <= 32 * eps
    # r = NaN stays NaN; b = 0 with mu = 0 is the noise term whatever P (both components are one Gaussian)
    assert np.isnan(fitting.outlier_terms([np.nan, 0.1], [0.1, 0.1], [1.0, 1.0], 0.0, 0.15, 1.5, 0.0)[0])
    r = np.array([0.03, -0.2, 0.5])
    base = fitting.outlier_terms(r, [0.1, 0.2, 0.1], [1.0, 0.5, 2.0], 0.05, 0.0, 0.0, 0.0)[0]
    for P in (1e-12, 0.3, 1.0 - 1e-12):
        assert fitting.outlier_terms(r, [0.1, 0.2, 0.1], [1.0, 0.5, 2.0], 0.05, P, 0.0, 0.0)[0] == pytest.approx(base, rel=1e-14)


def test_zero_fraction_is_the_noise_statement():
    """P = 0: sum w l = -(A + N) / 2 of nh.noise_chi2 with c = 0, to rounding (the same terms, summed per row instead of per sum), on
    the random cases of tests/test_noise_host.py; one set of parameters per walker broadcasts."""
    rng = np.random.default_rng(7)
    for _ in range(50):
        r, sig, w = nh._case(rng)
        for s in (0.0, 0.01, 0.1, 1.0):
            a = fitting.outlier_terms(r, sig, w, s, 0.0, 1.5, 0.3)
            b = -0.5 * float(nh.noise_chi2(r, sig, w, s, 0.0))
            assert a[0] == pytest.approx(b, rel=1e-13, abs=1e-300) and np.all(a[1] == 0.0)
    r = rng.standard_normal((5, 9))
    sig, w = rng.uniform(0.05, 0.3, 9), rng.uniform(0.5, 2.0, 9)
    s, P, b, mu = rng.uniform(0, 0.2, 5), rng.uniform(0, 0.9, 5), rng.uniform(0, 3, 5), rng.uniform(-1, 1, 5)
    lnl, p_out = fitting.outlier_terms(r, sig, w, s, P, b, mu)
    assert lnl.shape == (5,) and p_out.shape == (5, 9)
    for k in range(5):
        one = fitting.outlier_terms(r[k], sig, w, s[k], P[k], b[k], mu[k])
        assert one[0] == lnl[k] and np.array_equal(one[1], p_out[k])


def test_the_term_is_normalised():
    """exp(l) / (sqrt(2 pi) sigma) integrates to 1 over r: trapezoid sums on 400 001 points from 40 standard deviations of the wider
    component below the lower mean to 40 above the upper one.  The step is below 0.004 of the narrower component's width, where the
    trapezoid rule on a Gaussian is exact to far below rounding; what remains is the rounding of exp (eps |l|, |l| < 40 where the
    density counts) and of numpy's pairwise sum (eps log2 4e5): a few 1e-14, held to 1e-13."""
    for sig, s, P, b, mu in ((0.1, 0.0, 0.15, 1.5, 0.0), (0.1, 0.05, 0.5, 0.3, 0.7), (0.02, 0.2, 1e-6, 3.0, -2.0), (0.3, 0.0, 0.999, 0.0, 1.0)):
        wide = np.sqrt(sig ** 2 + s ** 2 + b ** 2)
        lo, hi = min(0.0, mu) - 40 * wide, max(0.0, mu) + 40 * wide
        r = np.linspace(lo, hi, 400001)
        g = np.log1p(-P) - 0.5 * r * r / (sig ** 2 + s ** 2) - 0.5 * np.log1p(s ** 2 / sig ** 2)
        ell = np.empty_like(r)
        for k0 in range(0, r.size, 50000):  # outlier_terms sums over its last axis: one row per call, in blocks
            blk = r[k0:k0 + 50000]
            ell[k0:k0 + 50000] = fitting.outlier_terms(blk[:, None], [sig], [1.0], s, P, b, mu)[0]
        assert np.all(ell >= g - 1e-12)  # the mixture is never below its inlier component
        dens = np.exp(ell) / (np.sqrt(2 * np.pi) * sig)
        total = float(np.sum(0.5 * (dens[1:] + dens[:-1]) * np.diff(r)))
        print("normalisation", (sig, s, P, b, mu), total - 1.0)
        assert abs(total - 1.0) <= 1e-13


# ---------------------------------------------------------------- 4. argument errors
T = np.array([3e6, 1e6, 2e6, 4e6])
F = np.array([3e-27, 1e-27, 2e-27, 4e-27])
E = 0.1 * F
THETA_V = P("theta_v", 0.0, 0.8)


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def test_outliers_keyword_errors():
    f = _fitter()
    adders = (lambda **kw: f.add_flux_density(3e9, T, F, E, **kw), lambda **kw: f.add_spectrum(1e6, T * 1e3, F, E, **kw),
              lambda **kw: f.add_flux((1e17, 1e18), T, F * 1e10, E * 1e10, **kw))
    for add in adders:
        with pytest.raises(ValueError, match="outliers needs noise"):
            add(outliers=True)
        for v in (1, "yes", 0.5, [True]):
            with pytest.raises(ValueError, match="outliers must be a bool"):
                add(noise="a", outliers=v)
        with pytest.raises(ValueError, match="cannot have both outliers=True and a calibration"):
            add(noise="a", outliers=True, calibration=0.05)
    assert not f.has_noise_groups and not f.has_outlier_groups and not f._point_t and not f._band_obs  # a refused call records nothing
    add = adders[0]
    add(noise="a", outliers=True)
    add(noise="a")  # not stated: agrees
    add(noise="d", outliers=True, calibration=0.0)  # no calibration is no conflict
    with pytest.raises(ValueError, match="outliers=True from an earlier call"):
        adders[1](noise="a", outliers=False)
    with pytest.raises(ValueError, match="cannot have both"):
        adders[2](noise="a", calibration=0.1)
    add(noise="b", calibration=0.1)
    with pytest.raises(ValueError, match="cannot have both"):
        adders[1](noise="b", outliers=True)
    add(noise="c", outliers=False)
    with pytest.raises(ValueError, match="outliers=False from an earlier call"):
        add(noise="c", outliers=True)
    assert len(f._point_t) == 5 and not f._band_obs
    assert f.has_outlier_groups and f._noise_labels == ["a", "d", "b", "c"] and f._noise_robust == {"a": True, "d": True, "c": False}
    add(outliers=False)  # False needs no group
    assert not _fitter().has_outlier_groups


def test_outlier_parameter_errors_and_build_spec():
    g = _fitter()
    g.add_flux_density(3e9, T, F, E, noise="radio", outliers=True)
    g.add_flux((1e17, 1e18), T, F * 1e10, E * 1e10, noise="xray")
    g.add_flux((2e17, 2e18), T, F * 1e10, E * 1e10, noise="radio")
    top = float(np.nextafter(1.0, 0.0))
    for check in (g.validate_parameters, g.build_spec):
        for name in ("out_frac_x", "out_scale_x", "out_shift_x"):
            with pytest.raises(ValueError, match="needs data added with noise='x', outliers=True"):
                check([THETA_V, P(name, 0.0, 0.5)])
        with pytest.raises(ValueError, match="needs data added with noise='xray', outliers=True"):  # a plain noise group
            check([THETA_V, P("out_frac_xray", 0.0, 0.5)])
        for v in (-0.1, 1.0, 1.5, np.nan, np.inf):
            with pytest.raises(ValueError, match=r"fixed out_frac_radio must be finite and in \[0, 1\)"):
                check([THETA_V, P("out_frac_radio", v, v, FIXED)])
        for v in (-0.1, np.nan, np.inf):
            with pytest.raises(ValueError, match="fixed out_scale_radio must be finite and >= 0"):
                check([THETA_V, P("out_scale_radio", v, v, FIXED)])
        for v in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match="fixed out_shift_radio must be finite"):
                check([THETA_V, P("out_shift_radio", v, v, FIXED)])
        for lo, hi in ((-0.1, 0.5), (0.0, 1.0), (0.0, 2.0)):
            with pytest.raises(ValueError, match="free outlier fraction"):
                check([THETA_V, P("out_frac_radio", lo, hi)])
        with pytest.raises(ValueError, match="free outlier fraction"):
            check([THETA_V, P("out_frac_radio", 1e-6, 1.0, LOG)])
        with pytest.raises(ValueError):  # (validate_parameters names the log scale first, build_spec the fraction)
            check([THETA_V, P("out_frac_radio", 0.0, 0.5, LOG)])
        with pytest.raises(ValueError, match="free outlier scatter"):
            check([THETA_V, P("out_scale_radio", -1.0, 2.0)])
        with pytest.raises(ValueError):
            check([THETA_V, P("out_scale_radio", 0.0, 2.0, LOG)])
        with pytest.raises(ValueError, match="free on linear scale only"):
            check([THETA_V, P("out_shift_radio", 0.1, 2.0, LOG)])
        check([THETA_V, P("out_frac_radio", 0.0, top), P("out_scale_radio", 0.0, 5.0), P("out_shift_radio", -3.0, 3.0)])
        check([THETA_V, P("out_frac_radio", 1e-6, 0.5, LOG), P("out_scale_radio", 1e-3, 10.0, LOG)])
        check([THETA_V, P("out_frac_radio", 0.0, 0.0, FIXED), P("out_scale_radio", 0.0, 0.0, FIXED), P("out_shift_radio", -2.0, -2.0, FIXED)])
    with pytest.raises(ValueError, match="out_frac_radio"):  # no robust group at all
        h = _fitter()
        h.add_flux_density(3e9, T, F, E, noise="radio")
        h.build_spec([THETA_V, P("out_frac_radio", 0.0, 0.5)])
    # the spec: the mask, the slots, the fixed values (0 when not given); the request carries the block
    d = [THETA_V, P("out_scale_radio", 1e-3, 10.0, LOG), P("sys_radio", 0.0, 1.0), P("out_frac_radio", 0.2, 0.2, FIXED),
         P("out_shift_radio", 0.0, 3.0), P("sys_xray", 0.1, 0.1, FIXED)]
    spec, lower, upper = g.build_spec(d)
    rb = spec._robust
    assert g.has_outlier_groups and g._noise_labels == ["radio", "xray"] and rb.n_groups == 2 and rb.mask == 1
    assert rb.frac_fixed[:8] == [0.2] + [0.0] * 7 and rb.scale_fixed[:8] == [0.0] * 8 and rb.shift_fixed[:8] == [0.0] * 8
    assert list(spec.slot[:4]) == [_lib.PARAM_SLOTS["theta_v"], _lib.P_ROBUST_SCALE0, _lib.P_NOISE_SYS0, _lib.P_ROBUST_SHIFT0]
    assert list(spec.is_log[:4]) == [0, 1, 0, 0] and spec.ndim == 4 and lower[1] == -3.0 and upper[1] == 1.0
    req = fitting.loglike_request(spec)
    assert req.robust.contents.mask == 1 and req.noise.contents.n_groups == 2 and not req.cov
    assert g._params_at([0.3, 0.0, 0.1, 1.0], d)[0].theta_obs == 0.3  # the outlier parameters are no Model fields
    plain = _fitter()
    plain.add_flux_density(3e9, T, F, E, noise="radio")
    spec0 = plain.build_spec([THETA_V])[0]
    assert spec0._robust is None and not fitting.loglike_request(spec0).robust and not plain.has_outlier_groups
    # a group flagged robust after a calibration was recorded cannot come to be, but a spec filled by hand says so too
    late = _fitter()
    late.add_flux_density(3e9, T, F, E, noise="radio", outliers=True)
    late._noise_calib["radio"] = 0.05
    with pytest.raises(ValueError, match="outliers=True and calibration=0.05"):
        late.build_spec([THETA_V])


# ---------------------------------------------------------------- 5. the planted flares on the CPU checker's model values
def test_planted_flares_stand_out_on_the_cpu_checker(oracle):
    """The problem built from the CPU checker's values at the truth; at the truth with sys_a = 0, out_frac = 0.15, out_scale = 1.5,
    out_shift = 0, on the checker's own model values: every planted row has p_out > 0.9, every clean detection p_out < 0.1.  By hand:
    a flare of x5 at sigma = 0.1 has g - o = -(ln 5)^2 / 0.02 + (ln 5)^2 / 4.52 - ln(0.15 / 0.85) + ln(226) / 2 = -124, p_out =
    1 - e^-124; a clean row at r = 0.5 sigma has o - g = ln(0.15 / 0.85) - ln(226) / 2 + 0.125 = -4.32, p_out = 0.013."""
    prm = _abi.make_params(**configs.C4_TRUTH)
    t, nu = point_rows()
    order = np.argsort(t, kind="stable")  # the checker takes ascending times
    truth = np.empty(70)
    truth[order] = oracle.flux_density(prm, t[order], nu[order])
    band_truth = {key: oracle.flux(prm, bt, band[0], band[1], 7) for key, (band, bt) in BANDS.items()}
    prob = problem(np.asarray(truth, dtype=np.float64), band_truth)
    f = make_fitter(prob)
    f._consolidate_data()
    assert f.has_outlier_groups and f._noise_labels == ["a", "b", "c"] and (f._all_grp == 0).sum() == 30
    M = oracle.flux_density(prm, f._all_t, f._all_nu)
    Mb = oracle.flux(prm, BANDS["a"][1], BANDS["a"][0][0], BANDS["a"][0][1], 7)
    sel = f._all_grp == 0
    det = f._all_lim["kind"][sel] == 0
    r = f._all_log_flux[sel] - np.log(np.maximum(M[sel], 1e-300))
    p = np.full(sel.sum(), np.nan)
    p[det] = fitting.outlier_terms(r[det], f._all_log_err[sel][det], f._all_weights[sel][det], 0.0, FRAC_TRUE, SCALE_TRUE, 0.0)[1]
    bd = f._band_obs[2]
    rb = bd["ln_flux"] - np.log(np.maximum(Mb, 1e-300))
    pb = fitting.outlier_terms(rb, bd["ln_err"], bd["weights"], 0.0, FRAC_TRUE, SCALE_TRUE, 0.0)[1]
    groups = [dict(label="a", p_out=np.concatenate([p, pb]), residual=np.concatenate([np.where(det, r, np.nan), rb]))]
    check_flare_probabilities(f, prob, groups)
    # the likelihood on the same values prefers the mixture by hundreds of ln L, and the plain group by a little without flares
    d = defs()
    th = np.array([truth_sample(d, sys_a=0.0, out_frac_a=FRAC_TRUE, out_scale_a=SCALE_TRUE, out_shift_a=0.0),
                   truth_sample(d, sys_a=0.0, out_frac_a=0.0, out_scale_a=SCALE_TRUE, out_shift_a=0.0)])
    bands = [np.tile(oracle.flux(prm, bt, band[0], band[1], 7), (2, 1)) for band, bt in (BANDS[k] for k in ("c", "b", "a"))]
    lnl = formula(f, d, th, np.tile(M, (2, 1)), bands)
    print("ln L at the truth: mixture", lnl[0], "P = 0", lnl[1])
    assert np.all(np.isfinite(lnl)) and lnl[0] > lnl[1] + 500


# ---------------------------------------------------------------- 6. sharding
def test_sharded_calls_refuse_outlier_groups():
    from vegasafterglow_amd import dist
    f = _fitter()
    f.add_flux_density(3e9, T, F, E, noise="radio", outliers=True)
    with pytest.raises(NotImplementedError, match="noise="):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
    with pytest.raises(NotImplementedError) as e:
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
    assert str(e.value) == dist._NO_NOISE
