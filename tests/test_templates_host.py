"""CPU tests of the additive templates of the likelihood (vag_loglike_tmpl_batch, the ``templates`` keyword of the Fitter's
add_flux_density / add_spectrum / add_flux, Fitter.add_template and the parameters ``amp_<name>``), and of the numpy statement of
the term that tests/test_templates.py holds the device to (fitting.template_terms):

1. the ctypes layout of vag_template_fit_spec and the new constants against the C header; the new symbols in _lib.EXPORTS and in the
   library built for gfx950; vag_abi_version() stays 13;
2. template_terms against an evaluation with math.fsum;
3. every argument error raises, and a refused call records nothing;
4. build_spec of data given in shuffled time order: the template values follow the sort, for point rows and for a band group;
5. a fit without templates has no template spec; sharded likelihood calls refuse a fitter with templates."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define S(f) offsetof(vag_template_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_template_fit_spec), S(n_templates), S(n_bands), S(point), S(bands),
           S(amp_fixed), S(extinguished));
    printf("%d %d %d %d\n", VAG_P_TMPL_AMP0, VAG_TMPL_MAX, VAG_ABI_VERSION, VAG_P_N_H);
    printf("%zu %zu\n", sizeof(((vag_template_fit_spec*)0)->amp_fixed) / sizeof(double),
           sizeof(((vag_template_fit_spec*)0)->extinguished) / sizeof(int32_t));
    return 0;
}
"""


def test_ctypes_layout_matches_header(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(LAYOUT_SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    S = _lib.TemplateFitSpec
    assert [int(x) for x in lines[0].split()] == [C.sizeof(S)] + [getattr(S, n).offset for n in (
        "n_templates", "n_bands", "point", "bands", "amp_fixed", "extinguished")]
    assert [int(x) for x in lines[1].split()] == [_lib.P_TMPL_AMP0, _lib.TMPL_MAX, 13, _lib.P_N_H]
    assert _lib.P_TMPL_AMP0 == 1017 == _lib.P_N_H + 1 and _lib.TMPL_MAX == 8
    assert [int(x) for x in lines[2].split()] == [8, 8]


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_tmpl_batch", "vag_loglike_tmpl_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13
    assert _lib.P_TMPL_AMP0 == 1017


# ---------------------------------------------------------------- 2. the term
def test_template_terms_against_fsum():
    """400 random cases with 1 to 8 templates, 1 to 12 rows, amplitudes over 6 decades, values in [0, 3] with zeros mixed in: e and x
    against math.fsum over the exact products (each a * T split into its rounded value and its rounding error, so the reference sum
    is the correctly rounded one), to 2 ulp of the reference."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(400):
        nt, n = int(rng.integers(1, 9)), int(rng.integers(1, 13))
        T = rng.uniform(0.0, 3.0, (nt, n)) * (rng.random((nt, n)) < 0.8)
        amp = 10.0 ** rng.uniform(-30.0, -24.0, nt)
        flags = rng.random(nt) < 0.4
        e, x = fitting.template_terms(T, amp, flags)
        assert e.shape == x.shape == (n,)
        for got, sel in ((e, ~flags), (x, flags)):
            for i in range(n):
                parts = []
                for c in np.flatnonzero(sel):
                    p = float(amp[c]) * float(T[c, i])
                    # (the product's rounding error is a double itself: the difference of the exact rationals)
                    parts += [p, float(Fraction(float(amp[c])) * Fraction(float(T[c, i])) - Fraction(p))]
                want = math.fsum(parts)
                if want == 0.0:
                    assert got[i] == 0.0
                    continue
                worst = max(worst, abs(got[i] - want) / math.ulp(want))
    print("template_terms vs fsum: worst", worst, "ulp")
    assert worst <= 2.0
    # one set of amplitudes per walker, and the shapes that are refused
    e, x = fitting.template_terms([[1.0, 2.0], [3.0, 0.0]], [[1.0, 0.5], [0.0, 2.0]], [0, 1])
    assert np.array_equal(e, [[1.0, 2.0], [0.0, 0.0]]) and np.array_equal(x, [[1.5, 0.0], [6.0, 0.0]])
    with pytest.raises(ValueError, match="template_terms"):
        fitting.template_terms(np.ones((2, 3)), np.ones(3), [0, 1])


# ---------------------------------------------------------------- 3. argument errors
T = np.array([3e6, 1e6, 2e6, 4e6])
F = np.array([3e-27, 1e-27, 2e-27, 4e-27])
E = 0.1 * F
P = fitting.ParamDef
THETA_V = P("theta_v", 0.0, 0.8)


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def test_template_argument_errors():
    f = _fitter()
    adders = (lambda **kw: f.add_flux_density(3e9, T, F, E, **kw), lambda **kw: f.add_spectrum(1e6, T * 1e3, F, E, **kw),
              lambda **kw: f.add_flux((1e17, 1e18), T, F * 1e10, E * 1e10, **kw))
    for add in adders:
        for name in ("", "a b", "a-b", "host!", 3, b"a"):
            with pytest.raises(ValueError, match="template name must match"):
                add(templates={name: 1.0})
        with pytest.raises(ValueError, match="must be a dict"):
            add(templates=["host"])
        for values in (np.ones(3), np.ones((4, 1)), np.ones((2, 2))):
            with pytest.raises(ValueError, match="shape of the rows"):
                add(templates={"host": values})
        for values in (-1.0, np.nan, np.inf, [1.0, -1e-300, 1.0, 1.0], [1.0, 1.0, np.nan, 1.0]):
            with pytest.raises(ValueError, match="finite and >= 0"):
                add(templates={"host": values}, noise="g")  # (the noise group is not recorded either)
        with pytest.raises(ValueError, match="at most 8 templates"):
            add(templates={f"t{k}": 1.0 for k in range(9)})
    assert not f.has_templates and not f.has_noise_groups and not f._point_t and not f._band_obs  # a refused call records nothing
    with pytest.raises(ValueError, match="template name must match"):
        f.add_template("a b")
    with pytest.raises(ValueError, match="extinguished must be a bool"):
        f.add_template("sn", extinguished=2)
    for k in range(8):
        adders[k % 3](templates={f"t{k}": 1.0 if k % 2 else np.full(4, 2.0)})
    assert f.has_templates and f._tmpl_names == [f"t{k}" for k in range(8)]  # numbered in order of first mention
    with pytest.raises(ValueError, match="at most 8 templates, 't8' would be one more"):
        f.add_flux_density(3e9, T, F, E, templates={"t3": 1.0, "t8": 1.0})
    with pytest.raises(ValueError, match="at most 8 templates"):
        f.add_template("t8")
    n_calls = len(f._point_t)
    f.add_flux_density(3e9, T, F, E, templates={"t3": 1.0})  # a known name is not a ninth
    assert len(f._tmpl_names) == 8 and len(f._point_t) == n_calls + 1

    g = _fitter()
    g.add_template("sn", extinguished=True)
    g.add_template("sn", extinguished=False)  # no row carries it yet: the flag may still change
    g.add_template("sn", extinguished=True)
    g.add_flux_density(3e9, T, F, E, templates={"sn": 1.0, "host": 2.0})
    assert g._tmpl_names == ["sn", "host"] and g._tmpl_ext == [True, False]  # a template mentioned without add_template is plain
    with pytest.raises(ValueError, match="rows already carry template 'sn'"):
        g.add_template("sn", extinguished=False)
    with pytest.raises(ValueError, match="rows already carry template 'host'"):
        g.add_template("host", extinguished=True)
    g.add_template("sn", extinguished=True)  # the same flag again is no change
    for check in (g.validate_parameters, g.build_spec):
        with pytest.raises(ValueError, match="needs the template 'x'"):
            check([THETA_V, P("amp_x", 0.0, 1.0)])
        with pytest.raises(ValueError, match="needs the template 'x'"):
            check([THETA_V, P("amp_x", 0.1, 0.1, fitting.Scale.fixed)])
        with pytest.raises(ValueError, match="fixed amp_host must be finite and >= 0"):
            check([THETA_V, P("amp_host", -0.1, -0.1, fitting.Scale.fixed)])
        with pytest.raises(ValueError, match="fixed amp_host must be finite and >= 0"):
            check([THETA_V, P("amp_host", 0.0, 1.0, fitting.Scale.fixed, initial=np.nan)])
        with pytest.raises(ValueError, match="lower >= 0"):
            check([THETA_V, P("amp_host", -1e-30, 1e-27)])
        with pytest.raises(ValueError):  # (validate_parameters names the log scale first, build_spec the amplitude)
            check([THETA_V, P("amp_sn", 0.0, 1e-27, fitting.Scale.log)])
        check([THETA_V, P("amp_host", 0.0, 1e-27)])
        check([THETA_V, P("amp_sn", 1e-30, 1e-27, fitting.Scale.log)])
        check([THETA_V, P("amp_host", 0.0, 0.0, fitting.Scale.fixed)])
    plain = _fitter()
    plain.add_flux_density(3e9, T, F, E)
    with pytest.raises(ValueError, match="amp_host"):  # no template at all
        plain.build_spec([THETA_V, P("amp_host", 0.0, 1.0)])
    assert not plain.has_templates and plain.build_spec([THETA_V])[0]._tmpl is None


def test_spec_amplitudes_and_flags():
    f = _fitter()
    f.add_template("sn", extinguished=True)
    f.add_flux_density(3e9, T, F, E, templates={"host": 1.0})
    f.add_flux((1e17, 1e18), T, F * 1e10, E * 1e10)  # a band group no template touches: a null pointer
    f.add_flux((1e15, 1e16), T, F * 1e10, E * 1e10, templates={"sn": T / 4e6})
    d = [THETA_V, P("amp_host", 0.0, 1e-26), P("amp_sn", 1e-20, 1e-14, fitting.Scale.log)]
    spec, lo, hi = f.build_spec(d)
    tp = spec._tmpl
    assert tp.n_templates == 2 and tp.n_bands == 2 and tp.extinguished[:2] == [1, 0] and tp.amp_fixed[:8] == [0.0] * 8
    assert list(spec.slot[:3])[1:] == [_lib.P_TMPL_AMP0 + 1, _lib.P_TMPL_AMP0] and list(spec.is_log[:3]) == [0, 0, 1]
    assert lo[2] == -20.0 and hi[2] == -14.0
    assert not tp.bands[0] and np.array_equal(np.ctypeslib.as_array(tp.bands[1], (2, 4)), [np.sort(T) / 4e6, np.zeros(4)])
    assert np.array_equal(np.ctypeslib.as_array(tp.point, (2, 4)), [np.zeros(4), np.ones(4)])
    assert f.template_amplitudes([0.3, 2e-27, -17.0], d) == {"sn": 1e-17, "host": 2e-27}
    fixed = [THETA_V, P("amp_sn", 3e-16, 3e-16, fitting.Scale.fixed)]
    assert f.build_spec(fixed)[0]._tmpl.amp_fixed[:2] == [3e-16, 0.0]  # amp_host is not given: 0
    assert f.template_amplitudes([0.3], fixed) == {"sn": 3e-16, "host": 0.0}
    assert f._params_at([0.3, 2e-27, -17.0], d)[0].theta_obs == 0.3  # an amplitude is no Model field


# ---------------------------------------------------------------- 4. build_spec
def test_build_spec_of_shuffled_input_times():
    rng = np.random.default_rng(5)
    t1, t2, t3 = np.linspace(1e5, 2e6, 9), np.linspace(1.5e5, 3e6, 7), np.linspace(2.5e5, 1e6, 5)
    w1, w2, w3 = rng.uniform(0.5, 2.0, 9), rng.uniform(0.5, 2.0, 7), rng.uniform(0.5, 2.0, 5)
    lim1 = np.arange(9) % 4 == 1
    fl = lambda t: 1e-27 * (t / 1e6) ** -0.7  # noqa: E731
    bump = lambda t: np.exp(-0.5 * (np.log(t / 8e5) / 0.4) ** 2)  # noqa: E731

    def build(shuffle):
        p1, p2, p3 = (rng.permutation(a.size) if shuffle else np.arange(a.size) for a in (t1, t2, t3))
        f = _fitter()
        f.add_template("sn", extinguished=True)
        f.add_flux_density(3e9, t1[p1], fl(t1)[p1], 0.1 * fl(t1)[p1], weights=w1[p1], upper_limit=lim1[p1], noise="radio",
                           templates={"host_r": 1.0, "sn": bump(t1)[p1]})
        f.add_flux_density(5e14, t2[p2], fl(t2)[p2], 0.2 * fl(t2)[p2], weights=w2[p2])
        f.add_flux_density(np.full(5, 2e17), t3[p3], fl(t3)[p3], 0.3 * fl(t3)[p3], weights=w3[p3], templates={"sn": 2.0 * bump(t3)[p3]})
        f.add_flux((1e17, 1e18), t3[p3], (fl(t3) * 1e10)[p3], (fl(t3) * 1e9)[p3], weights=w3[p3],
                   templates={"host_x": (1.0 + t3 / 1e6)[p3], "sn": bump(t3)[p3]})
        f.add_flux((1e15, 1e16), t2[p2], (fl(t2) * 1e10)[p2], (fl(t2) * 1e9)[p2])
        return f, f.build_spec([THETA_V, P("amp_host_r", 0.0, 1e-26)])[0]
    f, spec = build(True)
    g, ref = build(False)
    n = spec.n_data
    assert n == 21 and f.has_templates and f._tmpl_names == ["sn", "host_r", "host_x"]
    tp, tr = spec._tmpl, ref._tmpl
    assert tp.n_templates == 3 and tp.n_bands == 2 and not tp.bands[1]
    for name in ("t", "nu", "ln_flux", "ln_err", "weight"):  # the shuffled input gives the sorted input's rows ...
        assert np.array_equal(np.array(getattr(spec, name)[:n]), np.array(getattr(ref, name)[:n])), name
    a, b = np.ctypeslib.as_array(tp.point, (3, n)), np.ctypeslib.as_array(tr.point, (3, n))
    assert np.array_equal(a, b)  # ... and its template values: they stay with their rows
    t, nu = np.array(spec.t[:n]), np.array(spec.nu[:n])
    assert np.array_equal(a[0], np.where(nu == 3e9, bump(t), np.where(nu == 2e17, 2.0 * bump(t), 0.0)))
    assert np.array_equal(a[1], np.where(nu == 3e9, 1.0, 0.0)) and not a[2].any()
    for name in ("t", "ln_flux", "ln_err", "weight"):
        assert spec.bands[0].n == 5 and getattr(spec.bands[0], name)[:5] == getattr(ref.bands[0], name)[:5], name
    ba, bb = np.ctypeslib.as_array(tp.bands[0], (3, 5)), np.ctypeslib.as_array(tr.bands[0], (3, 5))
    assert np.array_equal(ba, bb) and np.array_equal(ba, [bump(t3), np.zeros(5), 1.0 + t3 / 1e6])


# ---------------------------------------------------------------- 5. sharding, the entry point
def test_sharded_calls_refuse_templates():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_templates = True
    with pytest.raises(NotImplementedError, match="templates="):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_flux_density(3e9, T, F, E, templates={"host": 1.0})
    with pytest.raises(NotImplementedError, match="templates="):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)


def test_widest_entry_names_the_missing_symbol():
    class Old:  # a library from before the templates
        vag_loglike_fold_batch = staticmethod(lambda *a: 0)
        vag_loglike_index_batch = staticmethod(lambda *a: 0)

    class Older:
        vag_loglike_index_batch = staticmethod(lambda *a: 0)
    f = _fitter()
    f.add_flux_density(3e9, T, F, E, templates={"host": 1.0})
    spec = f.build_spec([THETA_V])[0]
    with pytest.raises(RuntimeError, match="vag_loglike_tmpl_batch"):
        fitting._widest_entry(Old, spec, "")
    g = _fitter()
    g.add_flux_density(3e9, T, F, E)
    plain = g.build_spec([THETA_V])[0]
    assert plain._tmpl is None
    fn, trailing = fitting._widest_entry(Old, plain, "")
    assert fn is Old.vag_loglike_fold_batch and trailing == (None,)
    fn, trailing = fitting._widest_entry(Older, plain, "")
    assert fn is Older.vag_loglike_index_batch and trailing == ()
    fn, trailing = fitting._widest_entry(_lib.load(), plain, "")
    assert trailing == (None, None)
