"""CPU tests of the correlated groups of the likelihood (vag_loglike_cov_batch, Fitter.add_correlated, Fitter.correlated) and of the
numpy statement of the term that tests/test_cov.py holds the device to (fitting.covariance_whitener, fitting.whitened_chi2):

0. the ctypes layouts of vag_cov_obs / vag_cov_fit_spec and the new constants against the C header; the new symbols in _lib.EXPORTS and
   in the library built for gfx950; vag_abi_version() stays 13;
1. covariance_whitener: lower triangular, positive diagonal, W C W^T = I, and what it refuses;
2. whitened_chi2 against r^T C^-1 r from a Cholesky solve in numpy.longdouble, and under a joint permutation of rows and covariance;
3. every argument error of add_correlated raises and records nothing; shuffled rows give the sorted rows' group;
4. build_spec's ctypes layout, the entry point _widest_entry picks, sharded calls;
5. every refusal of the host scan through the C-ABI, before any context is touched.

The cases -- shared with tests/test_cov.py -- are n in {1, 2, 63, 64, 65, 130, 256} rows (the lane-stride boundaries of the back
kernel and the cap) at times 1e3 .. 1e7 s with sigma_ln drawn from 0.03 .. 0.3, and two covariance families of ln F:
  "gp":  sigma_i sigma_j (1/2 delta_ij + 1/2 exp(-(ln t_i - ln t_j)^2 / (2 0.5^2))),
  "cal": diag(sigma^2) + 0.2^2.
Both have condition numbers of at most about 1e4.

The bound B (bound() below) is derived, not measured.  The term is chi^2 = sum_i y_i^2, y_i = sum_{j <= i} W_ij r_j,
r_j = ln F_obs,j - ln f_j.  With u = 2^-53 and a_i = sum_j |W_ij| |r_j|:
  * a dot product of i + 1 <= n terms summed in any order, with or without fma, has |fl(y_i) - y_i| <= gamma_n a_i,
    gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); |y_i| <= a_i, so
    |fl(y_i)^2 - y_i^2| <= (2 gamma_n + gamma_n^2) a_i^2, the square adds u a_i^2 and the sum of n squares gamma_n sum a_i^2:
    together at most (3 n + 1) u sum a_i^2 (1 + O(n u)) <= 3 (n + 2) u sum_i a_i^2;
  * r_j itself carries the difference of `log` and `exp` between two correctly working libraries: an ulp of ln f_j, an ulp of
    ln F_obs,j, and the ulp of exp(-A_V ext_j) relative to f_j, i.e. A_V ext_j in the logarithm; with a factor 4 for libraries good to
    an ulp or two rather than half of one, e_j = 4 u (|ln F_obs,j| + |ln f_j| + A_V ext_j).  It moves y_i by at most
    sum_j |W_ij| e_j and chi^2 by 2 sum_i a_i sum_j |W_ij| e_j to first order.
  B = 3 (n + 2) u sum_i a_i^2 + 2 sum_i a_i sum_j |W_ij| e_j.
On the inputs here B is at most 1.2e-12 chi^2, and float64 numpy against longdouble uses at most 0.2 % of it."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
LD = np.longdouble
U = 2.0 ** -53
NS = (1, 2, 63, 64, 65, 130, 256)
FAMILIES = ("gp", "cal")
CASES = [(n, kind) for n in NS for kind in FAMILIES]


def covariance(kind, t, sig):
    """The covariance of ln F of a family at times t with the marginal errors sig."""
    if kind == "gp":
        d = np.log(t)[:, None] - np.log(t)[None, :]
        return sig[:, None] * sig[None, :] * (0.5 * np.eye(t.size) + 0.5 * np.exp(-d * d / (2 * 0.5 ** 2)))
    if kind == "cal":
        return np.diag(sig ** 2) + 0.2 ** 2
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case(n, kind):
    """(t ascending, sigma_ln, C_ln, W) of a case: made once and shared (nobody writes to them)."""
    rng = np.random.default_rng(1000 * n + FAMILIES.index(kind))
    t = np.sort(10 ** rng.uniform(3, 7, n))
    sig = rng.uniform(0.03, 0.3, n)
    c_ln = covariance(kind, t, sig)
    W = fitting.covariance_whitener(c_ln)
    for a in (t, sig, c_ln, W):
        a.setflags(write=False)
    return t, sig, c_ln, W


def bound(W, r, ln_obs, ln_f, av_ext=0.0):
    """B of the module docstring; r, ln_obs, ln_f, av_ext [..., n] (one row per walker), W [n, n] lower triangular."""
    aW = np.abs(np.tril(W))
    r, ln_obs, ln_f = (np.asarray(v, dtype=np.float64) for v in (r, ln_obs, ln_f))
    a = np.abs(r) @ aW.T
    e = 4 * U * (np.abs(ln_obs) + np.abs(ln_f) + np.abs(av_ext))
    return 3 * (r.shape[-1] + 2) * U * np.sum(a * a, axis=-1) + 2 * np.sum(a * (e @ aW.T), axis=-1)


def chi2_longdouble(W, r):
    """The definition in numpy.longdouble: sum_i (sum_{j <= i} W_ij r_j)^2, r [..., n] given in longdouble or float64."""
    y = np.asarray(r, dtype=LD) @ np.tril(W).astype(LD).T
    return np.sum(y * y, axis=-1)


def _solve_chi2_longdouble(c_ln, r):
    """r^T C^-1 r from a Cholesky factorisation of C and a forward substitution, both in numpy.longdouble."""
    A, n = c_ln.astype(LD), c_ln.shape[0]
    L = np.zeros_like(A)
    for k in range(n):
        L[k, k] = np.sqrt(A[k, k] - np.dot(L[k, :k], L[k, :k]))
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    z, r = np.zeros(n, LD), r.astype(LD)
    for i in range(n):
        z[i] = (r[i] - np.dot(L[i, :i], z[:i])) / L[i, i]
    return np.sum(z * z)


def residuals(n, kind, seed):
    """(ln F_obs, ln f, r) of one walker: model log fluxes in -70 .. -55, observations 3 sigma around them."""
    sig = case(n, kind)[1]
    rng = np.random.default_rng(seed)
    ln_f = rng.uniform(-70.0, -55.0, n)
    ln_obs = ln_f + 3.0 * sig * rng.standard_normal(n)
    return ln_obs, ln_f, ln_obs - ln_f


# ---------------------------------------------------------------- 0. layout, symbols
LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define O(f) offsetof(vag_cov_obs, f)
#define S(f) offsetof(vag_cov_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_cov_obs), O(n), O(t), O(nu), O(ln_flux), O(ext), O(whitener), O(weight));
    printf("%zu %zu %zu\n", sizeof(vag_cov_fit_spec), S(n_groups), S(groups));
    printf("%d %d %d\n", VAG_COV_MAX_ROWS, VAG_COV_MAX_GROUPS, VAG_ABI_VERSION);
    return 0;
}
"""


def test_ctypes_layout_matches_header(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(LAYOUT_SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    O, S = _lib.CovObs, _lib.CovFitSpec
    assert [int(x) for x in lines[0].split()] == [C.sizeof(O)] + [getattr(O, n).offset for n in (
        "n", "t", "nu", "ln_flux", "ext", "whitener", "weight")]
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S), S.n_groups.offset, S.groups.offset]
    assert [int(x) for x in lines[2].split()] == [_lib.COV_MAX_ROWS, _lib.COV_MAX_GROUPS, 13] == [256, 8, 13]


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_cov_batch", "vag_loglike_cov_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


# ---------------------------------------------------------------- 1. the whitener
@pytest.mark.parametrize("n,kind", CASES)
def test_whitener_whitens(n, kind):
    """W is lower triangular with a positive diagonal and max |W C W^T - I|, formed in longdouble, is at most 2e-14 (the cases'
    condition numbers are at most about 1e4: checked here too)."""
    _, _, c_ln, W = case(n, kind)
    assert W.shape == (n, n) and np.array_equal(W, np.tril(W)) and np.all(np.diag(W) > 0) and np.all(np.isfinite(W))
    Wl = W.astype(LD)
    resid = float(np.abs(Wl @ c_ln.astype(LD) @ Wl.T - np.eye(n)).max())
    cond = np.linalg.cond(c_ln)
    print(f"whitener n={n} {kind}: cond {cond:.2e} max |W C W^T - I| {resid:.2e}")
    assert cond <= 2e4
    assert resid <= 2e-14


def test_whitener_refusals():
    _, sig, c_ln, _ = case(63, "cal")
    for bad in (np.ones(4), np.ones((3, 4)), np.ones((2, 2, 2)), np.zeros((0, 0)), 1.0):
        with pytest.raises(ValueError, match=r"must be \[n, n\]"):
            fitting.covariance_whitener(bad)
    for v in (np.nan, np.inf):
        c = c_ln.copy()
        c[5, 7] = c[7, 5] = v
        with pytest.raises(ValueError, match="finite"):
            fitting.covariance_whitener(c)
    c = c_ln.copy()
    c[5, 7] += 1e-9 * np.sqrt(c[5, 5] * c[7, 7])
    with pytest.raises(ValueError, match="not symmetric"):
        fitting.covariance_whitener(c)
    c = c_ln.copy()
    c[5, 7] = c[7, 5] = 2.0 * np.sqrt(c[5, 5] * c[7, 7])  # a correlation coefficient of 2
    with pytest.raises(ValueError, match="not positive definite"):
        fitting.covariance_whitener(c)
    c = c_ln.copy()
    c[3, 3] = -c[3, 3]
    with pytest.raises(ValueError, match="not positive definite"):
        fitting.covariance_whitener(c)
    s = sig.copy()
    s[10] = s[11] = 1e-9  # two rows of "cal" that become identical as sigma -> 0
    with pytest.raises(ValueError, match="ill-conditioned|not positive definite"):
        fitting.covariance_whitener(np.diag(s ** 2) + 0.2 ** 2)
    with pytest.raises(ValueError, match="at most 256 rows"):
        fitting.covariance_whitener(np.eye(257))
    assert np.array_equal(fitting.covariance_whitener(np.diag([4.0, 0.25])), np.diag([0.5, 2.0]))


# ---------------------------------------------------------------- 2. the statement
@pytest.mark.parametrize("n,kind", CASES)
def test_whitened_chi2_against_a_longdouble_solve(n, kind):
    """whitened_chi2 against r^T C^-1 r from a longdouble Cholesky solve of C, within B; and, within B, against itself after a joint
    permutation of rows and covariance, factored anew.  The definition in longdouble on the same W is within B as well."""
    _, _, c_ln, W = case(n, kind)
    ln_obs, ln_f, r = residuals(n, kind, seed=7 * n + 1)
    got = float(fitting.whitened_chi2(r, W))
    B = float(bound(W, r, ln_obs, ln_f))
    want = _solve_chi2_longdouble(c_ln, r)
    p = np.random.default_rng(n).permutation(n)
    again = float(fitting.whitened_chi2(r[p], fitting.covariance_whitener(c_ln[np.ix_(p, p)])))
    print(f"whitened_chi2 n={n} {kind}: chi2 {got:.6g} B / chi2 {B / got:.2e}; against the solve {float(abs(got - want)) / B:.2e} B, "
          f"permuted {abs(again - got) / B:.2e} B, against the definition in longdouble {float(abs(got - chi2_longdouble(W, r))) / B:.2e} B")
    assert 0 < B <= 1e-9 * got
    assert abs(got - want) <= B
    assert abs(again - got) <= B
    assert abs(got - chi2_longdouble(W, r)) <= B


def test_whitened_chi2_shapes():
    W = case(65, "gp")[3]
    r = np.random.default_rng(2).standard_normal((3, 2, 65))
    out = fitting.whitened_chi2(r, W)
    assert out.shape == (3, 2) and out[1, 1] == fitting.whitened_chi2(r[1, 1], W)
    upper = W + np.triu(np.ones((65, 65)), 1)  # the entries above the diagonal are not read
    assert np.array_equal(fitting.whitened_chi2(r, upper), out)
    with pytest.raises(ValueError, match="whitened_chi2"):
        fitting.whitened_chi2(r, W[:64, :64])


# ---------------------------------------------------------------- 3. add_correlated
P = fitting.ParamDef
THETA_V = P("theta_v", 0.0, 0.8)


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def _data(n=5, kind="gp", seed=3):
    """(nu, t, f_nu, cov in flux units) of n rows in shuffled time order."""
    t, sig, c_ln, _ = case(n, kind)
    rng = np.random.default_rng(seed)
    p = rng.permutation(n)
    f = 1e-27 * (t / 1e5) ** -0.9
    nu = 10 ** rng.uniform(9, 10, n)
    cov = c_ln * np.outer(f, f)
    return nu[p], t[p], f[p], cov[np.ix_(p, p)]


def test_shuffled_rows_give_the_sorted_rows_group():
    n = 65
    nu, t, f, cov = _data(n, "gp")
    o = np.argsort(t, kind="stable")
    a, b = _fitter(), _fitter()
    a.add_correlated(nu, t, f, cov, weight=0.37)
    b.add_correlated(nu[o], t[o], f[o], cov[np.ix_(o, o)], weight=0.37)
    ga, gb = a._cov_obs[0], b._cov_obs[0]
    assert a.has_correlated and len(a._cov_obs) == 1 and ga["weight"] == 0.37
    for key in ("t", "nu", "ln_flux", "whitener"):
        assert np.array_equal(ga[key], gb[key]), key
    assert np.all(np.diff(ga["t"]) > 0) and np.array_equal(ga["ln_flux"], np.log(f[o])) and np.array_equal(ga["nu"], nu[o])
    # the whitener is that of C_ln in sorted order, factored after the permutation
    c_ln = cov[np.ix_(o, o)] / np.outer(f[o], f[o])
    assert np.array_equal(ga["whitener"], fitting.covariance_whitener(c_ln))
    # equal times keep their given order (a stable sort); a scalar nu fills the rows
    c = _fitter()
    c.add_correlated(3e9, [2e5, 1e5, 2e5, 1e5], [1.0, 2.0, 3.0, 4.0], np.diag([0.01, 0.04, 0.09, 0.16]))
    gc = c._cov_obs[0]
    assert np.array_equal(gc["t"], [1e5, 1e5, 2e5, 2e5]) and np.array_equal(gc["ln_flux"], np.log([2.0, 4.0, 1.0, 3.0]))
    assert np.array_equal(gc["nu"], np.full(4, 3e9)) and gc["weight"] == 1.0
    assert np.allclose(np.diag(gc["whitener"]), [2.0 / 0.2, 4.0 / 0.4, 1.0 / 0.1, 3.0 / 0.3], rtol=1e-15)


def test_add_correlated_argument_errors():
    f = _fitter()
    nu, t, fl, cov = _data(5)
    ok = dict(nu=nu, t=t, f_nu=fl, cov=cov)
    neg = cov.copy()
    neg[0, 1] = neg[1, 0] = 2.0 * np.sqrt(cov[0, 0] * cov[1, 1])
    asym = cov.copy()
    asym[0, 1] += 1e-9 * np.sqrt(cov[0, 0] * cov[1, 1])
    nan = cov.copy()
    nan[2, 2] = np.nan
    big = np.arange(1, 258, dtype=float)
    bad = [dict(t=[]), dict(t=t.reshape(5, 1)), dict(t=t[:4]), dict(t=np.where(np.arange(5) == 1, 0.0, t)),
           dict(t=np.where(np.arange(5) == 1, -1.0, t)), dict(t=np.where(np.arange(5) == 1, np.nan, t)),
           dict(t=np.where(np.arange(5) == 1, np.inf, t)), dict(nu=nu[:4]), dict(nu=0.0), dict(nu=-3e9), dict(nu=np.nan),
           dict(nu=np.where(np.arange(5) == 3, np.inf, nu)), dict(f_nu=fl[:4]), dict(f_nu=np.where(np.arange(5) == 2, 0.0, fl)),
           dict(f_nu=np.where(np.arange(5) == 2, -1e-27, fl)), dict(f_nu=np.where(np.arange(5) == 2, np.nan, fl)),
           dict(f_nu=np.where(np.arange(5) == 2, np.inf, fl)), dict(cov=cov[:4, :4]), dict(cov=np.diag(cov)), dict(cov=neg),
           dict(cov=asym), dict(cov=nan), dict(cov=np.zeros((5, 5))), dict(weight=-1.0), dict(weight=np.nan), dict(weight=np.inf),
           dict(weight=[1.0] * 5), dict(t=big * 1e3, nu=3e9, f_nu=big, cov=np.diag(big))]
    for change in bad:
        with pytest.raises(ValueError, match="add_correlated"):
            f.add_correlated(**{**ok, **change})
        assert not f.has_correlated and not f._cov_obs, change
    with pytest.raises(ValueError, match="add_correlated"):
        f.build_spec([THETA_V])  # the "no data" message names the new method
    for k in range(8):
        f.add_correlated(**ok, weight=float(k))
    with pytest.raises(ValueError, match="at most 8 correlated groups"):
        f.add_correlated(**ok)
    assert len(f._cov_obs) == 8 and [g["weight"] for g in f._cov_obs] == [float(k) for k in range(8)]
    assert not f._point_t and not f._band_obs and f.build_spec([THETA_V])[0]._cov.n_groups == 8


# ---------------------------------------------------------------- 4. the spec, the entry point, sharding
def test_build_spec_layout():
    f = _fitter()
    f.add_correlated(*_data(5, "gp"), weight=0.37)
    f.add_correlated(*_data(2, "cal"))
    spec, _, _ = f.build_spec([THETA_V])
    cs = spec._cov
    assert spec.n_data == 0 and spec.n_bands == 0 and cs.n_groups == 2
    for o, gd in zip(cs.groups[:2], f._cov_obs):
        n = gd["t"].size
        assert o.n == n and o.weight == gd["weight"] and not o.ext
        for name in ("t", "nu", "ln_flux"):
            assert np.array_equal(np.ctypeslib.as_array(getattr(o, name), (n,)), gd[name]), name
        assert np.array_equal(np.ctypeslib.as_array(o.whitener, (n, n)), gd["whitener"])
    del f  # the spec keeps what it points at alive
    assert cs.groups[0].weight == 0.37 and np.ctypeslib.as_array(cs.groups[0].t, (5,))[0] > 0
    # with an extinction law every group carries the kernel of its own rows, formed as for the point rows
    g = _fitter(extinction="smc")
    nu, t, fl, cov = _data(5, "gp")
    g.add_correlated(nu, t, fl, cov)
    g.add_flux_density(nu, t, fl, 0.1 * fl)
    spec, _, _ = g.build_spec([THETA_V, P("A_V", 0.0, 1.0)])
    ext = np.ctypeslib.as_array(spec._cov.groups[0].ext, (5,))
    assert np.all(ext > 0) and np.array_equal(ext, np.ctypeslib.as_array(spec.ext_kernel, (5,)))  # the same rows, the same kernel
    plain = _fitter()
    plain.add_flux_density(nu, t, fl, 0.1 * fl)
    assert not plain.has_correlated and plain.build_spec([THETA_V])[0]._cov is None


def test_widest_entry_picks_the_cov_entry():
    class Old:  # a library from before the correlated groups
        vag_loglike_tmpl_batch = staticmethod(lambda *a: 0)
        vag_loglike_fold_batch = staticmethod(lambda *a: 0)
        vag_loglike_index_batch = staticmethod(lambda *a: 0)
    nu, t, fl, cov = _data(5)
    f = _fitter()
    f.add_correlated(nu, t, fl, cov)
    spec = f.build_spec([THETA_V])[0]
    lib = _lib.load()
    for suffix in ("", "_dev"):
        fn, trailing = fitting._widest_entry(lib, spec, suffix)
        assert fn is getattr(lib, "vag_loglike_cov_batch" + suffix)
        assert fn.__name__ == "vag_loglike_cov_batch" + suffix and len(trailing) == 3 and trailing[0] is None and trailing[1] is None
        assert trailing[2] is not None
        with pytest.raises(RuntimeError, match="vag_loglike_cov_batch" + suffix):
            fitting._widest_entry(Old, spec, suffix)
    g = _fitter()
    g.add_flux_density(nu, t, fl, 0.1 * fl)
    plain = g.build_spec([THETA_V])[0]
    fn, trailing = fitting._widest_entry(Old, plain, "")  # a fit without correlated groups falls back
    assert fn is Old.vag_loglike_tmpl_batch and trailing == (None, None)
    fn, trailing = fitting._widest_entry(lib, plain, "")  # and makes the call it always made
    assert fn.__name__ == "vag_loglike_tmpl_batch" and trailing == (None, None)


def test_sharded_calls_refuse_correlated_groups():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_correlated = True
    with pytest.raises(NotImplementedError, match="add_correlated"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_correlated(*_data(5))
    with pytest.raises(NotImplementedError, match="add_correlated"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)


# ---------------------------------------------------------------- 5. the host scan
NAMES = ("vag_loglike_cov_batch", "vag_loglike_cov_batch_dev")


def _call(name, spec, cov, ctx=None, tmpl_call=False):
    """The host-pointer or _dev entry point with four walkers and no context: whatever the host scan refuses is refused before the
    context is looked at."""
    lib = _lib.load()
    th, out = np.full((4, spec.ndim), 0.3), np.empty(4)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    args = [ctx, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise), ref(spec._counts),
            ref(spec._index), ref(spec._fold), ref(spec._tmpl)]
    if not tmpl_call:
        args.append(cov)
    if name.endswith("_dev"):
        rc = getattr(lib, name)(*args, th.ctypes.data, 4, spec.ndim, out.ctypes.data)
    else:
        rc = getattr(lib, name)(*args, th.ctypes.data_as(dp), 4, spec.ndim, out.ctypes.data_as(dp))
    return rc, lib.vag_last_error().decode()


def test_the_host_scan_refuses_bad_groups_without_a_device():
    f = _fitter(extinction="smc")
    f.add_correlated(*_data(5, "gp"))
    f.add_correlated(3e9, [1e5, 2e5, 2e5, 3e5], [1e-27, 2e-27, 3e-27, 1e-27], np.diag([1e-56, 1e-56, 4e-56, 1e-56]), weight=0.5)
    spec, _, _ = f.build_spec([THETA_V])
    cs = spec._cov
    exts = cs._keep_alive[2]
    for name in NAMES:
        rc, msg = _call(name, spec, C.byref(cs))
        assert rc == _lib.VAG_E_INVALID and msg == "null context", (rc, msg)  # a valid spec (equal times included) reaches the context check

    def refused(*words):
        for name in NAMES:
            rc, msg = _call(name, spec, C.byref(cs))
            assert rc == _lib.VAG_E_INVALID and all(w in msg for w in words), (name, rc, msg, words)
    g0, g1 = (dict(gd, ext=e) for gd, e in zip(f._cov_obs, exts))
    rows = [("t", 0, 0.0, "times"), ("t", 0, -1.0, "times"), ("t", 1, np.nan, "times"), ("t", 2, np.inf, "times"), ("t", 3, 1.5e5, "times"),
            ("nu", 1, 0.0, "frequency"), ("nu", 2, -3e9, "frequency"), ("nu", 0, np.nan, "frequency"), ("nu", 3, np.inf, "frequency"),
            ("ln_flux", 2, np.nan, "ln_flux"), ("ln_flux", 0, -np.inf, "ln_flux"), ("ext", 1, np.nan, "ext"), ("ext", 3, np.inf, "ext")]
    for key, row, value, word in rows:
        keep = g1[key][row]
        g1[key][row] = value
        refused("correlated group 1", f"row {row}", word)
        g1[key][row] = keep
    W = g1["whitener"]
    for (i, j), value, word in (((2, 1), np.nan, "entry 1"), ((3, 0), np.inf, "entry 0"), ((1, 1), np.nan, "entry 1"),
                                ((2, 2), 0.0, "diagonal"), ((0, 0), -1.0, "diagonal")):
        keep = W[i, j]
        W[i, j] = value
        refused("correlated group 1", f"row {i}", "whitener", word)
        W[i, j] = keep
    keep = W[1, 3]
    W[1, 3] = np.nan  # above the diagonal: not read
    for name in NAMES:
        assert _call(name, spec, C.byref(cs)) == (_lib.VAG_E_INVALID, "null context")
    W[1, 3] = keep
    o = cs.groups[0]
    for field, value, word in (("n", 0, "n (rows)"), ("n", -3, "n (rows)"), ("n", 257, "n (rows)"), ("weight", -0.5, "weight"),
                               ("weight", np.nan, "weight"), ("weight", np.inf, "weight")):
        keep = getattr(o, field)
        setattr(o, field, value)
        refused("correlated group 0", word)
        setattr(o, field, keep)
    for name in ("t", "nu", "ln_flux", "whitener"):
        setattr(o, name, None)
        refused("correlated group 0", "null array")
        setattr(o, name, g0[name].ctypes.data_as(dp))
    o.ext = None  # (optional: a group without an extinction kernel is valid)
    for name in NAMES:
        assert _call(name, spec, C.byref(cs)) == (_lib.VAG_E_INVALID, "null context")
    o.ext = g0["ext"].ctypes.data_as(dp)
    for v in (-1, 9):
        cs.n_groups = v
        refused("n_groups")
    cs.n_groups = 2
    addr = C.cast(cs.groups, C.c_void_p).value  # (a pointer read from the struct is a view of the field: keep the address)
    cs.groups = None
    refused("null group list")
    cs.groups = C.cast(addr, C.POINTER(_lib.CovObs))
    for name in NAMES:
        assert _call(name, spec, C.byref(cs)) == (_lib.VAG_E_INVALID, "null context")  # everything restored: valid again


def test_null_or_empty_cov_spec_forwards_to_the_template_call():
    f = _fitter()
    f.add_flux_density(3e9, np.array([1e6, 2e6]), np.array([1e-27, 2e-27]), np.array([1e-28, 2e-28]), templates={"host": 1.0})
    spec, _, _ = f.build_spec([THETA_V])
    assert spec._cov is None and spec._tmpl is not None
    empty = _lib.CovFitSpec()
    for name in NAMES:
        want = _call(name.replace("cov", "tmpl"), spec, None, tmpl_call=True)
        assert want == (_lib.VAG_E_INVALID, "null context")
        for cs in (None, C.byref(empty)):
            assert _call(name, spec, cs) == want  # the same error code and message with a null context
    np.ctypeslib.as_array(spec._tmpl.point, (1, 2))[0, 1] = -1.0  # what the template call refuses, the forwarded call refuses in its words
    for name in NAMES:
        want = _call(name.replace("cov", "tmpl"), spec, None, tmpl_call=True)
        assert want[0] == _lib.VAG_E_INVALID and "template 0" in want[1]
        for cs in (None, C.byref(empty)):
            assert _call(name, spec, cs) == want
