"""CPU tests of the photon-count groups of the likelihood (vag_loglike_counts_batch, Fitter.add_counts), and the pure-numpy statement
of the term that tests/test_counts.py holds the device to:

1. the ctypes layouts of vag_counts_obs / vag_counts_fit_spec against the C header; the new symbols in _lib.EXPORTS and in the library
   built for gfx950; vag_abi_version() stays 13;
2. the term in numpy (counts_lnl) against mpmath at 40 digits;
3. the sample times add_counts builds: midpoints, contiguous bins, overlapping windows;
4. every refusal of the host scan, through the C entry point with no context (the scan runs before the device is touched), and
   every boundary error of add_counts, which leaves the Fitter unchanged;
5. a NULL or empty counts spec forwards to vag_loglike_noise_batch;
6. sharded likelihood calls refuse a fitter with counts groups."""
import ctypes as C
import os

import numpy as np
import pytest

from vegasafterglow_amd import _lib, fitting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)


# ---------------------------------------------------------------- the numpy statement of the term
def poisson_const(N):
    """S(N) = N ln N - N - ln N! (0 for N = 0).  N >= 16: Stirling's remainder series, -(ln(2 pi N) / 2 + 1/(12 N) - 1/(360 N^3) + ..)
    through N^-11 (the next term is below 2e-18 there); N < 16: the three-term difference with ln N! as the log of the exact integer
    factorial (|terms| <= 41: a few 1e-15 absolute)."""
    import math
    N = np.asarray(N, float)
    out = np.zeros(N.shape)
    big = N >= 16
    i = 1.0 / np.where(big, N, 1.0)
    i2 = i * i
    series = i * (1 / 12 + i2 * (-1 / 360 + i2 * (1 / 1260 + i2 * (-1 / 1680 + i2 * (1 / 1188 + i2 * (-691 / 360360))))))
    out = np.where(big, -(0.5 * np.log(2 * np.pi * np.where(big, N, 1.0)) + series), out)
    small = (N > 0) & ~big
    if small.any():
        vals = np.array([n * math.log(n) - n - math.log(math.factorial(int(n))) for n in N[small]])
        out[small] = vals
    return out


def poisson_deviance(N, mu):
    """D(N, mu) = mu - N - N ln(mu / N) (mu for N = 0), without cancellation: within |mu - N| <= N / 2, with x = (mu - N) / N and
    r = x / (2 + x), D = N r (x - 2 r^2 sum_k r^(2k) / (2k + 3)) (40 terms); else the direct form."""
    N, mu = np.broadcast_arrays(np.asarray(N, float), np.asarray(mu, float))
    with np.errstate(divide="ignore", invalid="ignore"):
        Ns = np.where(N > 0, N, 1.0)
        d = mu - Ns
        x = d / Ns
        r = x / (2.0 + x)
        r2 = r * r
        s = np.zeros(x.shape)
        for k in range(39, -1, -1):
            s = s * r2 + 1.0 / (2 * k + 3)
        near = Ns * (r * (x - 2.0 * r2 * s))
        far = d - Ns * np.log(mu / Ns)
        D = np.where(np.abs(d) <= 0.5 * Ns, near, far)
    return np.where(N > 0, D, mu)


def counts_mu(B, a, idx, F):
    """mu [..., n] = B + a sum_k F[..., idx[:, k]], summed in k order; F [..., n_samples], idx [n, m]."""
    F, idx = np.asarray(F, float), np.asarray(idx)
    total = np.zeros(F.shape[:-1] + (idx.shape[0],))
    for k in range(idx.shape[1]):
        total = total + F[..., idx[:, k]]
    return np.asarray(B, float) + np.asarray(a, float) * total


def counts_lnl(N, B, a, idx, w, F):
    """What one counts group adds to ln L on model fluxes F [..., n_samples]: sum_i w_i [N_i ln mu_i - mu_i - ln N_i!], formed as
    -sum w D + sum w S; a row with w = 0 adds nothing.  -inf where some row with w > 0 has mu = 0 and N > 0."""
    N, w = np.asarray(N, float), np.asarray(w, float)
    mu = counts_mu(B, a, idx, F)
    D = poisson_deviance(N, mu)
    with np.errstate(invalid="ignore"):
        terms = np.where(w > 0, w * D, 0.0)
    return -np.sum(terms, axis=-1) + np.sum(np.where(w > 0, w * poisson_const(N), 0.0))


# ---------------------------------------------------------------- 1. layout, symbols
LAYOUT_SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "vegasafterglow_amd.h"
#define O(f) offsetof(vag_counts_obs, f)
#define S(f) offsetof(vag_counts_fit_spec, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(vag_counts_obs), O(nu_min), O(nu_max), O(num_points), O(n),
           O(m), O(n_samples), O(t_sample), O(sample_idx), O(counts), O(background), O(scale), O(weight));
    printf("%zu %zu %zu %zu\n", sizeof(vag_counts_fit_spec), S(n_groups), S(pad), S(groups));
    printf("%d %d %d\n", VAG_ABI_VERSION, (int)VAG_MATH_POISSON_DEVIANCE, (int)VAG_MATH_COUNT);
    return 0;
}
"""


def test_ctypes_layouts_match_header(tmp_path):
    src, exe = tmp_path / "c.c", tmp_path / "c"
    src.write_text(LAYOUT_SRC)
    import subprocess
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    O = _lib.CountsObs
    assert [int(x) for x in lines[0].split()] == [C.sizeof(O)] + [getattr(O, n).offset for n in (
        "nu_min", "nu_max", "num_points", "n", "m", "n_samples", "t_sample", "sample_idx", "counts", "background", "scale", "weight")]
    S = _lib.CountsFitSpec
    assert [int(x) for x in lines[1].split()] == [C.sizeof(S), S.n_groups.offset, S.pad.offset, S.groups.offset]
    assert [int(x) for x in lines[2].split()] == [13, _lib.MATH_MORE["poisson_deviance"], len(_lib.MATH) + len(_lib.MATH_MORE)]
    assert _lib.MATH_MORE["poisson_deviance"] == 23 and _lib.MATH["log_ndtr"] == 22  # appended: the earlier ids keep their values
    assert not set(_lib.MATH) & set(_lib.MATH_MORE) and not set(_lib.MATH.values()) & set(_lib.MATH_MORE.values())


def test_new_symbols_exported_and_abi_version_unchanged():
    lib = _lib.load()  # the library the project's build makes for gfx950
    for s in ("vag_loglike_counts_batch", "vag_loglike_counts_batch_dev"):
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.vag_abi_version() == 13


# ---------------------------------------------------------------- 2. the term
GRID_N = [0, 1, 2, 3, 15, 16, 50, 1e4, 1e6, 1e9]
GRID_RATIO = [1e-3, 0.5, 1 - 1e-6, 1.0, 1 + 1e-6, 2.0, 1e3]


def test_the_numpy_term_against_40_digits():
    """ln P(N | mu) = N ln mu - mu - ln N! of counts_lnl against mpmath at 40 digits over N x mu / N (for N = 0 the ratios are mu
    itself): the relative error, with a floor of 1 on the denominator, must stay below 1e-14.  Also each half alone: D and S."""
    import mpmath as mp
    worst = worst_d = worst_s = 0.0
    one = np.zeros((1, 1), dtype=int)
    with mp.workdps(40):
        for N in GRID_N:
            for ratio in GRID_RATIO:
                mu = float(ratio if N == 0 else N * ratio)
                got = float(counts_lnl([N], [0.0], [1.0], one, [1.0], np.array([mu])))
                Nm, mum = mp.mpf(N), mp.mpf(mu)
                ref = Nm * mp.log(mum) - mum - mp.loggamma(Nm + 1) if N > 0 else -mum
                worst = max(worst, float(abs(mp.mpf(got) - ref) / max(mp.mpf(1), abs(ref))))
                if N > 0:
                    dref = mum - Nm - Nm * mp.log(mum / Nm)
                    d = float(poisson_deviance(N, mu))
                    worst_d = max(worst_d, float(abs(mp.mpf(d) - dref) / dref) if dref != 0 else abs(d))
            if N > 0:
                sref = Nm * mp.log(Nm) - Nm - mp.loggamma(Nm + 1)
                worst_s = max(worst_s, float(abs(mp.mpf(float(poisson_const(N))) - sref) / abs(sref)))
    print("counts_lnl vs 40 digits: ln P", worst, "D alone", worst_d, "S alone", worst_s)
    assert worst < 1e-14 and worst_d < 1e-14 and worst_s < 1e-14


def test_the_numpy_term_edges_and_shapes():
    one = np.zeros((1, 1), dtype=int)
    assert poisson_deviance(7.0, 7.0) == 0.0 and poisson_deviance(0.0, 2.5) == 2.5
    assert poisson_deviance(3.0, 0.0) == np.inf and np.isnan(poisson_deviance(3.0, np.nan))
    assert poisson_const(0.0) == 0.0 and poisson_const(1.0) == -1.0
    assert counts_lnl([4], [0.0], [1.0], one, [1.0], np.array([0.0])) == -np.inf  # mu = 0 with N > 0
    assert counts_lnl([0], [0.0], [1.0], one, [1.0], np.array([0.0])) == 0.0      # mu = 0 with N = 0
    assert counts_lnl([4], [0.0], [1.0], one, [0.0], np.array([0.0])) == 0.0      # w = 0: the row adds nothing
    assert np.isnan(counts_lnl([4], [0.0], [1.0], one, [1.0], np.array([np.nan])))
    # two walkers, three rows of two samples each, summed in k order; against the textbook form
    from math import lgamma, log
    F = np.array([[1.0, 2.0, 4.0, 8.0], [0.5, 0.25, 3.0, 1.0]])
    idx = np.array([[0, 1], [1, 2], [3, 3]])
    N, B, a, w = np.array([3.0, 0.0, 20.0]), np.array([0.5, 0.1, 0.0]), np.array([1.0, 2.0, 1.5]), np.array([1.0, 0.5, 2.0])
    mu = counts_mu(B, a, idx, F)
    assert np.array_equal(mu[0], [0.5 + 3.0, 0.1 + 12.0, 24.0]) and np.array_equal(mu[1], [0.5 + 0.75, 0.1 + 6.5, 3.0])
    want = [sum(w[i] * (N[i] * log(mu[b, i]) - mu[b, i] - lgamma(N[i] + 1)) for i in range(3)) for b in range(2)]
    np.testing.assert_allclose(counts_lnl(N, B, a, idx, w, F), want, rtol=1e-14)


# ---------------------------------------------------------------- 3. sample times
P = fitting.ParamDef
THETA_V = P("theta_v", 0.0, 0.8)
BAND = (7.25e16, 2.42e18)


def _fitter(**kw):
    return fitting.Fitter(z=0.0098, lumi_dist=1.23e26, jet="gaussian", medium="ism", **kw)


def _own_times(cd):
    return cd["t_sample"][cd["sample_idx"]]


def test_midpoint_samples():
    f = _fitter()
    assert not f.has_counts
    t0, ex = np.array([3e6, 1e6, 2e6]), np.array([4e4, 1e4, 2e4])
    f.add_counts(BAND, t0, ex, [5, 0, 12], 2e11, background=[0.5, 0.0, 1.0], weights=[1.0, 2.0, 0.0])
    assert f.has_counts and len(f._counts_obs) == 1
    cd = f._counts_obs[0]
    assert cd["m"] == 1 and np.array_equal(cd["t_sample"], [1e6 + 5e3, 2e6 + 1e4, 3e6 + 2e4])
    assert np.array_equal(cd["sample_idx"], [[2], [0], [1]]) and cd["sample_idx"].dtype == np.int32  # the rows keep their order
    assert np.array_equal(cd["counts"], [5, 0, 12]) and np.array_equal(cd["background"], [0.5, 0.0, 1.0])
    assert np.array_equal(cd["scale"], 2e11 * ex) and np.array_equal(cd["weights"], [1.0, 2.0, 0.0])
    spec, _, _ = f.build_spec([THETA_V])  # a fit with nothing but a counts group
    assert spec.n_data == 0 and spec.n_bands == 0 and spec._counts.n_groups == 1 and spec._noise is None
    o = spec._counts.groups[0]
    assert (o.n, o.m, o.n_samples, o.num_points) == (3, 1, 3, 5) and (o.nu_min, o.nu_max) == BAND
    assert o.t_sample[:3] == list(cd["t_sample"]) and o.sample_idx[:3] == [2, 0, 1] and o.scale[:3] == list(2e11 * ex)


def test_contiguous_bins_share_their_end_points():
    edges = np.array([1e5, 2e5, 4e5, 8e5, 1.6e6])  # (exact in binary arithmetic: t_start + exposure is the next t_start)
    f = _fitter()
    f.add_counts(BAND, edges[:-1], np.diff(edges), [100, 40, 9, 0], [1e11, 2e11, 3e11, 4e11], num_exposure_points=3)
    cd = f._counts_obs[0]
    want = np.array([1e5, 1.5e5, 2e5, 3e5, 4e5, 6e5, 8e5, 1.2e6, 1.6e6])
    assert np.array_equal(cd["t_sample"], want) and np.all(np.diff(cd["t_sample"]) > 0)  # 9 times, not 12: shared ends once
    assert np.array_equal(cd["sample_idx"], [[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7, 8]])
    own = edges[:-1, None] + np.arange(3)[None, :] * (np.diff(edges) / 2)[:, None]
    assert np.array_equal(_own_times(cd), own)
    assert np.array_equal(cd["scale"], np.array([1e11, 2e11, 3e11, 4e11]) * np.diff(edges) / 3)


def test_overlapping_windows_interleave():
    f = _fitter()
    t0, ex = np.array([2e5, 1e5, 1.5e5]), np.array([2e5, 4e5, 1e5])  # windows [2, 4], [1, 5], [1.5, 2.5] x 1e5, given out of order
    f.add_counts(BAND, t0, ex, [7, 30, 2], 1e11, num_exposure_points=5)
    cd = f._counts_obs[0]
    own = t0[:, None] + np.arange(5)[None, :] * (ex / 4)[:, None]
    assert np.all(np.diff(cd["t_sample"]) > 0) and np.array_equal(_own_times(cd), own)
    assert np.array_equal(cd["t_sample"], np.unique(own)) and cd["t_sample"].size < 15  # 2e5, 2.5e5, 3e5, 4e5 are shared
    assert np.all(np.diff(cd["sample_idx"], axis=1) > 0)  # every row's own samples ascend, in k order
    f.add_counts((1e17, 1e18), [5e5], [1e4], [3], 1e11, num_points=7)  # a second group is its own list
    assert len(f._counts_obs) == 2 and f._counts_obs[1]["t_sample"].tolist() == [5e5 + 5e3]


# ---------------------------------------------------------------- 4. refusals
def _call(name, spec, counts, ctx=None, noise=False):
    """The host-pointer or _dev entry point with four walkers and no context: whatever the host scan refuses is refused before
    the context is looked at."""
    lib = _lib.load()
    th, out = np.full((4, spec.ndim), 0.3), np.empty(4)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    args = [ctx, C.byref(spec), ref(spec._sky), ref(spec._vis), ref(spec._pol), ref(spec._lim), ref(spec._noise)]
    if not noise:
        args.append(counts)
    if name.endswith("_dev"):
        rc = getattr(lib, name)(*args, th.ctypes.data, 4, spec.ndim, out.ctypes.data)
    else:
        rc = getattr(lib, name)(*args, th.ctypes.data_as(dp), 4, spec.ndim, out.ctypes.data_as(dp))
    return rc, lib.vag_last_error().decode()


def _two_groups():
    f = _fitter()
    f.add_counts(BAND, [1e6, 2e6, 3e6], [1e4, 2e4, 4e4], [5, 0, 12], 2e11, background=0.5)
    f.add_counts((1e17, 1e18), [1e5, 2e5], [1e5, 2e5], [1000, 3], 1e11, num_exposure_points=3, weights=[1.0, 0.5])
    return f


def test_the_host_scan_refuses_bad_groups_without_a_device():
    f = _two_groups()
    spec, _, _ = f.build_spec([THETA_V])
    cs = spec._counts
    for name in ("vag_loglike_counts_batch", "vag_loglike_counts_batch_dev"):
        rc, msg = _call(name, spec, C.byref(cs))
        assert rc == _lib.VAG_E_INVALID and msg == "null context", (rc, msg)  # a valid spec reaches the context check

    def refused(*words):
        for name in ("vag_loglike_counts_batch", "vag_loglike_counts_batch_dev"):
            rc, msg = _call(name, spec, C.byref(cs))
            assert rc == _lib.VAG_E_INVALID and all(w in msg for w in words), (name, rc, msg, words)
    g1 = f._counts_obs[1]
    cases = [("counts", 1, 2.5, "counts"), ("counts", 0, -1.0, "counts"), ("counts", 1, np.nan, "counts"), ("counts", 0, np.inf, "counts"),
             ("counts", 1, 2.0 ** 53 + 2, "2^53"), ("background", 0, -0.1, "background"), ("background", 1, np.nan, "background"),
             ("background", 1, np.inf, "background"), ("scale", 1, 0.0, "scale"), ("scale", 0, -1.0, "scale"), ("scale", 1, np.inf, "scale"),
             ("scale", 0, np.nan, "scale"), ("weights", 1, -1.0, "weight"), ("weights", 0, np.nan, "weight"), ("weights", 1, np.inf, "weight")]
    for key, row, value, word in cases:
        keep = g1[key][row]
        g1[key][row] = value
        refused("counts group 1", f"row {row}", word)
        g1[key][row] = keep
    for row, k, value in ((0, 0, -1), (1, 2, 5), (1, 1, 2 ** 30)):
        keep = g1["sample_idx"][row, k]
        g1["sample_idx"][row, k] = value
        refused("counts group 1", f"row {row}", "sample index")
        g1["sample_idx"][row, k] = keep
    ts = f._counts_obs[0]["t_sample"]
    for j, value in ((1, ts[0]), (2, ts[1] * 0.5), (0, 0.0), (0, -1.0), (1, np.nan), (2, np.inf)):
        keep = ts[j]
        ts[j] = value
        refused("counts group 0", f"sample {j}", "strictly ascending")
        ts[j] = keep
    o = cs.groups[1]
    for field, value, word in (("m", 0, "m (samples per row)"), ("m", -3, "m (samples per row)"), ("n", 0, "no rows"),
                               ("n_samples", 0, "no sample times"), ("num_points", 1, "num_points"), ("num_points", 65, "num_points"),
                               ("nu_min", 0.0, "band"), ("nu_min", -1e17, "band"), ("nu_min", 1e18, "band"), ("nu_max", np.inf, "band"),
                               ("nu_max", np.nan, "band")):
        keep = getattr(o, field)
        setattr(o, field, value)
        refused("counts group 1", word)
        setattr(o, field, keep)
    o.counts = None
    refused("counts group 1", "null array")
    o.counts = g1["counts"].ctypes.data_as(dp)
    cs.n_groups = -1
    refused("n_groups")
    cs.n_groups = 2
    rc, msg = _call("vag_loglike_counts_batch", spec, C.byref(cs))
    assert msg == "null context"  # everything restored: valid again


def test_add_counts_boundary_errors_leave_the_fitter_unchanged():
    f = _fitter()
    t0, ex, N = np.array([1e6, 2e6]), np.array([1e4, 2e4]), np.array([3.0, 0.0])
    ok = dict(band=BAND, t_start=t0, exposure=ex, counts=N, conversion=2e11)
    bad = [dict(band=1e17), dict(band=(1e18, 1e17)), dict(band=(0.0, 1e17)), dict(band=(1e17, np.inf)), dict(num_points=1),
           dict(num_points=2.5), dict(num_exposure_points=0), dict(num_exposure_points=1.5), dict(t_start=[]), dict(t_start=[[1e6, 2e6]]),
           dict(t_start=[1e6]), dict(t_start=[0.0, 2e6]), dict(t_start=[np.nan, 2e6]), dict(exposure=[0.0, 1e4]),
           dict(exposure=[-1.0, 1e4]), dict(exposure=[np.inf, 1e4]), dict(exposure=[1e4]), dict(counts=[2.5, 0]), dict(counts=[-1, 0]),
           dict(counts=[np.nan, 0]), dict(counts=[np.inf, 0]), dict(counts=[2.0 ** 53 + 2, 0]), dict(counts=[1, 2, 3]),
           dict(conversion=0.0), dict(conversion=-1.0), dict(conversion=np.nan), dict(conversion=[1e11, np.inf]),
           dict(conversion=[1e11, 1e11, 1e11]), dict(background=-0.1), dict(background=[0.0, np.nan]), dict(background=[0.0]),
           dict(weights=[1.0]), dict(weights=[1.0, -1.0]), dict(weights=[np.nan, 1.0]), dict(conversion=1e308, exposure=[1e4, 1e300])]
    for change in bad:
        with pytest.raises(ValueError, match="add_counts"):
            f.add_counts(**{**ok, **change})
        assert not f.has_counts and not f._counts_obs, change
    for word in ("noise", "calibration", "upper_limit"):  # Poisson is its own noise model, N = 0 its own non-detection
        with pytest.raises(TypeError, match=word):
            f.add_counts(**ok, **{word: None})
    with pytest.raises(ValueError, match="add_counts"):
        f.build_spec([THETA_V])  # the "no data" message names the new method
    f.add_counts(**ok)
    assert f.has_counts and not f._point_t and not f._band_obs
    spec, _, _ = f.build_spec([THETA_V])
    assert spec._counts.n_groups == 1


# ---------------------------------------------------------------- 5. forwarding
def test_null_or_empty_counts_spec_forwards_to_the_noise_call():
    f = _fitter()
    f.add_flux_density(3e9, np.array([1e6, 2e6]), np.array([1e-27, 2e-27]), np.array([1e-28, 2e-28]), noise="radio")
    spec, _, _ = f.build_spec([THETA_V])
    empty = _lib.CountsFitSpec()
    for name in ("vag_loglike_counts_batch", "vag_loglike_counts_batch_dev"):
        want = _call(name.replace("counts", "noise"), spec, None, noise=True)
        assert want == (_lib.VAG_E_INVALID, "null context")
        for cs in (None, C.byref(empty)):
            assert _call(name, spec, cs) == want  # the same error code and message with a null context
    spec._noise.n_groups = 9  # what the noise call refuses, the forwarded call refuses in its words
    for name in ("vag_loglike_counts_batch", "vag_loglike_counts_batch_dev"):
        want = _call(name.replace("counts", "noise"), spec, None, noise=True)
        assert want[0] == _lib.VAG_E_INVALID and "n_groups must be in 0..8" in want[1]
        for cs in (None, C.byref(empty)):
            assert _call(name, spec, cs) == want
    spec._noise.n_groups = 1


# ---------------------------------------------------------------- 6. sharding
def test_sharded_calls_refuse_counts():
    from vegasafterglow_amd import dist

    def eval_dev(theta):
        raise AssertionError("not reached")
    eval_dev.has_counts = True
    with pytest.raises(NotImplementedError, match="add_counts"):
        dist.WalkerSharder(eval_dev)
    f = _fitter()
    f.add_counts(BAND, [1e6], [1e4], [3], 2e11)
    with pytest.raises(NotImplementedError, match="add_counts"):
        dist.sharded_loglike(np.zeros((4, 1)), f.loglike_batch)
