"""Chain autocorrelation's host side (no GPU): the header's pieces, the numpy statement, the refusals.

1. csrc/vag_chain_stats.h -- the text the kernels compile -- runs its means, lag sums, window rule and whole small estimates in
   tests/chain_stats_check.cpp, a stand-alone program built under AddressSanitizer + UndefinedBehaviorSanitizer as
   tests/test_tempering_host.py builds tempering_check.cpp and run as a child process; sampling.chain_mean, sampling.sokal_window and
   sampling.chain_autocorr give the same bits over its tables (a window on its threshold, no window, C(0) = 0, n = 2).  Nothing is
   loaded into this process;
2. the numpy statement against an extended-precision reference (np.longdouble direct sums, tests/_chainref.py) on AR(1) chains with
   means and widths like the C4 parameters: |rho - reference| <= 8 n 2^-53, equal windows, and no window decision of the reference on
   its threshold;
3. against an FFT estimator written here (the one of profiles/moves_timing.py): equal windows and tau to 1e-9 wherever the FFT
   estimator's window lies within the lag range, and both failing rows >= tol tau where it does not;
4. against the exact tau = (1 + phi) / (1 - phi) of AR(1), within four of Sokal's standard deviations;
5. the Python-side refusals, max_lag and first, and rho(l) not depending on max_lag."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import _lib, sampling
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale

import _chainref as ref
import test_fit_request_host as host  # FLAGS, STATIC: the sanitizer build of the other stand-alone programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
compile_cmd = host.compile_cmd  # (the module-scoped fixture: [compiler, flags...] or a skip where no sanitised hello-world links)

SHAPES = ((2048, 6, 3), (1500, 4, 5), (4096, 8, 2))  # (n, W, D)
SEEDS = (1, 2, 3)


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- 1. the header under the host sanitizers ----

@pytest.fixture(scope="module")
def header_rows(compile_cmd, tmp_path_factory):
    exe = tmp_path_factory.mktemp("chain_stats") / "chain_stats_check"
    built = host.run(compile_cmd + [os.path.join(ROOT, "tests", "chain_stats_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "Sanitizer" not in ran.stdout and "runtime error" not in ran.stdout, ran.stdout
    assert ran.returncode == 0, ran.stdout
    rows = {"mean": [], "lag": [], "window": [], "chain": []}
    for ln in ran.stdout.splitlines():
        kind, *words = ln.split()
        rows[kind].append(np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64))
    return rows


def test_header_means_are_the_numpy_means_to_the_bit(header_rows):
    rows = header_rows["mean"]
    assert len(rows) >= 8
    for r in rows:
        n = int(r[0])
        x, m = r[1:1 + n], r[1 + n]
        assert r.size == n + 2 and same_bits(sampling.chain_mean(x[:, None])[0], m), (x, m)
        exact = float(np.sum(x.astype(np.longdouble)) / n)
        if np.abs(x).max() < 1e15:  # (the rows with huge cancelling terms only show that both sides round alike)
            assert abs(m - exact) <= 2.0 ** -52 * abs(exact), (x, m, exact)
    assert any(int(r[0]) == 2 for r in rows) and any(int(r[0]) == 1 for r in rows)
    constant = [r for r in rows if int(r[0]) > 2 and np.all(r[1:-1] == r[1])]
    assert constant and all(r[-1] == r[1] for r in constant)  # a constant series has its value as mean: y = 0 exactly
    # a row that tells the two-pass mean from the one-pass mean
    assert any(np.cumsum(r[1:-1])[-1] / int(r[0]) != r[-1] for r in rows)


def test_header_lag_sums(header_rows):
    rows = header_rows["lag"]
    assert len(rows) >= 5
    for r in rows:
        n, lag, m = int(r[0]), int(r[1]), r[2]
        x, c = r[3:3 + n], r[3 + n]
        y = x.astype(np.longdouble) - np.longdouble(m)  # (about the header's own mean: the chain of fmas alone is looked at)
        terms = y[:n - lag] * y[lag:]
        assert abs(c - float(terms.sum())) <= (n + 2) * 2.0 ** -53 * float(np.abs(terms).sum()), (n, lag, c)
    assert {int(r[1]) for r in rows} >= {0, 1, 11}  # the lag n - 1 of one term among them


def test_header_window_rule_is_the_numpy_rule_to_the_bit(header_rows):
    rows = header_rows["window"]
    assert len(rows) >= 10
    seen = set()
    for r in rows:
        c, L = r[0], int(r[1])
        rho, tau, M = r[2:3 + L], r[3 + L], int(r[4 + L])
        assert r.size == L + 5
        want_tau, want_M = sampling.sokal_window(rho, c)
        assert int(want_M) == M and same_bits(want_tau, tau), (rho, c, tau, M, want_tau, want_M)
        if M >= 0 and M == c * tau:
            seen.add("threshold")
        if M < 0:
            seen.add("nan" if np.isnan(tau) else "none")
            assert np.isnan(tau) or tau == 2.0 * np.cumsum(rho)[-1] - 1.0  # tau(L), the lower bound
        if M >= 0:
            taus = 2.0 * np.cumsum(rho) - 1.0
            assert np.all(np.arange(M) < c * taus[:M]) and M >= c * taus[M]  # the smallest such M
        if L == 0:
            seen.add("L = 0")
    assert seen == {"threshold", "none", "nan", "L = 0"}, seen


def test_header_estimates_are_the_numpy_statement_to_the_bit(header_rows):
    rows = header_rows["chain"]
    assert len(rows) >= 5
    seen = set()
    for r in rows:
        n, W, D, c, L = int(r[0]), int(r[1]), int(r[2]), r[3], int(r[4])
        x = r[5:5 + n * W * D].reshape(n, W, D)
        tau, window, rho = np.split(r[5 + n * W * D:], [D, 2 * D])
        assert rho.size == (L + 1) * D
        got = sampling.chain_autocorr(x, c=c, max_lag=L)
        assert got.n_rows == n and got.max_lag == L
        assert same_bits(got.tau, tau) and np.array_equal(got.window, window.astype(np.int32)), (got, tau, window)
        assert same_bits(got.rho, rho.reshape(L + 1, D)), (got.rho, rho)
        if n == 2:
            seen.add("n = 2")
            assert got.tau.tolist() == [0.0] and got.window.tolist() == [1] and got.rho[:, 0].tolist() == [1.0, -0.5]
        if np.any(np.isnan(tau)):
            seen.add("C(0) = 0")
            assert np.isnan(tau[0]) and window[0] == -1 and np.all(x[:, :, 0] == x[0, :, 0]) and not got.reliable[0]
            assert np.isfinite(tau[1]) and window[1] >= 0  # the other parameter is untouched
        if W == 2 and D == 1 and np.all(x[:, 0, 0] == x[0, 0, 0]):
            seen.add("one walker never moved")
            alone = sampling.chain_autocorr(x[:, 1:], c=c, max_lag=L)
            assert same_bits(got.tau, alone.tau) and np.all(np.isfinite(got.tau))  # it adds zeros to the pooled sums
    assert seen == {"n = 2", "C(0) = 0", "one walker never moved"}, seen


def test_the_entry_is_exported_and_the_spec_has_the_header_layout():
    lib = _lib.load()
    assert "vag_chain_autocorr_dev" in _lib.EXPORTS and hasattr(lib, "vag_chain_autocorr_dev") and lib.vag_abi_version() == 13
    assert ctypes.sizeof(_lib.ChainSpec) == 40
    assert [(_lib.ChainSpec.__dict__[n].offset) for n, _ in _lib.ChainSpec._fields_] == [0, 4, 8, 16, 24, 32]
    header = open(os.path.join(ROOT, "include", "vegasafterglow_amd.h")).read()
    assert "int32_t nwalkers, ndim;\n    int64_t n_rows, row_stride;\n    int32_t max_lag;\n    double c;\n} vag_chain_spec;" in header
    assert "#define VAG_CHAIN_SCRATCH_MAX (1ll << 30)" in header and _lib.CHAIN_SCRATCH_MAX == 1 << 30


# ---- 2. the numpy statement against the extended-precision reference ----

@pytest.fixture(scope="module")
def ar1_cases():
    cases = []
    for n, W, D in SHAPES:
        for seed in SEEDS:
            chain = ref.ar1_chain(n, W, D, seed)
            got = sampling.chain_autocorr(chain)
            cases.append((n, W, D, seed, chain, got, ref.Reference(chain, 5.0, got.max_lag)))
    return cases


def test_numpy_statement_against_the_extended_precision_reference(ar1_cases):
    missing = 0
    for n, W, D, seed, chain, got, want in ar1_cases:
        assert got.max_lag == min(n - 1, -(-5 * n // 50)) and got.n_rows == n and got.rho.shape == (got.max_lag + 1, D)
        err = float(np.abs(got.rho - want.rho).max())
        print((n, W, D), "seed", seed, "max |rho - reference|", err, "bound", ref.rho_bound(n), "windows", got.window.tolist(),
              "tau", got.tau.round(2).tolist(), "min margin", want.margin.min())
        assert want.margin.min() > 1e-6, want.margin  # a condition on the inputs: no decision of the reference sits on its threshold
        assert err <= ref.rho_bound(n), (err, ref.rho_bound(n))
        assert np.array_equal(got.window, want.window), (got.window, want.window)
        assert np.allclose(got.tau, want.tau, rtol=0, atol=2 * (got.max_lag + 1) * ref.rho_bound(n))
        assert np.array_equal(got.reliable, (want.window >= 0) & (n >= 50.0 * want.tau))
        missing += int(np.sum(got.window < 0))
        none = got.window < 0  # no window within L: tau(L) is a lower bound above n / tol
        assert np.all(got.tau[none] > n / 50.0) and not np.any(got.reliable[none])
    assert missing >= 2  # (the slow parameter of the 1500-row chains, for two of the three seeds)


# ---- 3. against an FFT estimator ----

def fft_estimate(chain, c=5.0):
    """tau[D], window[D] over the full lag range from the FFT autocorrelation function averaged over the walkers"""
    n, _, ndim = chain.shape
    size = 1 << (2 * n - 1).bit_length()
    tau, window = np.empty(ndim), np.empty(ndim, dtype=int)
    for d in range(ndim):
        x = chain[:, :, d] - chain[:, :, d].mean(axis=0)
        f = np.fft.rfft(x, n=size, axis=0)
        acf = np.fft.irfft(f * np.conj(f), n=size, axis=0)[:n].mean(axis=1)
        taus = 2.0 * np.cumsum(acf / acf[0]) - 1.0
        ok = np.arange(n) >= c * taus
        window[d] = np.argmax(ok) if ok.any() else -1
        tau[d] = taus[window[d]]
    return tau, window


def test_against_an_fft_estimator(ar1_cases):
    beyond = 0
    for n, W, D, seed, chain, got, want in ar1_cases:
        tau, window = fft_estimate(chain)
        inside = (window >= 0) & (window <= got.max_lag)
        assert np.array_equal(got.window[inside], window[inside])
        assert np.all(np.abs(got.tau[inside] / tau[inside] - 1.0) < 1e-9), (got.tau, tau)
        assert np.all(got.window[~inside] == -1) and np.all(n < 50.0 * tau[~inside]) and not np.any(got.reliable[~inside])
        beyond += int(np.sum(~inside))
    assert beyond >= 2  # (the slow parameter of the 1500-row chains, for two of the three seeds)


# ---- 4. against the exact tau of AR(1) ----

def test_against_the_exact_tau():
    n, W, D = 4096, 8, 4
    for seed in SEEDS:
        got = sampling.chain_autocorr(ref.ar1_chain(n, W, D, seed))
        exact = np.array([ref.exact_tau(p[2]) for p in ref.PARAMETERS[:D]])
        sigma = exact * np.sqrt(2.0 * (2 * got.window + 1) / (n * W))  # Sokal's variance of the windowed estimate
        print("seed", seed, "tau", got.tau, "exact", exact, "in sigmas", (got.tau - exact) / sigma)
        assert np.all(got.window >= 0) and np.all(got.reliable)
        assert np.all(np.abs(got.tau - exact) <= 4.0 * sigma), (got.tau, exact, sigma)


# ---- 5. refusals and invariances ----

def test_max_lag_and_first():
    chain = ref.ar1_chain(600, 4, 3, 7)
    full = sampling.chain_autocorr(chain)
    assert full.max_lag == 60 and sampling.default_max_lag(600) == 60 and sampling.default_max_lag(7) == 1
    assert sampling.default_max_lag(2) == 1 and sampling.default_max_lag(30, c=5.0, tol=2.0) == 29
    # rho(l) does not depend on the lag range
    for L in (1, 15, 16, 17, 599):
        got = sampling.chain_autocorr(chain, max_lag=L)
        k = min(L, 60) + 1
        assert got.max_lag == L and got.rho.shape == (L + 1, 3) and np.array_equal(got.rho[:k], full.rho[:k])
    # a window beyond a short range is not found, and tau is then tau(L)
    short = sampling.chain_autocorr(chain, max_lag=3)
    assert np.all(short.window[full.window > 3] == -1) and not np.any(short.reliable[full.window > 3])
    assert np.array_equal(short.tau[full.window > 3], (2.0 * np.cumsum(full.rho[:4], axis=0) - 1.0)[-1][full.window > 3])
    # first: the rows from there on
    cut = sampling.chain_autocorr(chain, first=100)
    alone = sampling.chain_autocorr(chain[100:])
    assert cut.n_rows == 500 and cut.max_lag == 50 and np.array_equal(cut.rho, alone.rho) and np.array_equal(cut.tau, alone.tau)
    assert sampling.chain_autocorr(chain, first=598).n_rows == 2
    # tol moves the default range and the verdict, c the window
    assert sampling.chain_autocorr(chain, tol=10.0).max_lag == 300 and sampling.chain_autocorr(chain, c=3.0).max_lag == 36
    assert not np.any(sampling.chain_autocorr(chain, tol=1000.0, max_lag=60).reliable)
    assert isinstance(full, sampling.ChainAutocorr) and full._fields == ("tau", "window", "reliable", "rho", "n_rows", "max_lag")


def test_python_side_refusals():
    chain = ref.ar1_chain(40, 4, 2, 1)
    for bad in (dict(max_lag=0), dict(max_lag=40), dict(max_lag=2.5), dict(first=-1), dict(first=41), dict(first=39), dict(c=0.0),
                dict(c=float("nan")), dict(c=-1.0), dict(tol=0.0), dict(tol=float("inf")), dict(first=30, max_lag=10)):
        with pytest.raises(ValueError, match="chain autocorrelation"):
            sampling.chain_autocorr(chain, **bad)
    for bad in (chain[0], chain[:1], chain[:, :, 0], np.zeros((10, 0, 2)), np.zeros((10, 2, 0))):
        with pytest.raises(ValueError, match="chain autocorrelation"):
            sampling.chain_autocorr(bad)
    with pytest.raises(ValueError, match="float64 torch tensor"):
        sampling.chain_autocorr_device(chain)
    for bad in (dict(check=0), dict(check=2.5), dict(tol=0.0), dict(rtol=-0.1), dict(rtol=float("nan")), dict(c=0.0)):
        with pytest.raises(ValueError, match="Convergence"):
            sampling.Convergence(**bad)
    rule = sampling.Convergence()
    assert (rule.check, rule.tol, rule.rtol, rule.c) == (100, 50.0, 0.01, 5.0)
    tau = np.array([10.0, 20.0])
    yes = np.array([True, True])
    assert rule.met(tau, yes, tau * 1.009) and not rule.met(tau, yes, tau * 1.011) and not rule.met(tau, yes, None)
    assert not rule.met(tau, np.array([True, False]), tau) and not rule.met(np.array([10.0, np.nan]), yes, tau)
    # the drivers refuse before any device is looked for
    fitter = Fitter(z=0.1, lumi_dist=1e27)
    fitter.add_flux_density(1e9, np.array([1e4, 1e5]), np.array([1e-3, 2e-3]), np.array([1e-4, 2e-4]))
    defs = [ParamDef("theta_c", 0.02, 0.5, Scale.linear), ParamDef("E_iso", 1e50, 1e54, Scale.log)]
    for bad in (dict(converge="yes"), dict(converge=100), dict(nburn=-1), dict(nburn=2.5)):
        with pytest.raises(ValueError, match="converge|nburn"):
            sampling.run_stretch_move_device(fitter, defs, np.zeros((4, 2)), nsteps=1, **bad)
        with pytest.raises(ValueError, match="converge|nburn"):
            sampling.run_moves_device(fitter, defs, np.zeros((8, 2)), nsteps=1, **bad)
        with pytest.raises(ValueError, match="converge|nburn"):
            sampling.run_tempered_device(fitter, defs, np.zeros((2, 4, 2)), [1.0, 0.5], nsteps=1, **bad)
    with pytest.raises(ValueError, match="converge"):
        sampling.fit(fitter, defs, nwalkers=8, nsteps=1, sampler="host", converge=sampling.Convergence())
    with pytest.raises(ValueError, match="converge"):
        fitter.fit(defs, nwalkers=8, nsteps=1, sampler="device", converge=50)
