"""Chain autocorrelation on the device (vag_chain_autocorr_dev, sampling.chain_autocorr_device) and the stopping rule of the device
run drivers (sampling.Convergence).

1. against the extended-precision reference of tests/_chainref.py (np.longdouble direct sums): |rho - reference| <= 8 n 2^-53, the
   device's tau and window are the numpy window rule on the device's own rho to the bit, the windows are the reference's, and no
   window decision of the reference sits on its threshold.  The shapes (n, W, D) are the smallest at which the kernels can go wrong:
   two and three rows, 17 rows with lag ranges around the tile of 16 lags, 102 series (a partial second wavefront), the 1500-row
   chain whose slow parameter finds no window, and 2048 x 64 x 8.
   What the bound covers and what the inputs must therefore keep: it is the rounding of an fma chain of n terms and one division.
   The mean of a series is itself a double, off by up to ulp(m) / 2 = |m| 2^-53, and that shift does not cancel in C(l) for l > 0: it
   leaves delta times the sum of the first and last l values of y, about (|m| / sigma) 2^-53 sqrt(2 l / W) / n in rho.  For the AR(1)
   chains with the C4 parameters' means and widths (|m| / sigma up to 524) that is far inside the bound from a few hundred rows on;
   the chains of 2 to 18 rows are drawn with |m| / sigma <= 2 (TINY) so that it is there too;
2. special inputs: a strided view (the cold rung of a tempered chain whose other rungs are NaN), a parameter that never moved, a series
   500 + 1e-6 noise (|m| / sigma = 5e8: by the estimate above inside the bound at 8192 rows x 256 walkers and 16 lags, where it is
   asserted; measured on the numpy statement, which has the device's means to the bit: 0.07 - 0.09 of the bound there, 9 - 15 times
   the bound at 2048 x 64 with the default 205 lags), a view whose rows lie more than 2^31 elements apart;
3. side effects and reproducibility, the refusals of the raw entry, the memory of a context;
4. end to end on a fitter with two free parameters: the run stops where the rule applied with the numpy statement to prefixes of the
   returned chain says, with the chain of a plain run of that many steps, through all three drivers; Fitter.fit's "tau"."""
import ctypes as C

import numpy as np
import pytest

import _chainref as ref
import configs
import test_sampler as ts
import test_sky_visfit as tv
from vegasafterglow_amd import _lib, fitting, sampling

pytestmark = pytest.mark.gpu

torch, c4_data, c4 = ts.torch, ts.c4_data, ts.c4  # (the module-scoped fixtures of the stretch sampler's tests)
TILE = 16  # VAG_CHAIN_TILE
TINY = ((0.3, 1.0, 0.5), (-1.0, 0.7, 0.8), (2.0, 1.5, 0.0))  # mean, width, phi with |mean| / width <= 2: see the docstring
# (n, W, D, seed, parameters, lag ranges; None = the default range)
CASES = [(2, 2, 1, 1, TINY, (1,)), (3, 2, 1, 2, TINY, (None, 2)), (17, 2, 3, 1, TINY, (TILE - 1, TILE)), (18, 2, 3, 1, TINY, (TILE + 1,)),
         (257, 34, 3, 1, ref.PARAMETERS, (None, 256)), (1500, 4, 5, 1, ref.PARAMETERS, (None,)), (2048, 64, 8, 1, ref.PARAMETERS, (None,))]
# (17 rows allow lags up to 16 = the tile = n - 1; the range of tile + 1 = 17 lags needs the 18th row and is n - 1 there)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def on_device(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def check_against_reference(got, chain, c=5.0):
    n = chain.shape[0]
    want = ref.Reference(chain, c, got.max_lag)
    err = float(np.abs(got.rho - want.rho).max())
    print(chain.shape, "L", got.max_lag, "max |rho - reference|", err, "bound", ref.rho_bound(n), "windows", got.window.tolist(),
          "reference", want.window.tolist(), "tau", got.tau.tolist(), "min margin", want.margin.min())
    assert want.margin.min() > 1e-6, want.margin  # a condition on the inputs
    assert err <= ref.rho_bound(n), (err, ref.rho_bound(n))
    tau, window = sampling.sokal_window(got.rho, c)  # the device's decisions are the numpy rule on the device's own rho
    assert same_bits(got.tau, tau) and np.array_equal(got.window, window)
    assert np.array_equal(got.window, want.window), (got.window, want.window)
    assert np.array_equal(got.reliable, (got.window >= 0) & (n >= 50.0 * got.tau))
    return want


# ---------------------------------------------------------------- 1. against the extended-precision reference
@pytest.mark.parametrize("n,W,D,seed,parameters,lags", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CASES])
def test_device_estimate_against_the_extended_precision_reference(torch, n, W, D, seed, parameters, lags):
    chain = ref.ar1_chain(n, W, D, seed, parameters)
    d_chain = on_device(torch, chain)
    for L in lags:
        got = sampling.chain_autocorr_device(d_chain, max_lag=L)
        assert got.n_rows == n and got.max_lag == (L if L is not None else sampling.default_max_lag(n)) and got.rho.shape == (got.max_lag + 1, D)
        check_against_reference(got, chain)
        host = sampling.chain_autocorr(chain, max_lag=L)  # the numpy statement: the same windows, rho within twice the bound
        assert np.array_equal(host.window, got.window) and np.abs(host.rho - got.rho).max() <= 2 * ref.rho_bound(n)
        if (n, L) == (1500, None):
            assert got.window[4] == -1 and got.tau[4] > n / 50.0 and not got.reliable[4] and np.all(got.window[:4] >= 0)
        if n == 17 and L == TILE:
            with pytest.raises(ValueError, match="max_lag"):
                sampling.chain_autocorr_device(d_chain, max_lag=TILE + 1)
    if n == 257:  # rho(l) does not depend on the lag range, to the bit
        short, full = (sampling.chain_autocorr_device(d_chain, max_lag=L).rho for L in lags)
        assert np.array_equal(bits(short), bits(full[:short.shape[0]]))


# ---------------------------------------------------------------- 2. special inputs
def test_cold_rung_view_of_a_tempered_chain(torch):
    chain = ref.ar1_chain(300, 10, 3, 4)
    tempered = np.full((300, 3, 10, 3), np.nan)
    tempered[:, 0] = chain
    d_tempered = on_device(torch, tempered)
    view = d_tempered[:, 0]
    assert not view.is_contiguous() and view.stride() == (90, 3, 1)
    got = sampling.chain_autocorr_device(view)
    want = sampling.chain_autocorr_device(on_device(torch, chain))
    assert np.all(np.isfinite(got.tau)) and np.all(np.isfinite(got.rho))
    assert same_bits(got.tau, want.tau) and same_bits(got.rho, want.rho) and np.array_equal(got.window, want.window)
    # first: the rows from there on, in place
    cut = sampling.chain_autocorr_device(view, first=100)
    alone = sampling.chain_autocorr_device(on_device(torch, chain[100:]))
    assert cut.n_rows == 200 and same_bits(cut.rho, alone.rho) and same_bits(cut.tau, alone.tau)
    # what is refused: a view whose last two dimensions are not contiguous, another dtype, a host tensor
    for bad in (d_tempered[:, :, 0], d_tempered[:, 0, :, :2], d_tempered[:, 0].transpose(1, 2), d_tempered, d_tempered[:, 0, 0]):
        with pytest.raises(ValueError, match="chain autocorrelation"):
            sampling.chain_autocorr_device(bad)
    with pytest.raises(ValueError, match="float64"):
        sampling.chain_autocorr_device(view.float())
    with pytest.raises(ValueError, match="must be on"):
        sampling.chain_autocorr_device(torch.from_numpy(chain))


def test_a_parameter_that_never_moved(torch):
    chain = ref.ar1_chain(300, 10, 3, 5)
    want = sampling.chain_autocorr_device(on_device(torch, chain))
    stuck = chain.copy()
    stuck[:, :, 1] = 52.4 + 0.1 * np.arange(10)  # every walker at a value of its own, none of them moving
    got = sampling.chain_autocorr_device(on_device(torch, stuck))
    assert np.isnan(got.tau[1]) and got.window[1] == -1 and not got.reliable[1] and np.all(np.isnan(got.rho[:, 1]))
    for d in (0, 2):  # the others are untouched, to the bit
        assert same_bits(got.tau[d], want.tau[d]) and got.window[d] == want.window[d] and same_bits(got.rho[:, d], want.rho[:, d])
    # one walker that never moved adds zeros to the pooled sums: the estimate is that of the others
    one = chain.copy()
    one[:, 9, 1] = 500.0
    got = sampling.chain_autocorr_device(on_device(torch, one))
    rest = sampling.chain_autocorr_device(on_device(torch, chain[:, :9]))
    assert same_bits(got.tau[1], rest.tau[1]) and same_bits(got.rho[:, 1], rest.rho[:, 1]) and np.isfinite(got.tau[1])
    # a value that is not finite spoils its own parameter alone
    bad = chain.copy()
    bad[17, 3, 2] = np.inf
    got = sampling.chain_autocorr_device(on_device(torch, bad))
    assert np.isnan(got.tau[2]) and got.window[2] == -1 and same_bits(got.tau[:2], want.tau[:2])


def test_small_noise_on_a_large_mean(torch):
    n, W = 8192, 256
    rng = np.random.default_rng(2)
    chain = np.stack([500.0 + 1e-6 * rng.standard_normal((n, W)), rng.standard_normal((n, W))], axis=-1)
    got = sampling.chain_autocorr_device(on_device(torch, chain), max_lag=TILE)
    check_against_reference(got, chain)
    assert np.all(np.abs(got.tau - 1.0) < 0.05)  # white noise
    # the one-pass mean is what would not do: its error alone is beyond the noise's own scale times the bound
    m1 = np.cumsum(chain[:, :, 0], axis=0)[-1] / n
    assert np.abs(m1 - sampling.chain_mean(chain[:, :, 0])).max() > 1e-6 * 1e-6


def test_rows_more_than_2_to_the_31_elements_apart(torch):
    stride = 2 ** 30 + 8  # elements between two rows: the third row starts beyond element 2^31
    need = 8 * (2 * stride + 64)
    if torch.cuda.mem_get_info(0)[0] < need + (4 << 30):
        pytest.skip("not enough free device memory for a 16 GiB view")
    chain = ref.ar1_chain(3, 8, 4, 6, TINY + ((0.5, 1.0, 0.3),))
    base = torch.empty(2 * stride + 32, dtype=torch.float64, device=torch.device("cuda", 0))
    view = base.as_strided((3, 8, 4), (stride, 4, 1))
    view.copy_(on_device(torch, chain))
    got = sampling.chain_autocorr_device(view, max_lag=2)
    want = sampling.chain_autocorr_device(on_device(torch, chain), max_lag=2)
    assert same_bits(got.tau, want.tau) and same_bits(got.rho, want.rho) and np.array_equal(got.window, want.window)
    assert np.all(np.isfinite(got.rho))
    del view, base
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 3. side effects, the raw entry, memory
def test_side_effects_and_reproducibility(torch):
    chain = ref.ar1_chain(257, 34, 3, 1)
    d_chain = on_device(torch, chain)
    first = sampling.chain_autocorr_device(d_chain)
    second = sampling.chain_autocorr_device(d_chain)
    assert same_bits(first.tau, second.tau) and same_bits(first.rho, second.rho) and np.array_equal(first.window, second.window)
    assert np.array_equal(bits(d_chain.cpu().numpy()), bits(chain))  # the chain is read only
    bare = sampling.chain_autocorr_device(d_chain, rho=False)  # d_rho = NULL
    assert bare.rho is None and same_bits(bare.tau, first.tau) and np.array_equal(bare.window, first.window)
    other = sampling.chain_autocorr_device(d_chain, c=3.0, tol=10.0)  # c moves the window, tol the range and the verdict
    host = sampling.chain_autocorr(chain, c=3.0, tol=10.0)
    assert other.max_lag == sampling.default_max_lag(257, 3.0, 10.0) == 78 and np.array_equal(other.window, host.window)
    assert np.all(other.window >= 0) and np.array_equal(other.reliable, 257 >= 10.0 * other.tau)


def test_refusals_launch_nothing_and_memory_returns(torch):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n, W, D, L = 64, 6, 2, 10
    chain = on_device(torch, ref.ar1_chain(n, W, D, 1))
    torch.cuda.synchronize()
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    in_use = lib.vag_device_bytes_in_use()

    def outputs():
        out = dict(rho=torch.full((L + 1, D), -7.0, dtype=torch.float64, device=dev), tau=torch.full((D,), -7.0, dtype=torch.float64, device=dev),
                   window=torch.full((D,), -7, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()  # (the context runs on a stream of its own)
        return out

    def call(out, ctx=ctx, spec="good", chain=chain, **null):
        sp = _lib.ChainSpec(W, D, n, W * D, L, 5.0) if spec == "good" else spec
        p = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
        rc = lib.vag_chain_autocorr_dev(ctx, C.byref(sp) if sp is not None else None, chain.data_ptr() if chain is not None else None,
                                        p["rho"], p["tau"], p["window"])
        if ctx is not None:
            _lib.check(lib.vag_ctx_synchronize(ctx))
        return rc

    def spec_with(**kw):
        sp = _lib.ChainSpec(W, D, n, W * D, L, 5.0)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def untouched(out):
        return bool((out["rho"] == -7.0).all() and (out["tau"] == -7.0).all() and (out["window"] == -7).all())

    refusals = [(dict(ctx=None), "null"), (dict(spec=None), "null"), (dict(chain=None), "null"), (dict(tau=True), "null"),
                (dict(window=True), "null"), (dict(spec=spec_with(n_rows=1)), "n_rows"), (dict(spec=spec_with(nwalkers=0)), "nwalkers"),
                (dict(spec=spec_with(ndim=0)), "ndim"), (dict(spec=spec_with(ndim=-3)), "ndim"),
                (dict(spec=spec_with(row_stride=W * D - 1)), "row_stride"), (dict(spec=spec_with(max_lag=0)), "max_lag"),
                (dict(spec=spec_with(max_lag=n)), "max_lag"), (dict(spec=spec_with(c=0.0)), "c must be"),
                (dict(spec=spec_with(c=float("nan"))), "c must be"), (dict(spec=spec_with(c=float("inf"))), "c must be")]
    for kw, text in refusals:
        out = outputs()
        assert call(out, **kw) == _lib.VAG_E_INVALID, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
        assert untouched(out) and lib.vag_device_bytes_in_use() == in_use, kw  # nothing was launched, no scratch was taken
    # lag sums above the cap: (max_lag + 1) nwalkers ndim 8 bytes > 1 GiB (no such chain is read: the refusal comes first)
    out = outputs()
    big = spec_with(nwalkers=2 ** 14, ndim=2 ** 4, row_stride=2 ** 18, n_rows=2 ** 20, max_lag=2 ** 9)
    assert call(out, spec=big) == _lib.VAG_E_CAPACITY and "exceed" in _lib.last_error() and untouched(out)
    assert lib.vag_device_bytes_in_use() == in_use
    # the context is usable afterwards, with and without rho; its scratch is counted and goes with it
    out = outputs()
    assert call(out) == _lib.VAG_OK
    want = sampling.chain_autocorr_device(chain, max_lag=L)
    assert same_bits(out["tau"].cpu().numpy(), want.tau) and same_bits(out["rho"].cpu().numpy(), want.rho)
    assert np.array_equal(out["window"].cpu().numpy(), want.window)
    assert lib.vag_device_bytes_in_use() >= in_use + 8 * ((L + 1) * W * D + W * D + (L + 1) * D)
    out = outputs()
    assert call(out, rho=True) == _lib.VAG_OK and same_bits(out["tau"].cpu().numpy(), want.tau) and bool((out["rho"] == -7.0).all())
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before


# ---------------------------------------------------------------- 4. end to end: the stopping rule
P = fitting.ParamDef
TRUTH2 = np.array([configs.C4_TRUTH["theta_c"], np.log10(configs.C4_TRUTH["E_iso"])])
CHECK = 50


def defs2():
    """two free parameters, the rest fixed at the truth: tau of a few tens of steps"""
    return [P("theta_c", 0.02, 0.3), P("E_iso", 1e50, 1e54, fitting.Scale.log)] + tv._c4_fixed(skip=("theta_c", "E_iso"))


def start2(f, shape, seed=11):
    _, lo, hi = f.build_spec(defs2())
    n = int(np.prod(shape))
    return sampling.initial_positions(lo, hi, n, np.random.default_rng(seed), center=TRUTH2, spread=0.02).reshape(*shape, 2)


def rule_on_prefixes(chain, rule, steps):
    """The stopping rule applied with the numpy statement to the prefixes chain[:step], step = check, 2 check, ... <= steps: the first
    step at which it is met (None if it never is) and the smallest margin of any decision on the way: |n - tol tau| / n per parameter
    with a window, | |tau - previous| - rtol tau | / tau from the second check on, and the window decisions' own (the reference's)."""
    previous, margin = None, np.inf
    for step in range(rule.check, steps + 1, rule.check):
        rec = sampling.chain_autocorr(chain[:step], c=rule.c, tol=rule.tol)
        margin = min(margin, ref.Reference(chain[:step], rule.c, rec.max_lag).margin.min())
        found = rec.window >= 0
        margin = min(margin, np.min(np.abs(step - rule.tol * rec.tau[found]) / step, initial=np.inf))
        if previous is not None:
            margin = min(margin, np.min(np.abs(np.abs(rec.tau - previous) - rule.rtol * rec.tau) / rec.tau))
        if rule.met(rec.tau, rec.reliable, previous):
            return step, margin, rec
        previous = rec.tau
    return None, margin, rec


def check_converged_run(out, plain, nmax, rule, cold=lambda chain: chain):
    *values, rec = out
    assert isinstance(rec, sampling.ConvergedAutocorr) and rec.converged and rec.steps % rule.check == 0 and 0 < rec.steps < nmax
    assert len(values) == len(plain) and values[0].shape[0] == rec.steps
    for got, want in zip(values, plain):  # a plain run of that many steps, to the bit
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    stop, margin, host = rule_on_prefixes(cold(values[0]), rule, rec.steps)
    print("stopped after", rec.steps, "steps; the rule on prefixes:", stop, "smallest margin", margin, "tau", rec.tau, "windows", rec.window)
    assert margin > 1e-6, margin  # a condition on the seed: no decision of the rule sits on its threshold
    assert stop == rec.steps
    assert rec.history.shape == (rec.steps // rule.check, 2) and same_bits(rec.history[-1], rec.tau) and rec.thin == 1
    assert np.all(rec.reliable) and rec.n_rows == rec.steps and rec.rho is None and np.array_equal(rec.window, host.window)
    assert np.allclose(rec.tau, host.tau, rtol=0, atol=2 * (rec.window.max() + 1) * ref.rho_bound(rec.steps))
    assert np.all(np.abs(rec.history[-1] - rec.history[-2]) <= rule.rtol * rec.tau) and np.all(rec.steps >= rule.tol * rec.tau)


def test_stretch_run_stops_where_the_rule_says(c4):
    d, nmax, rule = defs2(), 4000, sampling.Convergence(check=CHECK)
    pos0 = start2(c4, (32,))
    out = sampling.run_stretch_move_device(c4, d, pos0, nmax, seed=3, converge=rule)
    assert len(out) == 4
    plain = sampling.run_stretch_move_device(c4, d, pos0, out[3].steps, seed=3)
    check_converged_run(out, plain, nmax, rule)
    assert 0.2 < out[2].mean() < 0.9
    # too few steps allowed: exactly that many are run
    short = sampling.run_stretch_move_device(c4, d, pos0, 2 * CHECK + 20, seed=3, converge=rule, chunk=32)
    rec = short[3]
    assert not rec.converged and rec.steps == 2 * CHECK + 20 and short[0].shape[0] == rec.steps and rec.history.shape == (2, 2)
    assert np.array_equal(bits(short[0]), bits(out[0][:rec.steps])) and rec.n_rows == rec.steps  # (the record: the estimate at the end)
    assert rule_on_prefixes(short[0], rule, rec.steps)[0] is None
    # nburn and thin: the estimate runs over the stored rows from nburn // thin on
    late = sampling.run_stretch_move_device(c4, d, pos0, 3 * CHECK, seed=3, converge=rule, nburn=CHECK + 10, thin=2)
    rec = late[3]
    assert rec.steps == 3 * CHECK and late[0].shape[0] == 75 and rec.n_rows == 75 - 30 and rec.thin == 2 and np.all(np.isnan(rec.history[0]))
    host = sampling.chain_autocorr(late[0], first=30)
    assert np.array_equal(late[0], out[0][1:3 * CHECK:2]) and np.allclose(rec.tau, host.tau, rtol=1e-9) and np.array_equal(rec.window, host.window)


def test_move_mix_run_stops_where_the_rule_says(c4):
    d, nmax, rule = defs2(), 3000, sampling.Convergence(check=CHECK)
    pos0 = start2(c4, (32,))
    out = sampling.run_moves_device(c4, d, pos0, nmax, moves=sampling.REFERENCE_MOVES, seed=3, converge=rule)
    plain = sampling.run_moves_device(c4, d, pos0, out[3].steps, moves=sampling.REFERENCE_MOVES, seed=3)
    check_converged_run(out, plain, nmax, rule)


def test_tempered_run_stops_on_the_cold_rung(c4):
    d, nmax, rule = defs2(), 4000, sampling.Convergence(check=CHECK)
    pos0 = start2(c4, (2, 16))
    out = sampling.run_tempered_device(c4, d, pos0, [1.0, 0.3], nmax, seed=3, converge=rule)
    assert len(out) == 6
    plain = sampling.run_tempered_device(c4, d, pos0, [1.0, 0.3], out[5].steps, seed=3)
    check_converged_run(out, plain, nmax, rule, cold=lambda chain: chain[:, 0])


def test_fit_reports_tau(c4):
    d = defs2()
    _, lo, hi = c4.build_spec(d)
    res = c4.fit(d, nwalkers=32, nsteps=300, nburn=100, seed=1, sampler="device", center=TRUTH2, spread=0.02)
    assert "converged" not in res and "nsteps" not in res and res["chain"].shape == (300, 32, 2)
    host = sampling.chain_autocorr(res["chain"], first=100)
    lags = np.where(host.window >= 0, host.window, host.max_lag) + 1
    print("fit: tau", res["tau"], "numpy statement", host.tau, "windows", host.window)
    assert np.all(np.abs(res["tau"] - host.tau) <= 2 * lags * ref.rho_bound(200)), (res["tau"], host.tau)  # 2 (M + 1) 8 n 2^-53
    assert np.array_equal(res["tau_reliable"], host.reliable) and res["tau"].shape == (2,)
    # fewer than two rows kept: NaN
    res = c4.fit(d, nwalkers=32, nsteps=3, nburn=2, seed=1, sampler="device", center=TRUTH2, spread=0.02)
    assert np.all(np.isnan(res["tau"])) and not np.any(res["tau_reliable"]) and res["samples"].shape == (32, 2)
    # converge passes through: nsteps is a maximum, the keys say what happened
    res = c4.fit(d, nwalkers=32, nsteps=120, nburn=20, seed=1, sampler="device", center=TRUTH2, spread=0.02,
                 converge=sampling.Convergence(check=CHECK))
    assert res["converged"] is False and res["nsteps"] == 120 and res["chain"].shape == (120, 32, 2) and res["samples"].shape == (100 * 32, 2)
    res = c4.fit(d, nwalkers=16, nsteps=60, nburn=10, seed=1, sampler="tempered", ntemps=2, center=TRUTH2, spread=0.02)
    host = sampling.chain_autocorr(res["chain"], first=10)
    assert np.allclose(res["tau"], host.tau, rtol=1e-9) and np.array_equal(res["tau_reliable"], host.reliable)
