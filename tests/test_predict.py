"""Posterior-predictive quantile bands on the device (vag_column_quantiles_dev, vag_predict_bands_dev; sampling.column_quantiles_device,
Fitter.predict) against the numpy statement sampling.column_quantiles -- to the bit, any NaN equal to any NaN: order statistics are
exact and the interpolation is one subtraction inside one fma.

1. column_quantiles_device over the draw counts at which the network, the tile and the workgroup size change, column counts around the
   tile, one and sixteen unsorted levels, and columns that ascend, descend, are constant, hold heavy ties, zeros, subnormals, a spread
   from 1e-300 to 1e300, and lognormal values; 4097 draws are refused and the context serves the next call;
2. validity per draw on the device, the draws untouched, the same bits from a second run and from a second context;
3. Fitter.predict end to end against Fitter.flux_density_grid at every draw;
4. device memory returns when a context that served both entries is destroyed."""
import ctypes as C
import threading

import numpy as np
import pytest

import test_gpu_parity as tg
from vegasafterglow_amd import _lib, fitting, sampling
from vegasafterglow_amd.model import get_context

pytestmark = pytest.mark.gpu

DRAWS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4096)
WIDTH = 300
# sixteen unsorted levels with both ends, a repeated one, and levels whose rank is an integer at some of the draw counts
LEVELS16 = (0.84, 0.0, 0.5, 1.0, 0.025, 0.975, 0.16, 0.25, 0.999, 0.001, 0.5, 0.75, 1.0 / 3.0, 0.0625, 0.9, 0.31)


def k_law(lam_cm):
    """the smooth stand-in for a named extinction law of test_fitter_predictions_at_a_sample"""
    return (5.5e-5 / np.asarray(lam_cm)) ** 1.1


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def patterned(S, seed):
    """F[S, WIDTH]: column m follows pattern m % 8, so every window of eight adjacent columns holds all of them."""
    rng = np.random.default_rng(seed)
    F = np.empty((S, WIDTH))
    ramp = np.arange(S, dtype=np.float64)
    for m in range(WIDTH):
        kind = m % 8
        if kind == 0:
            F[:, m] = 1.5 * ramp + m                      # ascending
        elif kind == 1:
            F[:, m] = 0.5 * S - ramp                      # descending, through zero
        elif kind == 2:
            F[:, m] = 3.25 + m                            # constant
        elif kind == 3:
            F[:, m] = rng.choice([-1.5, 0.0, 2.0], S)     # heavy ties of three values
        elif kind == 4:
            F[:, m] = 0.0                                 # zeros
        elif kind == 5:
            F[:, m] = rng.integers(0, 50, S) * 2.0 ** -1074  # subnormals, with ties
        elif kind == 6:
            F[:, m] = 10.0 ** rng.uniform(-300.0, 300.0, S)  # 1e-300 .. 1e300 in one column
        else:
            F[:, m] = rng.lognormal(-60.0, 3.0, S)
    return F


# ---------------------------------------------------------------- 1. the quantile stage against the statement
@pytest.mark.parametrize("S", DRAWS)
def test_column_quantiles_are_the_numpy_statement_to_the_bit(torch, S):
    F = patterned(S, 100 + S)
    want, ok, n = sampling.column_quantiles(F, LEVELS16)  # (once per S: a column's quantiles do not depend on its neighbours)
    assert n == S and ok.all()
    d_F = torch.from_numpy(F).cuda()
    T = _lib.predict_tile_columns(S)
    assert T in (4, 8, 16)
    got, d_ok, d_n = sampling.column_quantiles_device(d_F, LEVELS16)
    assert d_n == S and d_ok.all() and got.shape == (16, WIDTH)
    assert same_bits(got, want), np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5]
    assert same_bits(sampling.column_quantiles_device(d_F, [LEVELS16[0]])[0], want[:1])
    for M in (1, T - 1, T, T + 1):
        for off in range(8) if M == 1 else (0, 3):
            window = d_F[:, off:off + M].contiguous()
            got, d_ok, d_n = sampling.column_quantiles_device(window, LEVELS16)
            assert d_n == S and d_ok.all() and same_bits(got, want[:, off:off + M]), (S, M, off)
            k = (M + off) % 16
            assert same_bits(sampling.column_quantiles_device(window, LEVELS16[k])[0], want[k:k + 1, off:off + M]), (S, M, off, k)
    assert np.array_equal(d_F.cpu().numpy().view(np.uint64), F.view(np.uint64))  # the draws are only read


def test_4097_draws_are_refused_and_the_context_serves_the_next_call(torch):
    lib = _lib.load()
    h, lock = get_context(0)
    dev = torch.device("cuda", 0)
    F = patterned(65, 7)[:, :20].copy()
    d_F = torch.from_numpy(F).to(dev)
    big = torch.zeros((4097, 2), dtype=torch.float64, device=dev)
    out = torch.full((1, 20), -7.0, dtype=torch.float64, device=dev)
    n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    spec = _lib.QuantileSpec(1, 0, (C.c_double * 16)(0.5))
    torch.cuda.synchronize()
    with lock:
        rc = lib.vag_column_quantiles_dev(h, C.byref(spec), big.data_ptr(), 4097, 2, None, out.data_ptr(), None, n.data_ptr())
        assert rc == _lib.VAG_E_CAPACITY and "VAG_PREDICT_MAX_DRAWS" in _lib.last_error()
        rc = lib.vag_column_quantiles_dev(h, C.byref(spec), big.data_ptr(), 4096, (1 << 15) + 1, None, out.data_ptr(), None, n.data_ptr())
        assert rc == _lib.VAG_E_CAPACITY and "VAG_PREDICT_MAX_VALUES" in _lib.last_error()  # (refused on its shape: nothing is read)
        for bad, text in ((_lib.QuantileSpec(0, 0), "nq"), (_lib.QuantileSpec(17, 0), "nq"),
                          (_lib.QuantileSpec(1, 0, (C.c_double * 16)(1.5)), "[0, 1]"),
                          (_lib.QuantileSpec(2, 0, (C.c_double * 16)(0.5, float("nan"))), "[0, 1]")):
            rc = lib.vag_column_quantiles_dev(h, C.byref(bad), d_F.data_ptr(), 65, 20, None, out.data_ptr(), None, n.data_ptr())
            assert rc == _lib.VAG_E_INVALID and text in _lib.last_error()
        for S, M in ((0, 20), (65, 0), (-1, 20)):
            rc = lib.vag_column_quantiles_dev(h, C.byref(spec), d_F.data_ptr(), S, M, None, out.data_ptr(), None, n.data_ptr())
            assert rc == _lib.VAG_E_INVALID
        _lib.check(lib.vag_ctx_synchronize(h))
    assert np.all(out.cpu().numpy() == -7.0) and int(n.cpu()[0]) == -7  # a refusal launches nothing
    with pytest.raises(ValueError, match="4097 draws exceed the maximum of 4096"):
        sampling.column_quantiles_device(big, [0.5])
    with pytest.raises(ValueError, match="contiguous"):
        sampling.column_quantiles_device(d_F[:, ::2], [0.5])
    with pytest.raises(ValueError, match="valid must be 65 flags"):
        sampling.column_quantiles_device(d_F, [0.5], valid=np.ones(64, dtype=bool))
    got, ok, cnt = sampling.column_quantiles_device(d_F, [0.5])
    assert cnt == 65 and same_bits(got, sampling.column_quantiles(F, [0.5])[0])


# ---------------------------------------------------------------- 2. validity on the device
def test_validity_is_per_draw_and_the_bits_do_not_depend_on_the_run_or_the_context(torch):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    S, M = 65, 40
    F = np.random.default_rng(5).lognormal(-60.0, 3.0, (S, M))
    F[7, 3] = np.nan
    F[20, 0] = np.inf
    F[33, 39] = -np.inf
    flags = np.ones(S, dtype=bool)
    flags[41] = False
    levels = (0.16, 0.5, 0.84, 0.0, 1.0)
    want, want_ok, want_n = sampling.column_quantiles(F, levels, valid=flags)
    assert want_n == 61 and not want_ok[[7, 20, 33, 41]].any() and want_ok.sum() == 61
    d_F = torch.from_numpy(F).to(dev)
    got, ok, n = sampling.column_quantiles_device(d_F, levels, valid=flags)
    assert n == want_n and np.array_equal(ok, want_ok) and same_bits(got, want)
    assert same_bits(d_F.cpu().numpy(), F) and np.array_equal(np.isnan(d_F.cpu().numpy()), np.isnan(F))  # d_F as it was
    again = sampling.column_quantiles_device(d_F, levels, valid=torch.from_numpy(flags).to(dev))
    assert same_bits(again[0], got) and np.array_equal(again[1], ok) and again[2] == n
    # without the flags the draw comes back; the values that are not finite still drop theirs
    got3, ok3, n3 = sampling.column_quantiles_device(d_F, levels)
    want3 = sampling.column_quantiles(F, levels)
    assert n3 == 62 and ok3[41] and same_bits(got3, want3[0]) and np.array_equal(ok3, want3[1])
    # a second context
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))
    try:
        other = sampling.column_quantiles_device(d_F, levels, valid=flags, context=(ctx, threading.RLock()))
        assert same_bits(other[0], got) and np.array_equal(other[1], ok) and other[2] == n
    finally:
        lib.vag_ctx_destroy(ctx)
    # every draw invalid
    none, ok0, n0 = sampling.column_quantiles_device(d_F, levels, valid=np.zeros(S, dtype=np.int32))
    assert n0 == 0 and not ok0.any() and none.shape == (5, M) and np.isnan(none).all()
    none, ok0, n0 = sampling.column_quantiles_device(torch.full((3, 17), float("nan"), dtype=torch.float64, device=dev), [0.5])
    assert n0 == 0 and not ok0.any() and np.isnan(none).all()


# ---------------------------------------------------------------- 3. end to end
P, SC = fitting.ParamDef, fitting.Scale
FIXED = [P("theta_c", 0.1, 0.1, SC.fixed), P("Gamma0", 300.0, 300.0, SC.fixed), P("n_ism", 1.0, 1.0, SC.fixed),
         P("eps_e", 0.1, 0.1, SC.fixed), P("eps_B", 0.01, 0.01, SC.fixed), P("p", 2.3, 2.3, SC.fixed)]
DEFS = [P("E_iso", 1e50, 1e54, SC.log), P("theta_v", 0.0, 0.5, SC.linear), P("A_V", 0.0, 2.0, SC.linear)] + FIXED
DEFS_NO_AV = [P("E_iso", 1e50, 1e54, SC.log), P("theta_v", 0.0, 0.5, SC.linear), P("A_V", 0.0, 0.0, SC.fixed)] + FIXED
GRID_T, GRID_NU = np.logspace(3, 7, 12), np.array([1e9, 4.84e14, 1e18])
QUANTILES = (0.16, 0.5, 0.84)
RTOL = tg.RTOL  # 2e-6


@pytest.fixture(scope="module")
def fitter():
    """The fitter of test_fitter_predictions_at_a_sample: a gaussian jet with forward SSC behind a smooth extinction law."""
    f = fitting.Fitter(z=0.5, lumi_dist=3e28, jet="gaussian", medium="ism", extinction=k_law, fwd_ssc=True)
    f.add_flux_density(4.84e14, GRID_T, np.full(GRID_T.size, 1e-28), np.full(GRID_T.size, 1e-29))
    f.validate_parameters(DEFS)
    return f


@pytest.fixture(scope="module")
def samples():
    """Nine draws near the sample of test_fitter_predictions_at_a_sample, and a tenth with a parameter that is not a number."""
    rng = np.random.default_rng(9)
    s = np.array([52.3, 0.17, 0.8]) + rng.standard_normal((10, 3)) * np.array([0.05, 0.01, 0.05])
    s[9, 0] = np.nan
    return s


@pytest.fixture(scope="module")
def full(fitter, samples):
    return fitter.predict(samples, DEFS, GRID_T, GRID_NU, quantiles=QUANTILES, return_draws=True)


def test_predict_draws_are_the_single_model_calls_and_the_bands_their_quantiles(fitter, samples, full):
    """Every valid draw against Fitter.flux_density_grid at its sample.

    A_V fixed at 0: the same arithmetic on both sides, but a grid request's partial sums are cut per workgroup and the rows of a
    workgroup follow the batch's total (bitwise from run to run, 1e-12 across batch sizes), so a draw of the
    batch of ten is not the bits of the batch of one: the observed maximum relative difference on the MI355X is 6.0e-14, and the
    rows are held to RTOL of tests/test_gpu_parity.py (2e-6).

    A free A_V: the two sides also group the factors of the exponent differently (three roundings each on an argument of magnitude
    below 10 at the radio and optical rows, a few ulp of each side's exp, together below 1e-14): at most 1e-13 relative; observed
    5.3e-14, of which the partial sums above are the larger part.  At 1e18 Hz the stand-in law gives both sides exp(-thousands) = 0,
    which is compared as it is."""
    assert full.n_valid == 9 and full.valid.tolist() == [True] * 9 + [False]  # a condition on the inputs: nine evaluable draws
    assert full.draws.shape == (10, 3, 12) and full.bands.shape == (3, 3, 12) and np.isnan(full.draws[9]).all()
    assert np.array_equal(full.draw_index, np.arange(10)) and np.array_equal(full.quantiles, QUANTILES)
    assert np.array_equal(full.t, GRID_T) and np.array_equal(full.nu, GRID_NU)
    worst = 0.0
    for s in range(9):
        want = fitter.flux_density_grid(samples[s], GRID_T, GRID_NU, DEFS).total
        assert np.all(want[:2] > 0) and np.all(np.isfinite(full.draws[s]))
        lit = want > 0  # (the law's k is in the thousands at 1e18 Hz: there both sides' factor underflows to 0)
        assert np.array_equal(full.draws[s][~lit], want[~lit])
        worst = max(worst, float(np.max(np.abs(full.draws[s][lit] / want[lit] - 1.0))))
    print("free A_V: max |draw / flux_density_grid - 1| over the nine draws", worst)
    assert worst <= 1e-13
    # the bands are the statement of the draws, to the bit
    want_bands, want_ok, want_n = sampling.column_quantiles(full.draws, QUANTILES)
    assert want_n == 9 and np.array_equal(want_ok, full.valid) and same_bits(full.bands, want_bands)
    assert np.all(full.bands[0] <= full.bands[1]) and np.all(full.bands[1] <= full.bands[2])
    # without return_draws: the same bands from the context's scratch
    lean = fitter.predict(samples, DEFS, GRID_T, GRID_NU, quantiles=QUANTILES)
    assert lean.draws is None and same_bits(lean.bands, full.bands) and lean.n_valid == 9
    # A_V fixed at 0
    plain = fitter.predict(samples[:, :2], DEFS_NO_AV, GRID_T, GRID_NU, quantiles=QUANTILES, return_draws=True)
    assert plain.n_valid == 9 and plain.valid.tolist() == [True] * 9 + [False]
    differ = 0.0
    for s in range(9):
        want = fitter.flux_density_grid(samples[s, :2], GRID_T, GRID_NU, DEFS_NO_AV).total
        assert np.all(want > 0)
        differ = max(differ, float(np.max(np.abs(plain.draws[s] / want - 1.0))))
    print("A_V = 0: max |draw / flux_density_grid - 1| over the nine draws", differ)
    assert differ <= RTOL
    assert same_bits(plain.bands, sampling.column_quantiles(plain.draws, QUANTILES)[0])
    assert np.all(plain.bands[:, 1:] > full.bands[:, 1:])  # the extinction dims the optical and the X-ray rows


def test_predict_draws_a_seeded_subset(fitter, samples, full):
    sub = fitter.predict(samples, DEFS, GRID_T, GRID_NU, quantiles=QUANTILES, draws=5, seed=3, return_draws=True)
    index = np.sort(np.random.default_rng(3).choice(10, 5, replace=False))
    assert np.array_equal(sub.draw_index, index) and sub.draws.shape == (5, 3, 12) and sub.valid.shape == (5,)
    assert np.array_equal(sub.valid, full.valid[index]) and sub.n_valid == int(full.valid[index].sum())
    # the rows of the full call, to what DESIGN.md section 7 states for grid requests across batch sizes (1e-12), and their bands
    lit = sub.valid
    rel = np.abs(sub.draws[lit][:, :2] / full.draws[index][lit][:, :2] - 1.0).max()
    print("five draws of ten: max relative difference of a draw between the two batches", rel)
    assert rel <= 1e-12 and np.array_equal(np.isnan(sub.draws), np.isnan(full.draws[index]))
    assert same_bits(sub.bands, sampling.column_quantiles(sub.draws, QUANTILES)[0])
    subset = sampling.column_quantiles(full.draws[index], QUANTILES)[0]
    assert np.all(np.abs(sub.bands[:, :2] / subset[:, :2] - 1.0) <= 1e-12) and np.array_equal(sub.bands[:, 2], subset[:, 2])
    assert not same_bits(sub.bands, full.bands)


def test_predict_resolution_reaches_the_models_and_wrong_widths_are_refused(fitter, samples, full):
    coarse = fitter.predict(samples, DEFS, GRID_T, GRID_NU, quantiles=QUANTILES, resolution=(0.1, 0.3, 8.0), return_draws=True)
    assert coarse.bands.shape == full.bands.shape and coarse.draws.shape == full.draws.shape and coarse.n_valid == 9
    assert np.array_equal(coarse.valid, full.valid) and np.array_equal(coarse.draw_index, full.draw_index)
    rel = np.abs(coarse.bands[:, :2] / full.bands[:, :2] - 1.0)  # (the X-ray row is 0 behind the stand-in law)
    assert 0.0 < rel.max() < 0.2  # another grid: other numbers, the same light curves
    assert fitter.resolution != (0.1, 0.3, 8.0)  # the fitter keeps its own
    again = fitter.predict(samples, DEFS, GRID_T, GRID_NU, quantiles=QUANTILES)
    assert same_bits(again.bands, full.bands)
    with pytest.raises(ValueError, match=r"samples must be \[N, 3\]"):
        fitter.predict(samples[:, :2], DEFS, GRID_T, GRID_NU)
    with pytest.raises(ValueError, match="draws=11 exceeds the 10 rows"):
        fitter.predict(samples, DEFS, GRID_T, GRID_NU, draws=11)


# ---------------------------------------------------------------- 4. memory
def test_refusals_leave_the_context_usable_and_memory_returns(torch, fitter, samples, full):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    spec, _, _ = fitter.build_spec(DEFS)
    ext = 0.4 * np.log(10.0) * k_law((2.99792458e10 / GRID_NU) / 1.5)
    S, nt, nnu = 10, GRID_T.size, GRID_NU.size
    d = dict(theta=torch.from_numpy(samples).to(dev), t=torch.from_numpy(GRID_T).to(dev), nu=torch.from_numpy(GRID_NU).to(dev),
             ext=torch.from_numpy(ext).to(dev), bands=torch.zeros((3, nnu, nt), dtype=torch.float64, device=dev),
             draws=torch.zeros((S, nnu, nt), dtype=torch.float64, device=dev), valid=torch.zeros(S, dtype=torch.int32, device=dev),
             n=torch.zeros(1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()  # (the context runs on a stream of its own)
    p = {k: v.data_ptr() for k, v in d.items()}
    qs = _lib.QuantileSpec(3, 0, (C.c_double * 16)(*QUANTILES))
    before = lib.vag_device_bytes_in_use()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def bands(ctx=ctx, spec=spec, S=S, ndim=3, nt=nt, nnu=nnu, qs=qs, **null):
        a = {k: (None if k in null else v) for k, v in p.items()}
        rc = lib.vag_predict_bands_dev(ctx, C.byref(spec) if spec is not None else None, a["theta"], S, ndim, a["t"], nt, a["nu"], nnu,
                                       a["ext"], C.byref(qs) if qs is not None else None, a["bands"], a["draws"], a["valid"], a["n"])
        if ctx is not None:
            _lib.check(lib.vag_ctx_synchronize(ctx))
        return rc

    assert bands() == _lib.VAG_OK
    first = [d[k].cpu().numpy() for k in ("bands", "draws", "valid", "n")]
    assert same_bits(first[0], full.bands) and same_bits(first[1], full.draws) and first[3][0] == 9
    assert np.array_equal(first[2] != 0, full.valid)
    for what, rc in [("null context", bands(ctx=None)), ("null spec", bands(spec=None)), ("null theta", bands(theta=1)),
                     ("null t", bands(t=1)), ("null nu", bands(nu=1)), ("null quantiles", bands(qs=None)), ("null bands", bands(bands=1)),
                     ("null n", bands(n=1)), ("ndim of another fit", bands(ndim=2)), ("no draw", bands(S=0)), ("no time", bands(nt=0)),
                     ("no frequency", bands(nnu=0)), ("nq 0", bands(qs=_lib.QuantileSpec(0, 0))),
                     ("q above 1", bands(qs=_lib.QuantileSpec(1, 0, (C.c_double * 16)(1.5))))]:
        assert rc == _lib.VAG_E_INVALID and _lib.last_error(), what
    assert bands(S=4097) == _lib.VAG_E_CAPACITY and "VAG_PREDICT_MAX_DRAWS" in _lib.last_error()
    bad = type(spec).from_buffer_copy(bytes(spec))
    bad.slot[1] = 500
    assert bands(spec=bad) == _lib.VAG_E_INVALID and "slot" in _lib.last_error()
    assert all(same_bits(u, d[k].cpu().numpy()) for u, k in zip(first, ("bands", "draws", "valid", "n")))  # nothing was written
    # the quantile entry on the same context, then the valid call as before; the optional buffers left out
    out = torch.zeros((3, nnu, nt), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    _lib.check(lib.vag_column_quantiles_dev(ctx, C.byref(qs), p["draws"], S, nnu * nt, None, out.data_ptr(), None, p["n"]))
    _lib.check(lib.vag_ctx_synchronize(ctx))
    assert same_bits(out.cpu().numpy(), full.bands)
    d["bands"].zero_()
    torch.cuda.synchronize()
    assert bands(draws=1, valid=1) == _lib.VAG_OK and same_bits(d["bands"].cpu().numpy(), full.bands)
    assert lib.vag_device_bytes_in_use() > before
    lib.vag_ctx_destroy(ctx)
    assert lib.vag_device_bytes_in_use() == before
