"""The engine's FP64 device routines against high-precision references (tests/_mathref.py), on the MI355X, through
vag_debug_device_math: the routines the product kernels inline, compiled in the library's own translation unit.

Metrics: relative error for exp2, 1/x, sqrt; absolute error in log2 units for the log2 family, softplus and the spectra (what reaches a
flux, which is exponentiated afterwards).  Gates are the bounds the code states.  Forms that claim the same bits as another form are
compared bit for bit (np.array_equal, NaN by position).  Run with -s to see the table of measured errors next to their gates."""
import ctypes as C

import numpy as np
import pytest

import _elecref as E
import _mathref as R
import _icref as IC
import _rsref as RS

pytestmark = pytest.mark.gpu

MEASURED = {}  # routine -> (measured max error, gate, metric)
_dp = C.POINTER(C.c_double)
ULP1 = np.spacing(1.0)


def record(name, err, gate, metric):
    MEASURED[name] = (float(err), float(gate), metric)
    return float(err)


@pytest.fixture(scope="module")
def dev():
    from vegasafterglow_amd import _lib
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.vag_ctx_create(0, C.byref(ctx)))

    def run(name, x, n_out=1):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.full((x.shape[0], n_out), np.nan)
        _lib.check(lib.vag_debug_device_math(ctx, ids[name], x.ctypes.data_as(_dp), x.shape[0], out.ctypes.data_as(_dp)))
        return out if n_out > 1 else out[:, 0]
    ids = {**_lib.MATH, **_lib.MATH_MORE}
    run.lib, run.ctx, run.ids = lib, ctx, ids
    yield run
    lib.vag_ctx_destroy(ctx)
    if MEASURED:
        print("\n[device math] routine                     measured      gate   metric")
        for k, (e, g, m) in MEASURED.items():
            print(f"[device math] {k:<26} {e:10.3e} {g:9.2e}   {m}")


def rel_err(got, ref):
    ref = R.to_ld(ref)
    return np.abs(got.astype(np.longdouble) - ref) / np.abs(ref)


def abs_err(got, ref):
    return np.abs(got.astype(np.longdouble) - R.to_ld(ref))


def ulp_err(got, ref):
    """|got - ref| in ulps of the correctly rounded result."""
    ref = R.to_ld(ref)
    return np.abs(got.astype(np.longdouble) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)


def nudge(x, k):
    """x moved by k ulps (k may be negative), elementwise."""
    x = np.asarray(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def around(x, ks=(-2, -1, 0, 1, 2)):
    return np.concatenate([nudge(x, k) for k in ks])


RNG = np.random.default_rng(20261016)


# ---------------------------------------------------------------- exp2
def exp2_inputs():
    k = np.arange(-1022, 1024, dtype=np.float64)
    half = np.concatenate([k + 0.5, k - 0.5])
    return np.concatenate([np.linspace(-1022, 1023.999, 1 << 20), RNG.uniform(-1, 1, 1 << 16), k, around(half), [0.0, -0.0]])


# exp2_ode keeps the degree-12 Taylor coefficients that vag_device.h's comment put at 3.3e-16: 3.66e-16 measured here (harmless: it
# only scales ODE steps integrated to 1e-6), so its gate is 3.7e-16
@pytest.mark.parametrize("name,gate", [("exp2_fast", 2.5e-16), ("exp2_ode", 3.7e-16)])
def test_exp2_relative_error_on_normal_results(dev, name, gate):
    x = exp2_inputs()
    x = x[(x >= -1022) & (x < 1024)]
    y = dev(name, x)
    worst = record(name, np.max(rel_err(y, R.exp2(x))), gate, "relative, normal results")
    assert worst <= gate, worst
    k = np.arange(-1022, 1024, dtype=np.float64)
    assert np.array_equal(dev(name, k), np.ldexp(1.0, k.astype(int))), "2^k for integer k must be exact"
    assert dev(name, np.array([0.0, -0.0])).tolist() == [1.0, 1.0]


# within 1 subnormal ulp for exp2_fast; exp2_ode's relative error of the polynomial (3.7e-16) alone reaches 2^52 x 3.7e-16 = 1.7
# subnormal ulps just below 2^-1022, plus the final rounding's 1/2
@pytest.mark.parametrize("name,sub_gate", [("exp2_fast", 1.0), ("exp2_ode", 0.5 + 2.0 ** 52 * 3.7e-16)])
def test_exp2_subnormal_band_and_saturation(dev, name, sub_gate):
    x = np.sort(np.concatenate([np.linspace(-1075, -1022, 200001), -1022 - RNG.uniform(0, 53, 5000)]))
    y = dev(name, x)
    sub_ulp = 2.0 ** -1074
    err = np.max(np.abs(y.astype(np.longdouble) - R.to_ld(R.exp2(x)))) / np.longdouble(sub_ulp)
    record(name + " subnormal", err, sub_gate, "subnormal ulps")
    assert err <= sub_gate, err
    assert np.all(np.diff(y) >= 0), "not monotone across the subnormal band"
    assert dev(name, np.array([1024.0, 1100.0])).tolist() == [np.inf, np.inf]
    assert dev(name, np.array([-1100.0]))[0] == 0.0
    assert dev(name, np.array([-1075.0]))[0] in (0.0, sub_ulp)


def test_exp2_sat_and_or_zero_are_exp2_fast_on_their_domains(dev):
    x = np.concatenate([exp2_inputs(), np.linspace(-1100, 1100, 100001), [-1100.0, 1100.0, -1075.0, 1024.0]])
    fast = dev("exp2_fast", x)
    assert np.array_equal(dev("exp2_sat", x), fast, equal_nan=True)
    assert dev("exp2_sat", np.array([np.inf, -np.inf, 1e300, -1e300])).tolist() == [np.inf, 0.0, np.inf, 0.0]
    assert np.isnan(dev("exp2_sat", np.array([np.nan]))[0])
    xf = np.concatenate([x, [-2000.0, -2000.5, -1e300, -5000.0]])
    assert np.array_equal(dev("exp2_or_zero", xf), dev("exp2_fast", np.maximum(xf, -2000.0)), equal_nan=True)
    z = dev("exp2_or_zero", np.array([np.nan, -np.inf]))
    assert z.tolist() == [0.0, 0.0] and not np.signbit(z).any()


# ---------------------------------------------------------------- log2
def log2_normals():
    e = np.arange(-1022, 1024, dtype=np.float64)
    p2 = np.ldexp(1.0, e.astype(int))
    edges = 1 + np.arange(65) / 64.0
    scales = np.ldexp(1.0, np.array([-1022, -300, -7, -1, 0, 1, 5, 64, 700, 1023]))
    with np.errstate(over="ignore"):
        slice_edges = (around(edges, (-1, 0, 1))[:, None] * scales[None, :]).ravel()
        root2 = np.sqrt(2.0) * scales
    x = np.concatenate([
        np.ldexp(1 + RNG.uniform(0, 1, 1 << 20), RNG.integers(-1022, 1024, 1 << 20)),
        1 + RNG.uniform(-1e-3, 1e-3, 1 << 16),
        np.array([nudge(1.0, k) for k in range(-64, 65)]),
        around(root2[np.isfinite(root2)], (-1, 0, 1)),
        slice_edges, p2, p2 * (2 - ULP1), [np.finfo(float).tiny, np.finfo(float).max]])
    return x[np.isfinite(x) & (x >= np.finfo(float).tiny)]


def test_log2_tab_error_relative_to_max_1_log2x(dev):
    x = log2_normals()
    ref = R.to_ld(R.log2(x))
    y = dev("log2_tab", x)
    worst = record("log2_tab", np.max(np.abs(y - ref) / np.maximum(1, np.abs(ref))), 4e-16, "abs / max(1, |log2 x|)")
    assert worst <= 4e-16, worst
    assert np.array_equal(dev("log2_tab_nb", x), y), "log2_tab_nb must give log2_tab's bits on positive normals"


def test_log2_fast_within_two_ulp_of_the_result(dev):
    x = log2_normals()
    x = x[x != 1.0]
    y = dev("log2_fast", x)
    worst = record("log2_fast", np.max(ulp_err(y, R.log2(x))), 2.0, "ulp of the result")
    assert worst <= 2.0, worst
    assert dev("log2_fast", np.array([1.0]))[0] == 0.0


@pytest.mark.parametrize("name", ["log2_fast", "log2_tab"])
def test_log2_special_arguments_take_the_library_log2(dev, name):
    special = np.array([0.0, -0.0, -1.0, -np.inf, np.inf, np.nan, -1e-300])
    y = dev(name, special)
    assert y[:2].tolist() == [-np.inf, -np.inf] and np.isnan(y[2]) and np.isnan(y[3]) and y[4] == np.inf and np.isnan(y[5])
    assert np.isnan(y[6])
    sub = np.concatenate([np.ldexp(1.0, -np.arange(1023, 1075)), RNG.uniform(0, 1, 4096) * np.finfo(float).tiny])
    sub = sub[sub > 0]
    assert np.max(ulp_err(dev(name, sub), R.log2(sub))) <= 1.0  # the library log2 (ocml: 1 ulp)


# ---------------------------------------------------------------- 1/x, sqrt
def mantissa_grid(emin, emax):
    m = np.array([1.0, 1 + ULP1, np.sqrt(2.0), 2 - ULP1])
    e = np.arange(emin, emax + 1)
    return (m[:, None] * np.ldexp(1.0, e)[None, :]).ravel()


# rcp_ode / rcp1 (one Newton step) and sqrt_ode / sqrt1 (one correction) were stated at 2e-15 / 4e-15: 2.16e-15 / 4.15e-15 measured
# here, inside right-hand sides integrated to 1e-6, so the gates are 2.2e-15 / 4.2e-15; sqrt_fast, stated 1.1e-16, measured 1.58e-16
# (0.71 ulp): 1.6e-16.  The comments beside the routines now give these figures.
@pytest.mark.parametrize("name,gate,metric", [("rcp_fast", 2.0, "ulp"), ("rcp_ode", 2.2e-15, "relative"), ("rcp1", 2.2e-15, "relative")])
def test_reciprocals(dev, name, gate, metric):
    x = np.concatenate([mantissa_grid(-1021, 1021), np.ldexp(1 + RNG.uniform(0, 1, 1 << 20), RNG.integers(-1021, 1022, 1 << 20))])
    x = np.concatenate([x, -x[::7]])
    y = dev(name, x)
    err = ulp_err(y, R.rcp(x)) if metric == "ulp" else rel_err(y, R.rcp(x))
    worst = record(name, np.max(err), gate, metric)
    assert worst <= gate, worst


@pytest.mark.parametrize("name,gate", [("sqrt_fast", 1.6e-16), ("sqrt_ode", 4.2e-15), ("sqrt1", 4.2e-15)])
def test_square_roots(dev, name, gate):
    x = np.concatenate([mantissa_grid(-1022, 1023), np.ldexp(1 + RNG.uniform(0, 1, 1 << 20), RNG.integers(-1022, 1024, 1 << 20))])
    x = x[np.isfinite(x)]
    y = dev(name, x)
    worst = record(name, np.max(rel_err(y, R.sqrt(x))), gate, "relative")
    assert worst <= gate, worst
    if name != "sqrt_ode":  # sqrt_ode: strictly positive arguments only
        assert dev(name, np.array([0.0]))[0] == 0.0


# ---------------------------------------------------------------- softplus
def sp_inputs():
    i = np.arange(0, 202, dtype=np.float64)
    edges = np.concatenate([(i + 0.5) / 10, (i - 0.5) / 10])
    edges = np.concatenate([edges, -edges])
    return np.concatenate([RNG.uniform(-22, 22, 1 << 20), np.linspace(-21, 21, 420001), around(edges, (-1, 0, 1)),
                           around(np.array([20.0, -20.0]), (-2, -1, 0, 1, 2)), [0.0, -0.0, 20.05, -20.05, 25.0, -25.0, 1e300, -1e300]])


def test_sp_fast_against_log2_softplus(dev):
    z = sp_inputs()
    y = dev("sp_fast", z)
    worst = record("sp_fast", np.max(abs_err(y, R.softplus(z))), 5e-14, "abs, log2 units")
    assert worst <= 5e-14, worst
    # continuity across the table's interval edges (i +- 1/2) / 10: both neighbours approximate the same function
    i = np.arange(0, 201, dtype=np.float64)
    e = np.concatenate([(i + 0.5) / 10, -(i + 0.5) / 10])
    lo, hi = dev("sp_fast", nudge(e, -1)), dev("sp_fast", nudge(e, 1))
    jump = np.max(np.abs(hi - lo) - np.abs(R.to_ld(R.softplus(nudge(e, 1))) - R.to_ld(R.softplus(nudge(e, -1)))))
    record("sp_fast edge jump", jump, 1e-13, "abs, log2 units")
    assert jump <= 1e-13, jump
    s = dev("sp_fast", np.array([np.inf, -np.inf, np.nan]))
    assert s[0] == np.inf and s[1] == 0.0 and np.isnan(s[2])


def test_sp_fast_forms_give_the_same_bits(dev):
    z = np.concatenate([sp_inputs(), [np.inf, -np.inf, np.nan]])
    y = dev("sp_fast", z)
    assert np.array_equal(dev("sp_fast_global", z), y, equal_nan=True), "LDS and global tables differ"
    assert np.array_equal(dev("sp_fast_sel", z), y, equal_nan=True), "sp_fast_sel differs from sp_fast"


@pytest.mark.parametrize("n", [1, 63, 65])
def test_elementwise_shapes(dev, n):
    x = np.linspace(-30, 30, 1 << 20)
    full = dev("exp2_fast", x)
    assert np.array_equal(dev("exp2_fast", x[:n]), full[:n])
    assert np.array_equal(dev("sp_fast", x[-n:]), dev("sp_fast", x)[-n:])
    # the electron stage and the forward shock's state (tests/test_electron_stage.py): rows of 12 -> 11 and of 5 -> 4 doubles
    for name, rows, n_out in (("elec_cell", E.probe_set(2.3)[0], 11), ("fwd_state", E.fwd_state_rows(), 4)):
        full = dev(name, rows, n_out)
        assert full.shape == (rows.shape[0], n_out) and not np.isnan(full[:, 0]).any()
        assert np.array_equal(dev(name, rows[:n], n_out), full[:n], equal_nan=True)
        assert np.array_equal(dev(name, rows[-n:], n_out), full[-n:], equal_nan=True)
    # the reverse shock's closed forms and cell state (tests/test_reverse_state.py): rows of 1 ... 65 -> 2 ... 48 doubles
    from vegasafterglow_amd import _lib
    for name, (n_in, n_out) in _lib.MATH_RS_SHAPES.items():
        rows = RS.probe_set(name)[0]
        full = dev(name, rows, n_out)
        assert rows.shape[1] == n_in and full.shape == (rows.shape[0], n_out) and not np.isnan(full).any()
        assert np.array_equal(dev(name, rows[:n], n_out), full[:n]) and np.array_equal(dev(name, rows[-n:], n_out), full[-n:])
    # the inverse-Compton routines (tests/test_ic_state.py): rows of 1 ... 21 -> 1 ... 18 doubles; the suffix scan takes whole wavefronts
    for name, (n_in, n_out) in _lib.MATH_IC_SHAPES.items():
        rows = IC.probe_set(name)[0]
        full = dev(name, rows, n_out).reshape(rows.shape[0], -1)
        assert rows.shape[1] == n_in and full.shape == (rows.shape[0], n_out) and not np.isnan(full).any()
        m = min(64 * n if name == "ic_suffix_scan" else n, rows.shape[0])
        assert np.array_equal(dev(name, rows[:m], n_out).reshape(m, -1), full[:m]) and np.array_equal(dev(name, rows[-m:], n_out).reshape(m, -1), full[-m:])


# ---------------------------------------------------------------- synchrotron cell
PS = [1.5, 2.05, 2.3, 3.0, 3.5, 4.5]
VP = R.VP
NPAR = R.NPAR


def syn_cells():
    """(physical inputs [n][7], log2 breaks): all six orderings of nu_a, nu_m, nu_c, near-ties, every p."""
    rng = np.random.default_rng(5)  # the same cells whichever tests run before
    B = 1.0
    lk = np.log2(R.K_SYN_FREQ * B)
    rows = []
    orders = [(-6, 0, 5), (-6, 5, 0), (0, -6, 5), (5, -6, 0), (0, 5, -6), (5, 0, -6)]  # (a, m, c) offsets in octaves
    ties = [(0, 0, 4), (1e-3, 0, 4), (-1e-3, 0, 4), (-4, 0, 1e-3), (-4, 0, -1e-3), (-4, 0, 0), (1e-3, 0, -1e-3), (0, 0, 0)]
    for p in PS:
        for lm in (30.0, 47.3):
            for da, dm, dc in orders + ties:
                l_m = lm + dm
                l = dict(a=lm + da, m=l_m, c=lm + dc, M=l_m + 28 + 3 * rng.uniform())
                g = {k: 2.0 ** ((v - lk) / 2) for k, v in l.items()}
                rows.append([g["m"], g["c"], g["a"], g["M"], 10.0 ** rng.uniform(15, 25), B, p])
    return np.array(rows)


def syn_freqs(cell_rows):
    """Per cell: far below nu_a through each break to past nu_M, the log2_x_far and nu_M - 20 octave thresholds +- ulp."""
    ph = R.photons_from_physical(*cell_rows.T)
    lm, la, lc, lM = (R.to_ld(ph[k]).astype(float) for k in ("l_m", "l_a", "l_c", "l_M"))
    xf = R.to_ld(ph["log2_x_far"]).astype(float)
    xs = []
    for i in range(cell_rows.shape[0]):
        lo = min(la[i], lm[i], lc[i]) - 12
        base = np.linspace(lo, lM[i] + 4, 96)
        brk = np.concatenate([b + np.array([-0.3, -0.05, 0.0, 0.05, 0.3]) for b in (la[i], lm[i], lc[i], lM[i])])
        thr = np.concatenate([around(np.array([lm[i] + xf[i]]), (-2, -1, 0, 1, 2)), around(np.array([lM[i] - 20]), (-2, -1, 0, 1, 2))])
        xs.append(np.concatenate([base, brk, thr]))
    return xs


def spec_gate(blk):
    """Bound on |device - formula| per cell, log2 units.  Each softplus evaluation is within the table bound TAB = 5e-14; the thin branch
    carries two of them weighted 1 / smooth_lo and 1 / smooth_hi, the thick branch one (weight <= 1, as every error of thin and of the
    thick branch enters smooth_one = thin - sp(s (thin - b)) / s with a factor <= 1), the combination one more weighted 1 / s_a_blend.
    The folded terms (2.5 log2 nu + TB, diff_hi log2 nu + BHI, LG2_I_SLO + smooth_one) reach ~250, whose ulp is 2.8e-14: eight such
    roundings.  So TAB (1/s_lo + 1/s_hi + 1 + 1/s_ab) + 8 * 2.8e-14, and never above 1e-12 (10^6 below the 2e-6 of the end-to-end
    oracle tests)."""
    TAB = 5e-14
    g = TAB * (np.abs(blk[:, VP["INV_SLO"]]) + np.abs(blk[:, VP["INV_SHI"]]) + 1 + np.abs(blk[:, VP["INV_SAB"]])) + 8 * 2.8e-14
    return np.minimum(g, 1e-12)


@pytest.fixture(scope="module")
def syn(dev):
    cells = syn_cells()
    xs = syn_freqs(cells)
    rows, ci = [], []
    for i, x in enumerate(xs):
        if x.size % 2:
            x = np.append(x, x[-1])
        pairs = x.reshape(-1, 2)
        rows.append(np.hstack([np.repeat(cells[i:i + 1], pairs.shape[0], 0), pairs]))
        ci.append(np.full(pairs.shape[0], i))
    inp = np.vstack(rows)
    out = dev("syn_cell", inp, R.NPAR + 8)
    return cells, np.concatenate(ci), inp, out


def test_synchrotron_spectra_against_the_formula(syn):
    cells, ci, inp, out = syn
    blk = out[:, :NPAR]
    x = inp[:, 7:9]
    gate = spec_gate(blk)
    # a cell's build (soft_offset's +-20 cut: l_c - l_m = 5 octaves exactly) and an evaluation may each sit at a threshold: every pairing
    phs = {s: R.photons_from_physical(*[inp[:, k][:, None] for k in range(7)], side=s) for s in (None, -1, 1)}
    refs = [R.to_ld(R.log2_I_nu(phs[b], x, side=s)) for b in (None, -1, 1) for s in (None, -1, 1)]
    for name, cols in (("log2_I_nu_fast", [NPAR, NPAR + 1]), ("log2_I_nu (libm)", [NPAR + 6, NPAR + 7])):
        got = out[:, cols]
        err = np.minimum.reduce([np.abs(got - r) for r in refs])
        assert np.array_equal(np.isfinite(got), np.isfinite(refs[0]))
        fin = np.isfinite(refs[0])
        # past |value| = 256 (the exponential cut-off far beyond nu_M) the rounding grows with the value: scale the bound with it
        scale = np.maximum(1, np.abs(np.where(fin, refs[0], 0)).astype(float) / 256)
        worst = float(np.max(np.where(fin, err / scale, 0)))
        ratio = float(np.max(np.where(fin, err / (gate[:, None] * scale), 0)))
        record(name, worst, float(np.max(gate)), f"abs, log2 units; worst / per-cell bound {ratio:.2f}")
        assert ratio <= 1.0, (name, worst)


def fold_ulps(a, b):
    """|a - b| in ulps of the folded terms: of max(256, |value|) (the terms of an evaluation reach ~250)."""
    return np.max(np.where(np.isnan(a) & np.isnan(b), 0, np.abs(a - b) / np.spacing(np.maximum(256, np.abs(b)))))


def test_synchrotron_forms_agree_to_one_ulp_of_the_folded_terms(syn):
    # Not the same bits, as vag_device.h claimed before these tests: the compiler contracts a * b - c * d into an FMA one way or the
    # other in each inlined copy, so the register-block, strided and two-frequency forms differ by one rounding of a term of ~250
    # (2.8e-14) or of one in [256, 512) (5.7e-14) on ~2 % of these points.  Pinned at one ulp of max(256, |value|), as measured.
    _, _, _, out = syn
    regs, strided, fast2 = out[:, NPAR:NPAR + 2], out[:, NPAR + 2:NPAR + 4], out[:, NPAR + 4:NPAR + 6]
    assert np.array_equal(np.isnan(strided), np.isnan(regs)) and np.array_equal(np.isnan(fast2), np.isnan(regs))
    d_strided = record("strided vs register block", fold_ulps(strided, regs), 1.0, "ulps of max(256, |value|)")
    d_fast2 = record("log2_I_nu_fast2 vs fast", fold_ulps(fast2, regs), 1.0, "ulps of max(256, |value|)")
    assert d_strided <= 1.0 and d_fast2 <= 1.0, (d_strided, d_fast2)


# ---------------------------------------------------------------- IC cell
Q = dict(LG2_NUC=0, L1PYC=1, HASIC=2, LG2_KB=3, NSEG=4, S0=5, L0=6, C0=7, S1=8, L1=9, C1=10, S2=11, L2=12, C2=13)


def ic_inputs(syn):
    cells, ci, inp, out = syn
    rng = np.random.default_rng(6)
    pick = np.unique(ci, return_index=True)[1][::3]
    rows = []
    for r in pick:
        blk, p = out[r, :NPAR], inp[r, 6]
        l_m = blk[VP["LG2_NUM"]]
        q = np.zeros(R.NQ)
        q[Q["LG2_NUC"]], q[Q["HASIC"]], q[Q["L1PYC"]], q[Q["LG2_KB"]] = l_m + 2.0, 1.0, 0.7, -l_m + 20.0
        # one segment, slope 0: z = c0 swept across +-20 (ic_thin_correction's table and its a > 20 tail)
        zs = np.concatenate([np.linspace(-24, 24, 481), around(np.array([20.0, -20.0]), (-2, -1, 0, 1, 2)),
                             rng.uniform(20, 22, 40), -rng.uniform(20, 22, 40)])
        for z in zs:
            qq = q.copy()
            qq[Q["NSEG"]], qq[Q["S0"]], qq[Q["C0"]] = 1, 0.0, z
            rows.append(np.concatenate([blk, qq, [p, l_m + 6.0, l_m + 9.5]]))
        # the `applies` boundary lg2_nu = lg2_nuc +- ulp
        qq = q.copy()
        qq[Q["NSEG"]], qq[Q["S0"]], qq[Q["C0"]] = 1, 0.0, 3.0
        for x in around(np.array([q[Q["LG2_NUC"]]]), (-2, -1, 0, 1, 2)):
            rows.append(np.concatenate([blk, qq, [p, x, q[Q["LG2_NUC"]] + 1]]))
        # three continuous segments, evaluated at lg = l1, l2 (+- ulp): lg = (lg2_nu + lg2_kb) / 2
        qq = q.copy()
        l1, l2 = 35.5, 38.25
        qq[Q["NSEG"]], qq[Q["S0"]], qq[Q["C0"]] = 3, 1.5, -60.0
        qq[Q["L1"]], qq[Q["S1"]] = l1, -0.5
        qq[Q["C1"]] = qq[Q["C0"]] + (qq[Q["S0"]] - qq[Q["S1"]]) * l1
        qq[Q["L2"]], qq[Q["S2"]] = l2, 2.0
        qq[Q["C2"]] = qq[Q["C1"]] + (qq[Q["S1"]] - qq[Q["S2"]]) * l2
        for lg in around(np.array([l1, l2]), (-1, 0, 1)):
            x = 2 * lg - q[Q["LG2_KB"]]
            if x > q[Q["LG2_NUC"]]:
                rows.append(np.concatenate([blk, qq, [p, x, x + 0.25]]))
    return np.array(rows)


def ic_reference(inp, side):
    blk, q = inp[:, :NPAR], inp[:, NPAR:NPAR + R.NQ]
    p = inp[:, NPAR + R.NQ]
    res = []
    for col in (1, 2):
        x = inp[:, NPAR + R.NQ + col]
        lg = 0.5 * (R.LD.arr(x) + R.LD.arr(q[:, Q["LG2_KB"]]))
        # (the hand-made segments are continuous at l1, l2: either side of a boundary gives the same z to an ulp)
        seg2 = (q[:, Q["NSEG"]] > 2) & (lg >= q[:, Q["L2"]])
        seg1 = ~seg2 & (q[:, Q["NSEG"]] > 1) & (lg >= q[:, Q["L1"]])
        z = np.where(seg2, q[:, Q["C2"]] + q[:, Q["S2"]] * lg,
                     np.where(seg1, q[:, Q["C1"]] + q[:, Q["S1"]] * lg, q[:, Q["C0"]] + q[:, Q["S0"]] * lg))
        applies = R._gt(R.LD.arr(x), R.LD.arr(q[:, Q["LG2_NUC"]]), side) & (q[:, Q["HASIC"]] != 0)
        corr = np.where(applies, R.LD.arr(q[:, Q["L1PYC"]]) - R.to_ld(R.log2_1p_exp2(z)), 0)
        res.append(R.to_ld(R.log2_I_nu_block(blk, p, x, side=side, thin_add=corr)))
    return np.stack(res, 1)


def test_ic_spectra_against_the_formula_and_each_other(dev, syn):
    inp = ic_inputs(syn)
    out = dev("ic_cell", inp, 6)
    plain, straight, pair = out[:, 0:2], out[:, 2:4], out[:, 4:6]
    assert np.array_equal(pair, plain, equal_nan=True), "log2_I_nu_ic_pair differs from log2_I_nu_ic"
    # the STRAIGHT form: one rounding of a folded term apart on some points, like the synchrotron forms above
    d = record("log2_I_nu_ic_straight vs ic", fold_ulps(straight, plain), 1.0, "ulps of max(256, |value|)")
    assert d <= 1.0, d
    refs = [ic_reference(inp, s) for s in (None, -1, 1)]
    err = np.minimum.reduce([np.abs(plain - r) for r in refs]) / np.maximum(1, np.abs(refs[0]).astype(float) / 256)
    # the spectrum's bound plus ic_thin_correction's own: the table (5e-14) or, beyond |z| = 20, the third-order term of log1p
    gate = spec_gate(inp[:, :NPAR]) + 5e-14
    worst = record("log2_I_nu_ic (3 forms)", np.max(err), float(np.max(gate)), f"abs, log2 units; worst / bound "
                   f"{float(np.max(err / gate[:, None])):.2f}")
    assert np.all(err <= gate[:, None]), worst
    # the tail window alone: thin-branch-dominated rows (6 and 9.5 octaves above nu_m) with 20 < |z| <= 22, where the first-order form
    # of ic_thin_correction was up to 6.6e-13 off; the spectrum's own rounding on these rows is 1.4e-13 (measured)
    z = inp[:, NPAR + Q["C0"]]
    tail = (inp[:, NPAR + Q["NSEG"]] == 1) & (np.abs(z) > 20) & (np.abs(z) <= 22)
    record("ic correction, |z| in (20, 22]", np.max(err[tail]), 2.5e-13, "abs, log2 units")
    assert np.max(err[tail]) <= 2.5e-13


# ---------------------------------------------------------------- wave routines
def kogge_stone(v):
    """wave_prefix_sum restated: row_shr 1, 2, 4, 8 inside rows of 16 lanes, then row_bcast:15 into rows 1, 3 and row_bcast:31 into
    rows 2, 3 -- the same IEEE additions in the same order."""
    x = v.reshape(-1, 64).copy()
    lane = np.arange(64)
    for k in (1, 2, 4, 8):
        src = np.where((lane % 16) >= k, np.roll(x, k, axis=1), 0.0)
        x = x + src
    add15 = np.where(np.isin(lane // 16, [1, 3]), x[:, np.clip((lane // 16) * 16 - 1, 0, 63)], 0.0)
    x = x + add15
    add31 = np.where(lane // 16 >= 2, x[:, [31]], 0.0)
    x = x + add31
    return x.ravel()


def wave_values(n):
    return np.ldexp(RNG.uniform(1, 2, n) * RNG.choice([-1.0, 1.0], n), RNG.integers(-30, 31, n))


def test_wave_prefix_sum_and_wave_sum(dev):
    n = 64 * 257
    ints = RNG.integers(-1000, 1001, n).astype(np.float64)
    pre = dev("wave_prefix_sum", ints)
    assert np.array_equal(pre, np.cumsum(ints.reshape(-1, 64), axis=1).ravel())
    assert np.array_equal(dev("wave_sum", ints), np.repeat(ints.reshape(-1, 64).sum(1), 64))
    v = wave_values(n)
    ks = kogge_stone(v)
    assert not np.array_equal(ks, np.cumsum(v.reshape(-1, 64), axis=1).ravel()), "values do not tell the trees apart"
    assert np.array_equal(dev("wave_prefix_sum", v), ks)
    assert np.array_equal(dev("wave_sum", v), np.repeat(ks.reshape(-1, 64)[:, 63], 64))


def lane_order_sums(vals, slots):
    out = np.zeros(64)
    for lane in range(64):
        out[slots[lane]] = out[slots[lane]] + vals[lane]
    return out


def test_sky_wave_sum_is_the_lane_order_sum(dev):
    n = 64 * 129
    v = wave_values(n)
    want = np.repeat([lane_order_sums(w, np.zeros(64, int))[0] for w in v.reshape(-1, 64)], 64)
    rev = np.repeat([lane_order_sums(w[::-1], np.zeros(64, int))[0] for w in v.reshape(-1, 64)], 64)
    assert not np.array_equal(want, rev)
    assert np.array_equal(dev("sky_wave_sum", v), want)


@pytest.mark.parametrize("pattern", ["one slot", "lane & 3", "lane >> 2", "lane >> 1"])
def test_lds_add_f64_adds_in_lane_order(dev, pattern):
    lane = np.arange(64)
    slots = {"one slot": 0 * lane, "lane & 3": lane & 3, "lane >> 2": lane >> 2, "lane >> 1": lane >> 1}[pattern]
    waves = 64 * 3
    v = wave_values(64 * waves)
    inp = np.stack([np.tile(slots, waves).astype(np.float64), v], 1)
    got = dev("lds_add", inp).reshape(-1, 64)
    want = np.array([lane_order_sums(w, slots) for w in v.reshape(-1, 64)])
    if pattern != "lane >> 1":  # two lanes per slot: a + b == b + a, no order to tell apart
        rev = np.array([lane_order_sums(w[::-1], slots[::-1]) for w in v.reshape(-1, 64)])
        assert not np.array_equal(want, rev), "values do not tell the orders apart"
    assert np.array_equal(got, want)
    assert np.array_equal(dev("lds_add", inp).reshape(-1, 64), got), "not the same bits run to run"


def test_probe_rejects_bad_arguments(dev):
    lib, ctx, ids = dev.lib, dev.ctx, dev.ids
    x = np.zeros(128)
    y = np.zeros(128)
    px, py = x.ctypes.data_as(_dp), y.ctypes.data_as(_dp)
    assert lib.vag_debug_device_math(ctx, 999, px, 1, py) == -1
    assert lib.vag_debug_device_math(ctx, -1, px, 1, py) == -1
    assert lib.vag_debug_device_math(ctx, ids["exp2_fast"], px, 0, py) == -1
    assert lib.vag_debug_device_math(ctx, ids["exp2_fast"], None, 1, py) == -1
    assert lib.vag_debug_device_math(ctx, ids["exp2_fast"], px, 1, None) == -1
    assert lib.vag_debug_device_math(None, ids["exp2_fast"], px, 1, py) == -1
    assert lib.vag_debug_device_math(ctx, ids["wave_sum"], px, 63, py) == -1
    for name in ("elec_cell", "fwd_state"):
        assert lib.vag_debug_device_math(ctx, ids[name], px, 0, py) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], px, -3, py) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], None, 1, py) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], px, 1, None) == -1
        assert lib.vag_debug_device_math(None, ids[name], px, 1, py) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], px, 1, py) == 0  # (128 doubles hold one point of either)
    # the reverse-state routines: the same argument checks, and the points they are not defined on
    from vegasafterglow_amd import _lib
    for name, (n_in, n_out) in _lib.MATH_RS_SHAPES.items():
        good = np.ascontiguousarray(RS.probe_set(name)[0][:2])
        pg, po = good.ctypes.data_as(_dp), np.zeros(2 * n_out).ctypes.data_as(_dp)
        assert lib.vag_debug_device_math(ctx, ids[name], pg, 2, po) == 0
        assert lib.vag_debug_device_math(ctx, ids[name], pg, 0, po) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], pg, -3, po) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], None, 2, po) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], pg, 2, None) == -1
        assert lib.vag_debug_device_math(None, ids[name], pg, 2, po) == -1
    # the inverse-Compton routines: the same argument checks (64 points: one of them is a wave routine)
    for name, (n_in, n_out) in _lib.MATH_IC_SHAPES.items():
        good = np.ascontiguousarray(IC.probe_set(name)[0][:64])
        pg, po = good.ctypes.data_as(_dp), np.zeros(64 * n_out).ctypes.data_as(_dp)
        assert lib.vag_debug_device_math(ctx, ids[name], pg, 64, po) == 0
        assert lib.vag_debug_device_math(ctx, ids[name], pg, 0, po) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], pg, -3, po) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], None, 64, po) == -1
        assert lib.vag_debug_device_math(ctx, ids[name], pg, 64, None) == -1
        assert lib.vag_debug_device_math(None, ids[name], pg, 64, po) == -1
    assert lib.vag_debug_device_math(ctx, ids["ic_suffix_scan"], pg, 63, po) == -1

    def ic_rejected(name, col, value, row=1):
        pts = np.ascontiguousarray(IC.probe_set(name)[0][:2]).copy()
        pts[row, col] = value
        return lib.vag_debug_device_math(ctx, ids[name], pts.ctypes.data_as(_dp), 2, np.zeros(2 * _lib.MATH_IC_SHAPES[name][1]).ctypes.data_as(_dp)) == -1
    assert ic_rejected("kn_lut", 0, 128.0) and ic_rejected("kn_lut", 0, -1.0) and ic_rejected("kn_lut", 0, 0.5) and ic_rejected("kn_lut", 0, np.nan)
    assert ic_rejected("ic_table", 0, 17.0) and ic_rejected("ic_table", 0, -2.0) and ic_rejected("ic_table", 0, 1.5) and ic_rejected("ic_table", 0, np.nan)
    assert ic_rejected("ic_column_den", 5, 7.0) and ic_rejected("ic_column_den", 5, -1.0) and ic_rejected("ic_column_den", 5, 2.5)
    assert ic_rejected("ic_y", 5, 2.0) and ic_rejected("ic_y", 5, 0.5) and ic_rejected("ic_y", 5, np.nan)
    assert ic_rejected("ic_step", 6, 2.0) and ic_rejected("ic_step", 6, -1.0) and ic_rejected("ic_fixed_point", 7, 0.5) and ic_rejected("ic_fixed_point", 7, np.nan)
    assert ic_rejected("ic_gamma_a", 7, 2.0) and ic_rejected("ic_gamma_a", 7, 0.5)
    assert ic_rejected("ic_table", 0, 17.0, row=0), "a bad first point"

    def rejected(name, col, value, row=1):
        pts = np.ascontiguousarray(RS.probe_set(name)[0][:2]).copy()
        pts[row, col] = value
        return lib.vag_debug_device_math(ctx, ids[name], pts.ctypes.data_as(_dp), 2, np.zeros(2 * _lib.MATH_RS_SHAPES[name][1]).ctypes.data_as(_dp)) == -1
    assert rejected("rvs_state", 10, 2.0) and rejected("rvs_state", 10, 0.5) and rejected("rvs_state", 10, -1.0) and rejected("rvs_state", 10, np.nan)
    t_num = RS.probe_set("cross_lattice")[0][1, 4]
    assert rejected("cross_lattice", 4, 1.0) and rejected("cross_lattice", 4, 0.0) and rejected("cross_lattice", 4, 7.5)
    assert rejected("cross_lattice", 4, 4097.0) and rejected("cross_lattice", 5, 0.0) and rejected("cross_lattice", 5, np.nan)
    assert rejected("cross_lattice", 6, -1.0) and rejected("cross_lattice", 6, t_num) and rejected("cross_lattice", 6, 0.5)
    assert rejected("cross_lattice", 0, 0.0) and rejected("cross_lattice", 1, 0.0) and rejected("cross_lattice", 0, np.inf)
    assert rejected("rvs_extrap", 64, 17.0) and rejected("rvs_extrap", 64, -1.0) and rejected("rvs_extrap", 64, 2.5)
    assert rejected("pair_init", 6, 2.0) and rejected("pair_init", 6, -1.0) and rejected("pair_init", 6, 0.5)
    assert rejected("pair_init", 0, 1.0) and rejected("pair_init", 3, 0.0) and rejected("pair_init", 4, -1.0)
    assert rejected("rvs_state", 10, 2.0, row=0), "a bad first point"
    assert lib.vag_debug_device_math(ctx, max(ids.values()) + 1, px, 1, py) == -1
    bad = np.zeros((64, 2))
    bad[5, 0] = 64.0
    assert lib.vag_debug_device_math(ctx, ids["lds_add"], bad.ctypes.data_as(_dp), 64, np.zeros(64).ctypes.data_as(_dp)) == -1
