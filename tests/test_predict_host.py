"""Posterior-predictive bands' host side (no GPU): the header's pieces, the numpy statement, the refusals.

1. csrc/vag_predict.h -- the text the kernels compile -- is held to hand-worked literals in tests/predict_check.cpp, a stand-alone
   program built under AddressSanitizer + UndefinedBehaviorSanitizer as tests/test_chain_stats_host.py builds its program and run as a
   child process; sampling.quantile_rank, sampling.column_quantiles and _lib.predict_tile_columns give the same bits over the rows it
   prints.  Nothing is loaded into this process;
2. the numpy statement against np.quantile(F, q, axis=0) on non-negative lognormal columns: at most 4 ulp of the larger value (both
   are roundings of the same exact interpolation between neighbours of one sign; 1 ulp was the largest seen when this was written);
3. order statistics where h is an integer are elements of the input to the bit;
4. validity per draw; 5. the Python-side refusals, each with its text; 6. the entries and the layout of the spec."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vegasafterglow_amd import _lib, sampling
from vegasafterglow_amd.fitting import Fitter, ParamDef, Scale

import test_fit_request_host as host  # FLAGS, STATIC: the sanitizer build of the other stand-alone programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
compile_cmd = host.compile_cmd  # (the module-scoped fixture: [compiler, flags...] or a skip where no sanitised hello-world links)

DRAWS = (1, 2, 3, 63, 64, 65, 101, 257, 4096)
LEVELS = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- 1. the header under the host sanitizers ----

@pytest.fixture(scope="module")
def header_rows(compile_cmd, tmp_path_factory):
    exe = tmp_path_factory.mktemp("predict") / "predict_check"
    built = host.run(compile_cmd + [os.path.join(ROOT, "tests", "predict_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "Sanitizer" not in ran.stdout and "runtime error" not in ran.stdout, ran.stdout
    assert "FAIL" not in ran.stdout, ran.stdout  # (a hand-worked literal was missed)
    assert ran.returncode == 0, ran.stdout
    rows = {"rank": [], "value": [], "column": [], "tile": []}
    for ln in ran.stdout.splitlines():
        kind, *words = ln.split()
        rows[kind].append(np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64))
    return rows


def test_header_ranks_are_the_numpy_ranks(header_rows):
    rows = header_rows["rank"]
    assert len(rows) >= 20
    for q, n, lo, g in rows:
        want_lo, want_g = sampling.quantile_rank(q, int(n))
        assert want_lo == int(lo) and same_bits(want_g, g), (q, n, lo, g)
        assert 0 <= lo <= n - 1 and 0.0 <= g < 1.0 and (lo < n - 1 or g == 0.0)
    assert {int(r[1]) for r in rows} >= {1, 2, 3, 101} and {r[0] for r in rows} >= {0.0, 1.0, 0.5, 0.16}
    assert any(r[3] != 0.0 for r in rows)  # an h that is not an integer


def test_header_values_are_the_exact_fma(header_rows):
    rows = header_rows["value"]
    assert len(rows) >= 8
    seen = set()
    for r in rows:
        n = int(r[0])
        y, lo, g, Q = r[1:1 + n], int(r[1 + n]), r[2 + n], r[3 + n]
        want = y[lo] if g == 0.0 else sampling._exact_fma(float(g), float(y[lo + 1] - y[lo]), float(y[lo]))
        assert same_bits(want, Q), (y, lo, g, Q, want)
        if lo == n - 1:
            seen.add("lo = n - 1")
            assert g == 0.0
        if g != 0.0 and y[lo] + g * (y[lo + 1] - y[lo]) != Q:
            seen.add("one rounding, not two")
    assert seen == {"lo = n - 1", "one rounding, not two"}, seen


def test_header_columns_are_the_numpy_statement_to_the_bit(header_rows):
    rows = header_rows["column"]
    assert len(rows) >= 200
    for r in rows:
        n = int(r[0])
        x, q, Q = r[1:1 + n], r[1 + n], r[2 + n]
        got, ok, n_valid = sampling.column_quantiles(x[:, None], [q])
        assert n_valid == n and ok.all() and same_bits(got[0, 0], Q), (x, q, Q, got)
    assert any(np.any(r[1:1 + int(r[0])] < 0) for r in rows) and any(np.signbit(r[1:1 + int(r[0])]).any() and r[-1] == 0 for r in rows)


def test_the_tile_is_the_headers(header_rows):
    rows = header_rows["tile"]
    assert {int(r[0]) for r in rows} >= {1, 2, 3, 63, 64, 65, 255, 256, 257, 4096}
    for S, P, T in rows:
        assert _lib.predict_tile_columns(int(S)) == int(T) and int(P) >= int(S) and int(P) & (int(P) - 1) == 0
        assert 8 * int(P) * int(T) <= 128 * 1024 and int(T) & (int(T) - 1) == 0


def test_the_entries_are_exported_and_the_spec_has_the_header_layout():
    lib = _lib.load()
    for name in _lib.PREDICT_ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and _lib.predict_entry(lib, name) is getattr(lib, name)
    assert _lib.PREDICT_ENTRIES == ("vag_column_quantiles_dev", "vag_predict_bands_dev") and lib.vag_abi_version() == 13
    assert ctypes.sizeof(_lib.QuantileSpec) == 136
    assert [(_lib.QuantileSpec.__dict__[n].offset) for n, _ in _lib.QuantileSpec._fields_] == [0, 4, 8]
    header = open(os.path.join(ROOT, "include", "vegasafterglow_amd.h")).read()
    assert "int32_t nq;\n    int32_t pad;\n    double q[VAG_PREDICT_MAX_Q];\n} vag_quantile_spec;" in header
    kernels = open(os.path.join(ROOT, "vegasafterglow_amd", "csrc", "vag_predict.h")).read()
    for text, value in (("#define VAG_PREDICT_MAX_DRAWS 4096", 4096), ("#define VAG_PREDICT_MAX_Q 16", 16),
                        ("#define VAG_PREDICT_MAX_VALUES (1ll << 27)", 1 << 27)):
        assert text in header and text in kernels
        name = text.split()[1].replace("VAG_", "")
        assert getattr(_lib, name) == getattr(sampling, name) == value
    # without a context the entries refuse before any device is looked for
    spec = _lib.QuantileSpec(1, 0, (ctypes.c_double * 16)(0.5))
    assert lib.vag_column_quantiles_dev(None, ctypes.byref(spec), None, 1, 1, None, None, None, None) == _lib.VAG_E_INVALID
    assert b"null context" in lib.vag_last_error()
    assert lib.vag_predict_bands_dev(None, None, None, 1, 1, None, 1, None, 1, None, ctypes.byref(spec), None, None, None,
                                     None) == _lib.VAG_E_INVALID


# ---- 2. the numpy statement against np.quantile ----

@pytest.fixture(scope="module")
def lognormal():
    rng = np.random.default_rng(20240607)
    return {S: rng.lognormal(mean=-60.0, sigma=3.0, size=(S, 5 if S == 4096 else 33)) for S in DRAWS}


def test_numpy_statement_against_np_quantile(lognormal):
    worst = 0.0
    for S, F in lognormal.items():
        got, ok, n = sampling.column_quantiles(F, LEVELS)
        want = np.quantile(F, LEVELS, axis=0)
        assert n == S and ok.all() and got.shape == want.shape == (len(LEVELS), F.shape[1])
        ulp = np.spacing(np.maximum(got, want))
        err = float(np.max(np.abs(got - want) / ulp))
        print("S", S, "max |statement - np.quantile| in ulp of the larger", err)
        worst = max(worst, err)
        assert err <= 4.0, (S, err)
        assert np.all(got[0] == F.min(axis=0)) and np.all(got[-1] == F.max(axis=0))
        assert np.all(np.diff(got, axis=0) >= 0)  # the levels ascend, so do the quantiles
    print("worst", worst)


# ---- 3. order statistics ----

def test_order_statistics_are_elements_of_the_input(lognormal):
    for S, F in lognormal.items():
        y = np.sort(F, axis=0)
        levels, ranks = [], []
        for lo in sorted({0, (S - 1) // 4, (S - 1) // 2, S - 1}):
            q = lo / (S - 1) if S > 1 else 0.5
            if sampling.quantile_rank(q, S) == (lo, 0.0):  # (a condition on the inputs: the one multiply lands on the integer)
                levels.append(q), ranks.append(lo)
        assert {0, S - 1} <= set(ranks)
        got, _, _ = sampling.column_quantiles(F, levels)
        assert same_bits(got, y[ranks])
    # the median of an odd number of draws, and a level whose product rounds to an integer though the level is not a ratio
    F = lognormal[101]
    assert same_bits(sampling.column_quantiles(F, [0.5, 0.16])[0], np.sort(F, axis=0)[[50, 16]])
    assert same_bits(sampling.column_quantiles(-F, [0.5])[0], -np.sort(F, axis=0)[[50]])
    # draws of more than two dimensions: the trailing ones are the columns
    cube = lognormal[64][:, :32].reshape(64, 4, 8)
    got, ok, n = sampling.column_quantiles(cube, LEVELS)
    assert got.shape == (7, 4, 8) and same_bits(got.reshape(7, 32), sampling.column_quantiles(cube.reshape(64, 32), LEVELS)[0])


# ---- 4. validity per draw ----

def test_validity_is_per_draw(lognormal):
    F = lognormal[65].copy()
    clean, _, _ = sampling.column_quantiles(np.delete(F, [7, 20, 41], axis=0), LEVELS)
    F[7, 3] = np.nan
    F[20, 0] = np.inf
    flags = np.ones(65, dtype=bool)
    flags[41] = False
    got, ok, n = sampling.column_quantiles(F, LEVELS, valid=flags)
    want_ok = np.ones(65, dtype=bool)
    want_ok[[7, 20, 41]] = False
    assert n == 62 and np.array_equal(ok, want_ok) and same_bits(got, clean)  # dropped for every column, not for their own alone
    assert same_bits(sampling.column_quantiles(F, LEVELS, valid=flags.astype(np.int32))[0], clean)
    F[20, 0] = -np.inf
    assert same_bits(sampling.column_quantiles(F, LEVELS, valid=flags)[0], clean)
    # every draw invalid
    got, ok, n = sampling.column_quantiles(F, LEVELS, valid=np.zeros(65, dtype=np.int32))
    assert n == 0 and not ok.any() and got.shape == (7, 33) and np.isnan(got).all()
    got, ok, n = sampling.column_quantiles(np.full((3, 2), np.nan), [0.5])
    assert n == 0 and not ok.any() and np.isnan(got).all()
    # one valid draw: every quantile is that draw
    one = np.zeros(65, dtype=bool)
    one[5] = True
    got, ok, n = sampling.column_quantiles(F, LEVELS, valid=one)
    assert n == 1 and same_bits(got, np.broadcast_to(F[5], (7, 33)))
    # zeros of either sign are +0
    z = np.array([[0.0], [-0.0], [-0.0]])
    assert same_bits(sampling.column_quantiles(z, [0.0, 0.5, 1.0])[0], np.zeros((3, 1)))


# ---- 5. refusals ----

def test_python_side_refusals():
    F = np.arange(12.0).reshape(4, 3)
    for bad in ([-0.1], [1.0000001], [0.5, float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match=r"every quantile must be in \[0, 1\]"):
            sampling.column_quantiles(F, bad)
    for bad in ([], np.linspace(0, 1, 17), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="between 1 and 16 quantiles"):
            sampling.column_quantiles(F, bad)
    assert sampling.column_quantiles(F, 0.5)[0].shape == (1, 3) and sampling.column_quantiles(F, np.linspace(0, 1, 16))[0].shape == (16, 3)
    with pytest.raises(ValueError, match="at least one draw and one column"):
        sampling.column_quantiles(np.zeros((0, 3)), [0.5])
    with pytest.raises(ValueError, match="at least one draw and one column"):
        sampling.column_quantiles(np.zeros((3, 0)), [0.5])
    with pytest.raises(ValueError, match="4097 draws exceed the maximum of 4096"):
        sampling.column_quantiles(np.zeros((4097, 1)), [0.5])
    with pytest.raises(ValueError, match="must be \\[draws, columns\\]"):
        sampling.column_quantiles(np.zeros(5), [0.5])
    for bad in (F.astype(np.float32), F.astype(np.int64)):
        with pytest.raises(ValueError, match="must be float64"):
            sampling.column_quantiles(bad, [0.5])
    for bad in (np.ones(3, dtype=bool), np.ones((4, 1), dtype=bool), np.ones(4)):
        with pytest.raises(ValueError, match="valid must be 4 flags"):
            sampling.column_quantiles(F, [0.5], valid=bad)
    with pytest.raises(ValueError, match="float64 torch tensor"):
        sampling.column_quantiles_device(F, [0.5])
    assert (sampling.PREDICT_MAX_DRAWS, sampling.PREDICT_MAX_Q, sampling.PREDICT_MAX_VALUES) == (4096, 16, 1 << 27)


def test_predict_refuses_before_any_device_is_looked_for():
    fitter = Fitter(z=0.1, lumi_dist=1e27)
    fitter.add_flux_density(1e9, np.array([1e4, 1e5]), np.array([1e-3, 2e-3]), np.array([1e-4, 2e-4]))
    defs = [ParamDef("theta_c", 0.02, 0.5, Scale.linear), ParamDef("E_iso", 1e50, 1e54, Scale.log)]
    samples = np.tile([0.1, 52.0], (10, 1))
    t, nu = np.array([1e4, 1e5]), np.array([1e9])
    with pytest.raises(ValueError, match=r"samples must be \[N, 2\]"):
        fitter.predict(np.zeros((10, 3)), defs, t, nu)
    with pytest.raises(ValueError, match=r"samples must be \[N, 2\]"):
        fitter.predict(np.zeros(2), defs, t, nu)
    with pytest.raises(ValueError, match="draws=11 exceeds the 10 rows"):
        fitter.predict(samples, defs, t, nu, draws=11)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="draws= must be a whole number"):
            fitter.predict(samples, defs, t, nu, draws=bad)
    with pytest.raises(ValueError, match="4097 samples exceed the 4096 draws of one call; pass draws="):
        fitter.predict(np.tile([0.1, 52.0], (4097, 1)), defs, t, nu)
    with pytest.raises(ValueError, match="draws=4097 exceeds the 4096 draws"):
        fitter.predict(np.tile([0.1, 52.0], (5000, 1)), defs, t, nu, draws=4097)
    with pytest.raises(ValueError, match="samples holds no row"):
        fitter.predict(np.zeros((0, 2)), defs, t, nu)
    with pytest.raises(ValueError, match=r"every quantile must be in \[0, 1\]"):
        fitter.predict(samples, defs, t, nu, quantiles=(0.5, 1.5))
    with pytest.raises(ValueError, match="between 1 and 16 quantiles"):
        fitter.predict(samples, defs, t, nu, quantiles=())
    for bad in (np.array([1e5, 1e4]), np.array([0.0, 1e4]), np.array([]), np.array([[1e4]]), np.array([1e4, np.nan])):
        with pytest.raises(ValueError, match="t must be a non-empty 1-D array"):
            fitter.predict(samples, defs, bad, nu)
    for bad in (np.array([-1e9]), np.array([]), np.array([np.inf])):
        with pytest.raises(ValueError, match="nu must be a non-empty 1-D array"):
            fitter.predict(samples, defs, t, bad)
    with pytest.raises(ValueError, match="exceed the 134217728 values of one call"):
        fitter.predict(np.tile([0.1, 52.0], (4096, 1)), defs, np.logspace(3, 7, 4097), np.logspace(9, 18, 8))
