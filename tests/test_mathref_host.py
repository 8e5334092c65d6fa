"""CPU checks of the high-precision references in tests/_mathref.py, which tests/test_device_math.py holds the device math to:

1. the longdouble and mpmath (40 digits) evaluations of every reference agree;
2. the restated synchrotron spectrum, evaluated from the oracle's own break frequencies, is the oracle's compute_log2_I_nu on every
   cell of several synchrotron-only models (forward and reverse shocks) at probe frequencies from far below nu_a to beyond nu_M:
   the restatement is the pinned formula, not a reading of it."""
import numpy as np
import pytest

import _abi
import _mathref as R
import configs

needs_mp = pytest.mark.skipif(R.mpmath is None or not R.LD_OK, reason="one high-precision backend only: nothing to cross-check")


def _agree(f, *args, **kw):
    a = R.to_ld(f(*args, B=R.LD, **kw))
    b = R.to_ld(f(*args, B=R.MP, **kw))
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1, np.abs(b[fin])))) if fin.any() else 0.0


@needs_mp
def test_longdouble_and_mpmath_references_agree():
    rng = np.random.default_rng(11)
    with R.mpmath.workdps(40):
        x = np.concatenate([rng.uniform(-1074, 1023, 600), rng.uniform(-1, 1, 200), [0.0, -0.0, 1.0, -1022.5, 1023.5]])
        assert _agree(R.exp2, x) < 1e-18
        pos = np.concatenate([2.0 ** rng.uniform(-1070, 1020, 600), 1 + rng.uniform(-1e-3, 1e-3, 200), [1.0, 2.0 ** -1074]])
        assert _agree(R.log2, pos) < 1e-18
        assert _agree(R.rcp, pos) < 1e-18
        assert _agree(R.sqrt, pos) < 1e-18
        z = np.concatenate([rng.uniform(-25, 25, 800), [-20.0, 20.0, 0.0, np.inf, -np.inf, np.nan]])
        assert _agree(R.softplus, z) < 1e-18
        assert _agree(R.log2_1p_exp2, z[np.isfinite(z)]) < 1e-18
        n = 400
        lm = rng.uniform(20, 60, n)
        cells = dict(nu_m=2.0 ** lm, nu_c=2.0 ** (lm + rng.uniform(-15, 15, n)), nu_a=2.0 ** (lm + rng.uniform(-15, 15, n)),
                     nu_M=2.0 ** (lm + rng.uniform(20, 40, n)), I_max=2.0 ** rng.uniform(-120, 10, n),
                     p=rng.choice([1.5, 2.05, 2.3, 3.0, 3.5, 4.5], n))
        x = lm + rng.uniform(-30, 45, n)

        def spec(B):
            return R.log2_I_nu(R.photons_build(**cells, B=B), x, B=B)
        got = _agree(lambda B: spec(B))
        print(f"\n[mathref] longdouble vs mpmath: spectrum {got:.2e} (log2 units, relative to max(1, |value|))")
        assert got < 1e-17


# synchrotron-only models: (name, kwargs, t, reverse shock?)
MODELS = [("C1a", configs.C1A, False), ("C2", configs.C2, False), ("C4", configs.C4_TRUTH, False),
          ("gaussian_p_below_2", configs.EXTRA["gaussian_p_below_2"][0], False)] + \
         [(f"{k}:{'rs' if rvs else 'fs'}", configs.RS_CASES[k][0], rvs) for k in ("rs_thin_tophat", "rs_thick_offaxis")
          for rvs in (False, True)]


@pytest.mark.parametrize("name,kw,rvs", MODELS, ids=[m[0] for m in MODELS])
def test_restated_spectrum_is_the_oracles_on_every_cell(oracle, name, kw, rvs):
    prm = _abi.make_params(**kw)
    d0 = oracle.details(prm, 1e2, 1e7, rvs=rvs)
    lo = np.log2(np.nanmin(np.where(d0["nu_a"] > 0, d0["nu_a"], np.inf)))
    hi = np.log2(np.nanmax(d0["nu_M"]))
    probe = np.concatenate([np.linspace(lo - 12, hi + 4, 40), np.log2(np.median(d0["nu_m"])) + [-0.5, 0.0, 0.5]])
    d = oracle.details(prm, 1e2, 1e7, probe_lg2_nu=probe, rvs=rvs)
    p = prm.rvs_p if rvs else prm.p
    ok = np.isfinite(d["nu_m"]) & (d["nu_m"] > 0) & (d["I_nu_max"] > 0)
    assert ok.sum() > 50
    ph = R.photons_build(d["nu_m"][ok][:, None], d["nu_c"][ok][:, None], d["nu_a"][ok][:, None], d["nu_M"][ok][:, None],
                         d["I_nu_max"][ok][:, None], p)
    want = d["lg2_I_probe"][ok]
    errs = [np.abs(R.to_ld(R.log2_I_nu(ph, probe[None, :], side=s)) - want) for s in (None, -1, 1)]
    err = np.minimum.reduce(errs)
    fin = np.isfinite(want)
    assert fin.mean() > 0.9
    assert np.array_equal(fin, np.isfinite(R.to_ld(R.log2_I_nu(ph, probe[None, :]))))
    # log2 units; past |value| = 256 (a flux below 2^-256 of the peak: the exponential cut-off far beyond nu_M reaches -1e10) the
    # oracle's own rounding grows with the value, so the error is taken relative to max(1, |value| / 256) there
    worst = float(np.max(err[fin] / np.maximum(1, np.abs(want[fin]) / 256)))
    print(f"\n[mathref] {name}: {int(ok.sum())} cells x {probe.size} frequencies, restated vs oracle lg2_I_probe {worst:.2e} (log2 units)")
    assert worst <= 1e-12, worst
