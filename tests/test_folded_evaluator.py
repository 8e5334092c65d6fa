"""The boundary-spectrum evaluator reads three per-cell constants folded once by the cells kernel (vag_common.h: VP_BHI, VP_TB,
VP_LG2_I_SLO) and the interpolation's exp2 takes its non-finite exponents through one clamp (exp2_or_zero).  Both move bits only in
the last places: the headline batch (bench.py's seeded configs[1] models) must match what the library computed before the change
to 1e-13 relative, and the oracle to the usual 2e-6."""
import ctypes as C
import os

import numpy as np
import pytest

import _abi
import configs
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "headline_c2_batch512.npz")


def c2_batch_params(nb, seed):
    """bench.py's headline batch: configs[1] with +-10 % log-uniform jitter (seeded)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nb):
        kw = dict(configs.C2)
        j = lambda: float(np.exp(rng.uniform(np.log(0.9), np.log(1.1))))
        kw["E_iso"] *= j()
        kw["Gamma0"] *= j()
        kw["n_ism"] *= j()
        kw["eps_e"] *= j()
        kw["eps_B"] *= j()
        kw["p"] = 2.3 + rng.uniform(-0.1, 0.1)
        kw["theta_c"] *= j()
        out.append(_abi.make_params(**kw))
    return out


@pytest.fixture(scope="module")
def headline():
    ref = np.load(FIXTURE)
    prms = c2_batch_params(int(ref["n_models"]), int(ref["seed"]))
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    h, lock = va.get_context(0)
    arr = (_lib.ModelParams * len(prms))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in prms])
    t, nu = np.ascontiguousarray(configs.C2_T), np.ascontiguousarray(configs.C2_NU)
    out = np.empty((len(prms), nu.size, t.size))
    _lib.check(lib.vag_flux_density_grid_batch(h, arr, len(prms), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                               out.ctypes.data_as(dp)))
    return prms, ref, out


def test_headline_batch_matches_the_library_before_the_fold(headline):
    prms, ref, out = headline
    got, want = out[ref["models"]], ref["flux"]
    assert np.all(np.isfinite(got)) and np.array_equal(got > 0, want > 0)
    err = np.max(np.abs(got - want) / np.where(want > 0, want, 1.0))
    assert err < 1e-13, err


def test_headline_batch_matches_the_oracle(headline):
    prms, ref, out = headline
    orc = _abi.load_oracle()
    for i in (0, 257):
        want = orc.flux_density_grid(prms[i], configs.C2_T, configs.C2_NU)
        err = np.max(np.abs(out[i] - want) / want)
        assert err < 2e-6, (i, err)
