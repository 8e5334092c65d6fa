"""The persistent, cost-ordered launch of the grid flux kernel changes where and when a (model, block of rows) item runs, never
what it sums or in which order: every result must be bit-for-bit the one of the launch with a workgroup per item
(VAG_FLUX_PERSISTENT=0).  The product takes the persistent form only for large launches of long items; the small cases here force
it (VAG_FLUX_PERSISTENT=2)."""
import ctypes as C

import numpy as np
import pytest

import _abi
import configs
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
OLD = {"VAG_FLUX_PERSISTENT": "0"}


@pytest.fixture(scope="module")
def eng():
    lib = _lib.load()  # raises if the HIP library is missing: no silent fallback
    h, lock = va.get_context(0)
    return lib, h


def grid(eng, prms, t, nu):
    lib, h = eng
    arr = (_lib.ModelParams * len(prms))(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in prms])
    t = np.ascontiguousarray(t, dtype=np.float64)
    nu = np.ascontiguousarray(nu, dtype=np.float64)
    out = np.empty((len(prms), nu.size, t.size))
    _lib.check(lib.vag_flux_density_grid_batch(h, arr, len(prms), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                               out.ctypes.data_as(dp)))
    return out


def scramble(eng):
    """A call of another shape, so that neither run below finds partial grids of its own shape left in the context's buffers (an
    item the launch skipped would then read as garbage, not as the other run's value)."""
    grid(eng, jittered(dict(configs.C2, resolutions=(0.2, 0.7, 12.0)), 3, seed=99), np.logspace(3, 7, 13), np.array([1e10, 1e15]))


def new_and_old(run, capfd, extra=None, force=True):
    """run() with the persistent launch (forced, or where the product takes it) and with the one-workgroup-per-item launch (both
    under the hooks in `extra`); asserts from the launch report that each run took the form it is meant to."""
    extra = dict(extra or {})
    extra["VAG_DEBUG_LAUNCH"] = "1"
    if force:
        extra["VAG_FLUX_PERSISTENT"] = "2"
    for k, v in extra.items():
        _lib.hooks[k] = v
    try:
        scramble(eng=run.eng)
        capfd.readouterr()
        new = run()
        err = capfd.readouterr().err
        assert "grid flux form: persistent" in err and "grid flux form: one item" not in err, err
        for k, v in OLD.items():
            _lib.hooks[k] = v
        scramble(eng=run.eng)
        capfd.readouterr()
        old = run()
        err = capfd.readouterr().err
        assert "grid flux form: one item" in err and "grid flux form: persistent" not in err, err
    finally:
        for k in OLD:
            _lib.hooks.pop(k, None)
        for k in extra:
            _lib.hooks.pop(k, None)
    return new, old


def jittered(kw0, nb, seed):
    """bench.py's batch: +-10 % log-uniform jitter of the physical parameters (seeded)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nb):
        kw = dict(kw0)
        j = lambda: float(np.exp(rng.uniform(np.log(0.9), np.log(1.1))))
        for name in ("E_iso", "Gamma0", "n_ism", "eps_e", "eps_B", "theta_c"):
            if name in kw:
                kw[name] *= j()
        kw["p"] = kw.get("p", 2.3) + rng.uniform(-0.1, 0.1)
        out.append(_abi.make_params(**kw))
    return out


def assert_bits(new, old):
    assert np.all(np.isfinite(new)) and new.max() > 0
    assert np.array_equal(new, old)


class Run:
    def __init__(self, eng, prms, t, nu):
        self.eng, self.prms, self.t, self.nu = eng, prms, t, nu

    def __call__(self):
        return grid(self.eng, self.prms, self.t, self.nu)


def test_bench_batch_is_bitwise_unchanged(eng, capfd):
    """The product's own choice: the bench batch takes the persistent form without being forced."""
    prms = jittered(configs.C2, 512, seed=0)
    new, old = new_and_old(Run(eng, prms, configs.C2_T, configs.C2_NU), capfd, force=False)
    assert_bits(new, old)


def test_ragged_batch_in_pieces_is_bitwise_unchanged(eng, capfd):
    """Mixed resolutions (rows and lattices of different lengths, so a cost order that is not the model order), staged in pieces
    of 12 lattice nodes."""
    prms = []
    for i, res in enumerate([(0.3, 1.0, 10.0), (0.15, 0.5, 10.0), (0.3, 1.0, 20.0), (0.2, 2.0, 5.0)] * 3):
        prms += jittered(dict(configs.C2, resolutions=res), 1, seed=10 + i)
    t, nu = np.logspace(2.5, 7.5, 37), np.array([1e9, 4.84e14, 1e18])
    new, old = new_and_old(Run(eng, prms, t, nu), capfd, {"VAG_FLUX_K_CAP": "12"})
    assert_bits(new, old)


def test_spreading_jet_is_bitwise_unchanged(eng, capfd):
    prms = jittered(dict(jet="GaussianJet", theta_obs=0.25, spreading=True), 6, seed=3)
    t, nu = np.logspace(2.5, 7.5, 40), np.array([1e9, 4.84e14, 1e18])
    new, old = new_and_old(Run(eng, prms, t, nu), capfd)
    assert_bits(new, old)


@pytest.mark.parametrize("form", ["VAG_FORCE_FUSED", "VAG_NO_FUSED"])
def test_ssc_is_bitwise_unchanged(eng, capfd, form):
    prms = jittered(dict(configs.C1B, ssc=True, kn=True), 4, seed=5)
    t, nu = np.logspace(2.5, 7.5, 30), np.array([1e9, 4.84e14, 1e18, 1e24])
    new, old = new_and_old(Run(eng, prms, t, nu), capfd, {form: "1"})
    assert_bits(new, old)


def test_batch_smaller_than_the_resident_workgroups_is_bitwise_unchanged(eng, capfd):
    prms = jittered(configs.C2, 2, seed=7)
    new, old = new_and_old(Run(eng, prms, configs.C2_T, configs.C2_NU), capfd)
    assert_bits(new, old)
