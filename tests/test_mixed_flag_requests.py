"""A batch of mixed flags through the host-pointer entry points that tests/test_gpu_parity.py does not take one through: sky image,
sky moments, exact centroid, visibilities, polarization, Stokes image, band flux and band components.  The batch is A B A -- plain
synchrotron, one model with a reverse shock, plain synchrotron again with other parameters --, so the split has to put the rows of
the first group back around the second's.  Each model must come back bit for bit as in a call of its own (np.array_equal), the
per-model polarization spec with it.  The grids are the coarsest the sky tests use: nt = 3, nnu = 2, npixel = 8, n_az = 32,
nbl = 4, a band of 5 nodes."""
import ctypes as C

import numpy as np
import pytest

import _abi
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
T, NU = np.array([1e4, 1e5, 1e6]), np.array([1e9, 4.84e14])
NPIX, N_AZ, NBL, FOV, PA = 8, 32, 4, 3e-9, 0.3
KWS = [dict(jet="GaussianJet", theta_obs=0.2), dict(jet="TophatJet", theta_obs=0.1, duration=50.0, rvs=dict(eps_e=0.1, eps_B=0.01, p=2.3)),
       dict(jet="GaussianJet", theta_obs=0.3, n_ism=0.3)]
POL = [(0.0, 0.5, 0.7, -1.0), (0.5, 0.0, -1.0, 0.6), (2.0, 1.0, 0.3, 0.3)]  # per model: b fwd, b rvs, pi_max fwd, pi_max rvs
ST = NU.size * T.size


def p(a):
    return a.ctypes.data_as(dp)


def pol_specs(idx):
    arr = (_lib.PolSpec * len(idx))()
    for i, m in enumerate(idx):
        arr[i].b[0], arr[i].b[1], arr[i].pi_max[0], arr[i].pi_max[1] = POL[m]
    return arr


@pytest.fixture(scope="module")
def uv():
    rng = np.random.default_rng(5)
    return rng.uniform(-2e7, 2e7, (2, ST * NBL))


def requests(lib, h, uv):
    """name -> (per-model sizes of the outputs, call(params, nb, models' indices, outputs))."""
    grid = lambda a, nb: (h, a, nb, p(T), T.size, p(NU), NU.size)
    band = lambda a, nb: (h, a, nb, p(T), T.size, 1e14, 1e15, 5)
    return {
        "sky image": ([ST * NPIX * NPIX, ST], lambda a, nb, idx, o: lib.vag_sky_image_batch(*grid(a, nb), FOV, NPIX, N_AZ, p(o[0]), p(o[1]))),
        "sky moments": ([ST * 6], lambda a, nb, idx, o: lib.vag_sky_moments_batch(*grid(a, nb), N_AZ, p(o[0]))),
        "exact centroid": ([ST * 6], lambda a, nb, idx, o: lib.vag_sky_centroid_batch(*grid(a, nb), p(o[0]))),
        "visibility": ([ST * NBL * 2], lambda a, nb, idx, o: lib.vag_sky_visibility_batch(*grid(a, nb), p(uv[0]), p(uv[1]), NBL, PA, N_AZ, p(o[0]))),
        "polarization": ([ST * 3], lambda a, nb, idx, o: lib.vag_sky_polarization_batch(*grid(a, nb), pol_specs(idx), PA, N_AZ, p(o[0]))),
        "Stokes image": ([ST * 3 * NPIX * NPIX, ST * 3],
                         lambda a, nb, idx, o: lib.vag_sky_stokes_image_batch(*grid(a, nb), pol_specs(idx), FOV, NPIX, N_AZ, p(o[0]), p(o[1]))),
        "band flux": ([T.size], lambda a, nb, idx, o: lib.vag_flux_batch(*band(a, nb), p(o[0]))),
        "band components": ([T.size] * 4, lambda a, nb, idx, o: lib.vag_flux_components4_batch(*band(a, nb), (dp * 4)(*[p(x) for x in o]))),
    }


@pytest.mark.parametrize("name", ["sky image", "sky moments", "exact centroid", "visibility", "polarization", "Stokes image", "band flux",
                                  "band components"])
def test_a_mixed_batch_equals_one_call_per_model(name, uv):
    lib = _lib.load()
    h, _ = va.get_context(0)
    prms = [_abi.make_params(**kw) for kw in KWS]
    assert prms[0].flags == prms[2].flags != prms[1].flags
    sizes, call = requests(lib, h, uv)[name]

    def run(idx):
        arr = (_lib.ModelParams * len(idx))(*[_lib.ModelParams.from_buffer_copy(bytes(prms[m])) for m in idx])
        outs = [np.full((len(idx), n), np.nan) for n in sizes]
        _lib.check(call(arr, len(idx), idx, outs))
        return outs

    mixed = run([0, 1, 2])
    for m in range(3):
        for q, own in enumerate(run([m])):
            assert np.array_equal(mixed[q][m].view(np.uint64), own[0].view(np.uint64)), (name, m, q)  # the bits, a NaN's included
    assert np.nanmax(np.abs(mixed[0])) > 0 and not np.isnan(mixed[0]).all()
    if name == "band components":  # (a model without a reverse shock has zeros there, the one with it has not)
        assert mixed[2][0].max() == 0 and mixed[2][1].max() > 0
