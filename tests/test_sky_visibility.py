"""Model.sky_visibilities on the device (vag_sky_visibility_batch, vag_sky.h) against the engine's own grid fluxes and moments, the
CPU checker (tests/sky_vis_checker.c, INTEGRATION.md's definition), the DFT of a fine sky image, its symmetries and its n_az
convergence; run-to-run bits, batches (same and mixed flags), the t-chunked path and broadcast baselines."""
import ctypes as C
import os

import numpy as np
import pytest

import _skycheck as sk
import _vischeck as vk
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
FIVE = ["a_c1a", "b_c2", "c_spread_3d", "d_c3_fwd_ssc", "e_rs_tophat"]
N_AZ = 256


def model(name):
    return va.Model.from_params(sk.params(name))


def mom_array(sm):
    return np.stack([getattr(sm, n) for n in va.SkyMoments.names], axis=-1)


def _live(m):
    return np.isfinite(m[..., 1]) & (m[..., 0] > 1e-10 * m[..., 0].max())


def _rho(m):
    r = np.sqrt(m[..., 1] ** 2 + m[..., 2] ** 2 + m[..., 3] + m[..., 4])
    return np.where(_live(m), r, 1.0)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return vk.build_checker(tmp_path_factory.mktemp("sky_vis_checker"))


@pytest.fixture(scope="module")
def moments():
    return {n: mom_array(model(n).sky_moments(sk.T, sk.NU, n_az=N_AZ)) for n in FIVE}


def batch_vis(params, t, nu, u, v, pa=0.0, n_az=0):
    lib = _lib.load()
    h, lock = va.get_context(0)
    nb = len(params)
    arr = (_lib.ModelParams * nb)(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in params])
    u, v = np.ascontiguousarray(u, float), np.ascontiguousarray(v, float)
    out = np.empty((nb, nu.size, t.size, u.shape[-1], 2))
    with lock:
        _lib.check(lib.vag_sky_visibility_batch(h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                u.ctypes.data_as(dp), v.ctypes.data_as(dp), u.shape[-1], pa, n_az,
                                                out.ctypes.data_as(dp)))
    return out[..., 0] + 1j * out[..., 1]


@pytest.mark.parametrize("name", FIVE)
def test_zero_baseline_is_the_grid_flux(name):
    m = model(name)
    V = m.sky_visibilities(sk.T, sk.NU, np.zeros(2), np.zeros(2))
    ref = m.flux_density_grid(sk.T, sk.NU).total
    live = sk.live_bins(ref)
    assert V.shape == (2, sk.T.size, 2) and V.dtype == np.complex128
    assert np.all(V.imag == 0)
    assert np.max(np.abs(V[..., 0].real - ref)[live] / ref[live]) <= 1e-12


@pytest.mark.parametrize("name", FIVE)
def test_against_the_checker(name, checker, moments):
    p = sk.params(name)
    u, v = vk.baselines(moments[name], 10.0, 24, seed=1)
    got = model(name).sky_visibilities(sk.T, sk.NU, u, v, pa=0.6, n_az=N_AZ)
    want = checker.visibility(p, sk.T, sk.NU, u, v, 0.6, N_AZ)
    F = checker.moments(p, sk.T, sk.NU, N_AZ)[..., 0][..., None]
    ok = _live(moments[name])
    err = (np.abs(got - want) / F)[ok]
    print(name, "max |dV| / F", err.max())
    assert err.max() <= 1e-6


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d", "d_c3_fwd_ssc"])
def test_short_baselines_give_the_moments(name, moments):
    m = moments[name]
    ok = _live(m)
    rho = _rho(m)
    eps = 1e-3 / (2 * np.pi * rho)
    ang = np.array([0.0, 0.5, 1.3, 2.9])
    pa = 0.4
    V = model(name).sky_visibilities(sk.T, sk.NU, eps[..., None] * np.cos(ang), eps[..., None] * np.sin(ang), pa=pa, n_az=N_AZ)
    F, X, Y, vx, vy, cxy = (m[..., q][..., None] for q in range(6))
    ce = np.cos(ang) * np.sin(pa) + np.sin(ang) * np.cos(pa)
    cn = np.cos(ang) * np.cos(pa) - np.sin(ang) * np.sin(pa)
    cen = ce * X + cn * Y
    second = ce ** 2 * (vx + X ** 2) + cn ** 2 * (vy + Y ** 2) + 2 * ce * cn * (cxy + X * Y)
    e, r = eps[..., None], rho[..., None]
    assert np.max((np.abs(V.imag / (-2 * np.pi * e * F) - cen) / r)[ok]) <= 1e-5
    assert np.max((np.abs((F - V.real) / (2 * np.pi ** 2 * e ** 2 * F) - second) / r ** 2)[ok]) <= 1e-5


@pytest.mark.parametrize("name", FIVE)
def test_hermitian_and_pa_rotation(name, moments):
    m = model(name)
    F = moments[name][..., 0][..., None]
    ok = _live(moments[name])
    u, v = vk.baselines(moments[name], 10.0, 16, seed=2)
    a = m.sky_visibilities(sk.T, sk.NU, u, v, pa=0.9)
    b = m.sky_visibilities(sk.T, sk.NU, -u, -v, pa=0.9)
    assert np.max((np.abs(b - np.conj(a)) / F)[ok]) <= 1e-14
    # PA = alpha with (u, v) equals PA = 0 with (u cos alpha - v sin alpha, u sin alpha + v cos alpha)
    al = 0.9
    c = m.sky_visibilities(sk.T, sk.NU, u * np.cos(al) - v * np.sin(al), u * np.sin(al) + v * np.cos(al), pa=0.0)
    assert np.max((np.abs(c - a) / F)[ok]) <= 1e-12


def test_on_axis_tophat_is_real_and_circular(moments):
    mo = moments["a_c1a"]
    ok = _live(mo)
    F = mo[..., 0][..., None]
    rho = _rho(mo)
    ang = np.linspace(0, 2 * np.pi, 7, endpoint=False)
    for turns in (0.5, 3.0, 10.0):
        b = turns / (2 * np.pi * rho)[..., None]
        V = model("a_c1a").sky_visibilities(sk.T, sk.NU, b * np.cos(ang), b * np.sin(ang), pa=0.3)
        assert np.max((np.abs(V.imag) / F)[ok]) <= 1e-9, turns
        assert np.max((np.abs(np.abs(V) - np.abs(V[..., :1])) / F)[ok]) <= 1e-9, turns


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d"])
def test_n_az_convergence(name, moments):
    """The midpoint parts at n_az = 1024 against 4096.  Per term the relative error is at most (dphi / S)^2 / 24 ((k rho)^2 + k rho),
    k = 2 pi |b|, dphi / S <= 2 pi / n_az, rho = max(|b|, |c|) of the term; rho is bounded by the farthest pixel corner of an image
    that holds every part."""
    m = model(name)
    mo = moments[name]
    F = mo[..., 0][..., None]
    s = np.sqrt(mo[..., 3] + mo[..., 4])
    fov = float(2 * np.nanmax(np.abs(mo[..., 1]) + np.abs(mo[..., 2]) + 30 * s))
    npix = 128
    si = m.sky_image(sk.T, sk.NU, fov, npixel=npix, n_az=1024)
    corner = np.abs(-fov / 2 + np.arange(npix + 1) * fov / npix)
    cmax = np.maximum(corner[:-1], corner[1:])
    r_pix = np.hypot(cmax[:, None], cmax[None, :])  # [iy][ix]
    rho = np.where(si.image > 0, r_pix, 0.0).max((-2, -1))
    ok = _live(mo) & (si.outside == 0)
    assert ok.sum() >= 0.5 * _live(mo).sum()
    u, v = vk.baselines(mo, 10.0, 16, seed=3)
    a = m.sky_visibilities(sk.T, sk.NU, u, v)  # n_az default 1024
    b = m.sky_visibilities(sk.T, sk.NU, u, v, n_az=4096)
    kr = 2 * np.pi * np.hypot(u, v) * rho[..., None]
    bound = (2 * np.pi / 1024) ** 2 / 24 * (kr ** 2 + kr) * (1 + 1 / 16)
    err = np.abs(a - b) / F
    print(name, "max |V1024 - V4096| / F", err[ok].max(), "at the longest baseline: max err / bound", (err / bound)[..., -1][ok].max())
    assert np.all(err[ok] <= bound[ok] + 1e-12)  # (+ the rounding of sums over 1024 and 4096 parts per ring)
    assert np.max(err[ok]) > 1e-9  # the parts have not converged yet at the longest baselines


def test_dft_of_a_fine_image():
    """The DFT of a 256^2 image (parts at their pixel centres) differs from V by at most sqrt(2) pi |b| Delta F, plus the weight
    outside the image."""
    name, t, nu = "b_c2", sk.T[2:4], np.array([1e9])
    m = model(name)
    mo = mom_array(m.sky_moments(t, nu, n_az=1024))
    s = np.sqrt(mo[..., 3] + mo[..., 4])
    fov = float(2 * np.max(np.abs(mo[..., 1]) + np.abs(mo[..., 2]) + 10 * s))
    npix = 256
    si = m.sky_image(t, nu, fov, npixel=npix, n_az=1024)
    F = mo[..., 0]
    assert np.max(si.outside / F) <= 1e-3
    delta = fov / npix
    xc = -fov / 2 + (np.arange(npix) + 0.5) * delta
    ang = np.linspace(0, np.pi, 5)
    lens = np.array([0.02, 0.05, 0.1]) / delta
    u = (lens[:, None] * np.cos(ang)).ravel()
    v = (lens[:, None] * np.sin(ang)).ravel()
    V = m.sky_visibilities(t, nu, u, v, n_az=1024)
    # PA = 0: east = Y (rows), north = X (columns)
    ph_y = np.exp(-2j * np.pi * u[:, None] * xc[None, :])  # [nbl][iy]
    ph_x = np.exp(-2j * np.pi * v[:, None] * xc[None, :])  # [nbl][ix]
    Vimg = np.einsum("lty x,by,bx->ltb".replace(" ", ""), si.image, ph_y, ph_x)
    bound = np.sqrt(2) * np.pi * np.hypot(u, v) * delta * F[..., None] + si.outside[..., None]
    print("max |V_dft - V| / bound", np.max(np.abs(Vimg - V) / bound))
    assert np.all(np.abs(Vimg - V) <= bound)


def test_bitwise_reproducible_batches_chunks_and_broadcast(moments):
    name = "b_c2"
    m = model(name)
    u1, v1 = vk.baselines(moments[name], 10.0, 70, seed=4)  # more than one block of 64 baselines
    a = m.sky_visibilities(sk.T, sk.NU, u1, v1, pa=0.2)
    assert np.array_equal(a, m.sky_visibilities(sk.T, sk.NU, u1, v1, pa=0.2))
    # a model alone against the same model inside a same-flag batch, and inside a mixed-flag batch
    same = batch_vis([sk.params("f_c4"), sk.params(name), sk.params(name)], sk.T, sk.NU, u1, v1, pa=0.2)
    assert np.array_equal(same[1], a) and np.array_equal(same[2], a)
    mixed = batch_vis([sk.params(n) for n in FIVE], sk.T, sk.NU, u1, v1, pa=0.2)
    for q, n in enumerate(FIVE):
        assert np.array_equal(mixed[q], model(n).sky_visibilities(sk.T, sk.NU, u1, v1, pa=0.2)), n
    # one time per chunk against one pass
    lib = _lib.load()
    os.environ["VAG_SKY_CHUNK_T"] = "1"
    lib.vag_reload_env_hooks()
    try:
        cut = m.sky_visibilities(sk.T, sk.NU, u1, v1, pa=0.2)
    finally:
        del os.environ["VAG_SKY_CHUNK_T"]
        lib.vag_reload_env_hooks()
    assert np.array_equal(cut, a)
    # 1-D baselines against the same values broadcast to (nnu, nt, nbl), and a scalar frequency
    w = np.linspace(-3e9, 3e9, 40)
    one = m.sky_visibilities(sk.T, sk.NU, w, w[::-1])
    full = m.sky_visibilities(sk.T, sk.NU, np.broadcast_to(w, (2, sk.T.size, 40)), np.broadcast_to(w[::-1], (2, sk.T.size, 40)))
    assert np.array_equal(one, full)
    sc = m.sky_visibilities(sk.T, sk.NU[0], w, w[::-1])
    assert sc.shape == (sk.T.size, 40) and np.array_equal(sc, one[0])
