"""Sky visibilities on the host: the CPU checker (tests/sky_vis_checker.c) follows INTEGRATION.md's definition of
Model.sky_visibilities, and these tests pin the checker itself (V(0, 0) = F, the short-baseline expansion against the checker's own
moments, Hermitian symmetry) and the Python front end's argument checks, which run before any device is touched."""
import numpy as np
import pytest

import _skycheck as sk
import _vischeck as vk
import vegasafterglow_amd as va

pytestmark = pytest.mark.filterwarnings("ignore")
N_AZ = 64


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return vk.build_checker(tmp_path_factory.mktemp("sky_vis_checker"))


def _live(m):
    return np.isfinite(m[..., 1]) & (m[..., 0] > 1e-10 * m[..., 0].max())


@pytest.mark.parametrize("name", ["a_c1a", "b_c2", "c_spread_3d", "e_rs_tophat"])
def test_checker_zero_baseline_is_the_flux(checker, name):
    p = sk.params(name)
    m = checker.moments(p, sk.T, sk.NU, N_AZ)
    V = checker.visibility(p, sk.T, sk.NU, np.zeros(3), np.zeros(3), 0.3, N_AZ)
    ok = _live(m)
    F = m[..., 0][..., None]
    assert np.all(V.imag == 0)
    assert np.max(np.abs(V.real - F)[ok] / F[ok]) <= 1e-13


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d", "e_rs_tophat"])
@pytest.mark.parametrize("pa", [0.0, 0.7])
def test_checker_short_baselines_give_the_moments(checker, name, pa):
    """V = F - 2 pi i eps F <d.x> - 2 pi^2 eps^2 F <(d.x)^2> + O((2 pi eps rho)^3) along the direction d of a baseline of length eps."""
    p = sk.params(name)
    m = checker.moments(p, sk.T, sk.NU, N_AZ)
    ok = _live(m)
    rho = np.sqrt(m[..., 1] ** 2 + m[..., 2] ** 2 + m[..., 3] + m[..., 4])
    rho = np.where(ok, rho, 1.0)
    eps = 1e-3 / (2 * np.pi * rho)
    ang = np.array([0.0, 0.5, 1.3, 2.9])
    u = eps[..., None] * np.cos(ang)
    v = eps[..., None] * np.sin(ang)
    V = checker.visibility(p, sk.T, sk.NU, u, v, pa, N_AZ)
    F, X, Y, vx, vy, cxy = (m[..., q][..., None] for q in range(6))
    # the projection of a point on d = (cos a, sin a) in (east, north)
    ce = np.cos(ang) * np.sin(pa) + np.sin(ang) * np.cos(pa)  # coefficient of X
    cn = np.cos(ang) * np.cos(pa) - np.sin(ang) * np.sin(pa)  # coefficient of Y
    cen = ce * X + cn * Y
    second = ce ** 2 * (vx + X ** 2) + cn ** 2 * (vy + Y ** 2) + 2 * ce * cn * (cxy + X * Y)
    e = eps[..., None]
    got_cen = V.imag / (-2 * np.pi * e * F)
    got_second = (F - V.real) / (2 * np.pi ** 2 * e ** 2 * F)
    r = rho[..., None] * np.ones_like(ang)
    assert np.max((np.abs(got_cen - cen) / r)[ok]) <= 1e-5
    assert np.max((np.abs(got_second - second) / r ** 2)[ok]) <= 1e-5


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d"])
def test_checker_hermitian(checker, name):
    p = sk.params(name)
    m = checker.moments(p, sk.T, sk.NU, N_AZ)
    u, v = vk.baselines(m, 10.0, 9)
    a = checker.visibility(p, sk.T, sk.NU, u, v, 0.4, N_AZ)
    b = checker.visibility(p, sk.T, sk.NU, -u, -v, 0.4, N_AZ)
    F = m[..., 0][..., None]
    ok = _live(m)
    assert np.max((np.abs(b - np.conj(a)) / F)[ok]) <= 1e-14
    assert np.max((np.abs(a) / F)[ok]) <= 1 + 1e-14


def _model():
    return va.Model(va.GaussianJet(0.1, 1e52, 300), va.ISM(1.0), va.Observer(1e28, 1.0, 0.3), va.Radiation(0.1, 0.01, 2.3))


U1 = np.array([0.0, 1e8, 3e8])


@pytest.mark.parametrize("kw, msg", [
    (dict(t=[], nu=1e9, u=U1, v=U1), "time array must be non-empty"),
    (dict(t=[1e5, 1e4], nu=1e9, u=U1, v=U1), "ascending"),
    (dict(t=[1e5, np.inf], nu=1e9, u=U1, v=U1), "positive and finite"),
    (dict(t=[1e5], nu=[], u=U1, v=U1), "frequency array must be non-empty"),
    (dict(t=[1e5], nu=1e9, u=U1, v=U1, n_az=0), "n_az"),
    (dict(t=[1e5], nu=1e9, u=U1, v=U1, n_az=2.5), "n_az"),
    (dict(t=[1e5], nu=1e9, u=U1, v=U1[:2]), "same shape"),
    (dict(t=[1e5, 2e5], nu=[1e9, 2e9], u=np.zeros((2, 3, 4)), v=np.zeros((2, 3, 4))), r"\(nnu, nt, nbl\)"),
    (dict(t=[1e5], nu=1e9, u=np.zeros((1, 1, 1, 2)), v=np.zeros((1, 1, 1, 2))), r"\(nnu, nt, nbl\)"),
    (dict(t=[1e5], nu=1e9, u=np.zeros(0), v=np.zeros(0)), "baselines"),
    (dict(t=[1e5], nu=1e9, u=np.zeros(65537), v=np.zeros(65537)), "baselines"),
    (dict(t=[1e5], nu=1e9, u=np.array([0.0, np.nan]), v=np.zeros(2)), "finite"),
    (dict(t=[1e5], nu=1e9, u=np.zeros(2), v=np.array([np.inf, 0.0])), "finite"),
    (dict(t=[1e5], nu=1e9, u=U1, v=U1, pa=float("nan")), "pa"),
    (dict(t=[1e5], nu=1e9, u=U1, v=U1, pa=float("inf")), "pa"),
])
def test_sky_visibilities_argument_errors(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _model().sky_visibilities(**kw)


def test_sky_visibility_entry_point_is_exported():
    from vegasafterglow_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vag_sky_visibility_batch") and "vag_sky_visibility_batch" in _lib.EXPORTS
