"""Linear polarization on the host: the CPU checker (tests/sky_pol_checker.c) follows INTEGRATION.md's bullet "Polarization", and
these tests pin the checker itself (symmetry of on-axis models, the isotropic field, linearity in pi_max, the sign of Q with the field
anisotropy, I against the grid flux, maps against the integrated values) and the Python front end's argument checks, which run before
any device is touched."""
import numpy as np
import pytest

import _polcheck as pk
import _skycheck as sk
import vegasafterglow_amd as va

pytestmark = pytest.mark.filterwarnings("ignore")
N_AZ = 256


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return pk.build_checker(tmp_path_factory.mktemp("sky_pol_checker"))


@pytest.mark.parametrize("name", ["a_c1a", "e_rs_tophat"])
def test_checker_on_axis_is_unpolarized(checker, name):
    p = sk.params(name)
    I, Q, U = checker.polarization(p, sk.T, sk.NU, N_AZ, b=0.0, pi_max=0.7)
    ok = sk.live_bins(I)
    print(name, "max |Q|/I", np.max(np.abs(Q / I)[ok]), "max |U|/I", np.max(np.abs(U / I)[ok]))
    assert np.max(np.abs(Q / I)[ok]) <= 1e-14 and np.max(np.abs(U / I)[ok]) <= 1e-14


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d", "e_rs_tophat"])
def test_checker_isotropic_field_is_unpolarized(checker, name):
    I, Q, U = checker.polarization(sk.params(name), sk.T, sk.NU, N_AZ, pa=0.4, b=1.0, pi_max=0.7)
    assert np.all(Q == 0) and np.all(U == 0) and np.any(I > 0)


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d"])
def test_checker_is_linear_in_pi_max(checker, name):
    p = sk.params(name)
    a = checker.polarization(p, sk.T, sk.NU, N_AZ, pa=0.3, b=0.0, pi_max=0.7)
    h = checker.polarization(p, sk.T, sk.NU, N_AZ, pa=0.3, b=0.0, pi_max=0.35)
    assert np.array_equal(h[0], a[0]) and np.array_equal(h[1], 0.5 * a[1]) and np.array_equal(h[2], 0.5 * a[2])
    assert np.any(a[1] != 0)


@pytest.mark.parametrize("name", ["b_c2", "f_c4"])
def test_checker_sign_of_q_follows_the_anisotropy(checker, name):
    """A field in the shock plane (b = 0) polarizes an off-axis jet along the projected axis (Q > 0), a field mostly along the normal
    (b = 4) across it; on a mirrored grid U is exactly 0."""
    p = sk.params(name)
    I, Q0, U0 = checker.polarization(p, sk.T, sk.NU, N_AZ, b=0.0, pi_max=0.7)
    _, Q4, U4 = checker.polarization(p, sk.T, sk.NU, N_AZ, b=4.0, pi_max=0.7)
    ok = sk.live_bins(I)
    print(name, "Q/I at b = 0, nu = 1e9 Hz:", (Q0 / I)[0])
    assert np.all(Q0[ok] > 0) and np.all(Q4[ok] < 0)
    assert np.all(U0 == 0) and np.all(U4 == 0)
    assert np.max(np.abs(Q0 / I)[ok]) <= 0.7


@pytest.mark.parametrize("name", ["b_c2", "d_c3_fwd_ssc", "e_rs_tophat"])
def test_checker_intensity_is_the_grid_flux(checker, name):
    p = sk.params(name)
    I, _, _ = checker.polarization(p, sk.T, sk.NU, N_AZ)
    F = checker.flux_grid(p, sk.T, sk.NU)
    ok = sk.live_bins(F)
    assert np.max(np.abs(I - F)[ok] / F[ok]) <= 1e-12


def test_checker_default_pi_max_is_the_power_law_value(checker):
    p = sk.params("b_c2")
    a = checker.polarization(p, sk.T, sk.NU, N_AZ, b=0.0)
    b = checker.polarization(p, sk.T, sk.NU, N_AZ, b=0.0, pi_max=(p.p + 1) / (p.p + 7.0 / 3.0))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d"])
def test_checker_maps_add_up_to_the_integrated_values(checker, name):
    p = sk.params(name)
    t, nu = sk.T[2:5], sk.NU[:1]
    fov = sk.fov_for(checker.moments(p, t, nu, N_AZ))
    img, out = checker.stokes_image(p, t, nu, fov, 32, N_AZ, b=0.0, pi_max=0.7)
    I, Q, U = checker.polarization(p, t, nu, N_AZ, b=0.0, pi_max=0.7)
    plain, plain_out = checker.image(p, t, nu, fov, 32, N_AZ)
    assert np.array_equal(img[:, :, 0], plain) and np.array_equal(out[..., 0], plain_out)
    tot = img.sum((-2, -1)) + out
    for q, ref in enumerate((I, Q, U)):
        assert np.max(np.abs(tot[..., q] - ref) / I) <= 1e-12
    assert np.any(out[..., 0] > 0) and np.any(img[:, :, 2] != 0)


def test_checker_position_angle_turns_q_into_u(checker):
    p = sk.params("b_c2")
    I, Q, U = checker.polarization(p, sk.T, sk.NU, N_AZ, b=0.0, pi_max=0.7)
    for pa in (np.pi / 4, 1.1):
        _, Qs, Us = checker.polarization(p, sk.T, sk.NU, N_AZ, pa=pa, b=0.0, pi_max=0.7)
        assert np.max(np.abs(Qs - Q * np.cos(2 * pa)) / I) <= 1e-15 and np.max(np.abs(Us - Q * np.sin(2 * pa)) / I) <= 1e-15


def _model():
    return va.Model(va.GaussianJet(0.1, 1e52, 300), va.ISM(1.0), va.Observer(1e28, 1.0, 0.3), va.Radiation(0.1, 0.01, 2.3))


BAD = [
    (dict(t=[], nu=1e9), "time array must be non-empty"),
    (dict(t=[1e5, 1e4], nu=1e9), "ascending"),
    (dict(t=[1e5, np.inf], nu=1e9), "positive and finite"),
    (dict(t=[1e5], nu=[]), "frequency array must be non-empty"),
    (dict(t=[1e5], nu=[1e9, -1.0]), "frequencies must be positive"),
    (dict(t=[1e5], nu=1e9, n_az=0), "n_az"),
    (dict(t=[1e5], nu=1e9, n_az=2.5), "n_az"),
    (dict(t=[1e5], nu=1e9, b=-0.1), "b must be finite"),
    (dict(t=[1e5], nu=1e9, b=float("nan")), "b must be finite"),
    (dict(t=[1e5], nu=1e9, b=float("inf")), "b must be finite"),
    (dict(t=[1e5], nu=1e9, b_rvs=-1.0), "b_rvs must be finite"),
    (dict(t=[1e5], nu=1e9, b_rvs=float("inf")), "b_rvs must be finite"),
    (dict(t=[1e5], nu=1e9, pi_max=1.5), "pi_max must be in"),
    (dict(t=[1e5], nu=1e9, pi_max=-0.1), "pi_max must be in"),
    (dict(t=[1e5], nu=1e9, pi_max=float("nan")), "pi_max must be in"),
    (dict(t=[1e5], nu=1e9, pi_max_rvs=1.01), "pi_max_rvs must be in"),
]


@pytest.mark.parametrize("kw, msg", BAD + [
    (dict(t=[1e5], nu=1e9, pa=float("nan")), "pa must be finite"),
    (dict(t=[1e5], nu=1e9, pa=float("inf")), "pa must be finite"),
])
def test_sky_polarization_argument_errors(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _model().sky_polarization(**kw)


@pytest.mark.parametrize("kw, msg", BAD + [
    (dict(t=[1e5], nu=1e9, fov=0.0), "fov"),
    (dict(t=[1e5], nu=1e9, fov=float("nan")), "fov"),
    (dict(t=[1e5], nu=1e9, npixel=0), "npixel"),
    (dict(t=[1e5], nu=1e9, npixel=5000), "npixel"),
])
def test_sky_stokes_image_argument_errors(kw, msg):
    kw = dict(dict(fov=1e-8), **kw)
    with pytest.raises(ValueError, match=msg):
        _model().sky_stokes_image(**kw)


def test_sky_polarization_result_ratios():
    iqu = np.array([[2.0, 1.0, 1.0], [0.0, 0.0, 0.0], [4.0, -2.0, 0.0]])
    r = va.SkyPolarization(iqu, np.array([1.0, 2.0, 3.0]), 1e9)
    assert np.allclose(r.q[[0, 2]], [0.5, -0.5]) and np.allclose(r.u[[0, 2]], [0.5, 0.0])
    assert np.allclose(r.degree[[0, 2]], [np.sqrt(0.5), 0.5]) and np.allclose(r.angle[[0, 2]], [np.pi / 8, np.pi / 2])
    assert all(np.isnan(x[1]) for x in (r.q, r.u, r.degree, r.angle))


def test_sky_polarization_entry_points_are_exported():
    from vegasafterglow_amd import _lib
    lib = _lib.load()
    for name in ("vag_sky_polarization_batch", "vag_sky_stokes_image_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
