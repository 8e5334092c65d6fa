"""Model.sky_polarization / Model.sky_stokes_image on the device (vag_sky_polarization_batch, vag_sky_stokes_image_batch, vag_sky.h)
against the CPU checker (tests/sky_pol_checker.c, INTEGRATION.md's bullet "Polarization"), the engine's own grid fluxes and sky
images, the symmetries of the definition, a pixel sum that does not go through the part logic of the new kernels; run-to-run bits,
batches (same and mixed flags) and the t-chunked path."""
import ctypes as C
import os

import numpy as np
import pytest

import _abi
import _polcheck as pk
import _skycheck as sk
import configs
import vegasafterglow_amd as va
from vegasafterglow_amd import _lib

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
N_AZ = 256
PA = 0.6
PARAMS = dict({n: sk.params(n) for n in sk.MODELS}, g_c3_full=_abi.make_params(**configs.C3),
              h_rs_offaxis=_abi.make_params(**dict(configs.RS_CASES["rs_thin_tophat"][0], theta_obs=0.15)))
SEVEN = list(sk.MODELS) + ["g_c3_full"]
MIRRORED = ["b_c2", "d_c3_fwd_ssc", "f_c4", "g_c3_full"]
ON_AXIS = ["a_c1a", "e_rs_tophat"]


def model(name):
    return va.Model.from_params(PARAMS[name])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return pk.build_checker(tmp_path_factory.mktemp("sky_pol_checker"))


def batch_pol(params, t, nu, specs, pa=0.0, n_az=0):
    """vag_sky_polarization_batch: out [nb][nnu][nt][3]."""
    lib = _lib.load()
    h, lock = va.get_context(0)
    nb = len(params)
    arr = (_lib.ModelParams * nb)(*[_lib.ModelParams.from_buffer_copy(bytes(p)) for p in params])
    sp = (_lib.PolSpec * nb)(*[_lib.PolSpec.from_buffer_copy(bytes(s)) for s in specs])
    out = np.empty((nb, nu.size, t.size, 3))
    with lock:
        _lib.check(lib.vag_sky_polarization_batch(h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size, sp, pa, n_az,
                                                  out.ctypes.data_as(dp)))
    return out


def iqu(r):
    return np.stack([r.I, r.Q, r.U], axis=-1)


@pytest.mark.parametrize("b", [0.0, 3.0])
@pytest.mark.parametrize("name", SEVEN)
def test_against_the_checker(name, b, checker):
    got = model(name).sky_polarization(sk.T, sk.NU, b=b, pa=PA, n_az=N_AZ)
    I, Q, U = checker.polarization(PARAMS[name], sk.T, sk.NU, N_AZ, pa=PA, b=b)
    ok = sk.live_bins(I)
    e_i = (np.abs(got.I - I) / I)[ok].max()
    e_qu = (np.maximum(np.abs(got.Q - Q), np.abs(got.U - U)) / I)[ok].max()
    print(name, "b", b, "max |dI| / I", e_i, "max(|dQ|, |dU|) / I", e_qu, "max |Q| / I", (np.abs(Q) / I)[ok].max())
    assert got.I.shape == (2, sk.T.size)
    assert e_i <= 1e-6 and e_qu <= 1e-6


@pytest.mark.parametrize("name", SEVEN)
def test_intensity_is_the_grid_flux(name):
    m = model(name)
    got = m.sky_polarization(sk.T, sk.NU, n_az=N_AZ)
    ref = m.flux_density_grid(sk.T, sk.NU).total
    live = sk.live_bins(ref)
    err = (np.abs(got.I - ref) / ref)[live].max()
    print(name, "max |I - F| / F", err)
    assert err <= 1e-12


@pytest.mark.parametrize("name", MIRRORED)
def test_u_vanishes_exactly_on_mirrored_grids(name):
    got = model(name).sky_polarization(sk.T, sk.NU, b=0.0, n_az=N_AZ)
    assert np.all(got.U == 0) and np.any(got.Q != 0)


@pytest.mark.parametrize("name", ON_AXIS)
def test_on_axis_is_unpolarized(name):
    got = model(name).sky_polarization(sk.T, sk.NU, b=0.0, pi_max=0.7, n_az=N_AZ)
    ok = sk.live_bins(got.I)
    print(name, "max |Q| / I", (np.abs(got.Q) / got.I)[ok].max(), "max |U| / I", (np.abs(got.U) / got.I)[ok].max())
    assert (np.abs(got.Q) / got.I)[ok].max() <= 1e-14 and (np.abs(got.U) / got.I)[ok].max() <= 1e-14


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d", "g_c3_full"])
def test_isotropic_field_pi_max_and_position_angle(name):
    m = model(name)
    iso = m.sky_polarization(sk.T, sk.NU, b=1.0, pa=PA, n_az=N_AZ)
    assert np.all(iso.Q == 0) and np.all(iso.U == 0) and np.any(iso.I > 0)
    a = m.sky_polarization(sk.T, sk.NU, b=0.0, pi_max=0.7, pi_max_rvs=0.7, pa=PA, n_az=N_AZ)
    h = m.sky_polarization(sk.T, sk.NU, b=0.0, pi_max=0.35, pi_max_rvs=0.35, pa=PA, n_az=N_AZ)
    assert np.array_equal(h.I, a.I) and np.array_equal(h.Q, 0.5 * a.Q) and np.array_equal(h.U, 0.5 * a.U)
    z = m.sky_polarization(sk.T, sk.NU, b=0.0, pi_max=0.7, pi_max_rvs=0.7, pa=0.0, n_az=N_AZ)
    c2, s2 = np.cos(2 * PA), np.sin(2 * PA)
    ok = sk.live_bins(z.I)
    assert np.array_equal(z.I, a.I)
    err = np.maximum(np.abs(a.Q - (z.Q * c2 - z.U * s2)), np.abs(a.U - (z.Q * s2 + z.U * c2))) / z.I
    assert err[ok].max() <= 1e-14
    assert np.allclose(a.angle[ok], 0.5 * np.arctan2(a.U, a.Q)[ok]) and np.allclose(a.degree[ok], (np.hypot(a.Q, a.U) / a.I)[ok])


@pytest.mark.parametrize("name", ["g_c3_full", "h_rs_offaxis"])
def test_emitters_add(name, checker):
    """(b, b_rvs) = (0, 1) polarizes the forward shock alone, (1, 0) the reverse shock alone; together they are (0, 0)."""
    m = model(name)
    fwd = m.sky_polarization(sk.T, sk.NU, b=0.0, b_rvs=1.0, n_az=N_AZ)
    rvs = m.sky_polarization(sk.T, sk.NU, b=1.0, b_rvs=0.0, n_az=N_AZ)
    both = m.sky_polarization(sk.T, sk.NU, b=0.0, b_rvs=0.0, n_az=N_AZ)
    ok = sk.live_bins(both.I)
    for x in ("Q", "U"):
        err = (np.abs(getattr(fwd, x) + getattr(rvs, x) - getattr(both, x)) / both.I)[ok].max()
        assert err <= 1e-13, (x, err)
    I, Q, _ = checker.polarization(PARAMS[name], sk.T, sk.NU, N_AZ, b=1.0, b_rvs=0.0)
    share_ref = (np.abs(Q) / I)[sk.live_bins(I)].max()
    share = (np.abs(rvs.Q) / rvs.I)[ok].max()
    print(name, "reverse shock alone: max |Q| / I", share, "checker", share_ref)
    assert share_ref >= 1e-6 and share >= 1e-6  # the reverse shock's share is there to be added
    assert np.any(fwd.Q != both.Q)


def stokes_maps(r):
    return np.stack([r.I, r.Q, r.U], axis=-3)


@pytest.mark.parametrize("name", ["b_c2", "c_spread_3d", "g_c3_full"])
def test_stokes_image(name, checker):
    m = model(name)
    t, nu = sk.T[1:5], sk.NU
    mo = m.sky_moments(t, nu, n_az=N_AZ)
    fov = sk.fov_for(np.stack([getattr(mo, n) for n in va.SkyMoments.names], axis=-1))
    npix = 96  # two tiles per side
    got = m.sky_stokes_image(t, nu, fov, npixel=npix, b=0.0, pi_max=0.7, n_az=N_AZ)
    plain = m.sky_image(t, nu, fov, npixel=npix, n_az=N_AZ)
    assert got.I.shape == (2, t.size, npix, npix) and got.outside.shape == (2, t.size, 3)
    assert np.array_equal(got.I, plain.image)
    want, want_out = checker.stokes_image(PARAMS[name], t, nu, fov, npix, N_AZ, b=0.0, pi_max=0.7)
    tot_i = want[:, :, 0].sum((-2, -1))
    err = (np.abs(got.Q - want[:, :, 1]).sum((-2, -1)) + np.abs(got.U - want[:, :, 2]).sum((-2, -1))) / tot_i
    print(name, "max (sum |dQ| + sum |dU|) / sum I", err[tot_i > 0].max())
    assert err[tot_i > 0].max() <= 1e-5 and np.any(tot_i > 0)
    whole = m.sky_polarization(t, nu, b=0.0, pi_max=0.7, pa=0.0, n_az=N_AZ)
    live = whole.I > 0
    tot = stokes_maps(got).sum((-2, -1)) + got.outside
    for q, x in enumerate("IQU"):
        e = (np.abs(tot[..., q] - getattr(whole, x))[live] / whole.I[live]).max()
        assert e <= 1e-12, (x, e)
    assert np.any(got.outside[..., 0] > 0) and np.any(got.U != 0)
    one = m.sky_stokes_image(t, nu[0], fov, npixel=npix, b=0.0, pi_max=0.7, n_az=N_AZ)
    assert one.Q.shape == (t.size, npix, npix) and np.array_equal(one.Q, got.Q[0]) and np.array_equal(one.outside, got.outside[0])


@pytest.mark.parametrize("name", ["b_c2", "f_c4"])
def test_angle_convention_against_a_pixel_sum(name, checker):
    """With pi_max = 1 and b = 1e12 every part is fully polarized along the projected radial direction, so Q = -sum w cos 2 psi: the
    same sum over the pixels of a plain 256^2 sky_image (psi at the pixel centres) checks the angle convention without the part logic
    of the polarization kernels.  One time at a time, the field of view fitted to it; the pixelation error is the checker's own (its
    image against its Q), the device is held to twice that plus 1e-6 I, and only times where the checker's error is <= 1e-3 I count."""
    m, p = model(name), PARAMS[name]
    nu = sk.NU[:1]
    kw = dict(b=1e12, pi_max=1.0)
    passed = []
    for i, t1 in enumerate(sk.T):
        t = np.array([t1])
        mo = m.sky_moments(t, nu, n_az=N_AZ)
        if not (mo.F[0, 0] > 0):
            continue
        fov = float(2 * (abs(mo.Xbar[0, 0]) + 4 * np.sqrt(mo.varX[0, 0] + mo.varY[0, 0])))
        ci, cout = checker.image(p, t, nu, fov, 256, N_AZ)
        cI, cQ, _ = checker.polarization(p, t, nu, N_AZ, **kw)
        ref_err = abs(pk.pixel_q(ci, fov)[0, 0] - cQ[0, 0]) / cI[0, 0]
        img = m.sky_image(t, nu, fov, npixel=256, n_az=N_AZ)
        got = m.sky_polarization(t, nu, n_az=N_AZ, **kw)
        dev_err = abs(pk.pixel_q(img.image, fov)[0, 0] - got.Q[0, 0]) / got.I[0, 0]
        print(name, f"t = {t1:.3g}: Q / I {got.Q[0, 0] / got.I[0, 0]:.4f}, pixel sum off by {dev_err:.3g} I, the checker's {ref_err:.3g} I")
        if ref_err <= 1e-3:
            passed.append(i)
            assert dev_err <= 2 * ref_err + 1e-6
    assert sk.T.size - 1 in passed


def test_bitwise_reproducible_batches_and_chunks():
    name = "b_c2"
    m = model(name)
    kw = dict(b=0.0, pi_max=0.7, pa=0.2, n_az=N_AZ)
    a = iqu(m.sky_polarization(sk.T, sk.NU, **kw))
    assert np.array_equal(a, iqu(m.sky_polarization(sk.T, sk.NU, **kw)))
    spec = pk.spec(b=0.0, pi_max=0.7)
    other = pk.spec(b=3.0)
    # a model alone against the same model inside a same-flag batch of 8, and inside a mixed-flag batch
    same = batch_pol([PARAMS["f_c4"], PARAMS[name]] * 4, sk.T, sk.NU, [other, spec] * 4, pa=0.2, n_az=N_AZ)
    assert all(np.array_equal(same[q], a) for q in (1, 3, 5, 7))
    assert np.array_equal(same[0], iqu(model("f_c4").sky_polarization(sk.T, sk.NU, b=3.0, pa=0.2, n_az=N_AZ)))
    names = SEVEN + ["h_rs_offaxis"]
    specs = [pk.spec(b=0.5 * q, pi_max=0.7, b_rvs=0.25 * q) for q in range(len(names))]
    mixed = batch_pol([PARAMS[n] for n in names], sk.T, sk.NU, specs, pa=0.2, n_az=N_AZ)
    for q, n in enumerate(names):
        alone = model(n).sky_polarization(sk.T, sk.NU, b=0.5 * q, pi_max=0.7, b_rvs=0.25 * q, pa=0.2, n_az=N_AZ)
        assert np.array_equal(mixed[q], iqu(alone)), n
    # the request cut along t
    whole_full = mixed[names.index("g_c3_full")]
    kw_full = dict(b=0.5 * names.index("g_c3_full"), pi_max=0.7, b_rvs=0.25 * names.index("g_c3_full"), pa=0.2, n_az=N_AZ)
    lib = _lib.load()
    fov = 2e-9
    maps = m.sky_stokes_image(sk.T, sk.NU, fov, npixel=32, b=0.0, pi_max=0.7, n_az=N_AZ)
    for chunk in ("1", "2"):
        os.environ["VAG_SKY_CHUNK_T"] = chunk
        lib.vag_reload_env_hooks()
        try:
            cut = iqu(m.sky_polarization(sk.T, sk.NU, **kw))
            cut_full = iqu(model("g_c3_full").sky_polarization(sk.T, sk.NU, **kw_full))
            cut_maps = m.sky_stokes_image(sk.T, sk.NU, fov, npixel=32, b=0.0, pi_max=0.7, n_az=N_AZ)
        finally:
            del os.environ["VAG_SKY_CHUNK_T"]
            lib.vag_reload_env_hooks()
        assert np.array_equal(cut, a), chunk
        assert np.array_equal(cut_full, whole_full), chunk
        assert np.array_equal(stokes_maps(cut_maps), stokes_maps(maps)) and np.array_equal(cut_maps.outside, maps.outside), chunk
    sc = m.sky_polarization(sk.T, sk.NU[1], **kw)
    assert sc.I.shape == (sk.T.size,) and np.array_equal(iqu(sc), a[1])


def test_c_abi_rejects_bad_specs():
    t, nu = sk.T, sk.NU
    for bad in (pk.spec(b=-1.0), pk.spec(b=float("nan")), pk.spec(pi_max=1.5), pk.spec(pi_max_rvs=float("nan")), pk.spec(b_rvs=float("inf"))):
        with pytest.raises(ValueError, match="pol"):
            batch_pol([PARAMS["b_c2"]], t, nu, [bad])
    with pytest.raises(ValueError, match="pa"):
        batch_pol([PARAMS["b_c2"]], t, nu, [pk.spec()], pa=float("nan"))
    lib = _lib.load()
    h, _ = va.get_context(0)
    assert lib.vag_sky_polarization_batch(h, None, 1, None, 0, None, 0, None, 0.0, 0, None) == _lib.VAG_E_INVALID
    assert lib.vag_sky_stokes_image_batch(h, None, 1, None, 0, None, 0, None, 1e-9, 8, 0, None, None) == _lib.VAG_E_INVALID
    assert lib.vag_sky_polarization_batch(None, None, 1, None, 0, None, 0, None, 0.0, 0, None) == _lib.VAG_E_INVALID
