"""Loader of the polarization CPU checker (tests/sky_pol_checker.c, which includes tests/sky_checker.c) with _skycheck's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

import _skycheck as sk

dp = C.POINTER(C.c_double)


class PolSpec(C.Structure):  # vag_pol_spec
    _fields_ = [("b", C.c_double * 2), ("pi_max", C.c_double * 2)]


def spec(b=0.0, pi_max=None, b_rvs=None, pi_max_rvs=None):
    """Model.sky_polarization's defaults: b_rvs = b, a pi_max of None from the shock's own p (-1 in the spec)."""
    s = PolSpec()
    s.b[0], s.b[1] = b, b if b_rvs is None else b_rvs
    s.pi_max[0] = -1.0 if pi_max is None else pi_max
    s.pi_max[1] = -1.0 if pi_max_rvs is None else pi_max_rvs
    return s


class PolChecker(sk.SkyChecker):
    def __init__(self, path):
        super().__init__(path)
        ps = C.POINTER(PolSpec)
        self.lib.sky_checker_polarization.argtypes = [sk.pp, dp, C.c_int, dp, C.c_int, ps, C.c_double, C.c_int, dp]
        self.lib.sky_checker_stokes_image.argtypes = [sk.pp, dp, C.c_int, dp, C.c_int, ps, C.c_double, C.c_int, C.c_int, dp, dp]

    def polarization(self, p, t, nu, n_az, pa=0.0, **kw):
        """I, Q, U on the sky, each [nnu][nt]."""
        t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
        out = np.zeros((nu.size, t.size, 3))
        s = spec(**kw)
        self._check(self.lib.sky_checker_polarization(C.byref(p), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                      C.byref(s), pa, n_az, out.ctypes.data_as(dp)))
        return out[..., 0], out[..., 1], out[..., 2]

    def stokes_image(self, p, t, nu, fov, npixel, n_az, **kw):
        """maps [nnu][nt][3][npixel][npixel] and outside [nnu][nt][3] in the jet frame."""
        t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
        img = np.zeros((nu.size, t.size, 3, npixel, npixel))
        out = np.zeros((nu.size, t.size, 3))
        s = spec(**kw)
        self._check(self.lib.sky_checker_stokes_image(C.byref(p), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                      C.byref(s), fov, npixel, n_az, img.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        return img, out


def build_checker(out_dir):
    """Compile the polarization checker with _skycheck.build_checker's flags into out_dir."""
    so = os.path.join(str(out_dir), "libsky_pol_checker.so")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, "-std=c11", "-O2", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-shared", "-w",
                           "-I" + os.path.join(os.path.dirname(sk.HERE), "include"), os.path.join(sk.HERE, "sky_pol_checker.c"), "-o",
                           so, "-lm"])
    return PolChecker(so)


def pixel_q(image, fov):
    """-sum I_pix cos 2 psi_pix over an I map [..., npixel, npixel], psi at the pixel centres: the Q of a map fully polarized along the
    projected radial direction (Pi = 1), independent of any part logic."""
    n = image.shape[-1]
    c = (np.arange(n) + 0.5) * (fov / n) - fov / 2
    X, Y = np.meshgrid(c, c)  # [iy][ix]
    r2 = X ** 2 + Y ** 2
    return -(image * ((X ** 2 - Y ** 2) / r2)).sum((-2, -1))
