"""Loader of the sky-image CPU checker (tests/sky_checker.c on top of the plain-C oracle) and the models of the sky-image tests."""
import ctypes as C
import os
import subprocess

import numpy as np

import _abi
import configs

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
pp = C.POINTER(_abi.ModelParams)

# (a) on-axis top hat, (b) the headline's off-axis Gaussian, (c) a spreading Gaussian on a full-circle grid, (d) the power-law jet in
# a wind with forward SSC only, (e) a top hat with a reverse shock, (f) the GW170817-like model
MODELS = {
    "a_c1a": dict(configs.C1A),
    "b_c2": dict(configs.C2),
    "c_spread_3d": dict(configs.SPREAD_CASES["gauss_spread"], jet="GaussianJet", axisymmetric=False),
    "d_c3_fwd_ssc": {k: v for k, v in configs.C3.items() if k != "rvs"},
    "e_rs_tophat": dict(configs.RS_CASES["rs_thin_tophat"][0]),
    "f_c4": dict(configs.C4_TRUTH),
}
AXISYMMETRIC = ("a_c1a", "b_c2", "d_c3_fwd_ssc", "e_rs_tophat", "f_c4")
T = np.geomspace(1e3, 1e7, 6)
NU = np.array([1e9, 4.84e14])


def params(name):
    return _abi.make_params(**MODELS[name])


class SkyChecker:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.sky_checker_image.argtypes = [pp, dp, C.c_int, dp, C.c_int, C.c_double, C.c_int, C.c_int, dp, dp]
        self.lib.sky_checker_moments.argtypes = [pp, dp, C.c_int, dp, C.c_int, C.c_int, dp]
        self.lib.vag_oracle_flux_density_grid.argtypes = [pp, dp, C.c_int, dp, C.c_int, dp]
        self.lib.vag_oracle_last_error.restype = C.c_char_p

    def _check(self, rc):
        if rc != 0:
            raise ValueError(self.lib.vag_oracle_last_error().decode())

    def image(self, p, t, nu, fov, npixel, n_az):
        t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
        img = np.zeros((nu.size, t.size, npixel, npixel))
        out = np.zeros((nu.size, t.size))
        self._check(self.lib.sky_checker_image(C.byref(p), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size, fov, npixel,
                                               n_az, img.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        return img, out

    def moments(self, p, t, nu, n_az):
        t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
        m = np.zeros((nu.size, t.size, 6))
        self._check(self.lib.sky_checker_moments(C.byref(p), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size, n_az,
                                                 m.ctypes.data_as(dp)))
        return m

    def flux_grid(self, p, t, nu):
        t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
        out = np.zeros((nu.size, t.size))
        self._check(self.lib.vag_oracle_flux_density_grid(C.byref(p), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                          out.ctypes.data_as(dp)))
        return out


def build_checker(out_dir):
    """Compile the checker with the oracle's flags into out_dir."""
    so = os.path.join(str(out_dir), "libsky_checker.so")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, "-std=c11", "-O2", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-shared", "-w",
                           "-I" + os.path.join(os.path.dirname(HERE), "include"), os.path.join(HERE, "sky_checker.c"), "-o", so, "-lm"])
    return SkyChecker(so)


def fov_for(m):
    """A field of view that holds most of the emission of every bin but cuts the outer parts of the widest ones."""
    s = np.sqrt(m[..., 3] + m[..., 4])
    ok = np.isfinite(s)
    return float(2 * np.median(np.abs(m[..., 1][ok]) + 1.5 * s[ok]))


def live_bins(ref, frac=1e-10):
    return ref > frac * ref.max()
