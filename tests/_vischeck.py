"""Loader of the visibility CPU checker (tests/sky_vis_checker.c, which includes tests/sky_checker.c) with _skycheck's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

import _skycheck as sk

dp = C.POINTER(C.c_double)


class VisChecker(sk.SkyChecker):
    def __init__(self, path):
        super().__init__(path)
        self.lib.sky_checker_visibility.argtypes = [sk.pp, dp, C.c_int, dp, C.c_int, dp, dp, C.c_int, C.c_double, C.c_int, dp]

    def visibility(self, p, t, nu, u, v, pa, n_az):
        """V [nnu][nt][nbl] complex for u, v [nnu][nt][nbl] (or (nbl,), broadcast)."""
        t, nu = np.ascontiguousarray(t, float), np.ascontiguousarray(nu, float)
        shape = (nu.size, t.size, np.shape(u)[-1])
        u = np.ascontiguousarray(np.broadcast_to(np.asarray(u, float), shape))
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, float), shape))
        out = np.zeros(shape + (2,))
        self._check(self.lib.sky_checker_visibility(C.byref(p), t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), nu.size,
                                                    u.ctypes.data_as(dp), v.ctypes.data_as(dp), shape[2], pa, n_az,
                                                    out.ctypes.data_as(dp)))
        return out[..., 0] + 1j * out[..., 1]


def build_checker(out_dir):
    """Compile the visibility checker with _skycheck.build_checker's flags into out_dir."""
    so = os.path.join(str(out_dir), "libsky_vis_checker.so")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, "-std=c11", "-O2", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-shared", "-w",
                           "-I" + os.path.join(os.path.dirname(sk.HERE), "include"), os.path.join(sk.HERE, "sky_vis_checker.c"), "-o",
                           so, "-lm"])
    return VisChecker(so)


def baselines(ref_m, turns, nbl, seed=0):
    """u, v [nnu][nt][nbl] of random directions whose lengths reach 2 pi |b| rho = turns, rho the slot's extent from moments ref_m."""
    rho = np.sqrt(ref_m[..., 1] ** 2 + ref_m[..., 2] ** 2 + ref_m[..., 3] + ref_m[..., 4])
    rho = np.where(np.isfinite(rho) & (rho > 0), rho, np.nanmax(rho))
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, nbl)
    frac = np.linspace(0, 1, nbl)
    b = turns / (2 * np.pi * rho)[..., None] * frac
    return b * np.cos(ang), b * np.sin(ang)
