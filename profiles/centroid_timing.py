"""Timing of the exact-centroid path on one GPU (profiles/sky_centroid_timing.txt): vag_sky_centroid_batch against
vag_flux_density_grid_batch and vag_sky_moments_batch for 512 jittered C2 models at 16 times and 1 frequency, and the time one
4-epoch centroid group adds to a 1024-walker C4 likelihood call.  Median (min) of repeated host-pointer calls, model stages
included.  Run from the repository root: python profiles/centroid_timing.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _abi  # noqa: E402
import configs  # noqa: E402
import vegasafterglow_amd as va  # noqa: E402
from vegasafterglow_amd import _lib, fitting, units  # noqa: E402

dp = C.POINTER(C.c_double)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    lib = _lib.load()
    h, lock = va.get_context(0)
    rng = np.random.default_rng(1)
    nb = 512
    ps = []
    for _ in range(nb):
        kw = dict(configs.C2)
        kw["E_iso"] *= rng.uniform(0.8, 1.25)
        kw["theta_obs"] *= rng.uniform(0.9, 1.1)
        ps.append(_lib.ModelParams.from_buffer_copy(bytes(_abi.make_params(**kw))))
    arr = (_lib.ModelParams * nb)(*ps)
    t = np.geomspace(1e4, 1e7, 16)
    nu = np.array([3e9])
    grid = np.empty((nb, 1, t.size))
    cen = np.empty((nb, 1, t.size, 6))
    mom = np.empty((nb, 1, t.size, 6))
    a = (h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), 1)
    with lock:
        g = timed(lambda: _lib.check(lib.vag_flux_density_grid_batch(*a, grid.ctypes.data_as(dp))), 9)
        c = timed(lambda: _lib.check(lib.vag_sky_centroid_batch(*a, cen.ctypes.data_as(dp))), 9)
        m = timed(lambda: _lib.check(lib.vag_sky_moments_batch(*a, 0, mom.ctypes.data_as(dp))), 5)
    live = grid[:, 0] > 0
    cons = np.max(np.abs(cen[:, 0, :, 0] - grid[:, 0])[live] / grid[:, 0][live])
    ok = live & np.isfinite(mom[:, 0, :, 1])
    s = np.sqrt(cen[:, 0, :, 3] + cen[:, 0, :, 4])[ok]
    dx = np.max(np.abs(mom[:, 0, :, 1] - cen[:, 0, :, 1])[ok] / s)
    print(f"512 jittered C2 models, 16 times, 1 frequency: vag_sky_centroid_batch median {c[0]:.3f} ms (min {c[1]:.3f}); "
          f"vag_flux_density_grid_batch median {g[0]:.3f} ms (min {g[1]:.3f}); ratio {c[0] / g[0]:.2f}; "
          f"vag_sky_moments_batch (n_az 256) median {m[0]:.3f} ms (min {m[1]:.3f}); max |F - grid| / grid {cons:.3g}; "
          f"max |Xbar(n_az 256) - Xbar(exact)| / size {dx:.3g}")

    tr = configs.C4_TRUTH
    truth = va.Model.from_params(_abi.make_params(**tr))
    lc_t = np.geomspace(10, 300, 20) * units.day

    def fitter(with_c):
        f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
        for band in configs.C4_BANDS:
            fl = truth.flux_density_grid(lc_t, band).total[0]
            f.add_flux_density(band, lc_t, fl, 0.1 * fl)
        if with_c:
            ct = np.array([75.0, 160.0, 230.0, 300.0]) * units.day
            sm = truth.sky_moments(ct, 8e9, exact=True)
            e = np.full(ct.size, 0.2 * units.mas)
            f.add_centroid(8e9, ct, np.zeros(ct.size), sm.Xbar, e, e)
        return f
    fixed = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed
    nw = 1024
    th = np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                               np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))
    fa, fb = fitter(False), fitter(True)
    la = timed(lambda: fa.loglike_batch(th, defs), 9)
    lb = timed(lambda: fb.loglike_batch(th, defs), 9)
    print(f"1024 C4 walkers, 3 bands x 20 epochs: vag_loglike_batch median {la[0]:.3f} ms (min {la[1]:.3f}); with one 4-epoch "
          f"centroid group (vag_loglike_sky_batch) median {lb[0]:.3f} ms (min {lb[1]:.3f}): +{lb[0] - la[0]:.3f} ms")


if __name__ == "__main__":
    main()
