"""Timing of the visibility path on one GPU (profiles/sky_visibility_timing.txt): Model.sky_visibilities of one C2 (configs[1])
model at 16 times, 1 frequency and 1024 baselines (n_az 1024) next to flux_density_grid and a 128x128 sky_image of the same model,
and vag_sky_visibility_batch for 512 jittered C2 models.  Median (min) of repeated host-pointer calls, model stages included.  Run
from the repository root: python profiles/visibility_timing.py"""
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
from vegasafterglow_amd import _lib  # noqa: E402

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
    t = np.geomspace(1e4, 1e7, 16)
    nu = np.array([3e9])
    rng = np.random.default_rng(7)
    nbl = 1024
    r, ang = 3e9 * np.sqrt(rng.uniform(0, 1, nbl)), rng.uniform(0, 2 * np.pi, nbl)
    u, v = r * np.cos(ang), r * np.sin(ang)
    m = va.Model.from_params(_abi.make_params(**configs.C2))
    mo = m.sky_moments(t, nu)
    fov = float(2 * np.nanmax(np.abs(mo.Xbar) + 3 * np.sqrt(mo.varX + mo.varY)))
    vis1 = timed(lambda: m.sky_visibilities(t, nu, u, v, n_az=1024), 9)
    grid1 = timed(lambda: m.flux_density_grid(t, nu), 9)
    img1 = timed(lambda: m.sky_image(t, nu, fov, npixel=128), 9)
    V = m.sky_visibilities(t, nu, u[:1] * 0, v[:1] * 0)
    cons1 = np.max(np.abs(V[0, :, 0].real - m.flux_density_grid(t, nu).total[0]) / m.flux_density_grid(t, nu).total[0])
    print(f"C2 (configs[1]) single model, 16 times, 1 frequency, {nbl} baselines, n_az 1024: Model.sky_visibilities median "
          f"{vis1[0]:.3f} ms (min {vis1[1]:.3f}); flux_density_grid median {grid1[0]:.3f} ms (min {grid1[1]:.3f}); "
          f"Model.sky_image 128x128 median {img1[0]:.3f} ms (min {img1[1]:.3f}); max |V(0, 0) - grid| / grid {cons1:.2e}", flush=True)
    nb = 512
    ps = []
    for _ in range(nb):
        kw = dict(configs.C2)
        kw["E_iso"] *= rng.uniform(0.8, 1.25)
        kw["theta_obs"] *= rng.uniform(0.9, 1.1)
        ps.append(_lib.ModelParams.from_buffer_copy(bytes(_abi.make_params(**kw))))
    arr = (_lib.ModelParams * nb)(*ps)
    U = np.ascontiguousarray(np.broadcast_to(u, (1, t.size, nbl)))
    W = np.ascontiguousarray(np.broadcast_to(v, (1, t.size, nbl)))
    out = np.empty((nb, 1, t.size, nbl, 2))
    grid = np.empty((nb, 1, t.size))
    a = (h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), 1)
    with lock:
        g = timed(lambda: _lib.check(lib.vag_flux_density_grid_batch(*a, grid.ctypes.data_as(dp))), 5)
        vb = timed(lambda: _lib.check(lib.vag_sky_visibility_batch(*a, U.ctypes.data_as(dp), W.ctypes.data_as(dp), nbl, 0.0, 1024,
                                                                   out.ctypes.data_as(dp))), 3)
    print(f"512 jittered C2 models, 16 times, 1 frequency, {nbl} baselines, n_az 1024: vag_sky_visibility_batch median {vb[0]:.3f} ms "
          f"(min {vb[1]:.3f}); vag_flux_density_grid_batch median {g[0]:.3f} ms (min {g[1]:.3f})", flush=True)


if __name__ == "__main__":
    main()
