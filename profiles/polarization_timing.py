"""Timing of the polarization path on one GPU (profiles/sky_polarization_timing.txt): vag_sky_polarization_batch against
vag_sky_moments_batch (the same parts) and vag_flux_density_grid_batch for 512 jittered C2 models at 16 times and 1 frequency, n_az 256,
in alternating runs, and one C2 model at 16 times against its flux_density_grid.  Median, min and max of repeated host-pointer
calls, model stages included.  Run from the repository root: python profiles/polarization_timing.py [--trace]
(--trace: two calls of the batch only, for a kernel trace of its own)."""
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


def stats(ts):
    return f"median {np.median(ts):.3f} ms (min {np.min(ts):.3f}, max {np.max(ts):.3f})"


def alternating(fns, reps):
    """Every function once per round, rounds repeated: [len(fns)][reps] milliseconds (after one untimed round)."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for q, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[q].append((time.perf_counter() - t0) * 1e3)
    return ts


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
    spec = (_lib.PolSpec * nb)()
    for s in spec:
        s.b[0], s.b[1], s.pi_max[0], s.pi_max[1] = 0.0, 0.0, -1.0, -1.0
    t = np.geomspace(1e4, 1e7, 16)
    nu = np.array([3e9])
    grid = np.empty((nb, 1, t.size))
    mom = np.empty((nb, 1, t.size, 6))
    pol = np.empty((nb, 1, t.size, 3))
    a = (h, arr, nb, t.ctypes.data_as(dp), t.size, nu.ctypes.data_as(dp), 1)
    f_pol = lambda: _lib.check(lib.vag_sky_polarization_batch(*a, spec, 0.0, 256, pol.ctypes.data_as(dp)))  # noqa: E731
    f_mom = lambda: _lib.check(lib.vag_sky_moments_batch(*a, 256, mom.ctypes.data_as(dp)))  # noqa: E731
    f_grid = lambda: _lib.check(lib.vag_flux_density_grid_batch(*a, grid.ctypes.data_as(dp)))  # noqa: E731
    if "--trace" in sys.argv:
        with lock:
            f_pol()
            f_pol()
        return
    with lock:
        tp, tm, tg = alternating([f_pol, f_mom, f_grid], 9)
    live = grid[:, 0] > 0
    cons = np.max(np.abs(pol[:, 0, :, 0] - grid[:, 0])[live] / grid[:, 0][live])
    print(f"512 jittered C2 models, 16 times, 1 frequency, n_az 256, 9 alternating rounds: vag_sky_polarization_batch {stats(tp)}; "
          f"vag_sky_moments_batch {stats(tm)}; vag_flux_density_grid_batch {stats(tg)}; polarization / moments "
          f"{np.median(tp) / np.median(tm):.2f}; max |I - grid| / grid {cons:.3g}; max Q / I {np.max(pol[..., 1][live[:, None]] / pol[..., 0][live[:, None]]):.3f}")
    m = va.Model.from_params(_abi.make_params(**configs.C2))
    one = alternating([lambda: m.sky_polarization(t, nu[0]), lambda: m.sky_moments(t, nu[0]), lambda: m.flux_density_grid(t, nu)], 9)
    print(f"one C2 model, 16 times, 1 frequency, n_az 256: Model.sky_polarization {stats(one[0])}; Model.sky_moments {stats(one[1])}; "
          f"Model.flux_density_grid {stats(one[2])}")


if __name__ == "__main__":
    main()
