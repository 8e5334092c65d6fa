"""Timing of the visibility groups of the likelihood on one GPU (profiles/sky_visfit_timing.txt): a C4 likelihood call (3 bands x 20
epochs, as profiles/centroid_timing.py) without and with one visibility group of 4 epochs x 256 visibilities at n_az 1024 and 64,
for 1024 and 128 walkers, against what the engine could do for the same numbers before the fused pass: vag_sky_visibility_batch on
the walkers' parameter structs (one fixed pa, rectangular 4 x 256 baselines, host pointers) plus the chi^2 in numpy.  The variants
alternate in one process; median (min) of 9 repeats after a warm-up.  Run from the repository root: python profiles/visfit_timing.py
(`python profiles/visfit_timing.py kernels` runs one call of each of the two visibility kernels, for a kernel trace)."""
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
REPS = 9
VIS_T = np.array([75.0, 160.0, 230.0, 300.0]) * units.day
VIS_NU, NBL, PA = 8e9, 256, 0.3


def alternate(fns, reps=REPS):
    """Median and minimum [ms] of every fn, the fns taking turns (one warm-up round first)."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for q, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[q].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


def main(kernels_only=False):
    lib = _lib.load()
    h, lock = va.get_context(0)
    rng = np.random.default_rng(1)
    tr = configs.C4_TRUTH
    truth = va.Model.from_params(_abi.make_params(**tr))
    lc_t = np.geomspace(10, 300, 20) * units.day
    sm = truth.sky_moments(VIS_T, VIS_NU, n_az=1024)
    rho = np.sqrt(sm.Xbar ** 2 + sm.Ybar ** 2 + sm.varX + sm.varY)
    ang = rng.uniform(0, 2 * np.pi, NBL)
    b = 10.0 / (2 * np.pi * rho)[:, None] * np.linspace(0, 1, NBL)  # lengths up to 2 pi |b| rho = 10
    u, v = b * np.cos(ang), b * np.sin(ang)  # [4][256]
    V = truth.sky_visibilities(VIS_T, VIS_NU, u, v, pa=PA)
    V = V + 0.05 * sm.F[:, None] * (rng.standard_normal(V.shape) + 1j * rng.standard_normal(V.shape))
    err = np.repeat(0.05 * sm.F, NBL)

    def fitter(n_az):
        f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
        for band in configs.C4_BANDS:
            fl = truth.flux_density_grid(lc_t, band).total[0]
            f.add_flux_density(band, lc_t, fl, 0.1 * fl)
        if n_az:
            f.add_visibilities(VIS_NU, np.repeat(VIS_T, NBL), u.ravel(), v.ravel(), V.ravel(), err, n_az=n_az)
        return f
    fixed = [fitting.ParamDef(k, val, val, fitting.Scale.fixed) for k, val in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"], pa=PA).items()]
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed
    f0, f1024, f64 = fitter(0), fitter(1024), fitter(64)
    u3, v3 = np.ascontiguousarray(u[None]), np.ascontiguousarray(v[None])
    nu_arr = np.array([VIS_NU])
    for nw in ((128,) if kernels_only else (1024, 128)):
        th = np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                                   np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))
        arr = (_lib.ModelParams * nw)(*[_lib.ModelParams.from_buffer_copy(bytes(f0._params_at(s, defs[:3] + fixed[:-1])[0])) for s in th])
        out = np.empty((nw, 1, VIS_T.size, NBL, 2))
        chi2 = {}

        def composed(n_az):
            with lock:
                _lib.check(lib.vag_sky_visibility_batch(h, arr, nw, VIS_T.ctypes.data_as(dp), VIS_T.size, nu_arr.ctypes.data_as(dp), 1,
                                                        u3.ctypes.data_as(dp), v3.ctypes.data_as(dp), NBL, PA, n_az, out.ctypes.data_as(dp)))
            r = (out[:, 0, :, :, 0] + 1j * out[:, 0, :, :, 1]) - V
            chi2[n_az] = np.sum((r.real ** 2 + r.imag ** 2).reshape(nw, -1) / err ** 2, axis=1)
        ll = {}
        if kernels_only:
            composed(1024)
            ll[1024] = f1024.loglike_batch(th, defs)
            print(f"{nw} walkers: one call of each visibility kernel at n_az 1024 done")
            return
        fns = [lambda: ll.__setitem__(0, f0.loglike_batch(th, defs[:-1])), lambda: ll.__setitem__(1024, f1024.loglike_batch(th, defs)),
               lambda: ll.__setitem__(64, f64.loglike_batch(th, defs)), lambda: composed(1024), lambda: composed(64)]
        t0, t1024, t64, c1024, c64 = alternate(fns)
        fmt = lambda t: f"median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"  # noqa: E731
        print(f"{nw} C4 walkers, 3 bands x 20 epochs: likelihood call without visibility data {fmt(t0)}")
        for n_az, tf, tc in ((1024, t1024, c1024), (64, t64, c64)):
            agree = np.max(np.abs(-2 * (ll[n_az] - ll[0]) - chi2[n_az]) / chi2[n_az])
            print(f"  one group of 4 epochs x 256 visibilities, n_az {n_az}: likelihood call {fmt(tf)}: fused pass +{tf[0] - t0[0]:.3f} ms "
                  f"(min - min +{tf[1] - t0[1]:.3f}); vag_sky_visibility_batch + numpy chi^2 {fmt(tc)}; ratio composed / fused "
                  f"{tc[0] / (tf[0] - t0[0]):.2f}; max |chi^2 fused - composed| / chi^2 {agree:.3g}")


if __name__ == "__main__":
    main(len(sys.argv) > 1 and sys.argv[1] == "kernels")
