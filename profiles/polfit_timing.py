"""What a polarization group costs in the walker likelihood on one GPU (profiles/polfit_timing.json): at 1024 and 8192 walkers
on the C4 fit (3 bands x 20 epochs), a host-pointer likelihood call without sky data, with one centroid group of four epochs, and
with one polarization group of the same epochs at n_az 256 and 64.  The four are timed in alternating repeats (one call of each
per round, each call ends in a device synchronise); medians, minima and maxima in ms.  --trace: one warmed call per fitter at
1024 walkers, for a kernel trace of its own.  Run from the repository root: python profiles/polfit_timing.py [--out FILE]"""
import argparse
import json
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
from vegasafterglow_amd import fitting, units  # noqa: E402

EPOCHS = np.array([75.0, 160.0, 230.0, 400.0]) * units.day


def fitters():
    tr = configs.C4_TRUTH
    truth = va.Model.from_params(_abi.make_params(**tr))
    lc_t = np.geomspace(10, 300, 20) * units.day
    pol = truth.sky_polarization(EPOCHS, 3e9, b=0.5, pa=0.3)
    sm = truth.sky_moments(EPOCHS, 8e9, exact=True)

    def fitter(kind):
        f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
        for band in configs.C4_BANDS:
            fl = truth.flux_density_grid(lc_t, band).total[0]
            f.add_flux_density(band, lc_t, fl, 0.1 * fl)
        if kind == "centroid":
            e = np.full(EPOCHS.size, 0.2 * units.mas)
            f.add_centroid(8e9, EPOCHS, sm.Xbar * np.sin(0.3), sm.Xbar * np.cos(0.3), e, e)
        elif kind.startswith("pol"):
            e = np.full(EPOCHS.size, 0.01)
            f.add_polarization(3e9, EPOCHS, pol.q, pol.u, e, e, n_az=int(kind[3:]))
        return f
    fixed = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    flux = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)]
    pa = fitting.ParamDef("pa", -1.0, 1.0)
    defs = {"none": flux + fixed, "centroid": flux + [pa] + fixed}
    defs["pol256"] = defs["pol64"] = flux + [pa, fitting.ParamDef("pol_b", 0.0, 3.0)] + fixed
    return {k: (fitter(k), d) for k, d in defs.items()}


def walkers(nw, rng):
    tr = configs.C4_TRUTH
    th = np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                          np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw), rng.uniform(0.0, 0.6, nw), rng.uniform(0.2, 0.8, nw)])
    return {"none": np.ascontiguousarray(th[:, :3]), "centroid": np.ascontiguousarray(th[:, :4]), "pol256": np.ascontiguousarray(th),
            "pol64": np.ascontiguousarray(th)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polfit_timing.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fs = fitters()
    rng = np.random.default_rng(1)
    if args.trace:
        th = walkers(1024, rng)
        for k, (f, d) in fs.items():
            f.loglike_batch(th[k], d)
            f.loglike_batch(th[k], d)
        return
    result = {"workload": "C4 fit, 3 bands x 20 epochs; one group of 4 epochs (75, 160, 230, 400 d)", "reps": args.reps, "unit": "ms"}
    for nw in (1024, 8192):
        th = walkers(nw, rng)
        ts = {k: [] for k in fs}
        for k, (f, d) in fs.items():  # warm every shape
            ll = f.loglike_batch(th[k], d)
            assert np.all(np.isfinite(ll)), k
        for _ in range(args.reps):
            for k, (f, d) in fs.items():
                t0 = time.perf_counter()
                f.loglike_batch(th[k], d)
                ts[k].append((time.perf_counter() - t0) * 1e3)
        row = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in ts.items()}
        for k in ("centroid", "pol256", "pol64"):
            row[k]["added_median"] = row[k]["median"] - row["none"]["median"]
        result[str(nw)] = row
        print(nw, "walkers:", json.dumps(row), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
