"""What upper-limit rows cost in the walker likelihood on one GPU (profiles/limits_timing.json): a 1024-walker host-pointer
likelihood call on the C4 fit (3 bands x 20 epochs) with 15 of the 60 rows as upper limits, against the same 60 rows as detections
on the same build.  The two are timed in alternating repeats (one call of each per round, each call ends in a device synchronise):
medians, minima and maxima in ms, and the spread of each.  --trace: one warmed call per fitter, for a kernel trace of its own.
Run from the repository root: python profiles/limits_timing.py [--out FILE]"""
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
from vegasafterglow_amd import fitting  # noqa: E402


def fitters():
    tr = configs.C4_TRUTH
    t, nu = configs.c4_mock_data()
    truth = va.Model.from_params(_abi.make_params(**tr)).flux_density(t, nu).total
    lim = np.zeros(t.size, dtype=bool)
    lim[1::4] = True  # 15 rows
    err = 0.1 * truth
    value = np.where(lim, truth + 2.0 * err, truth)  # 2 sigma above the truth

    def fitter(limits):
        f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
        f.add_flux_density(nu, t, value, err, upper_limit=lim if limits else None)
        return f
    fixed = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed
    return {"detections": fitter(False), "limits": fitter(True)}, defs


def walkers(nw, rng):
    tr = configs.C4_TRUTH
    return np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                                 np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limits_timing.json"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fs, defs = fitters()
    assert fs["limits"].has_limits and not fs["detections"].has_limits
    th = walkers(args.walkers, np.random.default_rng(1))
    for k, f in fs.items():  # warm every shape (twice: the second call runs in the evaluation order the first one left)
        for _ in range(2):
            assert np.all(np.isfinite(f.loglike_batch(th, defs))), k
    if args.trace:
        return
    ts = {k: [] for k in fs}
    for _ in range(args.reps):
        for k, f in fs.items():
            t0 = time.perf_counter()
            f.loglike_batch(th, defs)
            ts[k].append((time.perf_counter() - t0) * 1e3)
    row = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)),
                   spread=float(np.percentile(v, 84) - np.percentile(v, 16))) for k, v in ts.items()}
    row["added_median"] = row["limits"]["median"] - row["detections"]["median"]
    result = {"workload": f"C4 fit, 3 bands x 20 epochs, {args.walkers} walkers; 15 of the 60 rows as upper limits against all 60 as detections",
              "reps": args.reps, "unit": "ms", "spread": "84th - 16th percentile of the repeats", **row}
    print(json.dumps(result), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
