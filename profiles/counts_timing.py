"""What a counts group costs in the walker likelihood on one GPU (profiles/counts_timing.json): a 1024-walker host-pointer
likelihood call with one 20-row counts group (Fitter.add_counts, one sample per row) against the same call with those 20 rows as an
add_flux group on the same build -- the same band request on the same times; only the back kernel differs.  The two are timed in
alternating samples (one sample of each per round; a sample is --calls calls in a row, each ending in a device synchronise, so a
timed window is tens of milliseconds): medians, minima and maxima in ms per call, the spread of each, and the flux plan of each leg
(pairs per workgroup: pinned for the counts pass, the tuner's for the band group).  --trace: one warmed call of the counts fitter alone, for a kernel trace of its own.
Run from the repository root: python profiles/counts_timing.py [--out FILE]"""
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

BAND = (7.25e16, 2.42e18)


def fitters():
    tr = configs.C4_TRUTH
    t = configs.C4_EPOCHS  # 20 epochs: the sample times of the counts rows (midpoints) and the times of the band rows
    exposure = np.full(t.size, 5e4)
    truth = va.Model.from_params(_abi.make_params(**tr)).flux(t, BAND[0], BAND[1], 5).total
    mu = np.geomspace(1e-2, 1e6, t.size)
    counts = np.random.default_rng(11).poisson(mu).astype(float)

    def new():
        return fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    fc = new()
    fc.add_counts(BAND, t - 0.5 * exposure, exposure, counts, mu / (exposure * truth))
    fb = new()
    fb.add_flux(BAND, fc._counts_obs[0]["t_sample"], truth, 0.1 * truth)  # the counts rows' own sample times: the same request
    fixed = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed
    return {"band": fb, "counts": fc}, defs


def walkers(nw, rng):
    tr = configs.C4_TRUTH
    return np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                                 np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counts_timing.json"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20, help="likelihood calls per timed sample")
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fs, defs = fitters()
    assert fs["counts"].has_counts and not fs["band"].has_counts
    th = walkers(args.walkers, np.random.default_rng(1))
    if args.trace:
        fs = {"counts": fs["counts"]}
    plans = {}
    for k, f in fs.items():  # warm every shape (twice: the second call runs in the evaluation order the first one left)
        for _ in range(2):
            assert np.all(np.isfinite(f.loglike_batch(th, defs))), k
        plans[k] = dict(pairs_per_block=int(f.last_plan.pairs_per_block), total_pairs=int(f.last_plan.total_pairs),
                        flux_blocks=int(f.last_plan.flux_blocks))
    if args.trace:
        return
    ts = {k: [] for k in fs}
    for _ in range(args.reps):
        for k, f in fs.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                f.loglike_batch(th, defs)
            ts[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
    row = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)),
                   spread=float(np.percentile(v, 84) - np.percentile(v, 16))) for k, v in ts.items()}
    row["added_median"] = row["counts"]["median"] - row["band"]["median"]
    result = {"workload": f"C4, band {BAND[0]:g}-{BAND[1]:g} Hz, 20 epochs, {args.walkers} walkers; the rows as one counts group against "
                          "the same rows as one add_flux group",
              "reps": args.reps, "calls_per_sample": args.calls, "unit": "ms per call",
              "spread": "84th - 16th percentile of the samples", "plan": plans, **row}
    print(json.dumps(result), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
