"""What a spectral-index group costs in the walker likelihood on one GPU: a 1024-walker host-pointer likelihood call with one
index group of n = 20 rows and K = 2 frequencies (Fitter.add_spectral_index) against the same call with the group's 40 (t, nu)
points as point rows (Fitter.add_flux_density) on the same build -- the same series request on the same points; only the back
kernel differs.  After a warm-up of each leg, --reps repeats (5), the legs alternating; a repeat is --calls calls in a row, each
ending in a device synchronise.  Reported: the median, minimum and maximum in ms per call of each leg, and the difference of the
medians.  Run from the repository root: python profiles/index_timing.py [--out FILE]"""
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
    t = configs.C4_EPOCHS  # 20 epochs

    def new():
        return fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    fi = new()
    fi.add_spectral_index(BAND, t, np.full(t.size, 2.0), np.full(t.size, 0.1), num_points=2, convention="photon")
    gd = fi._index_obs[0]
    ts, nus = np.repeat(gd["t"], 2), np.tile(gd["nu"], t.size)  # the group's own points: the same request
    truth = va.Model.from_params(_abi.make_params(**tr)).flux_density(ts, nus).total
    fp = new()
    fp.add_flux_density(nus, ts, truth, 0.1 * truth)
    fixed = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed
    return {"points": fp, "index": fi}, defs


def walkers(nw, rng):
    tr = configs.C4_TRUTH
    return np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                                 np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the result to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="likelihood calls per timed repeat")
    ap.add_argument("--walkers", type=int, default=1024)
    args = ap.parse_args()
    fs, defs = fitters()
    assert fs["index"].has_spectral_indices and not fs["points"].has_spectral_indices
    th = walkers(args.walkers, np.random.default_rng(1))
    plans = {}
    for k, f in fs.items():  # warm every shape (twice: the second call runs in the evaluation order the first one left)
        for _ in range(2):
            assert np.all(np.isfinite(f.loglike_batch(th, defs))), k
        plans[k] = dict(pairs_per_block=int(f.last_plan.pairs_per_block), total_pairs=int(f.last_plan.total_pairs),
                        flux_blocks=int(f.last_plan.flux_blocks))
    ts = {k: [] for k in fs}
    for _ in range(args.reps):
        for k, f in fs.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                f.loglike_batch(th, defs)
            ts[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
    row = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in ts.items()}
    row["added_median"] = row["index"]["median"] - row["points"]["median"]
    result = {"workload": f"C4, band {BAND[0]:g}-{BAND[1]:g} Hz, 20 epochs x 2 frequencies, {args.walkers} walkers; the 40 points as one "
                          "index group against the same points as point rows",
              "reps": args.reps, "calls_per_repeat": args.calls, "unit": "ms per call", "plan": plans, **row}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
