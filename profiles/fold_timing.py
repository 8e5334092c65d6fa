"""What a count-spectrum (fold) group costs in the walker likelihood on one GPU: a host-pointer likelihood call with one fold group
of J = 64 bins, C = 130 channels, n = 3 contiguous windows and m = 3 samples per window (Fitter.add_count_spectrum; 7 sample
times, 448 points) at 1024 and 8192 walkers, against the same call with the group's 448 (t, nu) points as point rows
(Fitter.add_flux_density) on the same build -- the same series request on the same points; only the back kernel differs -- and
against the fold group with every weight 0 (the back kernel forms G and skips every channel).  The fold fitter holds nothing else, so
a call is one pass.  After a warm-up of each leg, --reps repeats (5), the legs alternating; a repeat is --calls calls in a row, each
ending in a device synchronise.  Reported per batch size: the median, minimum and maximum in ms per call of each leg, the difference
of the medians fold - points (the fold back kernel less the point back kernel), and, where torch's profiler can trace the device,
the fold back kernel's own mean duration and its share of the pass.  Run from the repository root:
python profiles/fold_timing.py [--out FILE]"""
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

J, NC = 64, 130
DAY = 86400.0
EDGES = np.array([60.0, 61.0, 63.0, 66.0]) * DAY


def fitters():
    tr = configs.C4_TRUTH
    rng = np.random.default_rng(2)

    def new():
        return fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    e = np.geomspace(0.3, 10.0, J + 1)
    centre = (np.arange(J) + 0.5) * NC / J
    R = np.exp(-0.5 * ((np.arange(NC)[:, None] + 0.5 - centre[None, :]) / (NC / J)) ** 2) * 100.0
    args = dict(energy_lo=e[:-1], energy_hi=e[1:], response=R, t_start=EDGES[:-1], exposure=np.diff(EDGES),
                counts=rng.poisson(20.0, (3, NC)).astype(float), background=0.05, num_exposure_points=3)
    ff, f0 = new(), new()
    ff.add_count_spectrum(**args)
    f0.add_count_spectrum(**args, weights=0.0)
    gd = ff._fold_obs[0]
    ts, nus = np.repeat(gd["t_sample"], J), np.tile(gd["nu"], gd["t_sample"].size)  # the group's own points: the same request
    truth = va.Model.from_params(_abi.make_params(**tr)).flux_density(ts, nus).total
    fp = new()
    fp.add_flux_density(nus, ts, truth, 0.1 * truth)
    fixed = [fitting.ParamDef(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    defs = [fitting.ParamDef("theta_c", 0.02, 0.3), fitting.ParamDef("theta_v", 0.0, 0.8),
            fitting.ParamDef("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed
    return {"points": fp, "fold": ff, "fold_w0": f0}, defs


def walkers(nw, rng):
    tr = configs.C4_TRUTH
    return np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                                 np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))


def back_kernel_ms(f, th, defs, calls):
    """Mean device time of vag_fit_back_fold_kernel per call from torch's profiler, or None where it cannot trace the device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                f.loglike_batch(th, defs)
        for ev in prof.key_averages():
            if "vag_fit_back_fold_kernel" in ev.key:
                total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                return float(total) / 1e3 / calls
    except Exception as e:  # noqa: BLE001  (a profiler that is not there is not this script's failure)
        print(f"[fold_timing] no kernel trace: {e}", file=sys.stderr)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the result to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="likelihood calls per timed repeat")
    ap.add_argument("--walkers", type=int, nargs="+", default=[1024, 8192])
    args = ap.parse_args()
    fs, defs = fitters()
    assert fs["fold"].has_count_spectra and not fs["points"].has_count_spectra
    result = {"workload": f"C4, 0.3-10 keV in {J} bins, {NC} channels, 3 contiguous windows x 3 samples (7 sample times, 448 points); one fold "
                          "group against the same points as point rows and against the group with every weight 0",
              "reps": args.reps, "calls_per_repeat": args.calls, "unit": "ms per call", "batches": {}}
    for nw in args.walkers:
        th = walkers(nw, np.random.default_rng(1))
        for k, f in fs.items():  # warm every shape (twice: the second call runs in the evaluation order the first one left)
            for _ in range(2):
                assert np.all(np.isfinite(f.loglike_batch(th, defs))), k
        ts = {k: [] for k in fs}
        for _ in range(args.reps):
            for k, f in fs.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    f.loglike_batch(th, defs)
                ts[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
        row = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in ts.items()}
        row["pass_median"] = row["fold"]["median"]
        row["added_median"] = row["fold"]["median"] - row["points"]["median"]
        row["contraction_median"] = row["fold"]["median"] - row["fold_w0"]["median"]
        kern = back_kernel_ms(fs["fold"], th, defs, 3)
        row["back_kernel"] = kern
        row["back_kernel_share"] = None if kern is None else kern / row["fold"]["median"]
        result["batches"][str(nw)] = row
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
