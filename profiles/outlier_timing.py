"""What the outlier mixture costs in the walker likelihood on one GPU.

A host-pointer likelihood call of 1024 walkers on the C4 light curves (3 bands x 20 epochs as point rows, 10 % errors), all 60 rows in
one noise group with a free systematic: once as a plain noise group (the pass ends in vag_fit_back_noise_kernel) and once with
outliers=True on the same rows and out_frac, out_scale, out_shift free (vag_fit_back_robust_kernel).  The call is one pass -- the
model stages, the series request at the 60 rows, the back kernel -- so the two differ by the back kernel alone.  After a warm-up,
--reps repeats (5) per fitter, the two alternating (plain robust robust plain ...); a repeat is --calls calls in a row, each ending
in a device synchronise.  Reported per fitter: the median, minimum and maximum in ms per call and, where torch's profiler can trace
the device, the back kernel's own mean duration and its share of the call.

Run from the repository root: python profiles/outlier_timing.py [--out FILE]   (default: profiles/outlier_timing.json)"""
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

KERNELS = {"plain": "vag_fit_back_noise_kernel", "robust": "vag_fit_back_robust_kernel"}


def param_defs(robust):
    tr = configs.C4_TRUTH
    P = fitting.ParamDef
    fixed = [P(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    free = [P("theta_c", 0.02, 0.3), P("theta_v", 0.0, 0.8), P("E_iso", 1e50, 1e54, fitting.Scale.log), P("sys_lc", 0.0, 1.0)]
    if robust:
        free += [P("out_frac_lc", 0.0, 0.9), P("out_scale_lc", 1e-2, 1e1, fitting.Scale.log), P("out_shift_lc", -3.0, 3.0)]
    return free + fixed


def fitter(robust):
    """The C4 light curves as point rows of the noise group "lc"."""
    tr = configs.C4_TRUTH
    t, nu = configs.c4_mock_data()
    truth = va.Model.from_params(_abi.make_params(**tr)).flux_density(t, nu).total
    f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
    for b in configs.C4_BANDS:
        sel = nu == b
        f.add_flux_density(b, t[sel], truth[sel], 0.1 * truth[sel], noise="lc", **({"outliers": True} if robust else {}))
    return f


def walkers(nw, robust, rng):
    tr = configs.C4_TRUTH
    cols = [tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
            np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw), rng.uniform(0.0, 0.3, nw)]
    if robust:
        cols += [rng.uniform(0.0, 0.5, nw), rng.uniform(-1.0, 0.7, nw), rng.uniform(-0.5, 2.0, nw)]
    return np.ascontiguousarray(np.column_stack(cols))


def back_kernel_ms(f, th, defs, kernel, calls):
    """Mean device time of the back kernel per call from torch's profiler, or None where it cannot trace the device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                f.loglike_batch(th, defs)
        for ev in prof.key_averages():
            if kernel in ev.key:
                total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                return float(total) / 1e3 / calls
    except Exception as e:  # noqa: BLE001  (a profiler that is not there is not this script's failure)
        print(f"[outlier_timing] no kernel trace: {e}", file=sys.stderr)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="likelihood calls per timed repeat")
    ap.add_argument("--walkers", type=int, default=1024)
    args = ap.parse_args()
    cases = {}
    for name, robust in (("plain", False), ("robust", True)):
        f, defs = fitter(robust), param_defs(robust)
        assert f.has_outlier_groups == robust and f.has_noise_groups
        th = walkers(args.walkers, robust, np.random.default_rng(1))
        for _ in range(2):  # warm the shape (twice: the second call runs in the evaluation order the first one left)
            assert np.all(np.isfinite(f.loglike_batch(th, defs)))
        cases[name] = dict(f=f, defs=defs, th=th, ms=[])
    for name in ("plain", "robust", "robust", "plain") * args.reps:
        c = cases[name]
        if len(c["ms"]) == args.reps:
            continue
        t0 = time.perf_counter()
        for _ in range(args.calls):
            c["f"].loglike_batch(c["th"], c["defs"])
        c["ms"].append((time.perf_counter() - t0) * 1e3 / args.calls)
    result = {"workload": f"the C4 light curves (60 point rows) in one noise group, {args.walkers} walkers, one pass; plain: "
                          "sys free; robust: outliers=True on the same rows, out_frac, out_scale, out_shift free too",
              "walkers": args.walkers, "reps": args.reps, "calls_per_repeat": args.calls, "unit": "ms per call", "order": "P R R P ..."}
    for name, c in cases.items():
        row = dict(median=float(np.median(c["ms"])), min=float(np.min(c["ms"])), max=float(np.max(c["ms"])))
        kern = back_kernel_ms(c["f"], c["th"], c["defs"], KERNELS[name], 3)
        row["back_kernel"] = kern
        row["back_kernel_share"] = None if kern is None else kern / row["median"]
        result[name] = row
        print(f"[outlier_timing] {name}: {row}", file=sys.stderr, flush=True)
    result["robust_over_plain"] = result["robust"]["median"] / result["plain"]["median"]
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
