"""What a sampler step costs on one GPU: the host sampler against the device sampler, on the C4 fitter of bench.py.

Both samplers run the same likelihood kernels on nwalkers / 2 proposals twice per step.  The host path (sampling.run_stretch_move
through Fitter.make_log_prob_batch) rebuilds the spec, rescans and hashes its blocks, copies theta up and ln L down and synchronises
the stream for every half-step, and forms the proposals in numpy; the device path (sampling.run_stretch_move_device) does the scans
and uploads once per chunk of steps and keeps positions, ln p and the chain in HBM.

Per ensemble size (1024 and 128 walkers, started in a ball of 2 % of the box around the truth): after a warm-up run of --warmup steps
(5) on each path, --reps repeats (5) of a run of --steps steps (50), the two paths alternating within the one process.  A run is timed
by the host clock from its call to its return; both return numpy arrays, so the device is idle at either end, and a run includes its
one full-ensemble call for the initial ln p.  Reported per size and path: the median, minimum and maximum in ms per step, the mean
acceptance, and the device path's ms per step over the host path's.

Run from the repository root: python profiles/sampler_timing.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (c4_fitter: the benchmark's own problem)
import configs  # noqa: E402
import vegasafterglow_amd as va  # noqa: E402
from vegasafterglow_amd import _lib, sampling  # noqa: E402

WALKERS = (1024, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    h, _ = va.get_context(0)
    fit, defs, _ = bench.c4_fitter(lib, h, _lib)
    _, lo, hi = fit.build_spec(defs)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    log_prob_batch = fit.make_log_prob_batch(defs)
    result = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "sizes": {}}
    for nw in WALKERS:
        pos0 = sampling.initial_positions(lo, hi, nw, np.random.default_rng(nw), center=truth, spread=0.02)

        def host(n):
            return sampling.run_stretch_move(log_prob_batch, pos0, n, rng=np.random.default_rng(1))

        def device(n):
            return sampling.run_stretch_move_device(fit, defs, pos0, n, seed=1)

        paths = {"host": host, "device": device}
        for run in paths.values():
            run(args.warmup)
        ms = {k: [] for k in paths}
        acc = {}
        for _ in range(args.reps):
            for k, run in paths.items():
                t0 = time.perf_counter()
                out = run(args.steps)
                ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
                acc[k] = float(out[2].mean())
                assert np.all(np.isfinite(out[1]))
        size = {k: {"ms_per_step_median": float(np.median(v)), "ms_per_step_min": min(v), "ms_per_step_max": max(v),
                    "acceptance": acc[k]} for k, v in ms.items()}
        size["device_over_host"] = size["device"]["ms_per_step_median"] / size["host"]["ms_per_step_median"]
        result["sizes"][str(nw)] = size
        print(f"{nw} walkers: host {size['host']['ms_per_step_median']:.2f} ms/step, device "
              f"{size['device']['ms_per_step_median']:.2f} ms/step ({size['device_over_host']:.3f} x)", flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
