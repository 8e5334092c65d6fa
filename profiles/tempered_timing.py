"""What a tempered step costs on one GPU: one ladder of T temperatures against T plain device-sampler runs, on the C4 fitter of
bench.py (the problem of profiles/sampler_timing.py).

A tempered step (sampling.run_tempered_device) sends the T nw / 2 proposals of all temperatures through ONE likelihood call per
half-step, and adds the split, the exchanges and three device-to-device copies per stored step.  The baseline is what a user without
tempering would run for the same number of walker-steps: T runs of sampling.run_stretch_move_device with nw walkers each, one after
the other (T nw / 2 proposals per half-step in T calls).  That path is older than tempering, which leaves its kernels and its entry
as they were; --paths plain_runs times it alone, also on a build from before tempering named by VAG_LIB_PATH.  The two do not evaluate the same models: the plain runs stay in a ball around the truth, the hot rungs of the
ladder spread over the prior box, where models cost more or are rejected by the engine's limits -- the ratio is what a run costs,
not a like-for-like kernel comparison.

Per shape (T = 8 with nw = 128 and nw = 1024; the ladder geometric_betas(8, 1e-3, prior_rung=True), every ensemble started in a ball of
2 % of the box around the truth): after a warm-up of --warmup steps (5) on each path, --reps repeats (5) of --steps steps (50), the
two paths alternating within the one process.  A run is timed by the host clock from its call to its return; both return numpy
arrays, so the device is idle at either end, and a run includes its full-ensemble call for the initial state.  Reported per shape:
median, minimum and maximum in ms per step of the tempered run and of the T plain runs together, and their ratio.

Run from the repository root: python profiles/tempered_timing.py [--out FILE]"""
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

SHAPES = ((8, 128), (8, 1024))  # (T, nw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="tempered,plain_runs", help="plain_runs alone also runs on an older build (VAG_LIB_PATH)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    h, _ = va.get_context(0)
    fit, defs, _ = bench.c4_fitter(lib, h, _lib)
    _, lo, hi = fit.build_spec(defs)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    result = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shapes": {}}
    for ntemps, nw in SHAPES:
        betas = sampling.geometric_betas(ntemps, 1e-3, prior_rung=True)
        pos0 = sampling.initial_positions(lo, hi, ntemps * nw, np.random.default_rng(nw), center=truth, spread=0.02).reshape(ntemps, nw, -1)

        def tempered(n):
            out = sampling.run_tempered_device(fit, defs, pos0, betas, n, seed=1)
            assert np.all(np.isfinite(out[1])) and np.all(np.isfinite(out[2]))
            return {"acceptance_cold": float(out[3][0].mean()), "acceptance_hot": float(out[3][-1].mean()),
                    "swap_fraction": [float(v) for v in out[4]]}

        def plain(n):
            acc = []
            for t in range(ntemps):
                out = sampling.run_stretch_move_device(fit, defs, pos0[t], n, seed=1 + t)
                assert np.all(np.isfinite(out[1]))
                acc.append(float(out[2].mean()))
            return {"acceptance": float(np.mean(acc))}

        paths = {k: run for k, run in (("tempered", tempered), ("plain_runs", plain)) if k in args.paths.split(",")}
        for run in paths.values():
            run(args.warmup)
        ms = {k: [] for k in paths}
        info = {}
        for _ in range(args.reps):
            for k, run in paths.items():
                t0 = time.perf_counter()
                info[k] = run(args.steps)
                ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
        shape = {k: dict(info[k], ms_per_step_median=float(np.median(v)), ms_per_step_min=min(v), ms_per_step_max=max(v))
                 for k, v in ms.items()}
        if len(shape) == 2:
            shape["tempered_over_plain"] = shape["tempered"]["ms_per_step_median"] / shape["plain_runs"]["ms_per_step_median"]
        result["shapes"][f"{ntemps}x{nw}"] = shape
        print(f"T = {ntemps}, {nw} walkers each: " +
              ", ".join(f"{k} {v['ms_per_step_median']:.2f} ms/step" for k, v in shape.items() if isinstance(v, dict)) +
              (f" ({shape['tempered_over_plain']:.3f} x)" if "tempered_over_plain" in shape else ""), flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
