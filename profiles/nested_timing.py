"""What a nested-sampling iteration costs on the device (sampling.run_nested_device: vag_nested_run_dev), and how much of it is spent
outside the likelihood calls.

The C4 fitter of bench.py (eight free parameters, so the default walk is 40), N = 1024 and 8192 live points started in a ball around
the truth (every point evaluates).  Per N, in this one process: runs of --iters (4) and of twice as many iterations, each ONE call, a
warm-up and then the median of --reps (3); their difference divided by --iters is an iteration (what a run spends once -- the first
evaluation of the N points, the copies in and out -- drops out).  Then what an iteration does outside its likelihood calls, timed
directly: one iteration's building blocks on the state the run left -- rank, retire, and `walk` times propose and accept
(sampling.NestedMove) with ln L of the proposals made up around L* -- from the first launch to the drained stream; driven from Python,
so an upper bound on what the run entry spends on them.  Their share of the iteration is the figure asked for; the expectation is
that an iteration costs its `walk` likelihood calls of N / 2 walkers plus a few percent.  For reference also `walk` calls of
sampling.loglike_split_device on N / 2 of the live points the run left: not the run's own calls -- its proposals are other points,
some outside the box and never evaluated, and every call here pays Python's way into the library -- so it is printed, not subtracted.
One JSON line at the end.

Run from the repository root: python profiles/nested_timing.py [--out FILE]"""
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

SIZES = (1024, 8192)


def median_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    h, _ = va.get_context(0)
    fit, defs, _ = bench.c4_fitter(lib, h, _lib)
    spec, lo, hi = fit.build_spec(defs, use_priors=True)
    walk = sampling.nested_default_walk(spec.ndim)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    result = {"reps": args.reps, "iters": args.iters, "walk": walk, "sizes": {}}
    for n in SIZES:
        live0 = sampling.initial_positions(lo, hi, n, np.random.default_rng(n), center=truth, spread=0.02)
        kept = {}
        run_ms = median_ms(lambda: sampling.run_nested_device(fit, defs, live0, args.iters, seed=1, chunk=args.iters), args.reps)
        twice_ms = median_ms(lambda: kept.update(run=sampling.run_nested_device(fit, defs, live0, 2 * args.iters, seed=1, chunk=2 * args.iters)),
                             args.reps)
        run = kept["run"]
        half = torch.from_numpy(np.ascontiguousarray(run.live[:n // 2])).cuda()
        lnl = torch.empty((n // 2,), dtype=torch.float64, device=half.device)
        lnprior = torch.empty_like(lnl)

        def calls():
            for _ in range(walk):
                sampling.loglike_split_device(fit, spec, half, lnl, lnprior)
            torch.cuda.synchronize()
        like_ms = median_ms(calls, args.reps)
        move = sampling.NestedMove(n, spec.ndim, walk, seed=1)
        k = n // 2
        live, d_lnl, d_lnprior = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (run.live, run.lnl, run.lnprior))
        dead = [torch.empty((k,) + tail, dtype=torch.float64, device=live.device) for tail in ((spec.ndim,), (), ())]
        accepted = torch.zeros((k,), dtype=torch.int64, device=live.device)
        made_up = torch.from_numpy(np.random.default_rng(n).uniform(-1.0, 3.0, k)).cuda()
        lnprior_new = torch.full((k,), float(run.lnprior[0]), dtype=torch.float64, device=live.device)

        def blocks():
            order, lstar = move.rank(d_lnl)
            move.retire(0, order, live, d_lnl, d_lnprior, *dead)
            lnl_new = made_up + lstar
            for m in range(1, walk + 1):
                prop = move.propose(0, m, order, live)
                move.accept(0, m, order, lstar, prop, lnl_new, lnprior_new, live, d_lnl, d_lnprior, accepted)
            torch.cuda.synchronize()
        blocks_ms = median_ms(blocks, args.reps)
        per_iter = (twice_ms[0] - run_ms[0]) / args.iters
        share = blocks_ms[0] / per_iter
        result["sizes"][str(n)] = {"run_ms": run_ms, "twice_ms": twice_ms, "ms_per_iteration": per_iter, "building_blocks_ms": blocks_ms, "outside_share": share,
                                   "likelihood_calls_of_live_points_ms": like_ms,
                                   "acceptance": float(run.accepted.mean() / (n // 2 * walk))}
        print(f"N = {n}, walk = {walk}: {per_iter:.1f} ms per iteration ({args.iters} iterations {run_ms[0]:.1f} ms, "
              f"{2 * args.iters} iterations {twice_ms[0]:.1f} ms); outside the likelihood calls {blocks_ms[0]:.2f} ms = "
              f"{100 * share:.1f} %; {walk} likelihood calls of {n // 2} live points from Python {like_ms[0]:.1f} ms; acceptance {run.accepted.mean() / (n // 2 * walk):.2f}", flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
