"""What the reference's proposals cost on one GPU, and what they buy: the device sampler with the stretch move against the device
sampler with the reference mix (DE at 0.8, snooker at 0.2), on the C4 fitter of bench.py (the problem of profiles/sampler_timing.py).

Both runs make the same two likelihood calls of nwalkers / 2 proposals per step; they differ in the two small launches around each
call (sampling.run_stretch_move_device: vag_stretch_run_dev; sampling.run_moves_device: vag_move_run_dev, which also chooses each
step's kind on the host).  The stretch path is older than the move mix, which leaves its kernels and its entry as they were;
--paths stretch times it alone, also on a build from before the move mix named by VAG_LIB_PATH.  The two paths do not evaluate the
same models: each chain goes where its proposals take it.

Timing, per ensemble size (128 and 1024 walkers, started in a ball of 2 % of the box around the truth): after a warm-up run of
--warmup steps (5) on each path, --reps repeats (5) of a run of --steps steps (50), the paths alternating within the one process.  A
run is timed by the host clock from its call to its return; both return numpy arrays, so the device is idle at either end, and a run
includes its one full-ensemble call for the initial ln p.  Reported per size and path: median, minimum and maximum in ms per step and
the mean acceptance.

Mixing (--tau-steps N, default 0 = skipped; 128 walkers): one run of N steps per path from the same start, the first quarter dropped;
the integrated autocorrelation time of every parameter in steps, from the autocorrelation function averaged over the walkers with
Sokal's automatic window (c = 5), as emcee estimates it (Goodman & Weare 2010; Foreman-Mackey et al. 2013).  An estimate from fewer
than 50 tau kept steps is marked unreliable.  No pass or fail: it is the number a user choosing between the moves wants.

Run from the repository root: python profiles/moves_timing.py [--tau-steps 4000] [--out FILE]"""
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

WALKERS = (128, 1024)


def autocorr_time(chain, c=5.0):
    """tau[ndim] in steps of chain[steps, walkers, ndim]: 2 sum rho - 1 up to the first lag M with M >= c tau(M), rho the
    autocorrelation function of each walker's series averaged over the walkers."""
    n, _, ndim = chain.shape
    size = 1 << (2 * n - 1).bit_length()
    tau = np.empty(ndim)
    for d in range(ndim):
        x = chain[:, :, d] - chain[:, :, d].mean(axis=0)
        f = np.fft.rfft(x, n=size, axis=0)
        acf = np.fft.irfft(f * np.conj(f), n=size, axis=0)[:n].mean(axis=1)
        rho = acf / acf[0]
        taus = 2.0 * np.cumsum(rho) - 1.0
        ok = np.arange(n) >= c * taus
        tau[d] = taus[np.argmax(ok)] if ok.any() else taus[-1]
    return tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="stretch,reference", help="stretch alone also runs on an older build (VAG_LIB_PATH)")
    ap.add_argument("--tau-steps", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    h, _ = va.get_context(0)
    fit, defs, _ = bench.c4_fitter(lib, h, _lib)
    _, lo, hi = fit.build_spec(defs)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    names = [n for n, _, _, _ in configs.C4_FREE]
    result = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "library": os.path.basename(_lib.LIB_PATH), "sizes": {}}

    def runs(pos0):
        def stretch(n):
            return sampling.run_stretch_move_device(fit, defs, pos0, n, seed=1)

        def reference(n):
            return sampling.run_moves_device(fit, defs, pos0, n, moves=sampling.REFERENCE_MOVES, seed=1)
        return {k: run for k, run in (("stretch", stretch), ("reference", reference)) if k in args.paths.split(",")}

    for nw in WALKERS:
        paths = runs(sampling.initial_positions(lo, hi, nw, np.random.default_rng(nw), center=truth, spread=0.02))
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
        if len(size) == 2:
            size["reference_over_stretch"] = size["reference"]["ms_per_step_median"] / size["stretch"]["ms_per_step_median"]
        result["sizes"][str(nw)] = size
        print(f"{nw} walkers: " + ", ".join(f"{k} {v['ms_per_step_median']:.3f} ({v['ms_per_step_min']:.3f} - {v['ms_per_step_max']:.3f}) "
                                            f"ms/step, acceptance {v['acceptance']:.2f}" for k, v in size.items() if isinstance(v, dict)),
              flush=True)
    if args.tau_steps > 0:
        nw = WALKERS[0]
        paths = runs(sampling.initial_positions(lo, hi, nw, np.random.default_rng(nw), center=truth, spread=0.02))
        result["tau"] = {"walkers": nw, "steps": args.tau_steps, "dropped": args.tau_steps // 4, "parameters": names}
        for k, run in paths.items():
            chain, logp, acceptance = run(args.tau_steps)
            kept = chain[args.tau_steps // 4:]
            tau = autocorr_time(kept)
            result["tau"][k] = {"tau_steps": [float(v) for v in tau], "acceptance": float(acceptance.mean()),
                                "reliable": bool(kept.shape[0] >= 50 * tau.max()), "mean_log_prob": float(logp[args.tau_steps // 4:].mean())}
            print(f"{k}: tau " + " ".join(f"{n} {v:.0f}" for n, v in zip(names, tau)) +
                  f" steps (max {tau.max():.0f}, {kept.shape[0]} kept steps, acceptance {acceptance.mean():.2f})", flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
