"""What a convergence check costs: the integrated autocorrelation times of a chain that lives on the device
(sampling.chain_autocorr_device: vag_chain_autocorr_dev, default lag range) against the route a user had before it -- copy the chain to
the host and run the FFT estimator of profiles/moves_timing.py (autocorr_time) -- and against the sampler steps between two checks.

Two chains, [rows, walkers, 8]: 4000 x 128 and 10000 x 1024, AR(1) series with the coefficients 0.5 ... 0.95 (what is in the chain does
not change the device's work; it moves the FFT route's window search a little).  Per chain, in this one process: the device estimate
(from the call to the numpy record it returns, so the stream is drained), a warm-up and then the median of --reps (5); the host route
(chain.cpu().numpy(), then autocorr_time), the median of --host-reps (2) without a warm-up, the copy and the estimator apart.  Then the
time of --check (100) steps of sampling.run_stretch_move_device on the C4 fitter of bench.py at the chain's ensemble size (a warm-up run,
then the median of --reps runs), and the check's share of it.  One JSON line at the end.

Run from the repository root: python profiles/autocorr_timing.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402  (c4_fitter: the benchmark's own problem)
import configs  # noqa: E402
import moves_timing  # noqa: E402  (autocorr_time: the host route)
import vegasafterglow_amd as va  # noqa: E402
from vegasafterglow_amd import _lib, sampling  # noqa: E402

CHAINS = ((4000, 128), (10000, 1024))
PHI = np.array([0.5, 0.8, 0.9, 0.0, 0.95, 0.7, 0.6, 0.85])


def ar1_on_device(torch, rows, walkers, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    phi = torch.from_numpy(PHI).cuda()
    x = torch.randn((rows, walkers, PHI.size), dtype=torch.float64, device="cuda", generator=gen)
    x[0] /= torch.sqrt(1.0 - phi ** 2)
    for t in range(1, rows):
        x[t] += phi * x[t - 1]
    return x


def median_ms(fn, reps, warm=True):
    if warm:
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--check", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    h, _ = va.get_context(0)
    fit, defs, _ = bench.c4_fitter(lib, h, _lib)
    _, lo, hi = fit.build_spec(defs)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    result = {"reps": args.reps, "host_reps": args.host_reps, "check": args.check, "chains": {}}
    for rows, walkers in CHAINS:
        chain = ar1_on_device(torch, rows, walkers, rows)
        torch.cuda.synchronize()
        record = {}
        device = median_ms(lambda: record.update(rec=sampling.chain_autocorr_device(chain, rho=False)), args.reps)
        host = {}

        def copy():
            host["chain"] = chain.cpu().numpy()

        def estimate():
            host["tau"] = moves_timing.autocorr_time(host["chain"])
        copy_ms = median_ms(copy, args.host_reps, warm=False)
        fft_ms = median_ms(estimate, args.host_reps, warm=False)
        rec = record["rec"]
        found = rec.window >= 0
        assert np.allclose(rec.tau[found], host["tau"][found], rtol=1e-6), (rec.tau, host["tau"])
        pos0 = sampling.initial_positions(lo, hi, walkers, np.random.default_rng(walkers), center=truth, spread=0.02)
        steps = median_ms(lambda: sampling.run_stretch_move_device(fit, defs, pos0, args.check, seed=1), args.reps)
        entry = {"max_lag": rec.max_lag, "tau": [float(v) for v in rec.tau], "window": [int(v) for v in rec.window],
                 "device_ms": device, "host_copy_ms": copy_ms, "host_fft_ms": fft_ms, "host_route_ms": copy_ms[0] + fft_ms[0],
                 "check_steps_ms": steps, "check_share": device[0] / steps[0]}
        result["chains"][f"{rows}x{walkers}x{PHI.size}"] = entry
        print(f"{rows} x {walkers} x {PHI.size} (L = {rec.max_lag}): device {device[0]:.2f} ms ({device[1]:.2f} - {device[2]:.2f}); host route "
              f"{copy_ms[0] + fft_ms[0]:.0f} ms (copy {copy_ms[0]:.0f}, FFT estimator {fft_ms[0]:.0f}); {args.check} sampler steps "
              f"{steps[0]:.1f} ms; a check is {100 * device[0] / steps[0]:.1f} % of them", flush=True)
        del chain, host
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
