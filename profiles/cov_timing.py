"""What a correlated group costs in the walker likelihood on one GPU, and that a fit without one costs what it did.

1. The share: a host-pointer likelihood call on a fit that holds one correlated group of n rows and nothing else (Fitter.add_correlated:
   n epochs over the C4 range, the three C4 bands in turn, C_ln = diag(0.1^2) + 0.2^2) for n = 64 and n = 256 at 1024 and 8192
   walkers: the call is one pass -- the model stages, the series request at the n rows, vag_fit_back_cov_kernel.  After a warm-up,
   --reps repeats (5); a repeat is --calls calls in a row, each ending in a device synchronise.  Reported per n and batch size: the
   median, minimum and maximum in ms per call and, where torch's profiler can trace the device, the back kernel's own mean duration
   and its share of the pass.
2. The walker legs, with --parent-lib PATH (a build of the parent commit): the C4 light curves as point rows, no correlated group, at
   128, 1024 and 8192 walkers, one child process per figure, the parent build and this build alternating (P N N P ...; VAG_LIB_PATH
   selects the library), --legs processes per build (3).  Reported: every process's median ms per call, per build.

Run from the repository root: python profiles/cov_timing.py [--parent-lib PATH] [--out FILE]"""
import argparse
import json
import os
import subprocess
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

KERNEL = "vag_fit_back_cov_kernel"
LEG_WALKERS = (128, 1024, 8192)
GROUP_ROWS = (64, 256)


def param_defs():
    tr = configs.C4_TRUTH
    P = fitting.ParamDef
    fixed = [P(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    return [P("theta_c", 0.02, 0.3), P("theta_v", 0.0, 0.8), P("E_iso", 1e50, 1e54, fitting.Scale.log)] + fixed


def new_fitter():
    tr = configs.C4_TRUTH
    return fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")


def plain_fitter():
    """The C4 light curves as point rows: the fit without a correlated group."""
    t, nu = configs.c4_mock_data()
    truth = va.Model.from_params(_abi.make_params(**configs.C4_TRUTH)).flux_density(t, nu).total
    f = new_fitter()
    for b in configs.C4_BANDS:
        sel = nu == b
        f.add_flux_density(b, t[sel], truth[sel], 0.1 * truth[sel])
    return f


def cov_fitter(n):
    """One correlated group of n rows: a shared zero point of 20 % on top of 10 % errors."""
    t = np.geomspace(configs.C4_EPOCHS[0], configs.C4_EPOCHS[-1], n)
    nu = configs.C4_BANDS[np.arange(n) % 3]
    truth = va.Model.from_params(_abi.make_params(**configs.C4_TRUTH)).flux_density(t, nu).total
    f = new_fitter()
    f.add_correlated(nu, t, truth, np.diag((0.1 * truth) ** 2) + 0.2 ** 2 * np.outer(truth, truth))
    return f


def walkers(nw, rng):
    tr = configs.C4_TRUTH
    return np.ascontiguousarray(np.column_stack([tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
                                                 np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]))


def back_kernel_ms(f, th, defs, calls):
    """Mean device time of the back kernel per call from torch's profiler, or None where it cannot trace the device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                f.loglike_batch(th, defs)
        for ev in prof.key_averages():
            if KERNEL in ev.key:
                total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                return float(total) / 1e3 / calls
    except Exception as e:  # noqa: BLE001  (a profiler that is not there is not this script's failure)
        print(f"[cov_timing] no kernel trace: {e}", file=sys.stderr)
    return None


def timed(f, th, defs, reps, calls):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            f.loglike_batch(th, defs)
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def legs(args):
    """The child process of one build: the call without correlated groups at every size, median ms per call."""
    f, defs = plain_fitter(), param_defs()
    row = {}
    for nw in LEG_WALKERS:
        th = walkers(nw, np.random.default_rng(1))
        for _ in range(2):
            assert np.all(np.isfinite(f.loglike_batch(th, defs)))
        row[str(nw)] = float(np.median(timed(f, th, defs, args.reps, args.calls)))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the result to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="likelihood calls per timed repeat")
    ap.add_argument("--walkers", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit: also time the walker legs of both builds")
    ap.add_argument("--legs", type=int, default=3, help="processes per build of the walker legs")
    ap.add_argument("--legs-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.legs_child:
        return legs(args)
    defs = param_defs()
    result = {"workload": "one correlated group of n rows (C4 epochs range, the three C4 bands in turn, diag(0.1^2) + 0.2^2 in ln F) "
                          "and nothing else: one pass",
              "reps": args.reps, "calls_per_repeat": args.calls, "unit": "ms per call", "groups": {}}
    for n in GROUP_ROWS:
        f = cov_fitter(n)
        assert f.has_correlated and f._cov_obs[0]["t"].size == n
        rows = {}
        for nw in args.walkers:
            th = walkers(nw, np.random.default_rng(1))
            for _ in range(2):  # warm the shape (twice: the second call runs in the evaluation order the first one left)
                assert np.all(np.isfinite(f.loglike_batch(th, defs)))
            v = timed(f, th, defs, args.reps, args.calls)
            row = dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
            kern = back_kernel_ms(f, th, defs, 3)
            row["back_kernel"] = kern
            row["back_kernel_share"] = None if kern is None else kern / row["median"]
            rows[str(nw)] = row
            print(f"[cov_timing] n={n} walkers={nw}: {row}", file=sys.stderr, flush=True)
        result["groups"][str(n)] = rows
    if args.parent_lib:
        runs = {"P": [], "N": []}
        left = {"P": args.legs, "N": args.legs}
        for b in "PNNP" * args.legs:
            if not left[b]:
                continue
            left[b] -= 1
            env = dict(os.environ)
            if b == "P":
                env["VAG_LIB_PATH"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("VAG_LIB_PATH", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--legs-child", "--reps", str(args.reps), "--calls", str(args.calls)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            runs[b].append(json.loads(out.strip().split("\n")[-1]))
            print(f"[cov_timing] legs {b}: {runs[b][-1]}", file=sys.stderr, flush=True)
        result["walker_legs"] = {"unit": "median ms per call, one process per figure", "order": "P N N P ...",
                                 "parent": runs["P"], "this_build": runs["N"]}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
