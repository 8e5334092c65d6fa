"""What additive templates cost in the walker likelihood on one GPU, and that a fit without them costs what it did.

1. The share: a host-pointer likelihood call on the C4 light curves (3 bands x 20 epochs, 60 point rows, one pass) with a host
   template on every band (templates={"host_k": 1.0}, three free amplitudes) at 1024 and 8192 walkers, against the same call without
   templates= on the same build -- the same series request; only the back kernel differs.  After a warm-up of each leg, --reps
   repeats (5), the legs alternating; a repeat is --calls calls in a row, each ending in a device synchronise.  Reported per batch
   size: the median, minimum and maximum in ms per call of each leg, the difference of the medians, and, where torch's profiler can
   trace the device, the template back kernel's own mean duration and its share of the pass.
2. The walker legs, with --parent-lib PATH (a build of the parent commit): the call without templates at 128, 1024 and 8192 walkers,
   one child process per figure, the parent build and this build alternating (P N N P ...; VAG_LIB_PATH selects the library), --legs
   processes per build (3).  Reported: every process's median ms per call, per build.

Run from the repository root: python profiles/template_timing.py [--parent-lib PATH] [--out FILE]"""
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

KERNEL = "vag_fit_back_tmpl_kernel"
LEG_WALKERS = (128, 1024, 8192)


def fitters(with_templates=True):
    tr = configs.C4_TRUTH
    t, nu = configs.c4_mock_data()
    truth = va.Model.from_params(_abi.make_params(**tr)).flux_density(t, nu).total
    P = fitting.ParamDef

    def new(templates):
        f = fitting.Fitter(z=tr["z"], lumi_dist=tr["lumi_dist"], jet="gaussian", medium="ism")
        for k, b in enumerate(configs.C4_BANDS):
            sel = nu == b
            host = float(truth[sel][-1])
            kw = dict(templates={f"host_{k}": 1.0}) if templates else {}
            f.add_flux_density(b, t[sel], truth[sel] + host, 0.1 * (truth[sel] + host), **kw)
        return f
    fixed = [P(k, v, v, fitting.Scale.fixed) for k, v in
             dict(Gamma0=tr["Gamma0"], n_ism=tr["n_ism"], eps_e=tr["eps_e"], eps_B=tr["eps_B"], p=tr["p"]).items()]
    flux = [P("theta_c", 0.02, 0.3), P("theta_v", 0.0, 0.8), P("E_iso", 1e50, 1e54, fitting.Scale.log)]
    hosts = [float(truth[nu == b][-1]) for b in configs.C4_BANDS]
    amps = [P(f"amp_host_{k}", 0.0, 10.0 * h) for k, h in enumerate(hosts)]
    out = {"plain": (new(False), flux + fixed)}
    if with_templates:
        out["templates"] = (new(True), flux + amps + fixed)
    return out, hosts


def walkers(nw, rng, hosts=()):
    tr = configs.C4_TRUTH
    cols = [tr["theta_c"] * rng.uniform(0.8, 1.2, nw), tr["theta_obs"] * rng.uniform(0.85, 1.15, nw),
            np.log10(tr["E_iso"]) + rng.uniform(-0.3, 0.3, nw)]
    return np.ascontiguousarray(np.column_stack(cols + [h * rng.uniform(0.5, 2.0, nw) for h in hosts]))


def back_kernel_ms(f, th, defs, calls):
    """Mean device time of the template back kernel per call from torch's profiler, or None where it cannot trace the device."""
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
        print(f"[template_timing] no kernel trace: {e}", file=sys.stderr)
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
    """The child process of one build: the call without templates at every size, median ms per call."""
    fs, _ = fitters(with_templates=False)
    f, defs = fs["plain"]
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
    fs, hosts = fitters()
    assert fs["templates"][0].has_templates and not fs["plain"][0].has_templates
    result = {"workload": "C4, 3 bands x 20 epochs as point rows (one pass), a host template with a free amplitude on every band, "
                          "against the same rows without templates",
              "reps": args.reps, "calls_per_repeat": args.calls, "unit": "ms per call", "batches": {}}
    for nw in args.walkers:
        th = {"plain": walkers(nw, np.random.default_rng(1)), "templates": walkers(nw, np.random.default_rng(1), hosts)}
        for k, (f, d) in fs.items():  # warm every shape (twice: the second call runs in the evaluation order the first one left)
            for _ in range(2):
                assert np.all(np.isfinite(f.loglike_batch(th[k], d))), k
        ts = {k: [] for k in fs}
        for _ in range(args.reps):
            for k, (f, d) in fs.items():
                ts[k] += timed(f, th[k], d, 1, args.calls)
        row = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in ts.items()}
        row["pass_median"] = row["templates"]["median"]
        row["added_median"] = row["templates"]["median"] - row["plain"]["median"]
        kern = back_kernel_ms(fs["templates"][0], th["templates"], fs["templates"][1], 3)
        row["back_kernel"] = kern
        row["back_kernel_share"] = None if kern is None else kern / row["templates"]["median"]
        result["batches"][str(nw)] = row
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
            print(f"[template_timing] legs {b}: {runs[b][-1]}", file=sys.stderr, flush=True)
        result["walker_legs"] = {"unit": "median ms per call, one process per figure", "order": "P N N P ...",
                                 "parent": runs["P"], "this_build": runs["N"]}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
