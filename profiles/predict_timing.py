"""What posterior-predictive bands cost (Fitter.predict, sampling.column_quantiles_device) against the routes a user had before them.

(a) The quantile stage alone: sampling.column_quantiles_device on draws F[S, M] that live on the device (from the call to the numpy
    arrays it returns, so the stream is drained) against copying F to the host and np.quantile(F, q, axis=0); S in {512, 4096},
    M in {300, 4096}, the three default levels, lognormal draws.
(b) Fitter.predict with 512 draws on 100 times x 3 frequencies, on the C4 fitter of bench.py (draws in a small ball around the truth),
    against the loop of 512 Fitter.flux_density_grid calls followed by np.quantile that it replaces; and the quantile stage's share of
    the call (its time at 512 x 300 from (a) over the call's).

All in this one process.  Per comparison a warm-up of both routes, then --rounds (5; the 512-call loop: --loop-rounds, 3) rounds in
which the routes alternate; medians (min - max).  A markdown table and one JSON line at the end.

Run from the repository root: python profiles/predict_timing.py [--out FILE]"""
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

LEVELS = (0.16, 0.5, 0.84)
SHAPES = ((512, 300), (512, 4096), (4096, 300), (4096, 4096))


def alternate(routes, rounds):
    """{name: (median, min, max)} in ms of the routes run in turn, `rounds` times, after one warm-up of each"""
    for fn in routes.values():
        fn()
    ms = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in ms.items()}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--draws", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"rounds": args.rounds, "loop_rounds": args.loop_rounds, "quantile_stage": {}, "predict": {}}
    table = ["| draws × columns | device, ms | copy + np.quantile, ms | host / device |", "|---|---|---|---|"]
    for S, M in SHAPES:
        F = torch.from_numpy(np.random.default_rng(S + M).lognormal(-60.0, 3.0, (S, M))).cuda()
        torch.cuda.synchronize()
        keep = {}
        got = alternate({"device": lambda: keep.update(dev=sampling.column_quantiles_device(F, LEVELS)[0]),
                         "host": lambda: keep.update(host=np.quantile(F.cpu().numpy(), LEVELS, axis=0))}, args.rounds)
        assert np.allclose(keep["dev"], keep["host"], rtol=1e-14, atol=0.0)
        result["quantile_stage"][f"{S}x{M}"] = got
        d, h = got["device"], got["host"]
        table.append(f"| {S} × {M} | {d[0]:.2f} ({d[1]:.2f} – {d[2]:.2f}) | {h[0]:.1f} ({h[1]:.1f} – {h[2]:.1f}) | {h[0] / d[0]:.0f} |")
        print(table[-1], flush=True)
        del F
        torch.cuda.empty_cache()
    lib = _lib.load()
    h, _ = va.get_context(0)
    fit, defs, _ = bench.c4_fitter(lib, h, _lib)
    _, lo, hi = fit.build_spec(defs)
    truth = np.array([np.log10(configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)]) if lg
                      else configs.C4_TRUTH[{"theta_v": "theta_obs"}.get(n, n)] for n, lg, _, _ in configs.C4_FREE])
    samples = sampling.initial_positions(lo, hi, args.draws, np.random.default_rng(args.draws), center=truth, spread=0.02)
    t, nu = np.logspace(4.5, 7.5, 100), np.array(configs.C4_BANDS, dtype=np.float64)
    keep = {}

    def loop():
        keep["draws"] = np.stack([fit.flux_density_grid(s, t, nu, defs).total for s in samples])
        keep["loop"] = np.quantile(keep["draws"], LEVELS, axis=0)

    call = alternate({"predict": lambda: keep.update(pred=fit.predict(samples, defs, t, nu, quantiles=LEVELS))}, args.rounds)["predict"]
    single = alternate({"loop": loop}, args.loop_rounds)["loop"]
    rel = float(np.max(np.abs(keep["pred"].bands / keep["loop"] - 1.0)))
    # draw by draw, reported and not gated: a grid request differs across batch sizes by the cut of its partial sums,
    # and a batch of this size has its ODE rows solved by the engine's refill kernel where a single model's go through the fast kernel
    # (run_model_stages: by the batch's row count) -- two solvers that agree to their tolerance (rtol 1e-6), not to the bit.  The count
    # of draws whose 10^theta the device rounds to another last bit than the host is printed beside it.
    both = fit.predict(samples, defs, t, nu, quantiles=LEVELS, return_draws=True).draws
    per_draw = np.max(np.abs(both / keep["draws"] - 1.0), axis=(1, 2))
    is_log = np.array([lg for _, lg, _, _ in configs.C4_FREE], dtype=bool)
    on_device = torch.pow(10.0, torch.from_numpy(samples[:, is_log]).cuda()).cpu().numpy()
    other_bit = np.any(on_device != 10.0 ** samples[:, is_log], axis=1)
    far = per_draw > 1e-10
    print(f"valid draws {keep['pred'].n_valid} of {args.draws}; max |bands / loop's bands - 1| {rel:.3g}; draws beyond 1e-10 of their "
          f"single-model call: {int(far.sum())} (max {per_draw.max():.3g}), the others at most {per_draw[~far].max():.3g}; draws with a "
          f"10^theta of another last bit on the device: {int(other_bit.sum())}, of the far ones {int((far & other_bit).sum())}", flush=True)
    assert keep["pred"].n_valid == args.draws and rel <= 1e-4  # (a sanity guard at plot level: a wrong transformer or law is off by orders)
    result["agreement"] = {"bands_max_rel": rel, "draws_beyond_1e-10": int(far.sum()), "draws_max_rel": float(per_draw.max()),
                           "draws_other_max_rel": float(per_draw[~far].max()), "draws_pow_other_bit": int(other_bit.sum()),
                           "far_and_pow_other_bit": int((far & other_bit).sum())}
    stage = result["quantile_stage"]["512x300"]["device"][0]
    result["predict"] = {"draws": args.draws, "nt": int(t.size), "nnu": int(nu.size), "predict_ms": call, "loop_ms": single,
                         "loop_over_predict": single[0] / call[0], "quantile_stage_share": stage / call[0]}
    table += ["", f"Fitter.predict, {args.draws} draws on {t.size} × {nu.size}: {call[0]:.1f} ms ({call[1]:.1f} – {call[2]:.1f}); the loop of "
              f"{args.draws} Fitter.flux_density_grid calls and np.quantile: {single[0]:.0f} ms ({single[1]:.0f} – {single[2]:.0f}); ratio "
              f"{single[0] / call[0]:.1f}; the quantile stage ({stage:.2f} ms at 512 × 300) is {100 * stage / call[0]:.2f} % of the call"]
    print("\n".join(table), flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(table) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
