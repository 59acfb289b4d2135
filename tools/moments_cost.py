"""Cost of the posterior-moments accumulator at the headline shape (65 536 ladders x 32 temperatures, folded RoughCarpet
dim 30, Normal proposal, swaps every 10, 2 000 steps per launch): chain-steps/s of six runs of the same sampler -
  none        plain ptrwm_run (the production kernel)
  cold_trace  a cold trace of replica 0 at trace_every = 10 (the fixture / trace twin without moments)
  mom_cold    moments of the cold chain, every = 10 (ptrwm_run_with_moments, temps = 1)
  mom_all     moments of every temperature, every = 10 (temps = 32)
  cmom_cold   per-chain moments of the cold chain, every = 10 (ptrwm_run_with_chain_moments, temps = 1)
  cmom_all    per-chain moments of every temperature, every = 10 (temps = 32)
Each: `--warmup` launches, then `--steps` launches timed with HIP events; one JSON line per run.  `--pkg DIR` imports
ptrwm_hip from another tree (a build of an earlier commit: the runs it lacks are skipped), for before / after numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "rwm-pt-pytorch_amd"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2000)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--temps", type=int, default=32)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--runs", default="none,cold_trace,mom_cold,mom_all,cmom_cold,cmom_all")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import numpy as np
    import torch

    import ptrwm_hip as E

    dev = torch.device("cuda:0")
    Cn, T, D = args.chains, args.temps, args.dim
    m = 15.0
    # folded RoughCarpet (modes -m, 0, +m; equal weights), as bench.py's headline target describes itself
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(D, device=dev, mode_centers=[-m, 0.0, m]).engine_target()
    betas = np.geomspace(1.0, 0.01, T).astype(np.float32)
    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(np.sqrt(2.38 ** 2 / D / betas), device=dev, dtype=torch.float32))
    for run in args.runs.split(","):
        st = torch.zeros(Cn, T, D, device=dev)
        lp = E.logdensity(tgt, st.view(-1, D)).view(Cn, T).contiguous()
        stats = dict(n_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                     sq_jump=torch.zeros(Cn, T, dtype=torch.float64, device=dev),
                     swap_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                     last_swap_ordinal=torch.zeros(Cn, T, dtype=torch.int64, device=dev))
        plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(betas, device=dev), swap_every=10, seed=7,
                         **stats)
        trace = None
        total = (args.warmup + args.steps) * args.inner
        if run == "cold_trace":
            trace = torch.zeros(total // args.every + 1, 1, 1, D, device=dev)
        elif run.startswith("mom_"):
            if not hasattr(plan, "set_moments"):
                print(json.dumps({"run": run, "skipped": "no moments in this build"}), flush=True)
                continue
            mt = 1 if run == "mom_cold" else T
            sums = [torch.zeros(mt, D, device=dev, dtype=torch.float64) for _ in range(2)]
            plan.set_moments(sums[0], sums[1], sum_logp=torch.zeros(mt, device=dev, dtype=torch.float64),
                             count=torch.zeros(mt, device=dev, dtype=torch.int64), every=args.every)
        elif run.startswith("cmom_"):
            if not hasattr(plan, "set_chain_moments"):
                print(json.dumps({"run": run, "skipped": "no per-chain moments in this build"}), flush=True)
                continue
            mt = 1 if run == "cmom_cold" else T
            sums = [torch.zeros(Cn, mt, D, device=dev, dtype=torch.float64) for _ in range(2)]
            plan.set_chain_moments(sums[0], sums[1], sum_logp=torch.zeros(Cn, mt, device=dev, dtype=torch.float64),
                                   count=torch.zeros(mt, device=dev, dtype=torch.int64), every=args.every)
        elif run != "none":
            raise SystemExit(f"unknown run {run}")
        step, row, ms = 0, 0, []
        for k in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if trace is not None:
                plan.launch(step, args.inner, trace=trace, trace_row0=row, trace_every=args.every)
                row += (step + args.inner) // args.every - step // args.every
            else:
                plan.launch(step, args.inner)
            e1.record()
            step += args.inner
            if k >= args.warmup:
                ms.append((e0, e1))
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) for a, b in ms)
        med = t[len(t) // 2]
        print(json.dumps({"run": run, "kind": E.last_launch_kind(), "ms_per_launch_median": med, "ms_min": t[0],
                          "ms_max": t[-1], "chain_steps_per_s": Cn * T * args.inner / (med * 1e-3),
                          "lib": E.LIB_PATH}), flush=True)
        del plan, st, lp, stats, trace
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
