"""Cost of replica flow (include/ptrwm.h ptrwm_flow_args) at the headline shape (65 536 ladders x 32 temperatures, folded
RoughCarpet dim 30, Normal proposal, swaps every 10, 2 000 steps per launch): ms per launch of four runs of the same sampler -
  none        plain ptrwm_run (the production kernel)
  full        a cold trace of replica 0 at trace_every = 10: the fixture / trace twin WITHOUT flow
  flow        the twin with flow (ptrwm_run_with_diagnostics, all four arrays), no trace
  cmom_cold   per-chain moments of the cold chain, every = 10: what profiles/ records as the cost of a diagnostic of this kind
Each: `--warmup` launches, then `--steps` launches timed with HIP events; one JSON line per run.  `--pkg DIR` imports ptrwm_hip
from another tree (a build of the parent commit: the runs it lacks are skipped), for parent - this - parent readings on one card
in one session."""
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
    ap.add_argument("--runs", default="none,full,flow,cmom_cold")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import numpy as np
    import torch

    import ptrwm_hip as E

    dev = torch.device("cuda:0")
    Cn, T, D = args.chains, args.temps, args.dim
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(D, device=dev, mode_centers=[-15.0, 0.0, 15.0]).engine_target()
    betas = np.geomspace(1.0, 0.01, T).astype(np.float32)
    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(np.sqrt(2.38 ** 2 / D / betas), device=dev, dtype=torch.float32))
    for run in args.runs.split(","):
        st = torch.zeros(Cn, T, D, device=dev)
        lp = E.logdensity(tgt, st.view(-1, D)).view(Cn, T).contiguous()
        stats = dict(n_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                     sq_jump=torch.zeros(Cn, T, dtype=torch.float64, device=dev),
                     swap_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                     last_swap_ordinal=torch.zeros(Cn, T, dtype=torch.int64, device=dev))
        plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(betas, device=dev), swap_every=10, seed=7, **stats)
        trace, keep = None, None
        total = (args.warmup + args.steps) * args.inner
        if run == "full":
            trace = torch.zeros(total // args.every + 1, 1, 1, D, device=dev)
        elif run == "flow":
            if not hasattr(plan, "set_flow"):
                print(json.dumps({"run": run, "skipped": "no replica flow in this build"}), flush=True)
                continue
            keep = [torch.arange(T, device=dev, dtype=torch.int32).repeat(Cn, 1).contiguous()] + \
                   [torch.zeros(Cn, T, dtype=torch.int64, device=dev) for _ in range(3)]
            plan.set_flow(*keep)
        elif run == "cmom_cold":
            keep = [torch.zeros(Cn, 1, D, device=dev, dtype=torch.float64) for _ in range(2)]
            plan.set_chain_moments(keep[0], keep[1], sum_logp=torch.zeros(Cn, 1, device=dev, dtype=torch.float64),
                                   count=torch.zeros(1, device=dev, dtype=torch.int64), every=args.every)
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
        out = {"run": run, "kind": E.last_launch_kind(), "ms_per_launch_median": med, "ms_min": t[0], "ms_max": t[-1],
               "chain_steps_per_s": Cn * T * args.inner / (med * 1e-3), "lib": E.LIB_PATH}
        if run == "flow":
            events = total // 10
            out["round_trips"] = int(keep[1].sum().item())
            out["events"] = events
            out["up_fraction"] = [round(float(v), 4) for v in (keep[2].sum(0).double() / (keep[2].sum(0) + keep[3].sum(0)).double()).tolist()]
        print(json.dumps(out), flush=True)
        del plan, st, lp, stats, trace, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
