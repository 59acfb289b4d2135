"""Cost of the pooled log-density sums along the ladder (include/ptrwm.h ptrwm_energy_args) at the headline shape (BASELINE
configs[2]: 65 536 ladders x 32 temperatures, folded RoughCarpet dim 30, Normal proposal, swaps every 10, 2 000 steps per launch):
ms per launch of
  none        plain ptrwm_run (the production kernel)
  every10     the sums in 16 groups, a snapshot every 10 steps
  every100    ... every 100 steps
and the two kernels of one snapshot alone, timed over back-to-back calls of ptrwm_energy on due steps and reported against the
bytes they read - n_chains n_temps floats of logp, 8 MiB at this shape - in TB/s and as a fraction of the 8 TB/s HBM peak of
DESIGN 3.4:
  snap        ref set (the first kernel returns at once), 16 groups
  snap_ref    ref cleared before every call: the one-workgroup kernel that chooses it runs too (once per run in practice)
Each run: `--warmup` launches, then `--steps` launches timed with HIP events, the median reported; one JSON line per run.
`--pkg DIR` imports ptrwm_hip from another tree (a build of the parent commit: the runs it lacks are skipped), for parent -
this - parent readings on one card in one session."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_TB_S = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "rwm-pt-pytorch_amd"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2000)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--temps", type=int, default=32)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--snap-calls", type=int, default=20)
    ap.add_argument("--runs", default="none,every10,every100,snap,snap_ref")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import numpy as np
    import torch

    import ptrwm_hip as E

    dev = torch.device("cuda:0")
    Cn, T, D, G = args.chains, args.temps, args.dim, args.groups
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(D, device=dev, mode_centers=[-15.0, 0.0, 15.0]).engine_target()
    betas = np.geomspace(1.0, 0.01, T).astype(np.float32)
    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(np.sqrt(2.38 ** 2 / D / betas), device=dev, dtype=torch.float32))
    runs = {"none": None, "every10": 10, "every100": 100, "snap": 1, "snap_ref": 1}
    for run in args.runs.split(","):
        if run not in runs:
            raise SystemExit(f"unknown run {run}")
        st = torch.zeros(Cn, T, D, device=dev)
        lp = E.logdensity(tgt, st.view(-1, D)).view(Cn, T).contiguous()
        stats = dict(n_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                     sq_jump=torch.zeros(Cn, T, dtype=torch.float64, device=dev),
                     swap_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                     last_swap_ordinal=torch.zeros(Cn, T, dtype=torch.int64, device=dev))
        plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(betas, device=dev), swap_every=10, seed=7, **stats)
        keep = None
        if runs[run] is not None:
            if not hasattr(plan, "set_energy"):
                print(json.dumps({"run": run, "skipped": "no log-density sums in this build"}), flush=True)
                continue
            keep = dict(count=torch.zeros(G, T, dtype=torch.int64, device=dev), ref=torch.zeros(T, dtype=torch.float64, device=dev),
                        ref_set=torch.zeros(1, dtype=torch.int32, device=dev), nonfinite=torch.zeros(1, dtype=torch.int64, device=dev),
                        **{k: torch.zeros(G, T, dtype=torch.float64, device=dev) for k in ("s1", "s2", "colder", "hotter")})

            def bind(every):
                plan.set_energy(keep["count"], keep["s1"], keep["s2"], keep["colder"], keep["hotter"], ref=keep["ref"],
                                ref_set=keep["ref_set"], nonfinite=keep["nonfinite"], every=every)

            bind(runs[run])
        if run.startswith("snap"):
            # log-densities worth summing: 200 steps from the start spread the replicas over the modes' neighbourhoods
            plan.set_energy(None)
            plan.launch(0, 200)
            bind(1)
            step = 200
            for _ in range(3):
                plan.split_energy(step)
                step += 1
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.snap_calls)]
            for e0, e1 in ev:
                if run == "snap_ref":
                    keep["ref_set"].zero_()
                e0.record()
                plan.split_energy(step)
                e1.record()
                step += 1
            torch.cuda.synchronize()
            t = sorted(a.elapsed_time(b) for a, b in ev)
            med = t[len(t) // 2]
            read = Cn * T * 4
            tb_s = read / (med * 1e-3) / 1e12
            print(json.dumps({"run": run, "groups": G, "ms_per_snapshot_median": med, "ms_min": t[0], "ms_max": t[-1], "bytes_read": read,
                              "TB_per_s": tb_s, "fraction_of_peak": tb_s / HBM_PEAK_TB_S, "count": int(keep["count"].sum().item()),
                              "overflow": bool(torch.isinf(keep["colder"]).any() or torch.isinf(keep["hotter"]).any()), "lib": E.LIB_PATH}),
                  flush=True)
        else:
            step, ms = 0, []
            for k in range(args.warmup + args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
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
            if keep is not None:
                out["snapshots_per_launch"] = args.inner // runs[run]
                out["count"] = int(keep["count"].sum().item())
            print(json.dumps(out), flush=True)
        del plan, st, lp, stats, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
