"""Cost of tuning the proposal scale during burn-in (ptrwm_run_with_adaptation) against plain burn-in of the same length:
the headline shape (65 536 ladders x 32 temperatures, dim 30, RoughCarpet), burn_in steps in one call, adapt_every in
--every.  A window ends a launch and is followed by the reduce kernel (the [n_chains, n_temps] int64 scratch read and zeroed:
16 MiB each way at the headline shape) and the update kernel; a warm-up launch also adds its acceptance counts to the scratch,
which a plain burn-in launch does not.  No step kernel differs between the two, so the plain burn-in timed here is the one any
build of the same kernels runs.  The variants alternate within every round; median (min .. max) over --runs rounds after
--warmup, HIP events around each call (a call is ~0.1 s of GPU work at the default shape).

    python tools/adapt_cost.py [--chains 65536 --temps 32 --dim 30 --burn-in 2000 --every 25 50 200] [--out profiles/NAME.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwm-pt-pytorch_amd"))
import ptrwm_hip as E  # noqa: E402
from algorithms import geometric_beta_ladder  # noqa: E402
from target_distributions import RoughCarpetDistributionTorch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--temps", type=int, default=32)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--burn-in", type=int, default=2000)
    ap.add_argument("--every", type=int, nargs="+", default=[25, 50, 200])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Cn, T, D, burn = a.chains, a.temps, a.dim, a.burn_in
    target = RoughCarpetDistributionTorch(D, device=dev, mode_centers=[-15.0, 0.0, 15.0]).engine_target()
    betas = geometric_beta_ladder(T, 0.01)
    init = torch.sqrt(torch.tensor([2.38 ** 2 / D / b for b in betas], device=dev, dtype=torch.float32))
    state = torch.zeros(Cn, T, D, device=dev)
    logp = E.logdensity(target, state.view(-1, D)).view(Cn, T).contiguous()
    beta = torch.tensor(betas, device=dev, dtype=torch.float32)
    stats = {k: torch.zeros(Cn, T, device=dev, dtype=torch.float64 if k == "sq_jump" else torch.int64)
             for k in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")}

    def plan(every):
        prop = E.Proposal(E.PROPOSAL_NORMAL, temp_scale=init.clone())
        p = E.RunPlan(target, prop, state=state, logp=logp, beta=beta, burn_in=burn, swap_every=100, seed=7, **stats)
        if every:
            p.set_adaptation(torch.zeros(Cn, T, device=dev, dtype=torch.int64), torch.zeros(T + 1, device=dev, dtype=torch.int64),
                             every=every, until=burn, min_scale=1e-6, max_scale=1e6)
        return p, prop

    variants = [(0, *plan(0))] + [(w, *plan(w)) for w in a.every]
    ms = {w: [] for w, _, _ in variants}
    for r in range(a.warmup + a.runs):
        for w, p, prop in variants:
            prop.temp_scale.copy_(init)  # every call is the same warm-up: from the initial scales, steps 0 .. burn_in - 1
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            p.launch(0, burn)
            t1.record()
            t1.synchronize()
            if r >= a.warmup:
                ms[w].append(t0.elapsed_time(t1))
    lines = [f"# tools/adapt_cost.py  {torch.cuda.get_device_name(0)}  {Cn} ladders x {T} temperatures, dim {D}, RoughCarpet; "
             f"{burn} burn-in steps in one call; median (min .. max) of {a.runs} rounds after {a.warmup}, variants alternating, HIP events",
             f"# library sources {E.source_hash()[:16]}"]
    base = statistics.median(ms[0])
    for w, _, _ in variants:
        med, mn, mx = statistics.median(ms[w]), min(ms[w]), max(ms[w])
        name = "plain burn-in" if w == 0 else f"adapt_every = {w} ({burn // w} windows)"
        extra = "" if w == 0 else f"  {100.0 * (med / base - 1.0):+6.2f} %  {1000.0 * (med - base) / (burn // w):7.1f} us per window"
        lines.append(f"{name:34s} {med:9.3f} ms  ({mn:.3f} .. {mx:.3f}){extra}")
    lines.append(f"# spread of plain burn-in: {100.0 * (max(ms[0]) - min(ms[0])) / base:.2f} % of its median")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
