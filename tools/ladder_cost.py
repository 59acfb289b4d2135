"""Cost of tuning the temperature ladder during burn-in (ptrwm_run_with_ladder) against plain burn-in of the same length: the
headline shape (65 536 ladders x 32 temperatures, dim 30, RoughCarpet), burn_in steps in one call, ladder_every in --every with
one probe per window.  A probe step ends a launch and is followed by the probe kernel (the [n_chains, n_temps] float logp read
once: 8 MiB at the headline shape) and, at the window's end, the one-workgroup update kernel; the launches themselves are the
plain burn-in launches.  No step kernel differs between the two, so the plain burn-in timed here is the one any build of the
same kernels runs.  The variants alternate within every round; median (min .. max) over --runs rounds after --warmup, HIP events
around each call (a call is ~0.1 s of GPU work at the default shape).

    python tools/ladder_cost.py [--chains 65536 --temps 32 --dim 30 --burn-in 2000 --every 50 100 200] [--out profiles/NAME.txt]
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
    ap.add_argument("--every", type=int, nargs="+", default=[50, 100, 200])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Cn, T, D, burn = a.chains, a.temps, a.dim, a.burn_in
    target = RoughCarpetDistributionTorch(D, device=dev, mode_centers=[-15.0, 0.0, 15.0]).engine_target()
    betas = geometric_beta_ladder(T, 0.01)
    init_beta = torch.tensor(betas, device=dev, dtype=torch.float32)
    init_scale = torch.sqrt(torch.tensor([2.38 ** 2 / D / b for b in betas], device=dev, dtype=torch.float32))
    state = torch.zeros(Cn, T, D, device=dev)
    logp = E.logdensity(target, state.view(-1, D)).view(Cn, T).contiguous()
    stats = {k: torch.zeros(Cn, T, device=dev, dtype=torch.float64 if k == "sq_jump" else torch.int64)
             for k in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")}

    def plan(every):
        prop, beta = E.Proposal(E.PROPOSAL_NORMAL, temp_scale=init_scale.clone()), init_beta.clone()
        p = E.RunPlan(target, prop, state=state, logp=logp, beta=beta, burn_in=burn, swap_every=100, seed=7, **stats)
        if every:
            p.set_ladder(torch.zeros(T, device=dev, dtype=torch.int64), every=every, until=burn)
        return p, prop, beta

    variants = [(0, *plan(0))] + [(v, *plan(v)) for v in a.every]
    ms = {v: [] for v, _, _, _ in variants}
    for r in range(a.warmup + a.runs):
        for v, p, prop, beta in variants:
            prop.temp_scale.copy_(init_scale)  # every call is the same warm-up: from the initial ladder, steps 0 .. burn_in - 1
            beta.copy_(init_beta)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            p.launch(0, burn)
            t1.record()
            t1.synchronize()
            if r >= a.warmup:
                ms[v].append(t0.elapsed_time(t1))
    lines = [f"# tools/ladder_cost.py  {torch.cuda.get_device_name(0)}  {Cn} ladders x {T} temperatures, dim {D}, RoughCarpet; "
             f"{burn} burn-in steps in one call; median (min .. max) of {a.runs} rounds after {a.warmup}, variants alternating, HIP events",
             f"# library sources {E.source_hash()[:16]}"]
    base = statistics.median(ms[0])
    for v, _, _, _ in variants:
        med, mn, mx = statistics.median(ms[v]), min(ms[v]), max(ms[v])
        name = "plain burn-in" if v == 0 else f"ladder_every = {v} ({burn // v} windows)"
        extra = "" if v == 0 else f"  {100.0 * (med / base - 1.0):+6.2f} %  {1000.0 * (med - base) / (burn // v):7.1f} us per window"
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
