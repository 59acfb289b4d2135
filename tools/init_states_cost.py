"""Cost of drawing the starting points (ptrwm_init_states, attempt 0) against a device-to-device copy of the same state
array: the draw writes every byte of `state` once and reads nothing, the copy reads and writes it, so the copy's time is
the yardstick for "bound by moving the bytes".  Median of --runs timed calls after --warmup, HIP events around each call.

    python tools/init_states_cost.py [--chains 65536 --temps 32 --dim 30] [--out profiles/NAME.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwm-pt-pytorch_amd"))
import ptrwm_hip as E  # noqa: E402


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--temps", type=int, default=32)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Cn, T, D = a.chains, a.temps, a.dim
    lines = [f"# tools/init_states_cost.py  {torch.cuda.get_device_name(0)}  state [{Cn}, {T}, {D}]  "
             f"median (min .. max) of {a.runs} calls after {a.warmup}, HIP events"]
    for dt in (torch.float32, torch.float64):
        state = torch.zeros(Cn, T, D, device=dev, dtype=dt)
        other = torch.ones(Cn, T, D, device=dev, dtype=dt)
        logp = torch.zeros(Cn, T, device=dev)
        plan = E.RunPlan(None, E.Proposal(E.PROPOSAL_NORMAL, temp_scale=torch.ones(T, device=dev)), state=state, logp=logp,
                         beta=torch.ones(T, device=dev), seed=1)
        lo, hi = torch.full((D,), -20.0, device=dev), torch.full((D,), 20.0, device=dev)
        mib = state.numel() * state.element_size() / 2**20
        rows = [("state.copy_(other)", lambda: state.copy_(other)),
                ("init_states attempt 0, shared", lambda: plan.init_states(lo, hi)),
                ("init_states attempt 0, per temperature", lambda: plan.init_states(lo, hi, per_temperature=True))]
        logp.fill_(float("-inf"))
        rows.append(("init_states attempt 1, every row redrawn", lambda: plan.init_states(lo, hi, attempt=1)))
        for name, fn in rows:
            med, mn, mx = timed(fn, a.warmup, a.runs)
            lines.append(f"{str(dt):14s} {mib:8.1f} MiB  {name:42s} {med:8.4f} ms  ({mn:.4f} .. {mx:.4f})")
        logp.zero_()
        med, mn, mx = timed(lambda: plan.init_states(lo, hi, attempt=1), a.warmup, a.runs)
        lines.append(f"{str(dt):14s} {mib:8.1f} MiB  {'init_states attempt 1, nothing to redraw':42s} {med:8.4f} ms  ({mn:.4f} .. {mx:.4f})")
        del state, other, plan
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
