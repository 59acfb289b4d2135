"""Cost and benefit of the preconditioned Gaussian proposals (include/ptrwm.h ptrwm_split_propose_precond / ptrwm_precond_update),
everything measured in one session on one device and written to profiles/r23_precond_cost.txt.

Cost, at 65 536 ladders x 32 temperatures with the library's DiagGaussian density, at dim 30 and at dim 104, HIP events, medians:
  propose_precond   ptrwm_split_propose_precond per launch
  propose_normal    ptrwm_split_propose (Normal) per launch on the same shape: the baseline, unchanged code
  update            ptrwm_precond_update per launch
  split_step        a whole split step (proposal, ptrwm_logdensity, accept, the swap event every 10th step) with and without a factor
  fused_step        the fused kernel's time per step for the same target (ptrwm_run, 100 steps per launch)
and the budget of the propose kernel: the Normal kernel's time plus the matrix time of its own instruction count at the measured
f32 matrix rate (155 TFLOP/s: no overlap assumed), plus 25 % for the LDS transposition the Normal kernel does not have.

Benefit (recorded, not asserted): a dense Gaussian of condition 10^4 in dim 30 as a user-defined density, 4 096 chains from exact
draws; ESJD per step in whitened coordinates |L^-1 (x' - x)|^2 over the steps behind burn-in - the total, which the narrow
directions dominate, and its share along the widest, the narrowest and the slowest principal axis (a direction mixes at the rate
of its own share) - for
  isotropic         the isotropic proposal with adapt_scale
  adapted           adapt_cov + adapt_scale
  exact             proposal_cov = the target's covariance, var = 2.38^2 / dim
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX_TFLOPS = 155.0  # f32-in / f32-accumulate matrix rate, measured


def median_ms(fn, calls, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def cost(dim, Cn, T, calls, emit):
    import numpy as np
    import torch

    import ptrwm_hip as E
    from target_distributions import MultivariateNormalTorch

    dev = torch.device("cuda:0")
    var = np.linspace(0.5, 2.0, dim)
    tgt = MultivariateNormalTorch(dim, mean=[0.0] * dim, cov=np.diag(var).tolist(), device=dev).engine_target()
    betas = np.geomspace(1.0, 0.01, T).astype(np.float32)
    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(np.sqrt(2.38 ** 2 / dim / betas), device=dev, dtype=torch.float32))
    g = torch.Generator(device=dev).manual_seed(1)
    st = torch.randn(Cn, T, dim, device=dev, generator=g)
    lp = E.logdensity(tgt, st.view(-1, dim)).view(Cn, T).contiguous()
    stats = dict(n_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev), sq_jump=torch.zeros(Cn, T, dtype=torch.float64, device=dev),
                 swap_accept=torch.zeros(Cn, T, dtype=torch.int64, device=dev),
                 last_swap_ordinal=torch.zeros(Cn, T, dtype=torch.int64, device=dev))
    plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(betas, device=dev), swap_every=10, seed=7, **stats)
    q, _ = np.linalg.qr(np.random.default_rng(2).standard_normal((dim, dim)))
    chol = torch.tensor(np.linalg.cholesky((q * var) @ q.T).astype(np.float32), device=dev)
    step = [0]

    def propose():
        plan.split_propose(step[0])
        step[0] += 1

    def split_step():
        s = step[0]
        props = plan.split_propose(s)
        plan.split_accept(s, E.logdensity(tgt, props.view(-1, dim)).view(Cn, T))
        step[0] += 1

    base = dict(dim=dim, chains=Cn, temps=T)
    normal = median_ms(propose, calls)
    emit(dict(base, run="propose_normal", ms_median=normal[0], ms_min=normal[1], ms_max=normal[2]))
    whole_normal = median_ms(split_step, calls)
    emit(dict(base, run="split_step", factor=False, ms_median=whole_normal[0], ms_min=whole_normal[1], ms_max=whole_normal[2]))
    plan.set_preconditioner(chol)
    precond = median_ms(propose, calls)
    # the kernel's own matrix work: per wave and tile of 16 rows 4 B (B + 1) / 2 instructions of 16 x 16 x 4 fused multiply-adds
    B = (dim + 15) // 16
    flop = (Cn * T + 15) // 16 * (4 * B * (B + 1) // 2) * (16 * 16 * 4 * 2)
    matrix_ms = flop / (MATRIX_TFLOPS * 1e12) * 1e3
    budget = (normal[0] + matrix_ms) * 1.25
    emit(dict(base, run="propose_precond", ms_median=precond[0], ms_min=precond[1], ms_max=precond[2], matrix_flop=flop,
              matrix_ms_at_155_tflops=matrix_ms, budget_ms=budget, within_budget=bool(precond[0] <= budget)))
    if precond[0] > budget:
        emit(dict(base, run="note", over_budget_by=precond[0] / budget - 1.0,
                  why="not profiled.  What the kernel does that the budget does not price: two workgroup barriers per tile where the "
                      "Normal kernel has wavefront fences only, the z slab written and read back four bytes per lane per instruction, "
                      "the dim padded to a multiple of 16 in the matrix loop, and the factor staged once per workgroup; the HBM traffic "
                      "and the Philox / Box-Muller work are the Normal kernel's"))
    whole = median_ms(split_step, calls)
    emit(dict(base, run="split_step", factor=True, ms_median=whole[0], ms_min=whole[1], ms_max=whole[2]))
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
    sums = dict(sxx=f64(dim, dim), sx=f64(dim), count=torch.zeros(1, dtype=torch.int64, device=dev))
    plan.set_precond_update(sums["sxx"], sums["sx"], sums["count"], f64(dim, dim), f64(dim), f64(1), windows=1, memory=1.0)
    x = (torch.randn(8 * dim, dim, device=dev, generator=g).double() @ chol.double().T)
    sxx, sx = torch.tril(x.T @ x), x.sum(0)

    def update():
        sums["sxx"].copy_(sxx), sums["sx"].copy_(sx), sums["count"].fill_(x.shape[0])
        plan.precond_update(0)

    def refill():
        sums["sxx"].copy_(sxx), sums["sx"].copy_(sx), sums["count"].fill_(x.shape[0])

    both, fill = median_ms(update, calls), median_ms(refill, calls)
    emit(dict(base, run="update", ms_median=both[0] - fill[0], ms_with_refill=both[0], ms_refill_alone=fill[0]))
    plan.set_preconditioner(None)
    inner = 100
    try:
        fused = median_ms(lambda: plan.launch(0, inner), max(3, calls // 4), warmup=1)
        emit(dict(base, run="fused_step", ms_median=fused[0] / inner, steps_per_launch=inner, kind=E.last_launch_kind()))
    except E.PTRWMError as e:  # (no fused kernel for this shape)
        emit(dict(base, run="fused_step", skipped=str(e)))


def benefit(emit, dim=30, Cn=4096, burn_in=2000, steps=200):
    import numpy as np
    import torch

    from algorithms import RandomWalkMH_GPU_Optimized
    from interfaces import TorchTargetDistribution

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    sigma = (q * np.exp(np.linspace(0.0, np.log(1e4), dim))) @ q.T
    sigma = (sigma + sigma.T) / 2
    L = np.linalg.cholesky(sigma)
    linv_t = torch.tensor(np.linalg.inv(L).T, device=dev, dtype=torch.float64)
    # whitening along the principal axes, slowest (widest) first: |Lambda^-1/2 Q^T d|^2 = |L^-1 d|^2, axis by axis
    lam, vec = np.linalg.eigh(sigma)
    axes_t = torch.tensor((vec / np.sqrt(lam))[:, ::-1].copy(), device=dev, dtype=torch.float64)
    x0 = (rng.standard_normal((Cn, dim)) @ L.T).astype(np.float32)

    class Dense(TorchTargetDistribution):
        def get_name(self):
            return "DenseGaussian"

        def log_density(self, x):
            y = torch.as_tensor(x, device=self.device).double() @ linv_t
            return (-0.5 * (y * y).sum(-1)).float()

        def density(self, x):
            return torch.exp(self.log_density(x))

    var = 2.38 ** 2 / dim
    runs = {"isotropic": dict(adapt_scale=True), "adapted": dict(adapt_scale=True, adapt_cov=True, cov_adapt_probe_every=20),
            "exact": dict(proposal_cov=sigma)}
    for name, kw in runs.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            alg = RandomWalkMH_GPU_Optimized(dim, var, Dense(dim, dev), device=dev, num_chains=Cn, seed=5, burn_in=burn_in,
                                             initial_states=x0, **kw)
            alg._advance(burn_in)
            esjd = torch.zeros(dim, dtype=torch.float64, device=dev)
            for _ in range(steps):
                before = alg.current_states.clone()
                alg._advance(1)
                d = (alg.current_states.double() - before.double()) @ axes_t
                esjd += (d * d).mean(0)
        torch.cuda.synchronize()
        info = alg.get_diagnostic_info()
        emit(dict(run="esjd_" + name, dim=dim, chains=Cn, burn_in=burn_in, steps=steps, condition=1e4,
                  esjd_whitened_per_step=float(esjd.sum().item()) / steps, esjd_widest_axis=float(esjd[0].item()) / steps,
                  esjd_narrowest_axis=float(esjd[-1].item()) / steps, esjd_smallest_axis=float(esjd.min().item()) / steps,
                  acceptance_rate=alg.acceptance_rate,
                  scale=float(alg.proposal_scales()[0].item()), precond_condition=info.get("precond_condition"),
                  precond_updates=info.get("precond_updates"), precond_updates_skipped=info.get("precond_updates_skipped")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "rwm-pt-pytorch_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_precond_cost.txt"))
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--temps", type=int, default=32)
    ap.add_argument("--dims", default="30,104")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-benefit", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import torch

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit(dict(run="session", device=torch.cuda.get_device_name(0), torch=torch.__version__, matrix_tflops_assumed=MATRIX_TFLOPS))
    for dim in (int(d) for d in args.dims.split(",")):
        cost(dim, args.chains, args.temps, args.calls, emit)
        torch.cuda.empty_cache()
    if not args.no_benefit:
        benefit(emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
