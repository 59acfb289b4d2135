"""Which calls of the C ABI a run with the warm-up tunings on makes, in which order and with which window: a spy in the place of the
plan's library handle (the technique of test_gpu_snapshot_calls.py).  One shape for both paths: dim 2, ladder [1.0, 0.5, 0.25], 3
replicas, burn-in 12, a swap event every 2 steps; the scale tuned in windows of 4 steps up to step 8, the ladder in windows of 6
probed every 3, the proposal factor in windows of 4 probed every 2.  The expected sequences below are written out from the rule -
include/ptrwm.h, the split-step recipe and the launch schedule of a deferred update - not recorded from a run."""
import pytest
import torch

gpu = pytest.mark.gpu

DIM, LADDER, REPLICAS, BURN, SWAP_EVERY = 2, [1.0, 0.5, 0.25], 3, 12, 2
SCALE = dict(adapt_scale=True, adapt_every=4, adapt_until=8)
LADDER_TUNING = dict(adapt_ladder=True, ladder_every=6, ladder_probe_every=3)
FACTOR = dict(adapt_cov=True, cov_adapt_every=4, cov_adapt_probe_every=2)
UPDATES = ("ptrwm_adapt_update", "ptrwm_ladder_update", "ptrwm_precond_update")  # (block, extent, window, stream)


class Spy:
    """Stands where RunPlan keeps its library handle: every function fetched from it records (name, step0 and n_steps of the run
    arguments at the call, arguments) and calls through."""

    def __init__(self, plan):
        self.lib, self.plan, self.calls = plan._lib, plan, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append((name, int(self.plan._a.step0), int(self.plan._a.n_steps), args))
            return fn(*args)

        return call


def sampler(device, **tunings):
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    return ParallelTemperingRWM_GPU_Optimized(
        DIM, 1.0, RoughCarpetDistributionTorch(DIM, device=device), beta_ladder=LADDER, swap_every=SWAP_EVERY, burn_in=BURN,
        device=device, num_replicas=REPLICAS, seed=11, trace="none", **tunings)


def spied(alg, monkeypatch):
    spy = Spy(alg._run._plan)
    monkeypatch.setattr(alg._run._plan, "_lib", spy)
    return spy


def split_rule(steps: int) -> list:
    """(name, window or None, step0 or None) behind every step counter c = 1..steps: the step's accept, the scale's reduce and
    update at the end of its windows, the ladder's probe and - at a window's end - update, the factor's probe and update."""
    out = []
    for c in range(1, steps + 1):
        out.append(("ptrwm_split_accept", None, None))
        if c in (4, 8):
            out += [("ptrwm_adapt_reduce", None, None), ("ptrwm_adapt_update", c // 4 - 1, None)]
        if c in (3, 6, 9, 12):
            out.append(("ptrwm_ladder_probe", None, None))
            if c in (6, 12):
                out.append(("ptrwm_ladder_update", c // 6 - 1, None))
        if c in (2, 4, 6, 8, 10, 12):
            out.append(("ptrwm_covariance", None, c - 1))
            if c in (4, 8, 12):
                out.append(("ptrwm_precond_update", c // 4 - 1, None))
    return out


@gpu
def test_split_steps_call_the_three_tunings_in_order_behind_their_steps(device, monkeypatch):
    with pytest.warns(UserWarning, match="preconditioned proposals run in split steps"):
        alg = sampler(device, **SCALE, **LADDER_TUNING, **FACTOR)
        alg._ensure_started()
    run = alg._run
    run.use_graph = False
    assert run.split
    spy = spied(alg, monkeypatch)
    run.advance(5)  # (ends between two cuts: the sequence does not depend on how the request is split)
    run.advance(9)
    torch.cuda.synchronize()
    expected = split_rule(14)
    names = {name for name, _, _ in expected}
    seen = [c for c in spy.calls if c[0] in names]
    assert [c[0] for c in seen] == [name for name, _, _ in expected]
    for (name, step0, _, args), (_, window, probe_step0) in zip(seen, expected):
        if name in UPDATES:
            assert args[2] == window, (name, args[2], window)
        if name == "ptrwm_covariance":
            assert step0 == probe_step0
    counts = {name: sum(c[0] == name for c in seen) for name in names}
    assert counts == {"ptrwm_split_accept": 14, "ptrwm_adapt_reduce": 2, "ptrwm_adapt_update": 2, "ptrwm_ladder_probe": 4,
                      "ptrwm_ladder_update": 2, "ptrwm_covariance": 6, "ptrwm_precond_update": 3}
    assert run.steps_done == 14


@gpu
def test_fused_steps_with_adapt_sync_stop_at_window_ends_for_the_deferred_updates(device, monkeypatch):
    shapes = []

    def sync(pooled):
        shapes.append(list(pooled.shape))
        return pooled

    alg = sampler(device, **SCALE, **LADDER_TUNING, adapt_sync=sync)
    alg._ensure_started()
    assert not alg._run.split
    spy = spied(alg, monkeypatch)
    alg._run.advance(14)
    torch.cuda.synchronize()
    seen = [(name, (step0, n_steps)) if name.startswith("ptrwm_run") else (name, args[2]) for name, step0, n_steps, args in spy.calls]
    run_with = "ptrwm_run_with_ladder"
    assert seen == [(run_with, (0, 4)), ("ptrwm_adapt_update", 0), (run_with, (4, 2)), ("ptrwm_ladder_update", 0),
                    (run_with, (6, 2)), ("ptrwm_adapt_update", 1), (run_with, (8, 4)), ("ptrwm_ladder_update", 1),
                    (run_with, (12, 2))]  # (no ptrwm_adapt_reduce: the launch reduces by itself)
    assert shapes == [[4], [3], [4], [3]]

    alone = sampler(device, **SCALE, **LADDER_TUNING)
    alone._ensure_started()
    spy = spied(alone, monkeypatch)
    alone._run.advance(14)
    torch.cuda.synchronize()
    assert [(name, step0, n_steps) for name, step0, n_steps, _ in spy.calls] == [(run_with, 0, 14)]
