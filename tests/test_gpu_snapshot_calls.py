"""Which calls of the C ABI a run with every accumulator on makes, in which order and with which step: a spy in the place of the
plan's library handle.  One shape for both paths: dim 3, ladder [1.0, 0.5, 0.2], 5 replicas, burn-in 4, a swap event every 2
steps; moments every step, histograms every 2 (8 bins over (-5, 5)), the autocovariance every 3 (max_lag 2), the covariance
every 4.  The expected calls and counts below are written out from the rule - an accumulator is added to behind every step whose
step counter is past burn-in and a multiple of its period - not recorded from a run."""
import pytest
import torch

import ptrwm_hip as E

gpu = pytest.mark.gpu

DIM, LADDER, REPLICAS, BURN, SWAP_EVERY, STEPS = 3, [1.0, 0.5, 0.2], 5, 4, 2, 12
EVERY = {"moments": 1, "hist": 2, "acf": 3, "cov": 4}
# the due step counters in (4, 12]: 5..12; 6, 8, 10, 12; 6, 9, 12; 8, 12
DUE = {"moments": 8, "hist": 4, "acf": 3, "cov": 2}


class Spy:
    """Stands where RunPlan keeps its library handle: every function fetched from it records (name, step0 of the run arguments
    at the call, arguments) and calls through."""

    def __init__(self, plan):
        self.lib, self.plan, self.calls = plan._lib, plan, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append((name, int(self.plan._a.step0), args))
            return fn(*args)

        return call


def sampler(device, target):
    from algorithms import ParallelTemperingRWM_GPU_Optimized

    return ParallelTemperingRWM_GPU_Optimized(
        DIM, 1.0, target, beta_ladder=LADDER, swap_every=SWAP_EVERY, burn_in=BURN, device=device, num_replicas=REPLICAS, seed=7,
        trace="none", moments="all", moments_every=EVERY["moments"], hist="all", hist_range=(-5.0, 5.0), hist_bins=8,
        hist_every=EVERY["hist"], acf="all", acf_every=EVERY["acf"], acf_max_lag=2, cov="all", cov_every=EVERY["cov"])


def spied_advance(alg, monkeypatch):
    alg._ensure_started()
    spy = Spy(alg._run._plan)
    monkeypatch.setattr(alg._run._plan, "_lib", spy)
    alg._run.advance(STEPS)
    torch.cuda.synchronize()
    return spy.calls


def check_counts(run):
    n_t = len(LADDER)
    assert run.moments()["count"].tolist() == [REPLICAS * DUE["moments"]] * n_t
    assert run.histogram()["count"].tolist() == [REPLICAS * DUE["hist"]] * n_t
    # (lag k pairs every snapshot but the first k)
    assert run.autocorr_sums()["pairs"].tolist() == [REPLICAS * DUE["acf"], REPLICAS * (DUE["acf"] - 1), REPLICAS * (DUE["acf"] - 2)]
    assert run.covariance_sums()["count"].tolist() == [REPLICAS * DUE["cov"]]


@gpu
def test_a_fused_run_is_one_call_with_every_snapshot_block(device, monkeypatch):
    from target_distributions import RoughCarpetDistributionTorch

    alg = sampler(device, RoughCarpetDistributionTorch(DIM, device=device))
    calls = spied_advance(alg, monkeypatch)
    assert not alg._run.split
    assert [c[0] for c in calls] == ["ptrwm_run_with_covariance"]
    # (target, proposal, args, moments, chain_moments, flow, hist, adapt, ladder, acf, cov, stream)
    target, proposal, args, moments, chain_moments, flow, hist, adapt, ladder, acf, cov, stream = calls[0][2]
    assert all(p is not None for p in (target, proposal, args, moments, hist, acf, cov))
    assert chain_moments is None and flow is None and adapt is None and ladder is None
    check_counts(alg._run)


@gpu
def test_split_steps_call_the_four_accumulators_behind_every_step(device, monkeypatch):
    from interfaces import TorchTargetDistribution

    class User(TorchTargetDistribution):
        def get_name(self):
            return "User"

        def log_density(self, x):
            return -0.5 * (torch.as_tensor(x, device=self.device) ** 2).sum(-1)

        def density(self, x):
            return torch.exp(self.log_density(x))

    with pytest.warns(UserWarning, match="no fused kernel"):
        alg = sampler(device, User(DIM, device))
        alg._ensure_started()
    alg._run.use_graph = False
    calls = spied_advance(alg, monkeypatch)
    assert alg._run.split
    per_step = ["ptrwm_split_propose", "ptrwm_split_accept", "ptrwm_split_moments", "ptrwm_histogram", "ptrwm_autocorr", "ptrwm_covariance"]
    assert [c[0] for c in calls] == per_step * STEPS
    accumulators = per_step[2:]
    assert [(name, step0) for name, step0, _ in calls if name in accumulators] == [(name, s) for s in range(STEPS) for name in accumulators]
    check_counts(alg._run)
