"""Posterior moments accumulated inside the step kernels (include/ptrwm.h ptrwm_moments_args) on the GPU.

Every case runs the same sampler three times from the same start: with moments of every temperature, with a trace of every
chain and temperature at trace_every = every, and plain.  The accumulators must equal the fp64 sums of the trace rows
after burn-in (to 1e-12 of the sum of |x|; counts exactly), and state, log-densities and every counter of the moments run
must be bit-identical to the plain run's (the accumulation perturbs nothing)."""
import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _target(kind, dim, device):
    from target_distributions import RoughCarpetDistributionTorch

    if kind == "rc":
        return RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0]).engine_target()
    raise ValueError(kind)


def _proposal(name, dim, betas, device):
    if name == "Normal":
        spec = H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim)
    elif name == "Laplace":
        spec = H.proposal_spec("Laplace", dim, betas, base_variance_vector=np.full(dim, 2.38 ** 2 / dim, np.float32))
    else:
        spec = H.proposal_spec("UniformRadius", dim, betas, base_radius=2.38 / np.sqrt(dim))
    return spec.engine(device)


def _one_run(device, tgt, prop, *, x0, beta, cuts, burn, se, seed, f64, mode, every, temps):
    """mode: 'moments' | 'trace' | 'plain'.  Returns numpy results (and the moment sums / the trace)."""
    Cn, T, D = x0.shape
    sdt = torch.float64 if f64 else torch.float32
    st = torch.tensor(x0, device=device, dtype=sdt)
    lp = E.logdensity(tgt, st.view(-1, D).float()).view(Cn, T).contiguous()
    stats = {k: torch.zeros(Cn, T, dtype=dt, device=device) for k, dt in
             (("n_accept", torch.int64), ("sq_jump", torch.float64), ("swap_accept", torch.int64),
              ("last_swap_ordinal", torch.int64))}
    plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(beta, device=device), burn_in=burn, swap_every=se,
                     seed=seed, n_accept=stats["n_accept"], sq_jump=stats["sq_jump"], swap_accept=stats["swap_accept"],
                     last_swap_ordinal=stats["last_swap_ordinal"])
    out = {}
    n_total = sum(cuts)
    if mode == "moments":
        m = {"sum": torch.zeros(temps, D, device=device, dtype=torch.float64),
             "sum_sq": torch.zeros(temps, D, device=device, dtype=torch.float64),
             "sum_logp": torch.zeros(temps, device=device, dtype=torch.float64),
             "count": torch.zeros(temps, device=device, dtype=torch.int64)}
        plan.set_moments(m["sum"], m["sum_sq"], sum_logp=m["sum_logp"], count=m["count"], every=every)
    if mode == "trace":
        rows = n_total // every
        trace = torch.zeros(max(rows, 1), Cn, T, D, device=device, dtype=sdt)
        trace_logp = torch.zeros(max(rows, 1), Cn, T, device=device)
    kinds = []
    s0, row = 0, 0
    for n in cuts:
        if mode == "trace":
            plan.launch(s0, n, trace=trace, trace_logp=trace_logp, trace_row0=row, trace_every=every)
            row += (s0 + n) // every - s0 // every
        else:
            plan.launch(s0, n)
        kinds.append(E.last_launch_kind())
        s0 += n
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in stats.items()}
    out["state"], out["logp"], out["kinds"] = st.cpu().numpy(), lp.cpu().numpy(), kinds
    if mode == "moments":
        out["moments"] = {k: v.cpu().numpy() for k, v in m.items()}
    if mode == "trace":
        out["trace"], out["trace_logp"] = trace.cpu().numpy(), trace_logp.cpu().numpy()
    return out


def _trace_sums(tr, trl, *, every, burn, temps):
    """fp64 sums of the trace rows whose step_counter ((row + 1) * every) is past burn-in: first `temps` temperatures."""
    rows = np.arange(tr.shape[0])
    keep = (rows + 1) * every > burn
    x = tr[keep][:, :, :temps].astype(np.float64)
    lp = trl[keep][:, :, :temps].astype(np.float64)
    return {"sum": x.sum((0, 1)), "sum_sq": (x * x).sum((0, 1)), "sum_logp": lp.sum((0, 1)),
            "abs": np.abs(x).sum((0, 1)), "abs_logp": np.abs(lp).sum((0, 1)),
            "count": np.full(temps, int(keep.sum()) * tr.shape[1], np.int64)}


def _check_against_trace(got, want):
    assert np.array_equal(got["count"], want["count"]), (got["count"], want["count"])
    assert want["count"].min() > 0  # the case accumulates something
    np.testing.assert_array_less(np.abs(got["sum"] - want["sum"]), RTOL * want["abs"] + 1e-300)
    np.testing.assert_array_less(np.abs(got["sum_sq"] - want["sum_sq"]), RTOL * want["sum_sq"] + 1e-300)
    np.testing.assert_array_less(np.abs(got["sum_logp"] - want["sum_logp"]), RTOL * want["abs_logp"] + 1e-300)


FIELDS = ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")

# (id, dim, n_temps, n_chains, proposal, form, f64, cuts, burn, every, swap_every, temps)
CASES = [
    # narrow thread form, dim 5, 8 temperatures, 1 024 ladders; burn-in ends inside the second launch; every = 3 does not
    # divide the launches; a run cut into three advance calls
    ("thread_narrow_d5", 5, 8, 1024, "Normal", E.FORM_THREAD, False, (13, 11, 16), 17, 3, 4, 8),
    # an exact dim (30) in the thread form, the headline ladder, cold chain only
    ("thread_d30_t32_cold", 30, 32, 256, "Normal", E.FORM_THREAD, False, (25,), 5, 2, 5, 1),
    ("thread_d30_t32_all", 30, 32, 256, "UniformRadius", E.FORM_THREAD, False, (12, 13), 5, 2, 5, 32),
    # a wide ladder: 100 temperatures, one ladder per workgroup
    ("thread_wide_t100", 30, 100, 24, "Laplace", E.FORM_THREAD, False, (20,), 3, 4, 3, 100),
    # a generic dim (41) in the lane-split form, forced
    ("quad_d41", 41, 8, 256, "UniformRadius", E.FORM_QUAD, False, (9, 21), 10, 5, 2, 8),
    ("quad_d41_laplace", 41, 6, 128, "Laplace", E.FORM_QUAD, False, (30,), 0, 7, 5, 3),
    # a wide dim (100): the lane-split form is the only one
    ("quad_d100", 100, 4, 96, "Normal", E.FORM_AUTO, False, (14, 14), 6, 4, 2, 4),
    # state_f64: the lane-split form with double states
    ("quad_f64_d30", 30, 8, 128, "Normal", E.FORM_AUTO, True, (11, 19), 4, 3, 3, 8),
    # lane-split form, a ladder of 20 temperatures (one workgroup per group of ladders)
    ("quad_wide_t20", 30, 20, 64, "Normal", E.FORM_QUAD, False, (16,), 2, 2, 4, 20),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_moments_equal_the_trace_and_perturb_nothing(device, case):
    name, dim, T, Cn, pname, form, f64, cuts, burn, every, se, temps = case
    rng = np.random.default_rng(dim * 1000 + T)
    betas = np.geomspace(1.0, 0.05, T).astype(np.float32)
    tgt = _target("rc", dim, device)
    prop = _proposal(pname, dim, betas, device)
    x0 = rng.normal(0.0, 2.0, size=(Cn, T, dim)).astype(np.float64 if f64 else np.float32)
    kw = dict(x0=x0, beta=betas, cuts=cuts, burn=burn, se=se, seed=1234 + dim, f64=f64, every=every, temps=temps)
    with E.kernel_form(form):
        mom = _one_run(device, tgt, prop, mode="moments", **kw)
        tra = _one_run(device, tgt, prop, mode="trace", **kw)
        plain = _one_run(device, tgt, prop, mode="plain", **kw)
    expect = E.LAUNCH_QUAD if (form == E.FORM_QUAD or f64 or dim > 64) else E.LAUNCH_THREAD
    assert mom["kinds"] == [expect] * len(cuts) and plain["kinds"] == mom["kinds"] and tra["kinds"] == mom["kinds"]
    for f in FIELDS:  # no perturbation: bit-identical to the run without moments (and to the traced run)
        assert np.array_equal(mom[f], plain[f]), f
        assert np.array_equal(tra[f], plain[f]), f
    _check_against_trace(mom["moments"], _trace_sums(tra["trace"], tra["trace_logp"], every=every, burn=burn, temps=temps))


def test_moments_of_split_steps_graph_and_eager(device):
    """Dense-covariance Gaussian (no fused kernel: split steps), three temperatures, moments of all: graph replay and
    eager agree to 1e-12 and both equal the sums of a trace of every chain."""
    from algorithms._engine_core import EngineRun
    from target_distributions import MultivariateNormalTorch

    dim, T, Cn, burn, se, every, n = 3, 3, 512, 7, 4, 3, 75
    target = MultivariateNormalTorch(dim, cov=[[1, 0.5, 0], [0.5, 1, 0], [0, 0, 1]], device=device)
    betas = [1.0, 0.5, 0.25]
    prop = _proposal("Normal", dim, np.array(betas, np.float32), device)

    def make(use_graph, mom):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = EngineRun(target_dist=target, proposal=prop, beta_ladder=betas, dim=dim, device=device, n_replicas=Cn,
                          initial_state=np.zeros(dim, np.float32), burn_in=burn, swap_every=se, swap_mode="exchange",
                          swap_order="sequential", seed=77, moments_temps=T if mom else 0, moments_every=every)
        r.use_graph = use_graph
        return r

    g, e, t = make(True, True), make(False, True), make(False, False)
    assert g.density_fn is not None  # split steps
    g.advance(40)
    g.advance(n - 40)
    e.advance(n)
    rows = n // every
    trace = torch.zeros(rows, Cn, T, dim, device=device)
    trace_logp = torch.zeros(rows, Cn, T, device=device)
    t.advance(n, trace=trace, trace_logp=trace_logp, trace_every=every)
    torch.cuda.synchronize()
    for r in (g, e):
        assert torch.equal(r.state, t.state) and torch.equal(r.logp, t.logp) and torch.equal(r.n_accept, t.n_accept)
        assert torch.equal(r.swap_accept, t.swap_accept) and torch.equal(r.sq_jump, t.sq_jump)
    want = _trace_sums(trace.cpu().numpy(), trace_logp.cpu().numpy(), every=every, burn=burn, temps=T)
    mg = {k: v.cpu().numpy() for k, v in g.moments().items() if k != "every"}
    me = {k: v.cpu().numpy() for k, v in e.moments().items() if k != "every"}
    _check_against_trace(mg, want)
    _check_against_trace(me, want)
    assert np.array_equal(mg["count"], me["count"])
    for k in ("sum", "sum_sq", "sum_logp"):
        assert np.all(np.abs(mg[k] - me[k]) <= RTOL * np.maximum(np.abs(me[k]), 1.0)), k


def test_posterior_mean_and_variance_of_a_diagonal_gaussian(device):
    """RWM on a diagonal Gaussian, dim 30, 65 536 chains: the pooled posterior mean and variance match the target within
    a tolerance measured from the spread of independent runs (different chain_offset), not guessed."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    dim, chains, burn, n, every, runs = 30, 65536, 1000, 1000, 5, 8
    mean = np.linspace(-2.0, 2.0, dim)
    var = np.linspace(0.5, 2.0, dim)
    target = MultivariateNormalTorch(dim, mean=mean.tolist(), cov=np.diag(var).tolist(), device=device)
    means, variances = [], []
    for k in range(runs):
        alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, target, burn_in=burn, device=device, num_chains=chains,
                                         seed=5, chain_offset=k * chains, moments="cold", moments_every=every)
        alg._advance(burn + n)
        assert int(alg.moment_count[0].item()) == chains * (n // every)
        means.append(alg.posterior_mean().cpu().numpy())
        variances.append(alg.posterior_variance().cpu().numpy())
        info = alg.get_diagnostic_info()
        assert np.array_equal(info["posterior_mean"][0].numpy(), means[-1])
        del alg
    means, variances = np.array(means), np.array(variances)
    # the standard error of one run's estimate, per coordinate, from the spread of the independent runs (chain_offset:
    # disjoint Philox subsequences); the grand mean over the runs is checked against the target at 8 of its standard
    # errors (Student t with runs - 1 degrees of freedom: a false alarm once in ~10^4 coordinates)
    se_m = means.std(0, ddof=1)
    se_v = variances.std(0, ddof=1)
    dev_m = np.abs(means.mean(0) - mean)
    dev_v = np.abs(variances.mean(0) - var)
    assert np.all(dev_m <= 8 * se_m / np.sqrt(runs)), (dev_m / (se_m / np.sqrt(runs))).max()
    assert np.all(dev_v <= 8 * se_v / np.sqrt(runs)), (dev_v / (se_v / np.sqrt(runs))).max()
    # and the estimates are informative: standard errors well below the posterior's own spread
    assert np.all(se_m < 0.05 * np.sqrt(var)) and np.all(se_v < 0.05 * var)


def test_drop_in_classes_pool_over_every_replica(device):
    """The PT class with moments='all': posterior_mean(t) is the trace-free pooled mean of temperature t, the same sums
    as the C ABI; reset() starts from zero; moments=None changes nothing and offers no estimate."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from interfaces.simulation_gpu import MCMCSimulation_GPU  # noqa: F401  (passthroughs exist)
    from target_distributions import RoughCarpetDistributionTorch

    dim, T, R, burn = 5, 4, 256, 10
    target = RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0])
    kw = dict(beta_ladder=[1.0, 0.6, 0.3, 0.1], swap_every=3, burn_in=burn, device=device, num_replicas=R, seed=9,
              trace="none")
    a = ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, target, moments="all", moments_every=2, **kw)
    b = ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, target, **kw)
    a.generate_samples(40)
    b.generate_samples(40)
    assert torch.equal(a._run.state, b._run.state) and torch.equal(a._run.n_accept, b._run.n_accept)
    assert a.moment_count.tolist() == [R * 20] * T
    for t in range(T):
        assert a.posterior_mean(t).shape == (dim,) and torch.isfinite(a.posterior_variance(t)).all()
    assert a.mean_log_density().shape == (T,)
    with pytest.raises(ValueError):
        a.posterior_mean(T)
    with pytest.raises(RuntimeError):
        b.posterior_mean()
    assert "posterior_mean" not in b.get_diagnostic_info() and "posterior_mean" in a.get_diagnostic_info()
    a.reset()
    assert a.moment_count.tolist() == [0] * T
    a.generate_samples(4)
    assert a.moment_count.tolist() == [R * 2] * T
