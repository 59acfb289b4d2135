"""Per-chain posterior moments accumulated inside the step kernels (include/ptrwm.h ptrwm_chain_moments_args) on the GPU.

Exactness: every case of tests/test_gpu_moments.py (and an RWM case under AUTO) runs the same sampler three times from the
same start - with per-chain moments, with a trace of every chain and temperature at trace_every = every, and plain.  The
accumulators must be BIT-EQUAL to a sequential float64 accumulation of the trace rows in step order (a float's square is
exact in float64, so there is nothing to round differently), the counts exact, and state, log-densities and every counter
bit-identical to the plain run.  The sums do not depend on where launches are cut nor on the kernel form.  Meaning: R-hat
flags chains stuck in different modes, and the between-chain ESS predicts the spread of independent runs' means."""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (tests/ on the path)
import ptrwm_hip as E
from test_gpu_moments import CASES as POOLED_CASES
from test_gpu_moments import FIELDS, _check_against_trace, _proposal, _target, _trace_sums

pytestmark = pytest.mark.gpu


def numpy_rhat_ess(x):
    """The estimators' formulas evaluated directly on draws x [M chains, N draws, dim]."""
    M, N = x.shape[:2]
    m_c = x.mean(1)
    s2_c = x.var(1, ddof=1)
    W = s2_c.mean(0)
    B = N * m_c.var(0, ddof=1)
    var_plus = (N - 1) / N * W + B / N
    return np.sqrt(var_plus / W), np.minimum(M * N, M * N * var_plus / B)


def _one_run(device, tgt, prop, *, x0, beta, cuts, burn, se, seed, f64, mode, every, temps):
    """mode: 'chain' | 'trace' | 'plain'.  Returns numpy results (and the per-chain sums / the trace)."""
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
    n_total = sum(cuts)
    if mode == "chain":
        m = {"sum": torch.zeros(Cn, temps, D, device=device, dtype=torch.float64),
             "sum_sq": torch.zeros(Cn, temps, D, device=device, dtype=torch.float64),
             "sum_logp": torch.zeros(Cn, temps, device=device, dtype=torch.float64),
             "count": torch.zeros(temps, device=device, dtype=torch.int64)}
        plan.set_chain_moments(m["sum"], m["sum_sq"], sum_logp=m["sum_logp"], count=m["count"], every=every)
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
    if mode == "chain":
        out["moments"] = {k: v.cpu().numpy() for k, v in m.items()}
    if mode == "trace":
        out["trace"], out["trace_logp"] = trace.cpu().numpy(), trace_logp.cpu().numpy()
    return out


def _sequential_sums(tr, trl, *, every, burn, temps):
    """What the header defines: per (chain, temperature) the float64 sums of the trace rows whose step_counter
    ((row + 1) * every) is past burn-in, added one row after the other in step order."""
    shape = tr.shape[1:2] + (temps,) + tr.shape[3:]
    s, q, l = np.zeros(shape), np.zeros(shape), np.zeros(shape[:2])
    n = 0
    for r in range(tr.shape[0]):
        if (r + 1) * every <= burn:
            continue
        v = tr[r, :, :temps].astype(np.float64)
        s += v
        q += v * v
        l += trl[r, :, :temps].astype(np.float64)
        n += 1
    return {"sum": s, "sum_sq": q, "sum_logp": l, "count": np.full(temps, n, np.int64)}


def _assert_bit_equal(got, want):
    assert np.array_equal(got["count"], want["count"]), (got["count"], want["count"])
    assert want["count"].min() > 0  # the case accumulates something
    for k in ("sum", "sum_sq", "sum_logp"):
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64
        assert np.array_equal(got[k], want[k]), (k, np.abs(got[k] - want[k]).max())
    assert np.abs(want["sum"]).max() > 0 and want["sum_sq"].min() > 0


# the case table of the pooled moments (narrow and wide thread form, lane-split generic dim, dim 100, state_f64, a
# 20-temperature lane-split ladder, launches cut unevenly, burn-in ending inside a launch) and, new, RWM (one temperature)
# at dim 30 under AUTO: 196 608 chains are three wavefronts per SIMD in the thread form; with per-chain moments the
# lane-split form must run (include/ptrwm.h: the thread form's workgroup would need a CU's whole LDS)
CASES = list(POOLED_CASES) + [
    ("rwm_d30_auto", 30, 1, 196608, "Normal", E.FORM_AUTO, False, (7, 9), 6, 2, 1, 1),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chain_moments_are_the_sequential_sums_of_the_trace_and_perturb_nothing(device, case):
    name, dim, T, Cn, pname, form, f64, cuts, burn, every, se, temps = case
    rng = np.random.default_rng(dim * 1000 + T)
    betas = np.geomspace(1.0, 0.05, T).astype(np.float32)
    tgt = _target("rc", dim, device)
    prop = _proposal(pname, dim, betas, device)
    x0 = rng.normal(0.0, 2.0, size=(Cn, T, dim)).astype(np.float64 if f64 else np.float32)
    kw = dict(x0=x0, beta=betas, cuts=cuts, burn=burn, se=se, seed=1234 + dim, f64=f64, every=every, temps=temps)
    with E.kernel_form(form):
        mom = _one_run(device, tgt, prop, mode="chain", **kw)
        tra = _one_run(device, tgt, prop, mode="trace", **kw)
        plain = _one_run(device, tgt, prop, mode="plain", **kw)
    if name == "rwm_d30_auto":
        assert mom["kinds"] == [E.LAUNCH_QUAD] * len(cuts)
    else:
        expect = E.LAUNCH_QUAD if (form == E.FORM_QUAD or f64 or dim > 64) else E.LAUNCH_THREAD
        assert mom["kinds"] == [expect] * len(cuts) and plain["kinds"] == mom["kinds"] and tra["kinds"] == mom["kinds"]
    for f in FIELDS:  # no perturbation: bit-identical to the run without moments (and to the traced run)
        assert np.array_equal(mom[f], plain[f]), f
        assert np.array_equal(tra[f], plain[f]), f
    _assert_bit_equal(mom["moments"], _sequential_sums(tra["trace"], tra["trace_logp"], every=every, burn=burn, temps=temps))


def test_chain_moments_do_not_depend_on_launch_cuts_nor_on_the_kernel_form(device):
    """300 ladders of 8 temperatures (the last exchange group of either form is partly empty), 24 steps: one launch, three
    uneven launches and 24 one-step launches, each in the thread form and in the lane-split form - six bit-identical sets of
    accumulators."""
    dim, T, Cn, burn, every, se, temps, n = 5, 8, 300, 7, 3, 4, 8, 24
    assert E.has_thread_variant(E.TARGET_ROUGH_CARPET, E.PROPOSAL_NORMAL, dim)
    assert E.has_quad_variant(E.TARGET_ROUGH_CARPET, E.PROPOSAL_NORMAL, dim, T)
    rng = np.random.default_rng(11)
    betas = np.geomspace(1.0, 0.05, T).astype(np.float32)
    tgt = _target("rc", dim, device)
    prop = _proposal("Normal", dim, betas, device)
    x0 = rng.normal(0.0, 2.0, size=(Cn, T, dim)).astype(np.float32)
    kw = dict(x0=x0, beta=betas, burn=burn, se=se, seed=99, f64=False, every=every, temps=temps)
    runs = {}
    for form, kind in ((E.FORM_THREAD, E.LAUNCH_THREAD), (E.FORM_QUAD, E.LAUNCH_QUAD)):
        for cuts in ((n,), (5, 12, 7), (1,) * n):
            with E.kernel_form(form):
                r = _one_run(device, tgt, prop, mode="chain", cuts=cuts, **kw)
            assert r["kinds"] == [kind] * len(cuts)
            runs[(form, cuts)] = r
    ref = runs[(E.FORM_THREAD, (n,))]
    assert ref["moments"]["count"].tolist() == [(n // every) - (burn // every)] * temps
    for key, r in runs.items():
        assert np.array_equal(r["moments"]["count"], ref["moments"]["count"]), key
        for k in ("sum", "sum_sq", "sum_logp"):
            assert np.array_equal(r["moments"][k], ref["moments"][k]), (key, k)
        for f in ("state", "logp", "n_accept", "swap_accept", "last_swap_ordinal"):
            assert np.array_equal(r[f], ref[f]), (key, f)


def test_auto_hands_over_to_the_form_whose_region_fits(device):
    """RWM at dim 32 (a run-time-dim thread kernel of width 32): 4 x 64 chains x 65 doubles do not fit the thread form's
    workgroup, 4 x 16 x 65 fit the lane-split form's.  Pinned to the thread form the launch is refused; under AUTO it runs
    the lane-split form, whatever the batch size."""
    dim, Cn = 32, 262144
    tgt = _target("rc", dim, device)
    prop = _proposal("Normal", dim, np.ones(1, np.float32), device)
    st = torch.zeros(Cn, 1, dim, device=device)
    lp = E.logdensity(tgt, st.view(-1, dim)).view(Cn, 1).contiguous()
    plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.ones(1, device=device), seed=3)
    s, q = (torch.zeros(Cn, 1, dim, device=device, dtype=torch.float64) for _ in range(2))
    cnt = torch.zeros(1, device=device, dtype=torch.int64)
    plan.set_chain_moments(s, q, count=cnt)
    with E.kernel_form(E.FORM_THREAD):
        with pytest.raises(E.PTRWMError):
            plan.launch(0, 4)
    torch.cuda.synchronize()
    assert cnt.item() == 0 and not s.any()
    with E.kernel_form(E.FORM_AUTO):
        plan.launch(0, 4)
        assert E.last_launch_kind() == E.LAUNCH_QUAD
    torch.cuda.synchronize()
    assert cnt.item() == 4 and q.min().item() >= 0 and s.any()


def test_chain_moments_of_split_steps_graph_and_eager(device):
    """Dense-covariance Gaussian (no fused kernel: split steps), three temperatures: graph replay and eager both give
    exactly the sequential sums of a trace of every chain."""
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
                          swap_order="sequential", seed=77, moments_temps=T if mom else 0, moments_every=every,
                          moments_per_chain=mom)
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
    want = _sequential_sums(trace.cpu().numpy(), trace_logp.cpu().numpy(), every=every, burn=burn, temps=T)
    for r in (g, e):
        _assert_bit_equal({k: v.cpu().numpy() for k, v in r.chain_moments().items() if k != "every"}, want)
        pooled = r.moments()  # the pooled view: the per-chain sums added over the replicas
        assert pooled["count"].tolist() == [int(want["count"][0]) * Cn] * T
        assert torch.equal(pooled["sum"], r.chain_moments()["sum"].sum(0))


def test_classes_rhat_and_ess_equal_the_formulas_on_a_full_trace(device):
    """The PT class with moments='all', moments_per_chain=True against a twin run traced in full: rhat() / ess() / the chain
    means and variances equal the NumPy formulas on the trace to 1e-10; the pooled estimates agree with a separate
    pooled-moments run to 1e-12 of sum |x|; reset() starts from zero."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from interfaces.simulation_gpu import MCMCSimulation_GPU  # noqa: F401  (passthroughs exist)
    from target_distributions import RoughCarpetDistributionTorch

    dim, T, R, burn, every, n = 5, 4, 256, 10, 2, 60
    target = RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0])
    kw = dict(beta_ladder=[1.0, 0.6, 0.3, 0.1], swap_every=3, burn_in=burn, device=device, num_replicas=R, seed=9,
              trace="none")
    a = ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, target, moments="all", moments_every=every,
                                           moments_per_chain=True, **kw)
    p = ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, target, moments="all", moments_every=every, **kw)
    b = ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, target, **kw)
    b._initial_state = p._initial_state = a._initial_state  # (drawn per instance: the twins start where `a` starts)
    a.generate_samples(n)
    p.generate_samples(n)
    b._ensure_started()
    rows = (burn + n) // every
    trace = torch.zeros(rows, R, T, dim, device=device)
    b._run.advance(burn + n, trace=trace, trace_every=every)
    torch.cuda.synchronize()
    assert torch.equal(a._run.state, b._run.state) and torch.equal(a._run.n_accept, b._run.n_accept)
    x = trace.cpu().numpy().astype(np.float64)[burn // every:]  # rows past burn-in: [N, R, T, dim]
    N = x.shape[0]
    assert a._run.chain_moments()["count"].tolist() == [N] * T
    for t in range(T):
        xt = np.transpose(x[:, :, t], (1, 0, 2))  # [R, N, dim]
        want_r, want_e = numpy_rhat_ess(xt)
        np.testing.assert_allclose(a.rhat(t).cpu().numpy(), want_r, rtol=1e-10, atol=0)
        np.testing.assert_allclose(a.ess(t).cpu().numpy(), want_e, rtol=1e-10, atol=0)
        np.testing.assert_allclose(a.chain_means(t).cpu().numpy(), xt.mean(1), rtol=0, atol=1e-10 * np.abs(xt).max())
        np.testing.assert_allclose(a.chain_variances(t).cpu().numpy(), xt.var(1, ddof=1), rtol=1e-9, atol=0)
        assert a.rhat(t).shape == (dim,) and a.chain_means(t).shape == (R, dim)
    with pytest.raises(ValueError):
        a.rhat(T)
    with pytest.raises(RuntimeError):
        p.rhat()
    # the pooled sums: .sum(0) of the per-chain ones against the pooled accumulators of a separate run
    pooled, cm = p._run.moments(), a._run.chain_moments()
    abs_x = np.abs(x).sum((0, 1))
    assert torch.equal(a.moment_count, p.moment_count)
    assert np.all(np.abs((cm["sum"].sum(0) - pooled["sum"]).cpu().numpy()) <= 1e-12 * abs_x)
    assert np.all(np.abs((cm["sum_sq"].sum(0) - pooled["sum_sq"]).cpu().numpy()) <= 1e-12 * (x * x).sum((0, 1)))
    assert torch.allclose(a.posterior_mean(1), p.posterior_mean(1), rtol=0, atol=1e-12)
    assert torch.allclose(a.posterior_variance(2), p.posterior_variance(2), rtol=1e-10, atol=0)
    assert torch.allclose(a.mean_log_density(), p.mean_log_density(), rtol=1e-12, atol=0)
    info = a.get_diagnostic_info()
    assert info["rhat_max"] == pytest.approx(float(a.rhat().max())) and info["ess_min"] == pytest.approx(float(a.ess().min()))
    assert "rhat_max" not in p.get_diagnostic_info()
    # reset: the accumulators start from zero
    a._run.reset_chain_moments()
    assert not a._run.chain_moments()["sum"].any() and a._run.chain_moments()["count"].tolist() == [0] * T
    a.reset()
    assert a.moment_count.tolist() == [0] * T
    a.generate_samples(4)
    assert a._run.chain_moments()["count"].tolist() == [2] * T and a.moment_count.tolist() == [2 * R] * T


def test_rhat_flags_chains_stuck_in_different_modes(device):
    """RoughCarpet with modes -15 / +15 and a single temperature: chains started in different modes stay there.  Modes 30
    apart with unit spread inside a mode give R-hat ~ 10 and more; anything above 3 is far from converged."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    dim, chains = 4, 512
    target = RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0])
    alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, target, burn_in=100, device=device, num_chains=chains, seed=4,
                                     moments="cold", moments_every=2, moments_per_chain=True)
    alg._ensure_started()
    r = alg._run
    start = torch.where(torch.arange(chains, device=device)[:, None, None] % 2 == 0, -15.0, 15.0).expand(chains, 1, dim)
    r.state.copy_(start)
    r.logp.copy_(E.logdensity(r.target, r.state.view(-1, dim)).view(chains, 1))
    alg._advance(100 + 400)
    rhat = alg.rhat()
    assert torch.isfinite(rhat).all() and rhat.min().item() > 3, rhat
    assert alg.get_diagnostic_info()["rhat_max"] > 3
    assert alg.ess().max().item() < chains * 200  # far fewer effective draws than draws


def test_ess_predicts_the_spread_of_independent_runs(device):
    """RWM on the diagonal Gaussian of the pooled-moments test (dim 30, 65 536 chains, 1 000 steps after 1 000 of burn-in,
    every 5th accumulated), K = 16 independent runs (disjoint chain_offset): 1 / ESS_d is the variance of the pooled mean
    in units of the posterior variance, so its mean over coordinates must agree with that of se_d^2 / var_d, se_d the
    spread of the K pooled means.  Tolerance: a variance estimated from K runs has relative sampling error sqrt(2/(K-1)),
    averaged over dim independent coordinates sqrt(2/(K-1)) / sqrt(dim); five of those = 0.33.
    Observed on an MI355X: mean 1/ESS 1.529e-6, mean se^2/var 1.487e-6, ratio 1.029."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    dim, chains, burn, n, every, K = 30, 65536, 1000, 1000, 5, 16
    mean = np.linspace(-2.0, 2.0, dim)
    var = np.linspace(0.5, 2.0, dim)
    target = MultivariateNormalTorch(dim, mean=mean.tolist(), cov=np.diag(var).tolist(), device=device)
    means, inv_ess, rhats = [], [], []
    for k in range(K):
        alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, target, burn_in=burn, device=device, num_chains=chains,
                                         seed=5, chain_offset=k * chains, moments="cold", moments_every=every,
                                         moments_per_chain=True)
        alg._advance(burn + n)
        assert int(alg.moment_count[0].item()) == chains * (n // every)
        means.append(alg.posterior_mean().cpu().numpy())
        inv_ess.append(1.0 / alg.ess().cpu().numpy())
        rhats.append(alg.rhat().cpu().numpy())
        del alg
    means, inv_ess, rhats = np.array(means), np.array(inv_ess), np.array(rhats)
    assert np.all(np.isfinite(inv_ess)) and np.all(np.isfinite(rhats))
    predicted = inv_ess.mean()
    observed = (means.var(0, ddof=1) / var).mean()
    ratio = predicted / observed
    tol = 5.0 * np.sqrt(2.0 / (K - 1)) / np.sqrt(dim)
    print(f"ess check: mean 1/ESS {predicted:.4e}, mean se^2/var {observed:.4e}, ratio {ratio:.4f}, tolerance {tol:.3f}")
    assert abs(ratio - 1.0) <= tol, (predicted, observed, ratio, tol)


def test_a_plan_holds_one_accumulator_and_either_setter_replaces_it(device):
    """One RunPlan, 12 steps as three launches of 4 with a full trace at every = 2: pooled moments in the first launch,
    per-chain ones in the second, none in the third.  Each set of accumulators holds the sums of its own launch alone, and
    state, log-density and counters are those of the same steps without an accumulator.  And on a fresh plan,
    set_chain_moments followed by set_moments accumulates the pooled sums and leaves the per-chain arrays alone."""
    from target_distributions import MultivariateNormalTorch

    dim, T, Cn, se, every, n = 5, 3, 8, 2, 2, 4
    target = MultivariateNormalTorch(dim, mean=np.linspace(-1.0, 1.0, dim).tolist(),
                                     cov=np.diag(np.linspace(0.5, 2.0, dim)).tolist(), device=device)
    tgt = target.engine_target()  # (DiagGaussian)
    betas = np.array([1.0, 0.5, 0.25], np.float32)
    prop = _proposal("Normal", dim, betas, device)
    x0 = np.random.default_rng(5).normal(0.0, 1.5, size=(Cn, T, dim)).astype(np.float32)

    def make():
        st = torch.tensor(x0, device=device)
        lp = E.logdensity(tgt, st.view(-1, dim)).view(Cn, T).contiguous()
        stats = {k: torch.zeros(Cn, T, dtype=dt, device=device) for k, dt in
                 (("n_accept", torch.int64), ("sq_jump", torch.float64), ("swap_accept", torch.int64),
                  ("last_swap_ordinal", torch.int64))}
        plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(betas, device=device), burn_in=0, swap_every=se,
                         seed=321, **stats)
        return plan, dict(stats, state=st, logp=lp)

    def accumulators(*lead):
        return {"sum": torch.zeros(*lead, T, dim, device=device, dtype=torch.float64),
                "sum_sq": torch.zeros(*lead, T, dim, device=device, dtype=torch.float64),
                "sum_logp": torch.zeros(*lead, T, device=device, dtype=torch.float64),
                "count": torch.zeros(T, device=device, dtype=torch.int64)}

    def bind(setter, m):
        setter(m["sum"], m["sum_sq"], sum_logp=m["sum_logp"], count=m["count"], every=every)

    def host(m):
        return {k: v.cpu().numpy() for k, v in m.items()}

    plan, out = make()
    pooled, chain = accumulators(), accumulators(Cn)
    rows = n // every
    trace = torch.zeros(3 * rows, Cn, T, dim, device=device)
    trace_logp = torch.zeros(3 * rows, Cn, T, device=device)
    for k, switch in enumerate((lambda: bind(plan.set_moments, pooled), lambda: bind(plan.set_chain_moments, chain),
                                lambda: plan.set_chain_moments(None))):
        switch()
        plan.launch(k * n, n, trace=trace, trace_logp=trace_logp, trace_row0=k * rows, trace_every=every)
    ref_plan, ref = make()
    for k in range(3):
        ref_plan.launch(k * n, n)
    torch.cuda.synchronize()
    tr, trl = trace.cpu().numpy(), trace_logp.cpu().numpy()
    want_pooled = _trace_sums(tr[:rows], trl[:rows], every=every, burn=0, temps=T)
    # (the final values: nothing was added to either set outside its own launch - launch 3 included)
    _check_against_trace(host(pooled), want_pooled)
    _assert_bit_equal(host(chain), _sequential_sums(tr[rows:2 * rows], trl[rows:2 * rows], every=every, burn=0, temps=T))
    for f in FIELDS:
        assert torch.equal(out[f], ref[f]), f

    plan2, _ = make()
    pooled2, chain2 = accumulators(), accumulators(Cn)
    bind(plan2.set_chain_moments, chain2)
    bind(plan2.set_moments, pooled2)
    plan2.launch(0, n)
    torch.cuda.synchronize()
    _check_against_trace(host(pooled2), want_pooled)  # (the same first four steps)
    assert not any(v.any().item() for v in chain2.values())
