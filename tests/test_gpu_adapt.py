"""Warm-up tuning of the proposal scale (include/ptrwm.h ptrwm_adapt_args, csrc/adapt.h) on the GPU, through the C ABI.

The yardstick is the library's own non-adaptive path: an adaptive run must equal, bit for bit, the same steps run as plain
ptrwm_run calls under the scales its history records, its integer acceptance history must equal the torch sum of a scratch the
same window fills when it is replayed with the documented recipe, nothing may depend on where the run is cut into calls or
shards, and a run that cannot adapt (no window, or a gain too small to move a float) must equal the non-adaptive run.  That the
rule TUNES is a condition, not a tolerance: fixed-scale runs 1.25x above and 0.8x below every adapted scale bracket the target
acceptance rate."""
import math
import warnings

import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E

gpu = pytest.mark.gpu

SEED = 20261019
W = 5
BURN = 3 * W + 7  # four adapting windows, then two steps of ordinary burn-in under the final scales
K = BURN // W
KEYS = ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")
INT32_MAX = 2 ** 31 - 1


def rc5_spec():
    return H.spec_from_params("RoughCarpetDistributionTorch", 5, {"modes": [-3.0, 0.0, 3.0], "weights": [0.5, 0.3, 0.2]})


def diag_spec(dim):
    return H.TargetSpec(kind=E.TARGET_DIAG_GAUSSIAN, dim=dim, p=(-0.5 * dim * math.log(2 * math.pi),), ip=(1,),
                        vec0=np.ones(dim, np.float32))


def proposal(kind, dim, betas, factor=1.0):
    if kind == "Laplace":
        return H.proposal_spec("Laplace", dim, betas, base_variance_vector=np.linspace(0.5, 1.5, dim) * factor)
    if kind == "UniformRadius":
        return H.proposal_spec("UniformRadius", dim, betas, base_radius=2.0 * math.sqrt(factor))
    return H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim * factor)


def starts(spec, Cn, T, offset=0, total=None):
    """A start per GLOBAL chain (so shards start where the whole run does), inside the support of every target used here."""
    rng = np.random.default_rng(7 + spec.dim)
    x = rng.uniform(0.5, 2.5, size=(total or offset + Cn, 1, spec.dim)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(x[offset:offset + Cn], (Cn, T, spec.dim)))


class Run:
    """One sampler run through the C ABI with every output on the device."""

    def __init__(self, device, spec, prop, betas, Cn, *, burn, se, x0=None, f64=False, chain_offset=0, seed=SEED, adapt=None,
                 recipe=False, total=None):
        T, dim = len(betas), spec.dim
        self.T, self.Cn, self.dim, self.device = T, Cn, dim, device
        self.tgt, self.prop = spec.engine(device), prop.engine(device)
        x0 = starts(spec, Cn, T, chain_offset, total) if x0 is None else x0
        self.st = torch.tensor(np.asarray(x0), device=device, dtype=torch.float64 if f64 else torch.float32)
        self.lp = E.logdensity(self.tgt, self.st.view(-1, dim).float()).view(Cn, T).contiguous()
        self.stats = {k: torch.zeros(Cn, T, dtype=(torch.float64 if k == "sq_jump" else torch.int64), device=device) for k in KEYS}
        kw = dict(self.stats)
        if recipe:  # the documented warm-up arguments: count from the first step into a scratch, no squared jump, no swap step
            burn, se = 0, INT32_MAX
            kw["sq_jump"] = None
        self.plan = E.RunPlan(self.tgt, self.prop, state=self.st, logp=self.lp, beta=torch.tensor(np.asarray(betas, np.float32), device=device),
                              burn_in=burn, swap_every=se, seed=seed, chain_offset=chain_offset, **kw)
        self.adapt = adapt
        if adapt is not None:
            a = dict(every=W, until=burn, target=0.234, gain=3.0, decay=0.5, min_scale=1e-6, max_scale=1e6, defer_update=False)
            a.update(adapt)
            self.K = K = a["until"] // a["every"]
            self.window_accept = torch.zeros(Cn, T, dtype=torch.int64, device=device)
            self.pooled = torch.zeros(T + 1, dtype=torch.int64, device=device)
            self.scale_history = torch.full((K + 1, T), -1.0, dtype=torch.float32, device=device)
            self.accept_history = torch.full((K, T), -1, dtype=torch.int64, device=device)
            self.plan.set_adaptation(self.window_accept, self.pooled, scale_history=self.scale_history,
                                     accept_history=self.accept_history, **a)

    def launches(self, cuts, step0=0):
        for n in cuts:
            self.plan.launch(step0, n)
            step0 += n
        return self

    def set_scales(self, row):
        self.prop.temp_scale.copy_(row)
        return self

    def out(self):
        torch.cuda.synchronize()
        o = {"state": self.st.cpu().numpy(), "logp": self.lp.cpu().numpy(), "scales": self.prop.temp_scale.cpu().numpy(),
             **{k: v.cpu().numpy() for k, v in self.stats.items()}}
        if self.adapt is not None:
            o.update(scale_history=self.scale_history.cpu().numpy(), accept_history=self.accept_history.cpu().numpy(),
                     window_accept=self.window_accept.cpu().numpy(), pooled=self.pooled.cpu().numpy())
        return o


def assert_same(a, b, what, keys=("state", "logp") + KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"


#          id             target     T   chains  proposal         f64    form
CASES = [("gamma_1x1", "gamma_d5", 1, 1, "Normal", False, None),
         ("rc_3x63", "rc5", 3, 63, "Normal", False, None),
         ("rc_4x1000", "rc5", 4, 1000, "Normal", False, None),   # several reduce workgroups, a ragged last tile
         ("rc_65x3", "rc5", 65, 3, "Normal", False, None),       # workgroup-wide ladders; n_temps divides no tile row
         ("rc_thread", "rc5", 3, 63, "Normal", False, E.FORM_THREAD),
         ("rc_quad", "rc5", 3, 63, "Normal", False, E.FORM_QUAD),
         ("rc_f64", "rc5", 3, 63, "Normal", True, None),
         ("rc_laplace", "rc5", 3, 63, "Laplace", False, None),
         ("rc_uniform", "rc5", 3, 63, "UniformRadius", False, None)]


def case_spec(name):
    return rc5_spec() if name == "rc5" else H.target_spec(name)


def test_every_case_has_a_step_kernel():
    """No GPU needed: no case below can fail for want of a variant."""
    for _, tname, T, _, pk, f64, form in CASES:
        spec, kind = case_spec(tname), H.PROPOSAL_KIND[pk]
        assert spec.dim == 5
        if form != E.FORM_QUAD and not f64:
            assert E.has_thread_variant(spec.kind, kind, 5)
        if form == E.FORM_QUAD or f64:
            assert E.has_quad_variant(spec.kind, kind, 5, T)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_adaptive_run_equals_its_replay_under_the_recorded_scales(device, case):
    _, tname, T, Cn, pk, f64, form = case
    spec = case_spec(tname)
    betas = np.geomspace(1.0, 0.05, T) if T > 1 else np.ones(1)
    prop = proposal(pk, 5, betas)
    se, burn = 4, BURN
    N = burn + 2 * se
    prev = E.set_kernel_form(form) if form is not None else None
    try:
        ad = Run(device, spec, prop, betas, Cn, burn=burn, se=se, f64=f64, adapt={}).launches([N])
        a = ad.out()
        assert ad.K == K == 4 and a["scale_history"].shape == (K + 1, T)
        assert np.array_equal(a["scale_history"][0], prop.temp_scale) and np.array_equal(a["scale_history"][K], a["scales"])
        assert (a["scale_history"][1] != a["scale_history"][0]).all()  # every temperature moved in the first window
        assert not a["window_accept"].any() and not a["pooled"].any()  # scratch and pooled are left zero
        # the same steps as plain ptrwm_run calls, one per segment, under the recorded scales
        rp = Run(device, spec, prop, betas, Cn, burn=burn, se=se, f64=f64)
        for k in range(K):
            rp.set_scales(ad.scale_history[k]).launches([W], step0=k * W)
        rp.set_scales(ad.scale_history[K]).launches([N - K * W], step0=K * W)
        assert_same(a, rp.out(), "adaptive run against its replay")
        assert (Cn == 1 or a["n_accept"].sum() > 0) and (T == 1 or a["swap_accept"].sum() > 0)
        # the integer history: window k replayed with the recipe arguments fills a scratch whose sum over chains it must equal
        rc = Run(device, spec, prop, betas, Cn, burn=burn, se=se, f64=f64, recipe=True)
        for k in range(K):
            rc.stats["n_accept"].zero_()
            rc.set_scales(ad.scale_history[k]).launches([W], step0=k * W)
            assert torch.equal(rc.stats["n_accept"].sum(0), ad.accept_history[k]), k
            assert int(ad.accept_history[k].max()) <= Cn * W
        r = rc.out()
        assert not r["swap_accept"].any() and not r["last_swap_ordinal"].any()  # the recipe performs no swap event
    finally:
        if prev is not None:
            E.set_kernel_form(prev)


def raw_run_with_adaptation(run, step0, n, hist=None, adapt=None):
    """ptrwm_run_with_adaptation itself, with whatever of hist / adapt is given (None: a NULL pointer)."""
    p = run.plan
    p._a.step0, p._a.n_steps = step0, n
    with p._guard:
        rc = p._lib.ptrwm_run_with_adaptation(p._refs[2], p._refs[3], p._refs[4], None, None, None, hist, adapt,
                                              torch.cuda.current_stream(run.device).cuda_stream)
    assert rc == 0, rc


@gpu
def test_nothing_else_moves(device):
    spec, T, Cn = rc5_spec(), 3, 63
    betas = np.geomspace(1.0, 0.05, T)
    prop = proposal("Normal", 5, betas)
    se, burn = 4, BURN
    N = burn + 2 * se
    cuts = [W] * K + [N - K * W]  # the launches of the adaptive run (sq_jump is exact between runs cut alike, include/ptrwm.h)

    def hist_run():
        r = Run(device, spec, prop, betas, Cn, burn=burn, se=se)
        r.counts = torch.zeros(1, 5, 10, dtype=torch.int64, device=device)
        r.plan.set_histogram(r.counts, torch.full((5,), -4.0, device=device), torch.full((5,), 1.0, device=device), n_bins=8, temps=1, every=2)
        return r

    base = hist_run().launches([N])  # ptrwm_run_with_histogram
    b = base.out()
    # adapt == NULL: exactly ptrwm_run_with_histogram
    null = hist_run()
    raw_run_with_adaptation(null, 0, N, hist=null.plan._hist[1], adapt=None)
    assert_same(b, null.out(), "adapt == NULL")
    assert torch.equal(base.counts, null.counts) and int(base.counts.sum()) > 0
    # until < every: no window adapts
    short = Run(device, spec, prop, betas, Cn, burn=burn, se=se, adapt={"until": W - 1})
    short.counts = torch.zeros(1, 5, 10, dtype=torch.int64, device=device)
    short.plan.set_histogram(short.counts, torch.full((5,), -4.0, device=device), torch.full((5,), 1.0, device=device), n_bins=8, temps=1, every=2)
    short.launches([N])
    s = short.out()
    assert_same(b, s, "until < every")
    assert torch.equal(base.counts, short.counts) and np.array_equal(s["scales"], prop.temp_scale) and short.K == 0
    # a gain too small to move a float: the warm-up overrides themselves touch neither state, logp nor any counter
    plain = Run(device, spec, prop, betas, Cn, burn=burn, se=se).launches(cuts)
    tiny = Run(device, spec, prop, betas, Cn, burn=burn, se=se, adapt={"gain": 1e-30}).launches([N])
    t = tiny.out()
    assert (t["scale_history"] == prop.temp_scale[None, :]).all() and t["accept_history"].min() > 0
    assert_same(plain.out(), t, "gain too small to move a scale")
    assert t["swap_accept"].sum() > 0 and t["last_swap_ordinal"].max() > 0


@gpu
def test_cuts_compose(device):
    spec, T, Cn = rc5_spec(), 3, 63
    betas = np.geomspace(1.0, 0.05, T)
    prop = proposal("Normal", 5, betas)
    se, burn = 4, BURN
    N = burn + 2 * se
    whole = Run(device, spec, prop, betas, Cn, burn=burn, se=se, adapt={}).launches([N]).out()
    every_step_of_window_1 = [[p, N - p] for p in range(W, 2 * W + 1)]
    later = [[3, 9, 1, 4, N - 17], [2 * W + 2, 5, 1, N - 2 * W - 8], [K * W + 1, 3, N - K * W - 4], [1] * N]
    for cuts in every_step_of_window_1 + later:
        assert sum(cuts) == N
        got = Run(device, spec, prop, betas, Cn, burn=burn, se=se, adapt={}).launches(cuts).out()
        assert_same(whole, got, f"cuts {cuts[:4]}", keys=("state", "logp", "scales", "scale_history", "accept_history", "pooled") + KEYS)
        assert not got["window_accept"].any()


@gpu
def test_shards_compose(device):
    spec, T, total = rc5_spec(), 4, 96
    betas = np.geomspace(1.0, 0.05, T)
    prop = proposal("Normal", 5, betas)
    se, burn = 4, BURN
    N = burn + 2 * se
    whole = Run(device, spec, prop, betas, total, burn=burn, se=se, adapt={}).launches([N]).out()
    shards = [Run(device, spec, prop, betas, cnt, burn=burn, se=se, chain_offset=off, total=total, adapt={"defer_update": True})
              for off, cnt in ((0, 40), (40, 56))]
    for k in range(K):
        for s in shards:
            s.launches([W], step0=k * W)
        pooled = shards[0].pooled + shards[1].pooled  # what the all-reduce of a sharded run computes
        assert int(pooled[T]) == total * W
        for s in shards:
            s.pooled.copy_(pooled)
            s.plan.adapt_update(k)
    for s in shards:
        s.launches([N - K * W], step0=K * W)
    outs = [s.out() for s in shards]
    for o in outs:
        assert_same(whole, o, "shard against the whole run", keys=("scales", "scale_history", "accept_history"))
        assert not o["window_accept"].any() and not o["pooled"].any()
    for k in ("state", "logp") + KEYS:
        assert np.array_equal(np.concatenate([o[k] for o in outs]), whole[k]), k
    # stepping past a pending window end: refused, and nothing was enqueued
    s = Run(device, spec, prop, betas, 40, burn=burn, se=se, total=total, adapt={"defer_update": True})
    before = s.out()
    with pytest.raises(E.PTRWMError) as err:
        s.launches([W + 1])
    assert err.value.code == -5
    with pytest.raises(E.PTRWMError):
        s.launches([3], step0=W - 2)
    assert_same(before, s.out(), "a refused request", keys=("state", "logp", "window_accept", "pooled"))
    s.launches([W])  # up to the window end is fine
    assert s.out()["pooled"][T] == 40 * W


def bracket_rates(device, spec, prop, betas, final_state, scales, factor, n_steps=400):
    """Acceptance rate per temperature of a fixed-scale run through the existing path from `final_state`."""
    Cn = final_state.shape[0]
    r = Run(device, spec, prop, betas, Cn, burn=0, se=INT32_MAX, x0=final_state, seed=SEED + 1)
    r.set_scales(torch.tensor(scales * np.float32(factor), device=device)).launches([n_steps])
    return r.out()["n_accept"].sum(0) / float(Cn * n_steps)


TUNE = [("gauss_d10_above", "gauss", 4, 400.0), ("gauss_d10_below", "gauss", 4, 1.0 / 400.0),
        ("rc_d5_above", "rc5", 8, 400.0), ("rc_d5_below", "rc5", 8, 1.0 / 400.0)]


@gpu
@pytest.mark.parametrize("case", TUNE, ids=[c[0] for c in TUNE])
def test_it_tunes(device, case):
    """var 400x too large / too small, adapt_every = 50, burn_in = 2500, 1024 ladders: for every temperature the acceptance
    rates of fixed-scale runs at 1.25 s* and 0.8 s* bracket 0.234.  (In a CPU simulation of the rule the two rates are about
    0.14 and 0.34 at dims 10 and 30, 0.17 and 0.31 at dim 2; the sampling error of 4 10^5 decisions is below 10^-3.)"""
    _, tname, T, factor = case
    spec = diag_spec(10) if tname == "gauss" else rc5_spec()
    betas = np.geomspace(1.0, 0.05, T)
    prop = proposal("Normal", spec.dim, betas, factor)
    Cn, burn = 1024, 2500
    ad = Run(device, spec, prop, betas, Cn, burn=burn, se=10, adapt={"every": 50}).launches([burn])
    a = ad.out()
    assert ad.K == 50 and np.isfinite(a["scale_history"]).all()
    above = bracket_rates(device, spec, prop, betas, a["state"], a["scales"], 1.25)
    below = bracket_rates(device, spec, prop, betas, a["state"], a["scales"], 0.8)
    print(f"{case[0]}: s* {a['scales']}, rate at 1.25 s* {above}, at 0.8 s* {below}, last window {a['accept_history'][-1] / (Cn * 50.0)}")
    assert (above < 0.234).all() and (below > 0.234).all(), (above, below)


# ---- the classes ---------------------------------------------------------------------------------------------------------
def dense_mvn(device):
    from target_distributions import MultivariateNormalTorch

    return MultivariateNormalTorch(3, cov=[[1, 0.5, 0], [0.5, 1, 0], [0, 0, 1]], device=device)


def pt_class(device, target, **kw):
    from algorithms import ParallelTemperingRWM_GPU_Optimized

    np.random.seed(4)  # (the samplers draw their 1e-8 N(0, 1) starting point from NumPy's global generator)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a target without a fused kernel says that it runs split steps)
        return ParallelTemperingRWM_GPU_Optimized(target.dim, 2.0, target, beta_ladder=[1.0, 0.4, 0.1], swap_every=4, device=device,
                                                  num_replicas=6, seed=SEED, trace="none", **kw)


@gpu
def test_split_steps(device):
    """A dense-covariance Gaussian has no fused kernel: eager split steps by the recipe during the adapting windows, graph replay
    from the end of warm-up.  History and final state equal an eager replay, step by step, and a non-adaptive eager run under
    the recorded scales."""
    burn, every, N = 14, 4, 14 + 50
    kw = dict(burn_in=burn, adapt_scale=True, adapt_every=every)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alg = pt_class(device, dense_mvn(device), **kw)
        alg._advance(N)
        assert alg._run.density_fn is not None and alg._run._graph is not None  # split steps; graph replay resumed after warm-up
        hist = alg.adaptation_history()
        assert tuple(hist["scales"].shape) == (4, 3) and bool(torch.isfinite(hist["scales"]).all()) and bool((hist["scales"][1] != hist["scales"][0]).all())
        eager = pt_class(device, dense_mvn(device), **kw)
        eager._ensure_started()
        eager._run.use_graph = False
        for _ in range(N):
            eager._advance(1)
        assert eager._run._graph is None
        assert torch.equal(eager.adaptation_history()["scales"], hist["scales"])
        assert torch.equal(eager.adaptation_history()["acceptance"], hist["acceptance"])
        fixed = pt_class(device, dense_mvn(device), burn_in=burn)
        fixed._ensure_started()
        fixed._run.use_graph = False
        for s in range(N):
            if s % every == 0 and s // every <= 3:
                fixed._run.proposal.temp_scale.copy_(hist["scales"][s // every])
            fixed._advance(1)
    torch.cuda.synchronize()
    for other, what in ((eager, "eager adaptive"), (fixed, "eager under the recorded scales")):
        for k in ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_ord"):
            assert torch.equal(getattr(alg._run, k), getattr(other._run, k)), (what, k)
    assert int(alg._run.swap_accept.sum()) > 0 and alg._run.post_burn_steps == 50


@gpu
def test_classes(device):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(5, device=device)
    burn, every, n = 120, 25, 40
    K = burn // every  # 4 windows; steps 100..119 are ordinary burn-in
    rw = RandomWalkMH_GPU_Optimized(5, 8.0, tgt, burn_in=burn, device=device, num_chains=300, seed=SEED, adapt_scale=True,
                                    adapt_every=every, moments="cold", hist="cold", hist_range=(-8, 8))
    pt = ParallelTemperingRWM_GPU_Optimized(5, 8.0, tgt, beta_ladder=[1.0, 0.5, 0.2, 0.05], swap_every=5, burn_in=burn, device=device,
                                            num_replicas=300, seed=SEED, trace="none", adapt_scale=True, adapt_every=every,
                                            moments="all", flow=True, hist="all", hist_range=(-8, 8))
    for alg, T in ((rw, 1), (pt, 4)):
        init = alg.proposal_scales().clone()
        alg.generate_samples(n)
        s, h, info = alg.proposal_scales(), alg.adaptation_history(), alg.get_diagnostic_info()
        assert tuple(s.shape) == (T,) and s.dtype == torch.float32
        assert tuple(h["scales"].shape) == (K + 1, T) and tuple(h["acceptance"].shape) == (K, T) and h["acceptance"].dtype == torch.float64
        assert torch.equal(h["scales"][0], init) and torch.equal(h["scales"][-1], s) and bool((s < init).all())  # var 8: far too large
        acc = h["acceptance"].cpu().numpy()
        assert ((acc >= 0) & (acc < 1)).all() and (acc[-1] > acc[0]).all()
        assert info["init_scales"] == init.cpu().tolist() and info["adapted_scales"] == s.cpu().tolist()
        # every diagnostic counts post-burn-in steps only, adaptation or not
        assert alg.moment_count.cpu().tolist() == [300 * n] * T
        assert int(alg._run.histogram()["count"][0]) == 300 * n
        assert int(alg._run.n_accept.sum(0).max()) <= 300 * n and int(alg._run.n_accept.sum()) > 0
        if T > 1:
            assert alg._run.flow()["events"] == n // 5 and int(alg._run.flow()["n_up"][:, 0].sum()) == 300 * (n // 5)
        # reset(): again from the initial scales, and with a fixed seed the same bits
        state = alg._run.state.clone()
        alg.reset()
        assert torch.equal(alg.proposal_scales(), init) and bool(torch.isnan(alg.adaptation_history()["scales"][1:]).all())
        alg.generate_samples(n)
        h2 = alg.adaptation_history()
        assert torch.equal(h2["scales"], h["scales"]) and torch.equal(h2["acceptance"], h["acceptance"]) and torch.equal(alg._run.state, state)


@gpu
def test_adapt_sync_cuts_the_run_at_window_ends(device):
    """adapt_sync (here: the identity all-reduce of a single shard, counting its calls) gives the bits of the run without it."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from algorithms.sharding import adaptation_sync
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(5, device=device)
    calls = []

    def sync(pooled):
        calls.append(tuple(pooled.shape))
        return adaptation_sync()(pooled)

    runs = []
    for fn in (None, sync):
        np.random.seed(4)  # (the samplers' 1e-8 N(0, 1) starting point)
        alg = ParallelTemperingRWM_GPU_Optimized(5, 50.0, tgt, beta_ladder=[1.0, 0.3, 0.1], swap_every=5, burn_in=60, device=device,
                                                 num_replicas=50, seed=SEED, trace="cold", adapt_scale=True, adapt_every=25, adapt_sync=fn)
        alg.step()
        cold = alg.generate_samples(30)
        runs.append((alg, cold.clone()))
    assert calls == [(4,), (4,)]
    (a, ca), (b, cb) = runs
    assert torch.equal(ca, cb) and torch.equal(a._run.state, b._run.state) and torch.equal(a._run.n_accept, b._run.n_accept)
    ha, hb = a.adaptation_history(), b.adaptation_history()
    assert torch.equal(ha["scales"], hb["scales"]) and torch.equal(ha["acceptance"], hb["acceptance"])
