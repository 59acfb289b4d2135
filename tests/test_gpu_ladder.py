"""Warm-up tuning of the temperature ladder (include/ptrwm.h ptrwm_ladder_args, csrc/ladder.h) on the GPU, through the C ABI and
the classes.

The yardsticks: the probe against a float64 evaluation of the same float inputs, within a bound derived from the arithmetic
(tests/ladder_reference.py probe()); an adaptive run against the same steps run as plain burn-in under the ladders and scales it
recorded, bit for bit; the update against the NumPy restatement within one float32 ulp; nothing may depend on where the run is
cut into calls, shards or kernel forms; and that the rule TUNES is a condition set beforehand, not a tolerance."""
import math
import warnings

import numpy as np
import pytest
import torch

import helpers as H
import ladder_reference as LR
import ptrwm_hip as E

gpu = pytest.mark.gpu

SEED = 20261020
V, P = 6, 3
BURN = 3 * V + 5  # three adapting windows, then five steps of ordinary burn-in under the final ladder
K = BURN // V
SE = 4
N = BURN + 2 * SE
KEYS = ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")
LADDER_KEYS = ("beta", "scales", "beta_history", "rate_history", "pooled", "skipped")


def rc5_spec():
    return H.spec_from_params("RoughCarpetDistributionTorch", 5, {"modes": [-3.0, 0.0, 3.0], "weights": [0.5, 0.3, 0.2]})


def diag_spec(dim):
    return H.TargetSpec(kind=E.TARGET_DIAG_GAUSSIAN, dim=dim, p=(-0.5 * dim * math.log(2 * math.pi),), ip=(1,),
                        vec0=np.ones(dim, np.float32))


def proposal(dim, betas):
    return H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim)


def starts(spec, Cn, T, offset=0, total=None):
    """A start per GLOBAL chain and temperature (so shards start where the whole run does, and the rungs of a ladder differ)."""
    rng = np.random.default_rng(11 + spec.dim)
    x = rng.uniform(0.5, 2.5, size=(total or offset + Cn, 256, spec.dim)).astype(np.float32)
    return np.ascontiguousarray(x[offset:offset + Cn, :T])


class Run:
    """One sampler run through the C ABI with every output on the device."""

    def __init__(self, device, spec, betas, Cn, *, burn=BURN, se=SE, f64=False, chain_offset=0, total=None, ladder=None,
                 adapt=None, x0=None):
        T, dim = len(betas), spec.dim
        self.T, self.Cn, self.dim, self.device = T, Cn, dim, device
        self.tgt, self.prop = spec.engine(device), proposal(dim, betas).engine(device)
        x0 = starts(spec, Cn, T, chain_offset, total) if x0 is None else x0
        self.st = torch.tensor(np.asarray(x0), device=device, dtype=torch.float64 if f64 else torch.float32)
        self.lp = E.logdensity(self.tgt, self.st.view(-1, dim).float()).view(Cn, T).contiguous()
        self.beta = torch.tensor(np.asarray(betas, np.float32), device=device)
        self.stats = {k: torch.zeros(Cn, T, dtype=(torch.float64 if k == "sq_jump" else torch.int64), device=device) for k in KEYS}
        self.plan = E.RunPlan(self.tgt, self.prop, state=self.st, logp=self.lp, beta=self.beta, burn_in=burn, swap_every=se,
                              seed=SEED, chain_offset=chain_offset, **self.stats)
        if adapt is not None:  # the scale's tuning next to the ladder's
            a = dict(every=25, until=burn, target=0.234, gain=3.0, decay=0.5, min_scale=1e-6, max_scale=1e6, defer_update=False)
            a.update(adapt)
            Ka = a["until"] // a["every"]
            self.window_accept = torch.zeros(Cn, T, dtype=torch.int64, device=device)
            self.adapt_pooled = torch.zeros(T + 1, dtype=torch.int64, device=device)
            self.scale_history = torch.full((Ka + 1, T), -1.0, dtype=torch.float32, device=device)
            self.plan.set_adaptation(self.window_accept, self.adapt_pooled, scale_history=self.scale_history, **a)
        self.ladder = ladder
        self.pooled = torch.zeros(T, dtype=torch.int64, device=device)
        self.skipped = torch.zeros(1, dtype=torch.int64, device=device)
        if ladder is not None:
            l = dict(every=V, probe_every=P, until=burn, gain=2.0, decay=0.5, rescale_scales=True, defer_update=False)
            l.update(ladder)
            self.K = Kl = l["until"] // l["every"]
            self.beta_history = torch.full((Kl + 1, T), -1.0, dtype=torch.float32, device=device)
            self.rate_history = torch.full((Kl, T), -1, dtype=torch.int64, device=device)
            self.plan.set_ladder(self.pooled, beta_history=self.beta_history, rate_history=self.rate_history, skipped=self.skipped, **l)

    def launches(self, cuts, step0=0):
        for n in cuts:
            self.plan.launch(step0, n)
            step0 += n
        return self

    def out(self):
        torch.cuda.synchronize()
        o = {"state": self.st.cpu().numpy(), "logp": self.lp.cpu().numpy(), "scales": self.prop.temp_scale.cpu().numpy(),
             "beta": self.beta.cpu().numpy(), "pooled": self.pooled.cpu().numpy(), "skipped": self.skipped.cpu().numpy(),
             **{k: v.cpu().numpy() for k, v in self.stats.items()}}
        if self.ladder is not None:
            o.update(beta_history=self.beta_history.cpu().numpy(), rate_history=self.rate_history.cpu().numpy())
        return o


def assert_same(a, b, what, keys=("state", "logp") + KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k}"


# ---- the probe --------------------------------------------------------------------------------------------------------------
# chains: 1, 3, and per T a count that spans at least three tiles of about 4096 / T chains with a ragged last one
PROBE = [(T, Cn) for T, big in ((3, 3000), (5, 1700), (32, 300), (65, 150), (128, 70)) for Cn in (1, 3, big)]


def probe_logp(rng, Cn, T):
    """Log-densities with every special case among them: -inf on one side of a pair, -inf on both sides, equal neighbours
    (lp = 0 exactly), neighbours one float apart (lp just above and just below 0), and pairs far enough apart for exp(lp) to
    fall below the quantum."""
    lp = (rng.normal(-20.0, 6.0, size=(Cn, T)) - np.arange(T)[None, :] * rng.uniform(0.0, 0.4)).astype(np.float32)
    for i in range(max(12, Cn)):  # (every kind at least twice, whatever the chain count; a later one may overwrite an earlier)
        c, kind, t = i % Cn, i % 8, int(rng.integers(0, T - 1))
        if kind >= 3 and not np.isfinite(lp[c, t]):
            lp[c, t] = np.float32(-15.0)  # (an earlier special case sat here)
        if kind == 1:
            lp[c, t] = -np.inf
        elif kind == 2:
            lp[c, t] = lp[c, t + 1] = -np.inf
        elif kind == 3:
            lp[c, t + 1] = lp[c, t]
        elif kind == 4:
            lp[c, t + 1] = np.nextafter(lp[c, t], np.float32(0))
        elif kind == 5:
            lp[c, t + 1] = np.nextafter(lp[c, t], np.float32(-100))
        elif kind == 6:
            lp[c, t + 1] = lp[c, t] - np.float32(3000.0)
    return lp


def probe_once(device, lp, betas, times=1):
    """ptrwm_ladder_probe of `lp` [Cn, T] under `betas`, `times` times into one pooled row."""
    Cn, T = lp.shape
    spec = diag_spec(2)
    r = Run(device, spec, betas, Cn, ladder={"until": 0}, x0=np.zeros((Cn, T, 2), np.float32))
    r.lp.copy_(torch.from_numpy(lp))
    for _ in range(times):
        r.plan.ladder_probe()
    torch.cuda.synchronize()
    return r.pooled.cpu().numpy()


@gpu
@pytest.mark.parametrize("T,Cn", PROBE, ids=[f"T{T}x{Cn}" for T, Cn in PROBE])
def test_probe_against_float64(device, T, Cn):
    """pooled[T - 1] counts the chains exactly; every pooled[t] lies within the sum over chains of the per-element bound that
    ladder_reference.probe derives from the arithmetic (the quantum, the seven float roundings of swap_log_prob, the two of
    hw_exp's argument and one ulp of v_exp_f32); pairs with an infinite log-density add exactly nothing; a second probe adds
    the same integers again."""
    rng = np.random.default_rng(1000 * T + Cn)
    betas = np.geomspace(1.0, 0.01, T).astype(np.float32)
    lp = probe_logp(rng, Cn, T)
    got = probe_once(device, lp, betas)
    want, bound, chains = LR.probe(lp, betas)
    err = np.abs(got[:T - 1].astype(np.float64) - want)
    print(f"T {T} chains {Cn}: worst |pooled - float64| / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, bound / chain {bound.max() / Cn:.2f} quanta")
    assert got[T - 1] == chains == Cn
    assert (got[:T - 1] >= 0).all() and (err <= bound).all(), (err, bound)
    assert np.array_equal(probe_once(device, lp, betas, times=2), 2 * got)
    # NaN and -inf: exact.  Every pair of every chain touches an infinite log-density: nothing is added anywhere
    dead = lp.copy()
    dead[:, 1::2] = -np.inf
    if Cn > 1:
        dead[1] = -np.inf
    got = probe_once(device, dead, betas)
    assert not got[:T - 1].any() and got[T - 1] == Cn
    assert not LR.probe(dead, betas)[0].any() and not LR.probe(dead, betas)[1].any()


# ---- an adaptive run equals its replay ---------------------------------------------------------------------------------------
#          id           target  T   chains
CASES = [("rc5_T8", "rc5", 8, 63), ("diag8_T32", "diag8", 32, 40), ("diag8_T65", "diag8", 65, 5)]


def case_spec(name):
    return rc5_spec() if name == "rc5" else diag_spec(8)


def test_every_case_has_a_step_kernel():
    """No GPU needed: no case below can fail for want of a variant."""
    for _, tname, T, _ in CASES:
        spec = case_spec(tname)
        assert E.has_thread_variant(spec.kind, H.PROPOSAL_KIND["Normal"], spec.dim) or \
            E.has_quad_variant(spec.kind, H.PROPOSAL_KIND["Normal"], spec.dim, T)
    assert E.has_thread_variant(rc5_spec().kind, H.PROPOSAL_KIND["Normal"], 5) and E.has_quad_variant(rc5_spec().kind, H.PROPOSAL_KIND["Normal"], 5, 8)


def replay(device, spec, betas, Cn, *, burn, se, n_total, seg, ladder, adapt=None, f64=False):
    """The adaptive run in segments of `seg` steps (every probe step ends one) next to plain burn-in steps under the ladder and
    scales the adaptive run held before each segment: state and logp bit-identical behind every segment, the pooled row of a
    second probe of the replay's logp equal to the recorded rate history.  Returns both runs."""
    ad = Run(device, spec, betas, Cn, burn=burn, se=se, ladder=ladder, adapt=adapt, f64=f64)
    rp = Run(device, spec, betas, Cn, burn=burn, se=se, ladder={"until": 0, "every": ad.plan._ladder[0].every,
                                                                  "probe_every": ad.plan._ladder[0].probe_every}, f64=f64)
    every, pe, end = ad.plan._ladder[0].every, ad.plan._ladder[0].probe_every, ad.K * ad.plan._ladder[0].every
    ad.scales_at = {}  # step -> the scales the adaptive run held before it
    s = 0
    while s < n_total:
        n = min(seg, n_total - s)
        ad.scales_at[s] = ad.prop.temp_scale.cpu().numpy()
        rp.beta.copy_(ad.beta)
        rp.prop.temp_scale.copy_(ad.prop.temp_scale)
        ad.launches([n], step0=s)
        rp.launches([n], step0=s)
        s += n
        assert torch.equal(ad.st, rp.st) and torch.equal(ad.lp, rp.lp), f"behind step {s - 1}"
        if s <= end and s % pe == 0:
            rp.plan.ladder_probe()
            if s % every == 0:
                assert torch.equal(rp.pooled, ad.rate_history[s // every - 1]), f"window {s // every - 1}"
                rp.pooled.zero_()
    return ad, rp


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_adaptive_run_equals_its_replay(device, case):
    _, tname, T, Cn = case
    spec = case_spec(tname)
    betas = np.linspace(1.0, 0.02, T).astype(np.float32)  # linear in beta: badly placed, the ladder moves
    ad, rp = replay(device, spec, betas, Cn, burn=BURN, se=SE, n_total=N, seg=P, ladder={})
    a, r = ad.out(), rp.out()
    assert_same(a, r, "adaptive run against its replay")  # every counter too: they see post-burn-in steps only
    assert a["swap_accept"].sum() > 0 and a["n_accept"].max() <= N - BURN
    assert ad.K == K and not a["pooled"].any() and a["skipped"][0] == 0
    bh, rh = a["beta_history"], a["rate_history"]
    assert np.array_equal(bh[0], betas) and np.array_equal(bh[K], a["beta"])
    assert (rh[:, T - 1] == Cn * (V // P)).all() and (rh[:, :T - 1] >= 0).all() and (rh[:, :T - 1] <= Cn * (V // P) << 24).all()
    assert np.array_equal(ad.scales_at[0], proposal(spec.dim, betas).temp_scale.astype(np.float32))
    for k in range(K):
        want, outcome = LR.update(bh[k], rh[k], 2.0 / math.sqrt(k + 1))
        assert outcome == 0 and LR.ulps(bh[k + 1], want).max() <= 1, k
        assert bh[k + 1][0] == betas[0] and bh[k + 1][-1] == betas[-1] and (bh[k + 1][:-1] > bh[k + 1][1:]).all()
        assert LR.ulps(ad.scales_at[(k + 1) * V], LR.rescale(ad.scales_at[k * V], bh[k], bh[k + 1])).max() <= 1, k
    assert (bh[1][1:-1] != bh[0][1:-1]).any() and np.array_equal(ad.scales_at[K * V], a["scales"])
    # the whole run in one call
    whole = Run(device, spec, betas, Cn, ladder={}).launches([N]).out()
    assert_same(whole, a, "one call against segments", keys=("state", "logp") + KEYS + LADDER_KEYS)


@gpu
def test_nothing_else_moves(device):
    spec, T, Cn = rc5_spec(), 8, 63
    betas = np.linspace(1.0, 0.02, T).astype(np.float32)

    def hist_run(**kw):
        r = Run(device, spec, betas, Cn, **kw)
        r.counts = torch.zeros(1, 5, 10, dtype=torch.int64, device=device)
        r.plan.set_histogram(r.counts, torch.full((5,), -4.0, device=device), torch.full((5,), 1.0, device=device), n_bins=8, temps=1, every=2)
        return r

    base = hist_run().launches([N])  # no ladder argument at all
    b = base.out()
    for what, ladder in (("until = 0", {"until": 0}), ("until < every", {"until": V - 1})):
        off = hist_run(ladder=ladder).launches([N])
        o = off.out()
        assert_same(b, o, what, keys=("state", "logp", "beta", "scales", "pooled", "skipped") + KEYS)
        assert torch.equal(base.counts, off.counts) and int(base.counts.sum()) > 0 and off.K == 0
    # past `until`: the run with the argument equals the run that drops it there
    on = hist_run(ladder={"until": V}).launches([V, N - V])
    drop = hist_run(ladder={"until": V}).launches([V])
    drop.plan.set_ladder(None)
    drop.launches([N - V], step0=V)
    o, d = on.out(), drop.out()
    assert_same(o, d, "past until", keys=("state", "logp", "beta", "scales", "pooled", "skipped", "beta_history", "rate_history") + KEYS)
    assert torch.equal(on.counts, drop.counts) and (o["beta"][1:-1] != betas[1:-1]).any()
    # ladder == NULL is ptrwm_run_with_adaptation
    null = hist_run()
    p = null.plan
    p._a.step0, p._a.n_steps = 0, N
    with p._guard:
        rc = p._lib.ptrwm_run_with_ladder(p._refs[2], p._refs[3], p._refs[4], None, None, None, p._hist[1], None, None,
                                          torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    assert_same(b, null.out(), "ladder == NULL")
    assert torch.equal(base.counts, null.counts)


@gpu
def test_cuts_compose(device):
    spec, T, Cn = rc5_spec(), 8, 63
    betas = np.linspace(1.0, 0.02, T).astype(np.float32)
    whole = Run(device, spec, betas, Cn, ladder={}).launches([N]).out()
    every_step_of_window_1 = [[p, N - p] for p in range(V, 2 * V + 1)]
    later = [[3, 9, 1, 4, N - 17], [2 * V + 2, 5, 1, N - 2 * V - 8], [K * V + 1, 3, N - K * V - 4], [1] * N]
    for cuts in every_step_of_window_1 + later:
        assert sum(cuts) == N
        got = Run(device, spec, betas, Cn, ladder={}).launches(cuts).out()
        assert_same(whole, got, f"cuts {cuts[:4]}", keys=("state", "logp") + KEYS + LADDER_KEYS)


@gpu
def test_forms(device):
    spec, T, Cn = rc5_spec(), 8, 63
    betas = np.linspace(1.0, 0.02, T).astype(np.float32)
    outs = []
    for form in (E.FORM_THREAD, E.FORM_QUAD):
        prev = E.set_kernel_form(form)
        try:
            outs.append(Run(device, spec, betas, Cn, ladder={}).launches([N]).out())
        finally:
            E.set_kernel_form(prev)
    assert_same(outs[0], outs[1], "thread against quad", keys=("state", "logp") + KEYS + LADDER_KEYS)
    assert (outs[0]["beta"][1:-1] != betas[1:-1]).any()


@gpu
def test_shards_compose(device):
    spec, T, total = rc5_spec(), 8, 300
    betas = np.linspace(1.0, 0.02, T).astype(np.float32)
    whole = Run(device, spec, betas, total, ladder={}).launches([N]).out()
    shards = [Run(device, spec, betas, 150, chain_offset=off, total=total, ladder={"defer_update": True}) for off in (0, 150)]
    for k in range(K):
        for s in shards:
            s.launches([V], step0=k * V)
        pooled = shards[0].pooled + shards[1].pooled  # what the all-reduce of a sharded run computes
        assert int(pooled[T - 1]) == total * (V // P)
        for s in shards:
            s.pooled.copy_(pooled)
            s.plan.ladder_update(k)
    for s in shards:
        s.launches([N - K * V], step0=K * V)
    outs = [s.out() for s in shards]
    for o in outs:
        assert_same(whole, o, "shard against the whole run", keys=LADDER_KEYS)
    for k in ("state", "logp") + KEYS:
        assert np.array_equal(np.concatenate([o[k] for o in outs]), whole[k]), k
    # stepping past a pending window end: refused, and nothing was enqueued
    s = Run(device, spec, betas, 150, total=total, ladder={"defer_update": True})
    before = s.out()
    with pytest.raises(E.PTRWMError) as err:
        s.launches([V + 1])
    assert err.value.code == -5
    assert_same(before, s.out(), "a refused request", keys=("state", "logp", "pooled", "beta"))
    s.launches([V])  # up to the window end is fine
    assert s.out()["pooled"][T - 1] == 150 * (V // P)


@gpu
def test_combined_with_adapt_scale(device):
    """W = 25 next to V = 50: both tunings rewrite temp_scale, the ladder's behind the scale's where their windows end together.
    The replay under both recorded histories - plain burn-in steps under the ladder and the scales the run held before each
    segment of 25 steps - is bit-identical."""
    spec, T, Cn = diag_spec(8), 8, 64
    betas = np.linspace(1.0, 0.02, T).astype(np.float32)
    burn = 110
    ad, rp = replay(device, spec, betas, Cn, burn=burn, se=SE, n_total=burn + 2 * SE, seg=25,
                    ladder={"every": 50, "probe_every": 25}, adapt={"every": 25})
    a = ad.out()
    assert_same(a, rp.out(), "both tunings against their replay")
    sh = ad.scale_history.cpu().numpy()
    assert ad.K == 2 and sh.shape == (5, T) and (sh[1] != sh[0]).all() and (a["beta_history"][1][1:-1] != betas[1:-1]).any()
    # the order at the shared end behind step 49: the scale's update (row 2 of its history), then the ladder's rescaling of it
    assert LR.ulps(ad.scales_at[50], LR.rescale(sh[2], a["beta_history"][0], a["beta_history"][1])).max() <= 1
    whole = Run(device, spec, betas, Cn, burn=burn, ladder={"every": 50, "probe_every": 25}, adapt={"every": 25}).launches([burn + 2 * SE]).out()
    assert_same(whole, a, "one call against segments", keys=("state", "logp") + KEYS + LADDER_KEYS)


# ---- it tunes ----------------------------------------------------------------------------------------------------------------
@gpu
def test_it_tunes(device):
    """Diag Gaussian dim 8, 8 rungs linear in beta from 1 to 0.01, 4096 ladders, 40 windows of 50 steps with gain 2, then 200
    frozen burn-in steps.  From the final logp NumPy float64 computes the pair rates: their spread max r - min r must be at most
    an eighth of the spread the same computation gives for the initial ladder after 200 steps, and max |log(beta_t / geometric_t)|
    at most an eighth of its initial value (2.06): for a Gaussian the equal-rate ladder is the geometric one.  An eighth: the
    ideal-equilibrium replay of the rule reaches a sixtieth (0.83 to below 0.02); the rest is allowance for chains that
    re-equilibrate within 50 steps.  The Monte-Carlo error of the spread is at most 4 x 0.5 / sqrt(4096) = 0.03."""
    spec, T, Cn = diag_spec(8), 8, 4096
    betas = np.linspace(1.0, 0.01, T).astype(np.float32)
    geo = np.geomspace(1.0, 0.01, T)
    x0 = np.zeros((Cn, T, 8), np.float32)
    init = Run(device, spec, betas, Cn, burn=200, x0=x0).launches([200]).out()
    spread0 = np.ptp(LR.pair_rates(init["logp"], betas))
    dev0 = np.abs(np.log(betas.astype(np.float64) / geo)).max()
    ad = Run(device, spec, betas, Cn, burn=2200, x0=x0, ladder={"every": 50, "probe_every": 50, "until": 2000}).launches([2200])
    a = ad.out()
    rates = LR.pair_rates(a["logp"], a["beta"])
    spread, dev = np.ptp(rates), np.abs(np.log(a["beta"].astype(np.float64) / geo)).max()
    print(f"spread {spread0:.4f} -> {spread:.4f} (bound {spread0 / 8:.4f}); log-distance to geometric {dev0:.4f} -> {dev:.4f} "
          f"(bound {dev0 / 8:.4f}); final ladder {a['beta']}, rates {rates}, skipped {a['skipped'][0]}")
    assert ad.K == 40 and abs(dev0 - 2.06) < 0.01 and spread0 > 0.5
    assert spread <= spread0 / 8
    assert dev <= dev0 / 8


# ---- the classes -------------------------------------------------------------------------------------------------------------
def dense_mvn(device):
    from target_distributions import MultivariateNormalTorch

    return MultivariateNormalTorch(3, cov=[[1, 0.5, 0], [0.5, 1, 0], [0, 0, 1]], device=device)


LADDER4 = [1.0, 0.7, 0.4, 0.05]


def pt_class(device, target, **kw):
    from algorithms import ParallelTemperingRWM_GPU_Optimized

    np.random.seed(4)  # (the samplers draw their 1e-8 N(0, 1) starting point from NumPy's global generator)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a target without a fused kernel says that it runs split steps)
        return ParallelTemperingRWM_GPU_Optimized(target.dim, 2.0, target, beta_ladder=LADDER4, swap_every=4, device=device,
                                                  num_replicas=40, seed=SEED, trace="none", **kw)


@gpu
def test_split_steps(device):
    """A dense-covariance Gaussian has no fused kernel: the host loop ends its blocks at every probe step.  Its ladder history
    equals the one obtained by driving plain split steps, the stand-alone probe and the stand-alone update by hand."""
    burn, every, pe, n = 40, 16, 8, 40 + 24
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alg = pt_class(device, dense_mvn(device), burn_in=burn, adapt_ladder=True, ladder_every=every, ladder_probe_every=pe)
        alg._advance(n)
        assert alg._run.density_fn is not None
        h = alg._run.ladder_history()
        hand = pt_class(device, dense_mvn(device), burn_in=burn)
        hand._ensure_started()
        run = hand._run
        pooled = torch.zeros(4, dtype=torch.int64, device=device)
        bh = torch.full((3, 4), -1.0, device=device)
        rh = torch.full((2, 4), -1, dtype=torch.int64, device=device)
        # (bound for the stand-alone entries: the hand-driven steps are plain split steps, which never see it)
        run._plan.set_ladder(pooled, every=every, probe_every=pe, until=burn, beta_history=bh, rate_history=rh)
        for s in range(n):
            run._advance_split_plain(1, None, None, 0, 1)
            if s < 2 * every and (s + 1) % pe == 0:
                run._plan.ladder_probe()
                if (s + 1) % every == 0:
                    run._plan.ladder_update((s + 1) // every - 1)
    torch.cuda.synchronize()
    assert torch.equal(h["betas"], bh) and torch.equal(h["pooled"], rh) and bool((bh[2][1:3] != bh[0][1:3]).all())
    assert h["probes"].tolist() == [40 * 2, 40 * 2]
    for k in ("state", "logp", "n_accept", "swap_accept", "beta"):
        assert torch.equal(getattr(alg._run, k), getattr(run, k)), k
    assert alg._run.post_burn_steps == 24 and int(alg._run.swap_accept.sum()) > 0


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_classes(device, dtype):
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from algorithms.sharding import adaptation_sync
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(5, device=device)
    burn, every, n, R = 120, 25, 40, 300
    Kc = burn // every  # 4 windows; steps 100..119 are ordinary burn-in
    calls = []

    def sync(pooled):
        calls.append(tuple(pooled.shape))
        return adaptation_sync()(pooled)

    def make(**kw):
        np.random.seed(4)
        return ParallelTemperingRWM_GPU_Optimized(5, 8.0, tgt, beta_ladder=LADDER4, swap_every=5, burn_in=burn, device=device,
                                                  num_replicas=R, seed=SEED, trace="none", dtype=dtype, adapt_ladder=True,
                                                  ladder_every=every, moments="all", flow=True, **kw)

    pt = make()
    init32 = [float(np.float32(b)) for b in LADDER4]
    assert pt.adapted_beta_ladder() == init32
    pt.generate_samples(n)
    h, info, cur = pt.ladder_history(), pt.get_diagnostic_info(), pt.adapted_beta_ladder()
    assert tuple(h["betas"].shape) == (Kc + 1, 4) and tuple(h["rates"].shape) == (Kc, 3) and h["rates"].dtype == torch.float64
    assert h["probes"].tolist() == [R] * Kc and h["betas"][0].tolist() == init32 and h["betas"][-1].tolist() == cur
    rates = h["rates"].cpu().numpy()
    assert ((rates > 0) & (rates <= 1)).all() and np.ptp(rates[-1]) < np.ptp(rates[0])
    assert cur[0] == 1.0 and cur[-1] == init32[-1] and cur[1:-1] != init32[1:-1] and all(x > y for x, y in zip(cur, cur[1:]))
    assert pt.beta_ladder == cur and pt.beta_tensor.tolist() == cur and info["beta_ladder"] == cur
    assert info["adapted_beta_ladder"] == cur and info["init_beta_ladder"] == init32 and info["ladder_updates_skipped"] == 0
    # what the class derives from the ladder follows it
    acc = pt._run.swap_accept.sum(0).cpu().double().numpy()
    assert pt._sq_beta_jumps() == pytest.approx(float((acc[:-1] * np.diff(np.asarray(cur, np.float64)) ** 2).sum()), rel=1e-12)
    # the scales followed their temperature (one ulp per window), and every diagnostic counts post-burn-in steps only
    want = LR.rescale(pt._init_scales().cpu().numpy(), np.float32(LADDER4), np.float32(cur)).astype(np.float64)
    assert (np.abs(pt.proposal_scales().cpu().numpy() / want - 1) <= (Kc + 1) * 2.0 ** -24).all()  # (a rounding per window, and one here)
    assert pt.moment_count.cpu().tolist() == [R * n] * 4 and pt._run.flow()["events"] == n // 5
    assert int(pt._run.n_accept.sum(0).max()) <= R * n and int(pt._run.n_accept.sum()) > 0
    # reset(): again from the initial ladder and scales, and with a fixed seed the same bits
    state, scales = pt._run.state.clone(), pt.proposal_scales()
    pt.reset()
    assert pt.beta_ladder == LADDER4 and pt.adapted_beta_ladder() == init32 and bool(torch.isnan(pt.ladder_history()["betas"][1:]).all())
    pt.generate_samples(n)
    h2 = pt.ladder_history()
    assert torch.equal(h2["betas"], h["betas"]) and torch.equal(h2["rates"], h["rates"]) and torch.equal(pt._run.state, state)
    assert torch.equal(pt.proposal_scales(), scales)
    # adapt_sync (the identity all-reduce of a single shard, counting its calls) gives the bits of the run without it
    sy = make(adapt_sync=sync)
    sy.step()
    sy.generate_samples(n - 1)
    assert calls == [(4,)] * Kc
    hs = sy.ladder_history()
    assert torch.equal(hs["betas"], h["betas"]) and torch.equal(hs["rates"], h["rates"])


# ---- both tunings at once, cut anywhere ----------------------------------------------------------------------------------------
def own_density(target):
    """The library's own density of `target` behind log_density() alone: without engine_target() the classes run it in split
    steps."""
    from interfaces import TorchTargetDistribution

    class OwnDensity(TorchTargetDistribution):
        def get_name(self):
            return "OwnDensity"

        def log_density(self, x):
            return target.log_density(x)

        def density(self, x):
            return torch.exp(self.log_density(x))

    return OwnDensity(target.dim, target.device)


def _both_tunings(device, split, sync, cuts):
    """36 steps of a 4 x 4 x 3 Gaussian run under both tunings, advanced by `cuts`; everything the run holds, on the host."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    target = MultivariateNormalTorch(3, device=device)
    np.random.seed(4)  # (the samplers draw their 1e-8 N(0, 1) starting point from NumPy's global generator)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a target without a fused kernel says that it runs split steps)
        alg = ParallelTemperingRWM_GPU_Optimized(3, 2.0, own_density(target) if split else target, beta_ladder=LADDER4, swap_every=3,
                                                 burn_in=26, device=device, num_replicas=4, seed=SEED, trace="none",
                                                 adapt_scale=True, adapt_every=6, adapt_ladder=True, ladder_every=4,
                                                 ladder_probe_every=2, adapt_sync=(lambda pooled: pooled) if sync else None)
        for n in cuts:
            alg._advance(n)
    run = alg._run
    assert (run.density_fn is not None) == split and run.steps_done == sum(cuts) == 36
    torch.cuda.synchronize()
    out = {"state": run.state, "logp": run.logp, "n_accept": run.n_accept, "swap_accept": run.swap_accept,
           "scales": alg.proposal_scales(), "beta": run.beta_ladder(),
           **{"scale " + k: v for k, v in run.adaptation_history().items()},
           **{"ladder " + k: v for k, v in run.ladder_history().items()}}
    assert alg.beta_ladder == out["beta"].tolist()
    return {k: v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for k, v in out.items()}


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_both_tunings_cut_anywhere(device, split):
    """adapt_every = 6 next to ladder_every = 4 with a probe every 2 steps, burn_in = 26: the scale's windows end behind steps
    5, 11, 17, 23, the ladder's behind 3, 7, .., 23 - interleaved, and together behind 11 and 23 - then two steps of plain
    burn-in and 10 steps with swap events.  Advanced in calls of every size 1 .. 13 (the size repeated until 36 steps are done),
    with and without adapt_sync (a callable that leaves the counts alone: the deferred-update path), every output has the bits
    of the single call: state, logp, scales, ladder, both histories, the acceptance counts."""
    outs = {}
    for sync in (False, True):
        whole = outs[sync] = _both_tunings(device, split, sync, [36])
        assert whole["ladder betas"].shape == (7, 4) and whole["scale scales"].shape == (5, 4) and whole["ladder skipped"] == 0
        assert np.isfinite(whole["ladder betas"]).all() and np.isfinite(whole["scale scales"]).all()  # every window has run
        assert (whole["ladder betas"][6][1:3] != whole["ladder betas"][0][1:3]).all() and (whole["scale scales"][4] != whole["scale scales"][0]).all()
        assert whole["ladder probes"].tolist() == [4 * 2] * 6 and whole["swap_accept"].sum() > 0 and whole["n_accept"].max() <= 10
        for size in range(1, 14):
            cuts = [size] * (36 // size) + ([36 % size] if 36 % size else [])
            got = _both_tunings(device, split, sync, cuts)
            assert got.keys() == whole.keys()
            for k in whole:
                assert np.array_equal(got[k], whole[k], equal_nan=True), f"calls of {size} steps, adapt_sync {sync}: {k}"
    for k in outs[False]:
        assert np.array_equal(outs[False][k], outs[True][k], equal_nan=True), f"adapt_sync against none: {k}"
