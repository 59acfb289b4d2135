"""Replica flow through the ladder (include/ptrwm.h ptrwm_flow_args, csrc/flow.h) on the GPU.

The yardstick is independent of the code under test: the engine's own swap_accept counters, read after every one-step
launch, say which pairs an event accepted; a NumPy replay below applies those to arange(T) - transpositions (exchange) or
copies (reference_copy), j ascending - and then the rule's steps 2 and 3.  walker, round_trips, n_up and n_down must be EQUAL
to the replay after every launch.  On top: flow does not depend on where launches are cut, on the kernel form or on sharding,
perturbs no other output, and is the same through split steps (eager and captured) and stand-alone sweeps.

Shapes (T, n_chains), each for a path that can go wrong: (2, 70) the ends are adjacent, 32 ladders per wave, a partial last
group; (5, 13) T does not divide 64: idle lanes; (8, 9); (64, 3) one ladder per wave; (70, 2) the wide thread-form group;
(20, 4) lane-split wide, three ladders per workgroup; (40, 2) lane-split wide, the one-lane scan under sequential exchange.
Long ladders get a ladder of nearly equal temperatures: almost every swap is accepted, so the walker that starts at the hot
end can reach the cold end - a completed trip by the rule - within the run, and a few of the thousands of attempts still fail.
"""
import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E

gpu = pytest.mark.gpu

DIM = 3
#        T   chains  beta_min  steps  swap_every  burn_in
SHAPES = [(2, 70, 0.30, 40, 2, 3),
          (5, 13, 0.30, 60, 1, 3),
          (8, 9, 0.30, 60, 1, 3),
          (64, 3, 0.75, 80, 1, 2),
          (70, 2, 0.75, 80, 1, 2),
          (20, 4, 0.90, 60, 1, 2),
          (40, 2, 0.70, 80, 1, 2)]
SHAPE_IDS = [f"T{s[0]}x{s[1]}" for s in SHAPES]
MODES = ["exchange", "reference_copy"]
ORDERS = ["sequential", "even_odd"]
# (kernel form, double states): double states run the lane-split form only
KINDS = [("thread", E.FORM_THREAD, False), ("quad", E.FORM_QUAD, False), ("quad_f64", E.FORM_QUAD, True)]
SEED = 20240607


def betas_of(T, beta_min):
    return np.geomspace(1.0, beta_min, T).astype(np.float32)




def _diag_spec():
    import math

    return H.TargetSpec(kind=E.TARGET_DIAG_GAUSSIAN, dim=DIM, p=(-0.5 * DIM * math.log(2 * math.pi),), ip=(1,),
                        vec0=np.ones(DIM, np.float32))


def proposal_spec(betas):
    return H.proposal_spec("Normal", DIM, betas, base_variance_scalar=2.38 ** 2 / DIM)


def start(T, Cn, f64=False):
    rng = np.random.default_rng(1000 * T + Cn)
    return rng.normal(0.0, 1.0, size=(Cn, T, DIM)).astype(np.float64 if f64 else np.float32)


def test_every_pinned_form_has_a_variant():
    """No GPU needed: every (shape, form) the tests below pin has a compiled variant, so no case can skip or silently run
    the other form."""
    spec, prop = _diag_spec(), proposal_spec(betas_of(2, 0.5))
    assert E.has_thread_variant(spec.kind, prop.kind, DIM)
    for T, *_ in SHAPES:
        assert E.has_quad_variant(spec.kind, prop.kind, DIM, T), T


# ---- the replay: 30 lines of NumPy ---------------------------------------------------------------------------------------
class Replay:
    def __init__(self, Cn, T, mode):
        self.lab = np.tile(np.arange(T, dtype=np.int64), (Cn, 1))
        self.dir = np.zeros((Cn, T), np.int64)  # 0 none, 1 up, 2 down
        self.trips, self.up, self.down = (np.zeros((Cn, T), np.int64) for _ in range(3))
        self.mode, self.events = mode, 0

    def event(self, acc):
        """acc [chains, T] 0/1: pair (j, j+1) accepted in this event (the increment of swap_accept)."""
        Cn, T = self.lab.shape
        for j in range(T - 1):  # ascending; the pairs of an even/odd event are disjoint
            m = acc[:, j] == 1
            for a in (self.lab, self.dir):
                lo, hi = a[m, j].copy(), a[m, j + 1].copy()
                a[m, j] = hi
                if self.mode == "exchange":
                    a[m, j + 1] = lo
        done = self.dir[:, 0] == 2  # step 2: a walker that came down from the hot end is back at the cold end
        np.add.at(self.trips, (np.nonzero(done)[0], self.lab[done, 0]), 1)
        self.dir[:, 0], self.dir[:, T - 1] = 1, 2
        self.up += self.dir == 1  # step 3
        self.down += self.dir == 2
        self.events += 1

    def walker(self):
        return (self.lab | (self.dir << 16)).astype(np.int32)


class Run:
    """One sampler run through the C ABI with every output on the device."""

    def __init__(self, device, T, Cn, beta_min, *, burn, se, mode, order, f64=False, flow=True, chain_offset=0, x0=None,
                 target=True, seed=SEED):
        self.T, self.Cn, self.device = T, Cn, device
        betas = betas_of(T, beta_min)
        self.spec, self.prop = _diag_spec(), proposal_spec(betas)
        self.tgt = self.spec.engine(device)
        x0 = start(T, Cn, f64) if x0 is None else x0
        self.st = torch.tensor(x0, device=device, dtype=torch.float64 if f64 else torch.float32)
        self.lp = E.logdensity(self.tgt, self.st.view(-1, DIM).float()).view(Cn, T).contiguous()
        self.stats = {k: torch.zeros(Cn, T, dtype=(torch.float64 if k == "sq_jump" else torch.int64), device=device)
                      for k in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")}
        self.plan = E.RunPlan(self.tgt if target else None, self.prop.engine(device), state=self.st, logp=self.lp,
                              beta=torch.tensor(betas, device=device), burn_in=burn, swap_every=se, swap_mode=E.SWAP_MODES[mode],
                              swap_order=E.SWAP_ORDERS[order], seed=seed, chain_offset=chain_offset, **self.stats)
        self.flow = None
        if flow:
            self.flow = {"walker": torch.arange(T, device=device, dtype=torch.int32).repeat(Cn, 1).contiguous(),
                         **{k: torch.zeros(Cn, T, dtype=torch.int64, device=device) for k in ("round_trips", "n_up", "n_down")}}
            self.plan.set_flow(self.flow["walker"], self.flow["round_trips"], self.flow["n_up"], self.flow["n_down"])

    def launches(self, cuts, step0=0):
        for n in cuts:
            self.plan.launch(step0, n)
            step0 += n
        return self

    def flow_np(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.flow.items()}

    def rest_np(self):
        torch.cuda.synchronize()
        return {"state": self.st.cpu().numpy(), "logp": self.lp.cpu().numpy(), **{k: v.cpu().numpy() for k, v in self.stats.items()}}


def assert_flow_equal(a, b, what=""):
    for k in ("walker", "round_trips", "n_up", "n_down"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:4].tolist())


def assert_rest_equal(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def check_invariants(f, events, T, exchange):
    assert (f["n_up"][:, 0] == events).all() and (f["n_down"][:, T - 1] == events).all()
    assert (f["n_up"][:, T - 1] == 0).all() and (f["n_down"][:, 0] == 0).all()
    assert (f["n_up"] + f["n_down"] <= events).all() and f["round_trips"].min() >= 0
    if exchange:
        assert (np.sort(f["walker"] & 0xFFFF, axis=1) == np.arange(T)).all()


# ---- 1. replay, 5. invariants --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_flow_equals_the_replay_of_the_accepted_swaps_after_every_launch(device, shape, mode, order, kind):
    T, Cn, beta_min, steps, se, burn = shape
    _, form, f64 = kind
    with E.kernel_form(form):
        r = Run(device, T, Cn, beta_min, burn=burn, se=se, mode=mode, order=order, f64=f64)
        rep = Replay(Cn, T, mode)
        prev = np.zeros((Cn, T), np.int64)
        attempts = 0
        for s in range(steps):
            r.plan.launch(s, 1)
            assert E.last_launch_kind() == (E.LAUNCH_THREAD if form == E.FORM_THREAD else E.LAUNCH_QUAD)
            f = r.flow_np()
            now = r.stats["swap_accept"].cpu().numpy()
            if s + 1 > burn and (s + 1) % se == 0:
                rep.event(now - prev)
                attempts += Cn * ((T - 1) if order == "sequential" else len(range((rep.events - 1) & 1, T - 1, 2)))
            else:
                assert np.array_equal(now, prev)
            prev = now
            want = {"walker": rep.walker(), "round_trips": rep.trips, "n_up": rep.up, "n_down": rep.down}
            assert_flow_equal(f, want, f"step {s}")
    assert rep.events == E.periodic_steps_in(0, steps, se, burn) and rep.events > 0
    check_invariants(f, rep.events, T, mode == "exchange")
    assert np.array_equal(f["round_trips"].sum(1), rep.trips.sum(1))
    print(f"T {T} chains {Cn} {mode} {order} {kind[0]}: {rep.events} events, {int(rep.trips.sum())} round trips, "
          f"{attempts - int(prev.sum())} of {attempts} swaps refused")
    assert rep.trips.sum() >= 1, "the run completes no round trip: the case does not exercise step 2"
    assert prev.sum() < attempts, "no swap was refused"


# ---- 2. cuts; nothing else changes ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("mode,order", [("exchange", "sequential"), ("reference_copy", "even_odd")])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_flow_does_not_depend_on_the_cuts_and_perturbs_nothing(device, shape, mode, order, kind):
    T, Cn, beta_min, steps, se, burn = shape
    _, form, f64 = kind
    kw = dict(burn=burn, se=se, mode=mode, order=order, f64=f64)
    with E.kernel_form(form):
        cuts = {"one launch": [steps], "one-step launches": [1] * steps, "7 + 1 + rest": [7, 1, steps - 8]}
        with_flow = {what: Run(device, T, Cn, beta_min, **kw).launches(c) for what, c in cuts.items()}
        plain = {what: Run(device, T, Cn, beta_min, flow=False, **kw).launches(c) for what, c in cuts.items()}
    f = with_flow["one launch"].flow_np()
    for what in ("one-step launches", "7 + 1 + rest"):
        assert_flow_equal(f, with_flow[what].flow_np(), "one launch against " + what)
    check_invariants(f, E.periodic_steps_in(0, steps, se, burn), T, mode == "exchange")
    # state, logp and every counter: bit-identical to the same run, cut the same way, without flow ...
    want = plain["one launch"].rest_np()
    for what in cuts:
        got = with_flow[what].rest_np()
        assert_rest_equal(got, plain[what].rest_np(), what)
        # ... and, but for the launch-wise partial sums of the squared jumps (a double per launch, added to the total when it
        # ends: exact for float states here, rounded for double ones), the same however the run is cut
        assert_rest_equal({k: v for k, v in got.items() if k != "sq_jump" or not f64}, {k: v for k, v in want.items() if k != "sq_jump" or not f64}, what)
    assert want["swap_accept"].sum() > 0 and f["n_up"].sum() > 0


# ---- 3. forms and shards --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,order", [("exchange", "sequential"), ("exchange", "even_odd"), ("reference_copy", "sequential")])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_flow_is_the_same_in_both_forms_and_in_two_shards(device, shape, mode, order):
    T, Cn, beta_min, steps, se, burn = shape
    kw = dict(burn=burn, se=se, mode=mode, order=order)
    with E.kernel_form(E.FORM_THREAD):
        th = Run(device, T, Cn, beta_min, **kw).launches([steps])
        assert E.last_launch_kind() == E.LAUNCH_THREAD
    with E.kernel_form(E.FORM_QUAD):
        qu = Run(device, T, Cn, beta_min, **kw).launches([5, steps - 5])
        assert E.last_launch_kind() == E.LAUNCH_QUAD
    f = th.flow_np()
    assert_flow_equal(f, qu.flow_np(), "thread form against lane-split form")
    assert_rest_equal(th.rest_np(), qu.rest_np(), "forms")
    # two shards with chain_offset: the same ladders, whichever group of whichever launch they sit in
    x0 = start(T, Cn)
    k = Cn // 2
    a = Run(device, T, k, beta_min, x0=x0[:k], **kw).launches([steps])
    b = Run(device, T, Cn - k, beta_min, x0=x0[k:], chain_offset=k, **kw).launches([steps])
    fa, fb = a.flow_np(), b.flow_np()
    assert_flow_equal(f, {key: np.concatenate([fa[key], fb[key]]) for key in fa}, "two shards against one run")


# ---- 4. split steps and the stand-alone sweep -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,order", [("exchange", "sequential"), ("reference_copy", "even_odd")])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5]], ids=[SHAPE_IDS[1], SHAPE_IDS[4], SHAPE_IDS[5]])
def test_split_steps_eager_and_captured_give_the_fused_runs_flow(device, shape, mode, order):
    T, Cn, beta_min, _, _, _ = shape
    burn, se, K, replays, tail = 3, 2, 8, 3, 3
    N = 1 + K * replays + tail  # the captured block starts at step 1... made a multiple of swap_every below
    kw = dict(burn=burn, se=se, mode=mode, order=order)
    s0 = 1  # (s0 + 1 = 2: after the one eager step the block starts at a multiple of swap_every)
    fused = Run(device, T, Cn, beta_min, **kw).launches([N], step0=s0)
    want, want_rest = fused.flow_np(), fused.rest_np()
    assert want["n_up"][:, 0].min() == E.periodic_steps_in(s0, s0 + N, se, burn) > 0

    # eager: host-side step indices
    eager = Run(device, T, Cn, beta_min, target=False, **kw)
    for s in range(s0, s0 + N):
        props = eager.plan.split_propose(s)
        eager.plan.split_accept(s, E.logdensity(eager.tgt, props.view(-1, DIM)).view(Cn, T))
    assert_flow_equal(eager.flow_np(), want, "eager split steps")
    assert_rest_equal(eager.rest_np(), want_rest, "eager split steps")

    # captured: device-step mode, the swap kernel enqueued only at the block's swap steps
    cap = Run(device, T, Cn, beta_min, target=False, **kw)
    counter = torch.full((1,), s0, dtype=torch.int64, device=device)
    cap.plan.set_device_step(counter)

    def step(offset=0, no_sweep=False, advance=1):
        props = cap.plan.split_propose(offset)
        cap.plan.split_accept(offset, E.logdensity(cap.tgt, props.view(-1, DIM)).view(Cn, T), no_sweep=no_sweep)
        if advance:
            cap.plan.split_advance(advance)

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()  # one step outside capture
    torch.cuda.current_stream(device).wait_stream(side)
    assert (s0 + 1) % se == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for j in range(K):
            step(offset=j, no_sweep=(j + 1) % se != 0, advance=K if j == K - 1 else 0)
    for _ in range(replays):
        g.replay()
    for _ in range(tail):
        step()  # (the swap kernel rides with every step and decides on the device: a step that is not due changes nothing)
    torch.cuda.synchronize()
    assert int(counter.item()) == s0 + N
    assert_flow_equal(cap.flow_np(), want, "captured split steps")
    assert_rest_equal(cap.rest_np(), want_rest, "captured split steps")

    # a PTRWM_SPLIT_NO_SWEEP step and a step that is not due change nothing of flow (here: two burn-in steps from counter 0)
    counter.zero_()
    before = cap.flow_np()
    step(no_sweep=True)
    step()
    assert_flow_equal(cap.flow_np(), before, "steps without an event")


@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[4]])
def test_a_sweep_on_the_fused_kernels_stream_reproduces_the_fused_event(device, shape, mode, order):
    """ptrwm_swap_sweep_with_flow with step0 = s and rng_stream = 1 is the swap event ptrwm_run performs at step s: run s
    steps fused, then either one more fused step with swap_every = 1, or its Metropolis part alone (a run that has no event
    there: swap_every too long) followed by the sweep.  State, log-densities, swap counters and flow agree."""
    T, Cn, beta_min, _, _, _ = shape
    s, burn = 12, 2
    kw = dict(burn=burn, mode=mode, order=order)
    fused = Run(device, T, Cn, beta_min, se=1, **kw).launches([s + 1])
    # the same run up to step s, then step s without its event: swap_every = 1 for the first s steps ...
    split = Run(device, T, Cn, beta_min, se=1, **kw).launches([s])
    # ... and a second plan over the SAME tensors whose schedule has no event at step s
    late = E.RunPlan(split.tgt, split.prop.engine(device), state=split.st, logp=split.lp, beta=torch.tensor(betas_of(T, beta_min), device=device),
                     burn_in=burn, swap_every=1000, swap_mode=E.SWAP_MODES[mode], swap_order=E.SWAP_ORDERS[order], seed=SEED,
                     **split.stats)
    late.set_flow(split.flow["walker"], split.flow["round_trips"], split.flow["n_up"], split.flow["n_down"])
    late.launch(s, 1)
    mid = split.flow_np()
    events_before = E.periodic_steps_in(0, s, 1, burn)
    assert (mid["n_up"][:, 0] == events_before).all()  # the step without an event left flow alone
    late.swap_sweep(rng_step=s, event_index=events_before, rng_stream=1)
    got, want = split.flow_np(), fused.flow_np()
    assert_flow_equal(got, want, "sweep against the fused event")
    a, b = split.rest_np(), fused.rest_np()
    for k in ("state", "logp", "swap_accept", "last_swap_ordinal", "n_accept"):
        assert np.array_equal(a[k], b[k]), k
    check_invariants(got, events_before + 1, T, mode == "exchange")


# ---- 6. the class ---------------------------------------------------------------------------------------------------------
def _pt(device, flow, **kw):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, geometric_beta_ladder
    from target_distributions import RoughCarpetDistributionTorch

    target = RoughCarpetDistributionTorch(4, device=device, mode_centers=[-3.0, 0.0, 3.0])
    return ParallelTemperingRWM_GPU_Optimized(4, 2.38 ** 2 / 4, target, beta_ladder=geometric_beta_ladder(8, 0.05), swap_every=2,
                                              burn_in=10, device=device, num_replicas=16, seed=77, trace="none", flow=flow, **kw)


@gpu
def test_class_accessors_reset_and_diagnostics(device):
    alg = _pt(device, True)
    alg.generate_samples(300)
    R, T = 16, 8
    events = (310 // 2) - (10 // 2)
    rt, uf, wp = alg.round_trips(), alg.up_fraction(), alg.walker_positions()
    assert rt.shape == (R, T) and rt.dtype == torch.int64 and rt.is_cuda
    assert uf.shape == (T,) and uf.dtype == torch.float64
    assert wp.shape == (R, T) and wp.dtype == torch.int32
    assert uf[0].item() == 1.0 and uf[-1].item() == 0.0 and bool(((uf >= 0) & (uf <= 1)).all())
    assert (wp.sort(dim=1).values.cpu() == torch.arange(T, dtype=torch.int32)).all()  # exchange: a permutation
    f = alg._run.flow()
    assert f["events"] == events
    check_invariants({k: v.cpu().numpy() for k, v in f.items() if k != "events"}, events, T, True)
    total = int(rt.sum().item())
    assert total >= 1 and alg.round_trip_rate() == total / (R * T * events)
    info = alg.get_diagnostic_info()
    assert info["round_trips_total"] == total and torch.equal(info["up_fraction"], uf.cpu())
    # _attempt_all_swaps keeps flow consistent: one more event
    alg._attempt_all_swaps()
    f2 = alg._run.flow()
    assert f2["events"] == events + 1
    check_invariants({k: v.cpu().numpy() for k, v in f2.items() if k != "events"}, events + 1, T, True)
    alg.reset()
    assert alg.walker_positions().cpu().tolist() == [list(range(T))] * R and int(alg.round_trips().sum().item()) == 0
    alg.generate_samples(20)
    assert alg._run.flow()["events"] == 10 and (alg._run.flow()["n_up"][:, 0] == 10).all()
    alg._run.reset_flow()
    assert alg._run.flow()["walker"].cpu().tolist() == [list(range(T))] * R and int(alg._run.flow()["n_up"].sum().item()) == 0
    assert alg._run.flow()["events"] == 0  # the event count restarts with the arrays: the invariants hold for what they cover
    alg._run.advance(6)
    f3 = alg._run.flow()
    assert f3["events"] == 3
    check_invariants({k: v.cpu().numpy() for k, v in f3.items() if k != "events"}, 3, T, True)


@gpu
def test_class_flow_changes_no_state_and_combines_with_moments(device):
    on, off = _pt(device, True), _pt(device, False)
    on.generate_samples(120)
    off.generate_samples(120)
    assert torch.equal(on._run.state, off._run.state) and torch.equal(on._run.logp, off._run.logp)
    for k in ("n_accept", "sq_jump", "swap_accept", "last_ord"):
        assert torch.equal(getattr(on._run, k), getattr(off._run, k)), k
    with pytest.raises(RuntimeError, match="flow=True"):
        off.up_fraction()
    both = _pt(device, True, moments="cold", moments_per_chain=True)
    both.generate_samples(120)
    assert torch.equal(both._run.state, off._run.state)
    assert torch.equal(both.round_trips(), on.round_trips()) and torch.equal(both.walker_positions(), on.walker_positions())
    assert int(both.moment_count[0].item()) == 16 * 120 and torch.isfinite(both.rhat()).all()
    mom = _pt(device, False, moments="cold", moments_per_chain=True)
    mom.generate_samples(120)
    assert torch.equal(mom._run.chain_moments()["sum"], both._run.chain_moments()["sum"])
    pooled = _pt(device, True, moments="all")
    pooled.generate_samples(120)
    assert torch.equal(pooled.round_trips(), on.round_trips()) and int(pooled.moment_count[-1].item()) == 16 * 120
    # double states
    d64 = _pt(device, True, dtype=torch.float64)
    d64.generate_samples(120)
    assert d64.up_fraction()[0].item() == 1.0 and d64.up_fraction()[-1].item() == 0.0 and d64._run.state.dtype == torch.float64
    from algorithms.sharding import allreduce_flow

    out = allreduce_flow(on._run.flow())  # no process group: the job is this shard
    assert torch.equal(out["up_fraction"], on.up_fraction()) and out["round_trip_rate"] == on.round_trip_rate()


@gpu
def test_class_flow_with_a_split_step_target_eager_and_graph(device):
    """A target without a fused kernel runs split steps: eager and through the captured graph, flow equals the fused run's."""
    from interfaces import TorchTargetDistribution

    fused = _pt(device, True)
    fused.generate_samples(90)
    tgt, name = fused.target_dist.engine_target(), fused.target_dist.get_name()
    assert "RoughCarpet" in name

    class Wrapped(TorchTargetDistribution):  # the same density, no engine_target(): split steps
        def __init__(self):
            super().__init__(4, device)

        def get_name(self):  # (the samplers' default starting point depends on the target's name: the wrapped target's)
            return name

        def density(self, x):
            return torch.exp(self.log_density(x))

        def log_density(self, x):
            return E.logdensity(tgt, x.contiguous())

        def to(self, dev):
            return self

    from algorithms import ParallelTemperingRWM_GPU_Optimized, geometric_beta_ladder

    for use_graph in (False, True):
        with pytest.warns(UserWarning, match="split steps"):
            alg = ParallelTemperingRWM_GPU_Optimized(4, 2.38 ** 2 / 4, Wrapped(), beta_ladder=geometric_beta_ladder(8, 0.05),
                                                     swap_every=2, burn_in=10, device=device, num_replicas=16, seed=77,
                                                     trace="none", flow=True)
            alg._ensure_started()
        alg._run.use_graph = use_graph
        alg.generate_samples(90)
        assert torch.equal(alg._run.state, fused._run.state), use_graph
        assert torch.equal(alg.round_trips(), fused.round_trips()) and torch.equal(alg._run.flow()["walker"], fused._run.flow()["walker"])
        assert torch.equal(alg._run.flow()["n_up"], fused._run.flow()["n_up"]) and torch.equal(alg._run.flow()["n_down"], fused._run.flow()["n_down"])


@gpu
def test_class_refuses_flow_on_a_one_temperature_ladder(device):
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    with pytest.raises(ValueError, match="two temperatures"):
        ParallelTemperingRWM_GPU_Optimized(4, 1.0, RoughCarpetDistributionTorch(4, device=device), beta_ladder=[1.0], device=device,
                                           flow=True)
