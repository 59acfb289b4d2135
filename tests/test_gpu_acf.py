"""Pooled lagged autocovariance (include/ptrwm.h ptrwm_acf_args, csrc/acf.h) on the GPU.  Every run goes through the C ABI.

Two yardsticks, both independent of the code under test:
  * hand-made states of small integers, where every product and every partial sum is exact in fp64 whatever the order of the
    atomics: the sums must EQUAL the NumPy replay;
  * a run with a full trace of the covered temperatures: the trace's terms - x_j x_{j-k} as one float64 product each, which is
    what csrc/acf.h's acf_term computes - summed with math.fsum, which is correctly rounded, so only the GPU's order of additions
    is in play.  Per element the bound is (n - 1) 2^-53 sum|term|, n the number of its terms: the standard bound for summation in
    any order.  `pairs` is equal.
"""
import math

import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E

gpu = pytest.mark.gpu

SEED = 20261020
U = 2.0 ** -53


def diag_spec(dim):
    return H.TargetSpec(kind=E.TARGET_DIAG_GAUSSIAN, dim=dim, p=(-0.5 * dim * math.log(2 * math.pi),), ip=(1,),
                        vec0=np.ones(dim, np.float32))


def due_rows(step0, n_steps, burn, every):
    """Indices, within a trace of every step of the request, of the steps whose step counter is due."""
    return [i for i in range(n_steps) if step0 + i + 1 > burn and (step0 + i + 1) % every == 0]


def replay(rows, max_lag, exact=False):
    """The sums of snapshot rows [snapshots, chains, temps, dim] and their bounds.  Every term in float64 as the kernel forms it
    (both values converted to double, one product); `exact`: plain NumPy sums (integer-valued states: every partial sum is exact),
    else math.fsum.  Returns ({sxy, head, tail} [temps, max_lag + 1, dim], pairs [max_lag + 1], bounds of the same shapes)."""
    rows = np.asarray(rows).astype(np.float64)  # (float -> double is exact; a double state stays what it is)
    S, Cn, Tc, D = rows.shape
    want = {k: np.zeros((Tc, max_lag + 1, D)) for k in ("sxy", "head", "tail")}
    bound = {k: np.zeros((Tc, max_lag + 1, D)) for k in ("sxy", "head", "tail")}
    pairs = np.zeros(max_lag + 1, np.int64)
    for k in range(min(max_lag, S - 1) + 1):
        x, y = rows[k:], rows[:S - k]  # x_j and x_{j-k}, j = k .. S - 1
        n = (S - k) * Cn
        pairs[k] = n
        for name, terms in (("sxy", x * y), ("head", x), ("tail", y)):
            flat = terms.reshape(n, Tc * D)
            tot = flat.sum(0) if exact else np.array([math.fsum(flat[:, e]) for e in range(Tc * D)])
            want[name][:, k] = tot.reshape(Tc, D)
            bound[name][:, k] = ((n - 1) * U * np.abs(flat).sum(0)).reshape(Tc, D)
    return want, pairs, bound


def assert_within(got, want, bound, what, factor=1.0):
    for k in ("sxy", "head", "tail"):
        err = np.abs(got[k] - want[k])
        worst = np.unravel_index(np.argmax(err - factor * bound[k]), err.shape)
        print(f"{what}: {k} max error {err.max():.3e}, at its worst element error {err[worst]:.3e} against a bound of {factor * bound[k][worst]:.3e}")
        assert (err <= factor * bound[k]).all(), (what, k, worst, err[worst], bound[k][worst])


class Acc:
    """The accumulator's arrays on the device, bound to a plan."""

    def __init__(self, plan, device, Cn, temps, dim, max_lag, every, dtype):
        self.ring = torch.full((max_lag, Cn, temps, dim), float("nan"), device=device, dtype=dtype)  # (a slot is written before it is read)
        self.sums = {k: torch.zeros(temps, max_lag + 1, dim, dtype=torch.float64, device=device) for k in ("sxy", "head", "tail")}
        self.pairs = torch.zeros(max_lag + 1, dtype=torch.int64, device=device)
        plan.set_autocorr(self.ring, self.sums["sxy"], self.sums["head"], self.sums["tail"], self.pairs, every=every)

    def np(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.sums.items()}, self.pairs.cpu().numpy()


# ---- 1. equality on hand-made states -----------------------------------------------------------------------------------
# tests/test_acf_host.py holds every row against acf_geometry itself.
EQUALITY_CASES = [dict(name="partial_tile", dim=5, T=1, temps=1, Cn=70, max_lag=3, snaps=12),        # 3 max_lag + 2 < 12: the ring wraps
                  dict(name="second_workgroup", dim=15, T=4, temps=2, Cn=300, max_lag=1, snaps=6),   # temps < n_temps; max_lag = 1
                  dict(name="narrowest", dim=1, T=1, temps=1, Cn=300, max_lag=8, snaps=5),           # the ring never fills
                  dict(name="widest", dim=64, T=4, temps=4, Cn=70, max_lag=2, snaps=9),
                  dict(name="t32_d30", dim=30, T=32, temps=32, Cn=70, max_lag=3, snaps=12),          # four column groups of 240
                  dict(name="d70_t8", dim=70, T=8, temps=8, Cn=40, max_lag=2, snaps=9)]              # three groups of 187, 187, 186


def test_equality_cases_cover_the_lags_the_issue_names():
    """No GPU needed."""
    assert any(c["max_lag"] == 1 for c in EQUALITY_CASES)
    assert any(c["snaps"] > 3 * c["max_lag"] + 2 for c in EQUALITY_CASES)
    assert any(c["snaps"] < c["max_lag"] for c in EQUALITY_CASES)


@gpu
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("case", EQUALITY_CASES, ids=[c["name"] for c in EQUALITY_CASES])
def test_standalone_snapshots_of_integer_states_equal_the_replay(device, case, f64):
    """ptrwm_autocorr on a sequence of states of small integers (|x| <= 9: products below 2^7, sums far below 2^53): sxy, head,
    tail and pairs EQUAL the NumPy replay.  every = 2 and burn_in = 3: the calls behind the steps that are not due add nothing."""
    dim, T, temps, Cn, L, S = (case[k] for k in ("dim", "T", "temps", "Cn", "max_lag", "snaps"))
    every, burn = 2, 3
    dtype = torch.float64 if f64 else torch.float32
    rng = np.random.default_rng(7 * dim + Cn + L)
    n_steps = 2 + every * S  # step counters 1 .. n_steps: the due ones are 4, 6, ..., 2 + 2 S
    states = rng.integers(-9, 10, size=(n_steps, Cn, T, dim)).astype(np.float64)
    st = torch.zeros(Cn, T, dim, device=device, dtype=dtype)
    plan = E.RunPlan(None, H.proposal_spec("Normal", dim, np.ones(T, np.float32), base_variance_scalar=1.0).engine(device), state=st,
                     logp=torch.zeros(Cn, T, device=device), beta=torch.ones(T, device=device), burn_in=burn)
    acc = Acc(plan, device, Cn, temps, dim, L, every, dtype)
    dev_states = torch.tensor(states, device=device, dtype=dtype)
    for s in range(n_steps):
        st.copy_(dev_states[s])
        plan.split_autocorr(s)  # (the state after step s; the library skips the steps that are not due)
    got, pairs = acc.np()
    rows = states[due_rows(0, n_steps, burn, every)][:, :, :temps]
    assert rows.shape[0] == S
    want, want_pairs, _ = replay(rows, L, exact=True)
    assert np.array_equal(pairs, want_pairs) and want_pairs[0] == S * Cn
    for k in ("sxy", "head", "tail"):
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, f"{k}: {len(bad)} elements differ; the first (t, lag, d): {bad[:5].tolist()}"
    assert np.abs(want["sxy"][:, 1:min(L, S - 1) + 1]).sum() > 0 and (want["sxy"][:, 0] > 0).all()
    assert (want["sxy"][:, S:] == 0).all()  # lags nobody reached stay zero
    assert torch.equal(st, dev_states[-1])  # a snapshot only reads the state


# ---- 2. replay of a full trace through real runs ------------------------------------------------------------------------
class Run:
    """One sampler run through the C ABI with every output on the device."""

    def __init__(self, device, dim, T, Cn, *, burn, se, temps=0, every=1, max_lag=3, f64=False, chain_offset=0, x0=None):
        self.dim, self.T, self.Cn, self.device, self.burn, self.every, self.temps, self.max_lag = dim, T, Cn, device, burn, every, temps, max_lag
        betas = np.geomspace(1.0, 0.3, T).astype(np.float32) if T > 1 else np.ones(1, np.float32)
        self.spec, self.prop = diag_spec(dim), H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim)
        self.tgt = self.spec.engine(device)
        if x0 is None:
            x0 = np.random.default_rng(1000 * T + Cn + dim).normal(0.0, 1.0, size=(Cn, T, dim))
        self.st = torch.tensor(x0, device=device, dtype=torch.float64 if f64 else torch.float32)
        self.lp = E.logdensity(self.tgt, self.st.view(-1, dim).float()).view(Cn, T).contiguous()
        self.stats = {k: torch.zeros(Cn, T, dtype=(torch.float64 if k == "sq_jump" else torch.int64), device=device)
                      for k in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")}
        self.plan = E.RunPlan(self.tgt, self.prop.engine(device), state=self.st, logp=self.lp, beta=torch.tensor(betas, device=device),
                              burn_in=burn, swap_every=se, seed=SEED, chain_offset=chain_offset, **self.stats)
        self.acc = Acc(self.plan, device, Cn, temps, dim, max_lag, every, self.st.dtype) if temps else None

    def launches(self, cuts, step0=0, trace=None):
        row = 0
        for n in cuts:
            if trace is None:
                self.plan.launch(step0, n)
            else:
                self.plan.launch(step0, n, trace=trace, trace_row0=row)
                row += n
            step0 += n
        return self

    def rest_np(self):
        torch.cuda.synchronize()
        return {"state": self.st.cpu().numpy(), "logp": self.lp.cpu().numpy(), **{k: v.cpu().numpy() for k, v in self.stats.items()}}


def assert_rest_equal(a, b, what, sq_jump_exact=True):
    for k in ("state", "logp", "n_accept", "swap_accept", "last_swap_ordinal"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    if sq_jump_exact:
        assert np.array_equal(a["sq_jump"], b["sq_jump"]), f"{what}: sq_jump"
    else:
        # the one documented exception of any change of cuts (include/ptrwm.h ptrwm_run_args.sq_jump): the last bits of a replica
        # that crosses the trust bound in mid-launch, both sums within ~3e-5 of the exact one
        assert np.allclose(a["sq_jump"], b["sq_jump"], rtol=1e-4, atol=0.0), f"{what}: sq_jump"


#             id           dim  T  chains temps every f64
TRACE_RUNS = [("pt_d3", 3, 4, 9, 4, 1, False),
              ("pt_d3_e7", 3, 4, 9, 2, 7, False),       # temps < n_temps
              ("pt_d30", 30, 4, 5, 4, 7, False),
              ("pt_d33", 33, 4, 5, 4, 1, False),        # odd dim
              ("rwm_d30", 30, 1, 70, 1, 1, False),
              ("rwm_d33_e7", 33, 1, 37, 1, 7, False),
              ("rwm_d3", 3, 1, 300, 1, 7, False),       # a second tile of chains
              ("pt_d3_f64", 3, 4, 9, 4, 1, True),       # double states
              ("pt_d3_f64_e7", 3, 4, 9, 4, 7, True)]


def test_every_shape_has_a_step_kernel():
    """No GPU needed: no case below can fail for want of a variant."""
    for _, dim, T, *_ in TRACE_RUNS:
        spec = diag_spec(dim)
        assert E.has_thread_variant(spec.kind, E.PROPOSAL_NORMAL, dim) or E.has_quad_variant(spec.kind, E.PROPOSAL_NORMAL, dim, T), dim
    assert E.has_quad_variant(diag_spec(3).kind, E.PROPOSAL_NORMAL, 3, 4)  # double states: the lane-split form


def trace_run_setup(every):
    """(N, burn, se): burn_in is no multiple of `every` (7) or trivially one (1); swap events every 2 steps, inside the window."""
    return (24, 5, 2) if every == 1 else (75, 5, 2)


@gpu
@pytest.mark.parametrize("shape", TRACE_RUNS, ids=[s[0] for s in TRACE_RUNS])
def test_sums_are_within_the_summation_bound_of_the_trace_replay(device, shape):
    _, dim, T, Cn, temps, every, f64 = shape
    N, burn, se = trace_run_setup(every)
    L = 3
    kw = dict(burn=burn, se=se, temps=temps, every=every, max_lag=L, f64=f64)
    traced = Run(device, dim, T, Cn, **kw)  # (a trace: the FULL twin of the step kernel between the snapshots)
    trace = torch.zeros(N, Cn, temps, dim, device=device, dtype=traced.st.dtype)
    traced.launches([N], trace=trace)
    got, pairs = traced.acc.np()
    rows = trace.cpu().numpy()[due_rows(0, N, burn, every)]
    assert rows.shape[0] == (19 if every == 1 else 10) > 3 * L  # the ring wraps
    want, want_pairs, bound = replay(rows, L)
    assert np.array_equal(pairs, want_pairs) and pairs[L] == (rows.shape[0] - L) * Cn
    assert_within(got, want, bound, "traced")
    if T > 1:
        assert traced.rest_np()["swap_accept"].sum() > 0  # swap events inside the window
    # the same run without a trace - the production step kernel between the snapshots
    plain = Run(device, dim, T, Cn, **kw).launches([N])
    got_p, pairs_p = plain.acc.np()
    assert np.array_equal(pairs_p, want_pairs)
    assert_within(got_p, want, bound, "production")
    assert_rest_equal(plain.rest_np(), traced.rest_np(), "with and without a trace", sq_jump_exact=False)


# ---- 3. cuts ------------------------------------------------------------------------------------------------------------
@gpu
def test_sums_do_not_depend_on_how_the_caller_cuts_the_run(device):
    dim, T, Cn, N, L = 3, 4, 9, 60, 4
    kw = dict(burn=7, se=3, temps=4, every=4, max_lag=L)
    traced = Run(device, dim, T, Cn, **kw)
    trace = torch.zeros(N, Cn, 4, dim, device=device)
    traced.launches([N], trace=trace)
    want, want_pairs, bound = replay(trace.cpu().numpy()[due_rows(0, N, 7, 4)], L)
    assert want_pairs.tolist() == [Cn * (14 - k) for k in range(L + 1)]  # step counters 8, 12, ..., 60
    one = Run(device, dim, T, Cn, **kw).launches([N])
    for cuts in ([N], [20, 20, 20], [1] * N, [25, 35], [7, 1, 3, 49]):
        r = Run(device, dim, T, Cn, **kw).launches(cuts)
        got, pairs = r.acc.np()
        assert np.array_equal(pairs, want_pairs), cuts
        assert_within(got, want, bound, f"cuts {cuts[:4]}")
        assert_rest_equal(r.rest_np(), one.rest_np(), f"cuts {cuts}", sq_jump_exact=False)
    # `every` larger than the request: no snapshot is due, the sums stay zero, and the run is the run without the accumulator
    none = Run(device, dim, T, Cn, burn=7, se=3, temps=4, every=100, max_lag=L).launches([N])
    assert all(float(np.abs(v).sum()) == 0.0 for v in none.acc.np()[0].values()) and int(none.acc.np()[1].sum()) == 0
    off = Run(device, dim, T, Cn, burn=7, se=3).launches([N])
    assert_rest_equal(none.rest_np(), off.rest_np(), "no due step")  # (the same launches: sq_jump bit-equal too)


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------
@gpu
def test_nothing_else_moves(device):
    """State, logp and every counter of a run with the accumulator equal the same run without; moments, flow and a histogram
    bound in the same call are what they are without it."""
    dim, T, Cn, N = 3, 4, 70, 40

    def make(acf):
        r = Run(device, dim, T, Cn, burn=5, se=2, **(dict(temps=2, every=3, max_lag=4) if acf else {}))
        mom = {"sum": torch.zeros(2, dim, dtype=torch.float64, device=device), "sum_sq": torch.zeros(2, dim, dtype=torch.float64, device=device),
               "sum_logp": torch.zeros(2, dtype=torch.float64, device=device), "count": torch.zeros(2, dtype=torch.int64, device=device)}
        r.plan.set_moments(mom["sum"], mom["sum_sq"], sum_logp=mom["sum_logp"], count=mom["count"], every=2)
        flow = {"walker": torch.arange(T, device=device, dtype=torch.int32).repeat(Cn, 1).contiguous(),
                **{k: torch.zeros(Cn, T, dtype=torch.int64, device=device) for k in ("round_trips", "n_up", "n_down")}}
        r.plan.set_flow(flow["walker"], flow["round_trips"], flow["n_up"], flow["n_down"])
        nb = 16
        lo, hi = np.full(dim, -0.8, np.float32), np.full(dim, 0.9, np.float32)
        hist = {"counts": torch.zeros(2, dim, nb + 2, dtype=torch.int64, device=device), "count": torch.zeros(2, dtype=torch.int64, device=device)}
        r.plan.set_histogram(hist["counts"], torch.tensor(lo, device=device), torch.tensor((np.float32(nb) / (hi - lo)).astype(np.float32), device=device),
                             n_bins=nb, temps=2, every=5, count=hist["count"])  # (another period than the accumulator's)
        r.launches([N])
        torch.cuda.synchronize()
        return r, {k: v.cpu().numpy() for k, v in mom.items()}, {k: v.cpu().numpy() for k, v in flow.items()}, {k: v.cpu().numpy() for k, v in hist.items()}

    (on, m_on, f_on, h_on), (off, m_off, f_off, h_off) = make(True), make(False)
    assert_rest_equal(on.rest_np(), off.rest_np(), "with moments, flow and a histogram", sq_jump_exact=False)
    for k in f_on:
        assert np.array_equal(f_on[k], f_off[k]), k
    for k in h_on:  # integers: exact
        assert np.array_equal(h_on[k], h_off[k]), k
    assert h_on["count"].tolist() == [Cn * 7] * 2 and np.array_equal(m_on["count"], m_off["count"])
    for k in ("sum", "sum_sq", "sum_logp"):  # atomics: the order of the additions is free, the last bits with it (tests/test_gpu_moments.py)
        assert np.allclose(m_on[k], m_off[k], rtol=1e-12, atol=1e-9), k
    assert on.acc.np()[1].tolist() == [Cn * (12 - k) for k in range(5)]  # step counters 6, 9, ..., 39
    # the accumulator alone: the production kernel's run, bit for bit
    alone = Run(device, dim, T, Cn, burn=5, se=2, temps=2, every=3, max_lag=4).launches([N])
    bare = Run(device, dim, T, Cn, burn=5, se=2).launches([N])
    assert_rest_equal(alone.rest_np(), bare.rest_np(), "the accumulator alone", sq_jump_exact=False)


@gpu
def test_the_production_kernel_runs_between_the_snapshots(device):
    """A snapshot at every step ends every launch after one step.  The streaming form of the step kernel exists as a production
    kernel only (kernel.h STREAM): last_launch_kind() says it ran, its outputs equal the classic form's, and the sums are within
    the bound of the replay of a traced twin."""
    dim, T, Cn, N, burn, L = 30, 32, 74, 12, 3, 2
    assert E.has_stream_variant(diag_spec(dim).kind, E.PROPOSAL_NORMAL, dim)
    kw = dict(burn=burn, se=2, temps=1, every=1, max_lag=L)
    runs = {}
    with E.kernel_form(E.FORM_THREAD):
        for mode in (E.STREAM_ON, E.STREAM_OFF):
            with E.stream_mode(mode):
                runs[mode] = Run(device, dim, T, Cn, **kw).launches([N])
                assert E.last_launch_kind() == (E.LAUNCH_STREAM if mode == E.STREAM_ON else E.LAUNCH_THREAD)
        traced = Run(device, dim, T, Cn, **kw)
        trace = torch.zeros(N, Cn, 1, dim, device=device)
        traced.launches([N], trace=trace)
    on, off = runs[E.STREAM_ON], runs[E.STREAM_OFF]
    assert_rest_equal(on.rest_np(), off.rest_np(), "streaming and classic")
    want, want_pairs, bound = replay(trace.cpu().numpy()[due_rows(0, N, burn, 1)], L)
    assert want_pairs.tolist() == [Cn * 9, Cn * 8, Cn * 7]  # step counters 4 .. 12
    for r, what in ((on, "streaming"), (off, "classic")):
        got, pairs = r.acc.np()
        assert np.array_equal(pairs, want_pairs)
        assert_within(got, want, bound, what)
    assert on.rest_np()["n_accept"].sum() > 0 and on.rest_np()["swap_accept"].sum() > 0


# ---- 5. shards ----------------------------------------------------------------------------------------------------------
@gpu
def test_two_shards_add_up_to_the_unsharded_sums(device):
    dim, T, Cn, N, L = 3, 4, 11, 30, 3
    kw = dict(burn=4, se=2, temps=4, every=5, max_lag=L)
    x0 = np.random.default_rng(3).normal(0.0, 1.0, size=(Cn, T, dim))
    whole = Run(device, dim, T, Cn, x0=x0, **kw)
    trace = torch.zeros(N, Cn, 4, dim, device=device)
    whole.launches([N], trace=trace)
    want, want_pairs, bound = replay(trace.cpu().numpy()[due_rows(0, N, 4, 5)], L)
    a = Run(device, dim, T, 4, x0=x0[:4], chain_offset=0, **kw).launches([N])
    b = Run(device, dim, T, Cn - 4, x0=x0[4:], chain_offset=4, **kw).launches([N])
    (ga, pa), (gb, pb), (gw, pw) = a.acc.np(), b.acc.np(), whole.acc.np()
    assert np.array_equal(pa + pb, want_pairs) and np.array_equal(pw, want_pairs) and want_pairs[0] == 6 * Cn
    assert_within({k: ga[k] + gb[k] for k in ga}, want, bound, "two shards")
    assert_within(gw, want, bound, "unsharded")
    from algorithms.sharding import allreduce_autocorr

    out = allreduce_autocorr({**whole.acc.sums, "pairs": whole.acc.pairs, "every": 5})  # no process group: this shard
    assert all(torch.equal(out[k], whole.acc.sums[k]) for k in whole.acc.sums) and torch.equal(out["pairs"], whole.acc.pairs)


# ---- 6. split steps -----------------------------------------------------------------------------------------------------
def _wrapped(device, dim):
    """The library's own density behind a user-defined class without engine_target(): split steps."""
    from interfaces import TorchTargetDistribution

    tgt = diag_spec(dim).engine(device)

    class Wrapped(TorchTargetDistribution):
        def __init__(self):
            super().__init__(dim, device)

        def get_name(self):
            return "Wrapped"

        def density(self, x):
            return torch.exp(self.log_density(x))

        def log_density(self, x):
            return E.logdensity(tgt, x.contiguous())

        def to(self, dev):
            return self

    return Wrapped()


@gpu
def test_split_steps_eager_and_captured_are_within_the_bound_of_the_replay(device):
    """A user-defined density: the eager loop against the replay of its own trace, the captured graph (device-step mode: the
    snapshot number is read off the device's step counter) against the same replay - the same Philox words, so the same states."""
    from algorithms._engine_core import EngineRun

    dim, T, Cn, N, burn, every, L = 3, 4, 9, 70, 6, 4, 3
    betas = np.geomspace(1.0, 0.3, T).astype(np.float32)
    x0 = np.random.default_rng(9).normal(0.0, 1.0, size=(Cn, T, dim)).astype(np.float32)

    def make():
        with pytest.warns(UserWarning, match="split steps"):
            return EngineRun(target_dist=_wrapped(device, dim), proposal=H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim).engine(device),
                             beta_ladder=list(betas), dim=dim, device=device, n_replicas=Cn, initial_state=x0, burn_in=burn, swap_every=2,
                             swap_mode="exchange", swap_order="sequential", seed=SEED, acf_temps=T, acf_every=every, acf_max_lag=L)

    def sums(run):
        torch.cuda.synchronize()
        a = run.autocorr_sums()
        return {k: a[k].cpu().numpy() for k in ("sxy", "head", "tail")}, a["pairs"].cpu().numpy()

    eager = make()
    trace = torch.zeros(N, Cn, T, dim, device=device)
    eager.advance(N, trace=trace)
    want, want_pairs, bound = replay(trace.cpu().numpy()[due_rows(0, N, burn, every)], L)
    assert want_pairs.tolist() == [Cn * (16 - k) for k in range(L + 1)]  # step counters 8, 12, ..., 68
    got, pairs = sums(eager)
    assert np.array_equal(pairs, want_pairs)
    assert_within(got, want, bound, "eager")
    graph = make()
    graph.advance(N)  # no trace: GRAPH_STEPS-step blocks are captured and replayed
    torch.cuda.synchronize()
    assert graph._graph is not None
    assert torch.equal(graph.state, eager.state)
    got_g, pairs_g = sums(graph)
    assert np.array_equal(pairs_g, want_pairs)
    assert_within(got_g, want, bound, "captured")
    assert graph.autocorr_sums()["every"] == every
    graph.reset_autocorr()
    assert all(float(v.abs().sum().item()) == 0.0 for k, v in graph.autocorr_sums().items() if k != "every")
    # the ring stays valid: the next snapshot pairs with the ones before the reset
    graph.advance(every)
    torch.cuda.synchronize()
    assert graph.autocorr_sums()["pairs"].tolist() == [Cn] * (L + 1)


# ---- 7. cross-check with an independent kernel --------------------------------------------------------------------------
@gpu
def test_lag_zero_agrees_with_the_pooled_moments(device):
    """moments and the accumulator at the same period see the same snapshots through different kernels: sxy[:, 0] is sum_sq and
    head[:, 0] is sum, each side within the summation bound of the exact sum, so within twice the bound of each other."""
    dim, T, Cn, N, burn, every, L = 30, 4, 70, 40, 5, 3, 2
    r = Run(device, dim, T, Cn, burn=burn, se=2, temps=1, every=every, max_lag=L)
    mom = {"sum": torch.zeros(1, dim, dtype=torch.float64, device=device), "sum_sq": torch.zeros(1, dim, dtype=torch.float64, device=device),
           "count": torch.zeros(1, dtype=torch.int64, device=device)}
    r.plan.set_moments(mom["sum"], mom["sum_sq"], count=mom["count"], every=every)
    trace = torch.zeros(N, Cn, 1, dim, device=device)
    r.launches([N], trace=trace)
    got, pairs = r.acc.np()
    rows = trace.cpu().numpy()[due_rows(0, N, burn, every)].astype(np.float64)
    n = rows.shape[0] * Cn
    assert pairs[0] == n == int(mom["count"].item())
    b_sq = (n - 1) * U * (rows * rows).sum((0, 1))
    b_s = (n - 1) * U * np.abs(rows).sum((0, 1))
    err_sq = np.abs(got["sxy"][:, 0] - mom["sum_sq"].cpu().numpy())
    err_s = np.abs(got["head"][:, 0] - mom["sum"].cpu().numpy())
    print(f"sxy_0 vs sum_sq: max error {err_sq.max():.3e}, bound {2 * b_sq.min():.3e}; head_0 vs sum: {err_s.max():.3e}, bound {2 * b_s.min():.3e}")
    assert (err_sq <= 2 * b_sq).all() and (err_s <= 2 * b_s).all()
    assert np.array_equal(got["head"][:, 0], got["tail"][:, 0])  # at lag 0 they are the same tile sums


@gpu
def test_class_lag_zero_is_the_posterior_variance(device):
    """autocovariance()[0] and posterior_variance() are the same expression, q / n - (s / n)^2, of sums that agree within
    2 B_q and 2 B_s (B = (n - 1) 2^-53 sum|term|; sum|x| <= sqrt(n q) by Cauchy-Schwarz): they differ by at most
    (2 B_q + 2 |mean| 2 B_s) / n, plus the rounding of the four operations of the expression itself, 4 2^-53 (q / n + mean^2)."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    dim, M = 4, 300
    alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, MultivariateNormalTorch(dim, device=device), burn_in=20, device=device,
                                     num_chains=M, seed=3, moments="cold", moments_every=5, acf="cold", acf_every=5, acf_max_lag=4)
    alg.generate_samples(100)
    c0 = alg.autocovariance()[0].numpy()
    var = alg.posterior_variance().cpu().numpy()
    a = alg._run.autocorr_sums()
    n = int(a["pairs"][0].item())
    assert n == M * 20
    q, mean = a["sxy"][0, 0].cpu().numpy(), (a["head"][0, 0] / n).cpu().numpy()
    tol = (2 * (n - 1) * U * q + 2 * np.abs(mean) * 2 * (n - 1) * U * np.sqrt(n * q)) / n + 4 * U * (q / n + mean * mean)
    print(f"c_0 {c0}, posterior variance {var}, difference {np.abs(c0 - var)}, tolerance {tol}")
    assert (np.abs(c0 - var) <= tol).all() and (c0 > 0.3).all()


# ---- 8. classes ---------------------------------------------------------------------------------------------------------
@gpu
def test_class_autocorrelation_equals_the_one_of_the_class_trace(device):
    """autocorrelation() of a class run against the same estimator in NumPy over the run's own full trace.  Both sides sum the
    same float64 terms, in different orders: every sum is within n 2^-53 (n <= 100) of sum|term|, and c_k = sxy / n - mean^2
    loses at most a factor (var + mean^2) / var to cancellation - a chain that stays in one mode of the rough carpet, mean 15 and
    variance of order one, gives ~200 - so rho agrees to ~1e-11; 1e-9 is asked for, far below what one wrong pair would move."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    dim, N, burn, every, L = 4, 300, 20, 3, 8
    kw = dict(swap_every=2, burn_in=burn, device=device, num_replicas=1, seed=11, trace="all", pre_allocate_steps=N)

    def pt(**more):
        return ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0]),
                                                  beta_ladder=[1.0, 0.3, 0.05, 0.01], **kw, **more)

    alg = pt(acf="all", acf_every=every, acf_max_lag=L)
    alg.generate_samples(N)
    rows = alg._trace[:alg._rows_used].cpu().numpy().astype(np.float64)  # row i: the state after step i (row 0: the start)
    snap = rows[[sc for sc in range(1, burn + N + 1) if sc > burn and sc % every == 0]]
    S = snap.shape[0]
    assert S == 100
    kept = {}
    for t in (0, 3):
        x = snap[:, 0, t, :]
        c = np.stack([(x[k:] * x[:S - k]).sum(0) / (S - k) - (x[k:].sum(0) / (S - k)) * (x[:S - k].sum(0) / (S - k)) for k in range(L + 1)])
        got_c, got_rho = alg.autocovariance(t).numpy(), alg.autocorrelation(t).numpy()
        assert got_c.shape == (L + 1, dim) and got_c.dtype == np.float64
        assert np.allclose(got_rho, c / c[0], rtol=0.0, atol=1e-9), np.abs(got_rho - c / c[0]).max()
        assert np.allclose(got_c, c, rtol=0.0, atol=1e-9 * np.abs(c[0]).max())
        assert (got_rho[0] == 1.0).all() and (np.abs(got_rho) <= 1.5).all()
        kept[t] = got_rho
    info = alg.get_diagnostic_info()
    assert set(info) - set(pt().get_diagnostic_info()) == {"act_max", "act_window_reached"}
    tau, window, reached = alg.integrated_autocorr_time()
    assert info["act_max"] == float(tau.max()) and info["act_window_reached"] == bool(reached.all())
    ess = alg.ess_autocorr()
    assert np.allclose(ess.numpy(), S / tau.numpy())
    # without acf nothing changes: the same run
    off = pt()
    off.generate_samples(N)
    assert torch.equal(off._run.state, alg._run.state) and torch.equal(off._run.logp, alg._run.logp)
    assert torch.equal(off._run.n_accept, alg._run.n_accept) and torch.equal(off._trace, alg._trace)
    with pytest.raises(RuntimeError, match="acf="):
        off.autocorrelation()
    # reset(): the sums read zero, the next run sums from zero
    alg.reset()
    assert torch.isnan(alg.autocorrelation()).all()
    alg.generate_samples(N)
    assert np.allclose(alg.autocorrelation(0).numpy(), kept[0], rtol=0.0, atol=1e-9)


@gpu
def test_window_reached_on_a_gaussian_and_not_on_a_short_run(device):
    """A diagonal Gaussian in dim 4, 4 096 chains at the textbook scale: the autocorrelation time is a few tens of steps, so with a
    snapshot every 10 steps and 32 lags Sokal's window is reached in every coordinate; with a snapshot at every step and a run
    of 20 steps there is no window of five autocorrelation times, and the class says so."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    dim, M = 4, 4096

    def rwm(**more):
        return RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, MultivariateNormalTorch(dim, device=device), burn_in=500, device=device,
                                          num_chains=M, seed=2024, acf="cold", **more)

    alg = rwm(acf_every=10, acf_max_lag=32)
    alg.generate_samples(1000)
    tau, window, reached = alg.integrated_autocorr_time()
    print(f"every 10: tau {tau.tolist()} snapshots, window {window.tolist()}, reached {reached.tolist()}, ESS {alg.ess_autocorr().tolist()}")
    assert reached.all() and (window < 32).all() and (tau >= 1.0).all() and (tau < 6.0).all()
    assert alg.get_diagnostic_info()["act_window_reached"] is True
    assert (alg.ess_autocorr() <= M * 100).all() and (alg.ess_autocorr() > M * 100 / 6.0).all()
    short = rwm(acf_every=1, acf_max_lag=32)
    short.generate_samples(20)
    tau1, window1, reached1 = short.integrated_autocorr_time()
    print(f"every 1, 20 steps: tau >= {tau1.tolist()}, window {window1.tolist()}, reached {reached1.tolist()}")
    assert not reached1.any() and (window1 == 19).all() and (tau1 > 5.0).all()  # 20 snapshots: lags 1..19 are there
    assert short.get_diagnostic_info()["act_window_reached"] is False
    assert torch.isnan(short.autocorrelation()[20:]).all() and torch.isfinite(short.autocorrelation()[:20]).all()
