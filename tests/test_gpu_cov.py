"""Pooled posterior covariance (include/ptrwm.h ptrwm_cov_args, csrc/cov.h) on the GPU.  Every run goes through the C ABI.

Two yardsticks, both independent of the code under test:
  * hand-made states of small integers, where every product and every partial sum is exact in fp64 whatever the order of the
    additions and whichever unit forms them: the sums must EQUAL the NumPy replay;
  * a run with a full trace of the covered temperatures: the trace's terms x_i x_j, one float64 product each, summed with
    math.fsum, which is correctly rounded, so only the GPU's order of additions (and, for double states, the fusing of a product
    into the running sum) is in play.  Per element the bound is n 2^-53 sum|term|, n the number of its terms: the any-order
    summation bound (n - 1) with one unit more for a fused product.  `count` is equal.
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
SENTINEL = -12345.5


def diag_spec(dim):
    return H.TargetSpec(kind=E.TARGET_DIAG_GAUSSIAN, dim=dim, p=(-0.5 * dim * math.log(2 * math.pi),), ip=(1,),
                        vec0=np.ones(dim, np.float32))


def due_rows(step0, n_steps, burn, every):
    """Indices, within a trace of every step of the request, of the steps whose step counter is due."""
    return [i for i in range(n_steps) if step0 + i + 1 > burn and (step0 + i + 1) % every == 0]


def replay(rows, exact=False):
    """The sums of snapshot rows [snapshots, chains, temps, dim] and their bounds.  Every term in float64 (both values converted
    to double, one product); `exact`: plain NumPy sums (integer-valued states: every partial sum is exact), else math.fsum.
    Returns (sxx [temps, dim, dim] - the lower triangle, zeros above it -, sx [temps, dim], count, bound_xx, bound_x)."""
    rows = np.asarray(rows).astype(np.float64)  # (float -> double is exact; a double state stays what it is)
    S, Cn, Tc, D = rows.shape
    n = S * Cn
    flat = rows.reshape(n, Tc, D)
    sxx, bxx = np.zeros((Tc, D, D)), np.zeros((Tc, D, D))
    sx, bx = np.zeros((Tc, D)), np.zeros((Tc, D))
    for t in range(Tc):
        x = flat[:, t, :]
        if exact:
            sxx[t] = np.tril(x.T @ x)
            sx[t] = x.sum(0)
        else:
            for i in range(D):
                sx[t, i] = math.fsum(x[:, i])
                for j in range(i + 1):
                    sxx[t, i, j] = math.fsum(x[:, i] * x[:, j])
        bxx[t] = np.tril(n * U * (np.abs(x).T @ np.abs(x)))
        bx[t] = n * U * np.abs(x).sum(0)
    return sxx, sx, n, bxx, bx


def assert_within(got, want, bound, what, factor=1.0):
    err = np.abs(got - want)
    worst = np.unravel_index(np.argmax(err - factor * bound), err.shape)
    print(f"{what}: max error {err.max():.3e}, at its worst element error {err[worst]:.3e} against a bound of {factor * bound[worst]:.3e}")
    assert (err <= factor * bound).all(), (what, worst, err[worst], bound[worst])


class Acc:
    """The accumulator's arrays on the device, bound to a plan; the strict upper triangle of sxx holds a sentinel."""

    def __init__(self, plan, device, temps, dim, every):
        self.temps, self.dim = temps, dim
        self.upper = np.triu(np.ones((dim, dim), bool), 1)
        sxx = np.zeros((temps, dim, dim))
        sxx[:, self.upper] = SENTINEL
        self.sxx = torch.tensor(sxx, device=device)
        self.sx = torch.zeros(temps, dim, dtype=torch.float64, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        plan.set_covariance(self.sxx, self.sx, self.count, every=every)

    def np(self):
        """(sxx with the upper triangle zeroed - after checking that nobody wrote there -, sx, count)"""
        torch.cuda.synchronize()
        sxx = self.sxx.cpu().numpy()
        assert (sxx[:, self.upper] == SENTINEL).all(), "the strict upper triangle was written"
        sxx[:, self.upper] = 0.0
        return sxx, self.sx.cpu().numpy(), int(self.count.item())


# ---- 1. equality on hand-made states -----------------------------------------------------------------------------------
# tests/test_cov_host.py holds every row against cov_geometry itself, and fills in the chain count of the last one.
EQUALITY_CASES = [dict(name="one_block", dim=1, T=1, temps=1, Cn=300),        # one block, 15 pad columns
                  dict(name="below_k", dim=5, T=1, temps=1, Cn=3),            # fewer chains than one matrix instruction's K
                  dict(name="exact_block", dim=16, T=4, temps=2, Cn=70),      # temps < n_temps, chains no multiple of 4, a partial tile
                  dict(name="second_block", dim=17, T=4, temps=4, Cn=70),     # a second block with one live column
                  dict(name="headline_row", dim=30, T=32, temps=32, Cn=70),
                  dict(name="ten_pairs", dim=64, T=4, temps=4, Cn=70),
                  dict(name="pairs_over_waves", dim=70, T=8, temps=8, Cn=40),
                  dict(name="largest_dim", dim=104, T=2, temps=2, Cn=40),     # 28 pairs
                  dict(name="second_tile", dim=30, T=2, temps=2, Cn=291)]     # a second tile of chains, partial: 256 + 32 + 3


@gpu
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("case", EQUALITY_CASES, ids=[c["name"] for c in EQUALITY_CASES])
def test_standalone_snapshots_of_integer_states_equal_the_replay(device, case, f64):
    """ptrwm_covariance on a sequence of states of small integers (|x| <= 9: products below 2^7, sums far below 2^53): sxx on
    j <= i, sx and count EQUAL the NumPy replay; the strict upper triangle keeps its sentinel and the state is untouched.
    every = 2 and burn_in = 3: the calls behind the steps that are not due add nothing."""
    dim, T, temps, Cn = (case[k] for k in ("dim", "T", "temps", "Cn"))
    every, burn, S = 2, 3, 3
    dtype = torch.float64 if f64 else torch.float32
    rng = np.random.default_rng(7 * dim + Cn)
    n_steps = 2 + every * S  # step counters 1 .. n_steps: the due ones are 4, 6, 8
    states = rng.integers(-9, 10, size=(n_steps, Cn, T, dim)).astype(np.float64)
    st = torch.zeros(Cn, T, dim, device=device, dtype=dtype)
    plan = E.RunPlan(None, H.proposal_spec("Normal", dim, np.ones(T, np.float32), base_variance_scalar=1.0).engine(device), state=st,
                     logp=torch.zeros(Cn, T, device=device), beta=torch.ones(T, device=device), burn_in=burn)
    acc = Acc(plan, device, temps, dim, every)
    dev_states = torch.tensor(states, device=device, dtype=dtype)
    for s in range(n_steps):
        st.copy_(dev_states[s])
        plan.split_covariance(s)  # (the state after step s; the library skips the steps that are not due)
    sxx, sx, count = acc.np()
    rows = states[due_rows(0, n_steps, burn, every)][:, :, :temps]
    assert rows.shape[0] == S
    want_xx, want_x, n, _, _ = replay(rows, exact=True)
    assert count == n == S * Cn
    bad = np.argwhere(sxx != want_xx)
    assert bad.size == 0, f"sxx: {len(bad)} elements differ; the first (t, i, j): {bad[:5].tolist()}"
    bad = np.argwhere(sx != want_x)
    assert bad.size == 0, f"sx: {len(bad)} elements differ; the first (t, i): {bad[:5].tolist()}"
    assert (np.diagonal(want_xx, axis1=1, axis2=2) > 0).all()
    assert dim == 1 or np.abs(want_xx[:, 1:, 0]).sum() > 0  # (off-diagonal terms: an asymmetric check of the layout)
    assert torch.equal(st, dev_states[-1])  # a snapshot only reads the state


# ---- 2. replay of a full trace through real fused runs ------------------------------------------------------------------
class Run:
    """One sampler run through the C ABI with every output on the device."""

    def __init__(self, device, dim, T, Cn, *, burn, se, temps=0, every=1, f64=False, chain_offset=0, x0=None):
        self.dim, self.T, self.Cn, self.device, self.burn, self.every, self.temps = dim, T, Cn, device, burn, every, temps
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
        self.acc = Acc(self.plan, device, temps, dim, every) if temps else None

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
TRACE_RUNS = [("rwm_d3", 3, 1, 70, 1, 1, False),
              ("pt_d3_e7", 3, 4, 9, 2, 7, False),       # temps < n_temps
              ("pt_d30", 30, 4, 5, 4, 7, False),
              ("rwm_d30", 30, 1, 70, 1, 1, False),
              ("pt_d33", 33, 4, 5, 4, 1, False),        # odd dim, a third block
              ("rwm_d33_e7", 33, 1, 37, 1, 7, False),
              ("pt_d3_f64", 3, 4, 9, 4, 7, True)]       # double states


def test_every_shape_has_a_step_kernel():
    """No GPU needed: no case below can fail for want of a variant, or of the entry points."""
    assert {"ptrwm_covariance", "ptrwm_run_with_covariance"} <= set(E.SYMBOLS) and hasattr(E.RunPlan, "split_covariance")
    for _, dim, T, *_ in TRACE_RUNS:
        spec = diag_spec(dim)
        assert E.has_thread_variant(spec.kind, E.PROPOSAL_NORMAL, dim) or E.has_quad_variant(spec.kind, E.PROPOSAL_NORMAL, dim, T), dim
    assert E.has_quad_variant(diag_spec(3).kind, E.PROPOSAL_NORMAL, 3, 4)  # double states: the lane-split form
    assert {s[1] for s in TRACE_RUNS} == {3, 30, 33} and {s[2] for s in TRACE_RUNS} == {1, 4} and {s[5] for s in TRACE_RUNS} == {1, 7}


def trace_run_setup(every):
    """(N, burn, se): burn_in is no multiple of 7; swap events every 2 steps, inside the window."""
    return (24, 5, 2) if every == 1 else (75, 5, 2)


@gpu
@pytest.mark.parametrize("shape", TRACE_RUNS, ids=[s[0] for s in TRACE_RUNS])
def test_sums_are_within_the_summation_bound_of_the_trace_replay(device, shape):
    _, dim, T, Cn, temps, every, f64 = shape
    N, burn, se = trace_run_setup(every)
    kw = dict(burn=burn, se=se, temps=temps, every=every, f64=f64)
    traced = Run(device, dim, T, Cn, **kw)  # (a trace: the FULL twin of the step kernel between the snapshots)
    trace = torch.zeros(N, Cn, temps, dim, device=device, dtype=traced.st.dtype)
    traced.launches([N], trace=trace)
    sxx, sx, count = traced.acc.np()
    rows = trace.cpu().numpy()[due_rows(0, N, burn, every)]
    assert rows.shape[0] == (19 if every == 1 else 10)
    want_xx, want_x, n, bxx, bx = replay(rows)
    assert count == n
    assert_within(sxx, want_xx, bxx, "traced sxx")
    assert_within(sx, want_x, bx, "traced sx")
    if T > 1:
        assert traced.rest_np()["swap_accept"].sum() > 0  # swap events inside the window
    # the same run without a trace, cut into other launches: the production step kernel between the snapshots
    plain = Run(device, dim, T, Cn, **kw).launches([10, 1, N - 11])
    sxx_p, sx_p, count_p = plain.acc.np()
    assert count_p == n
    assert_within(sxx_p, want_xx, bxx, "production sxx")
    assert_within(sx_p, want_x, bx, "production sx")
    assert_within(sxx_p, sxx, bxx, "two cuts, sxx", factor=2.0)
    assert_within(sx_p, sx, bx, "two cuts, sx", factor=2.0)
    assert_rest_equal(plain.rest_np(), traced.rest_np(), "with and without a trace", sq_jump_exact=False)


# ---- 3. nothing else moves ----------------------------------------------------------------------------------------------
@gpu
def test_nothing_else_moves(device):
    """State, logp and every counter of a run with the accumulator equal the same run without, byte for byte; sq_jump too when
    the cuts coincide, and within the documented exception otherwise."""
    dim, T, Cn, N = 3, 4, 70, 40
    on = Run(device, dim, T, Cn, burn=5, se=2, temps=2, every=3).launches([N])
    off = Run(device, dim, T, Cn, burn=5, se=2).launches([N])
    assert_rest_equal(on.rest_np(), off.rest_np(), "the accumulator alone", sq_jump_exact=False)
    assert on.acc.np()[2] == Cn * 12  # step counters 6, 9, ..., 39
    # the same cuts made by the caller: bit-equal sq_jump too
    cuts = [5] + [3] * 11 + [2]
    assert_rest_equal(on.rest_np(), Run(device, dim, T, Cn, burn=5, se=2).launches(cuts).rest_np(), "the same cuts")
    # no due step: the sums stay zero and the run is cut as without the accumulator
    none = Run(device, dim, T, Cn, burn=5, se=2, temps=4, every=100).launches([N])
    sxx, sx, count = none.acc.np()
    assert count == 0 and not sxx.any() and not sx.any()
    assert_rest_equal(none.rest_np(), off.rest_np(), "no due step")


# ---- 4. agreement with the moments --------------------------------------------------------------------------------------
@gpu
def test_diagonal_agrees_with_the_pooled_moments(device):
    """moments and the covariance at the same period see the same snapshots through different kernels: the diagonal of sxx is
    sum_sq and sx is sum, each side within its any-order bound of the exact sum, so within the sum of the two of each other."""
    dim, T, Cn, N, burn, every = 30, 4, 70, 40, 5, 3
    r = Run(device, dim, T, Cn, burn=burn, se=2, temps=1, every=every)
    mom = {"sum": torch.zeros(1, dim, dtype=torch.float64, device=device), "sum_sq": torch.zeros(1, dim, dtype=torch.float64, device=device),
           "count": torch.zeros(1, dtype=torch.int64, device=device)}
    r.plan.set_moments(mom["sum"], mom["sum_sq"], count=mom["count"], every=every)
    trace = torch.zeros(N, Cn, 1, dim, device=device)
    r.launches([N], trace=trace)
    sxx, sx, count = r.acc.np()
    rows = trace.cpu().numpy()[due_rows(0, N, burn, every)].astype(np.float64)
    n = rows.shape[0] * Cn
    assert count == n == int(mom["count"].item())
    b_sq = (n * U + (n - 1) * U) * (rows * rows).sum((0, 1))
    b_s = (n * U + (n - 1) * U) * np.abs(rows).sum((0, 1))
    err_sq = np.abs(np.diagonal(sxx[0]) - mom["sum_sq"].cpu().numpy()[0])
    err_s = np.abs(sx[0] - mom["sum"].cpu().numpy()[0])
    print(f"diag sxx vs sum_sq: max error {err_sq.max():.3e}, bound {b_sq.min():.3e}; sx vs sum: {err_s.max():.3e}, bound {b_s.min():.3e}")
    assert (err_sq <= b_sq).all() and (err_s <= b_s).all()


# ---- 5. split steps -----------------------------------------------------------------------------------------------------
def dense_sigma():
    """A 4 x 4 covariance with correlations of both signs and a condition number near 50: eigenvalues 5, 2, 0.5, 0.1 on a fixed
    orthogonal basis."""
    a = np.array([[1.0, 2.0, -1.0, 0.5], [0.3, -1.0, 2.0, 1.0], [2.0, 0.5, 1.0, -1.5], [-1.0, 1.5, 0.5, 2.0]])
    q, _ = np.linalg.qr(a)
    return (q * np.array([5.0, 2.0, 0.5, 0.1])) @ q.T


def dense_target(device):
    from target_distributions import MultivariateNormalTorch

    return MultivariateNormalTorch(4, mean=torch.zeros(4), cov=torch.tensor(dense_sigma(), dtype=torch.float32), device=device)


def test_the_dense_sigma_is_what_the_tests_say():
    """No GPU needed: correlations of both signs and a condition number of 50, by the library's own estimators."""
    from algorithms._engine_core import cov_condition, cov_correlation, cov_principal_axes

    s = dense_sigma()
    w, v = cov_principal_axes(s)
    assert np.allclose(w.numpy(), [5.0, 2.0, 0.5, 0.1]) and abs(cov_condition(s) - 50.0) < 1e-9
    assert np.allclose((v.numpy() * w.numpy()) @ v.numpy().T, s)
    off = cov_correlation(s).numpy()[np.tril_indices(4, -1)]
    assert (off > 0.05).any() and (off < -0.05).any()


def _wrapped(device, dim):
    """The library's own density behind a user-defined class without engine_target(): split steps, and a density whose values
    do not depend on whether it runs eagerly or inside a captured graph."""
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
def test_split_steps_eager_and_captured_share_one_trace(device):
    """A user-defined density: the eager loop against the replay of its own trace, and ONE advance(N) by graph replay against the
    same replay - the same Philox words and a density that does not care how it is launched, so the same states (torch.equal).
    Swap events every 2 steps, so a captured block covers 16 steps and the graph replays step counters 3..18, 19..34, 35..50 and
    51..66: the due step counters 8, 12, ..., 64 lie INSIDE replayed blocks, where the captured ptrwm_covariance reads the step
    off the device (device-step mode) and takes its due path; 68 comes behind the last block, step by step."""
    from algorithms._engine_core import EngineRun

    dim, T, Cn, N, burn, every = 3, 4, 9, 70, 6, 4
    betas = np.geomspace(1.0, 0.3, T).astype(np.float32)
    x0 = np.random.default_rng(9).normal(0.0, 1.0, size=(Cn, T, dim)).astype(np.float32)

    def make():
        with pytest.warns(UserWarning, match="split steps"):
            return EngineRun(target_dist=_wrapped(device, dim), proposal=H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim).engine(device),
                             beta_ladder=list(betas), dim=dim, device=device, n_replicas=Cn, initial_state=x0, burn_in=burn, swap_every=2,
                             swap_mode="exchange", swap_order="sequential", seed=SEED, cov_temps=T, cov_every=every)

    def sums(run):
        torch.cuda.synchronize()
        a = run.covariance_sums()
        return np.tril(a["sxx"].cpu().numpy()), a["sx"].cpu().numpy(), int(a["count"].item())

    eager = make()
    trace = torch.zeros(N, Cn, T, dim, device=device)
    eager.advance(N, trace=trace)
    want_xx, want_x, n, bxx, bx = replay(trace.cpu().numpy()[due_rows(0, N, burn, every)])
    assert n == Cn * 16  # step counters 8, 12, ..., 68
    graph = make()
    graph.advance(N)  # no trace: blocks of steps are captured and replayed
    torch.cuda.synchronize()
    assert graph._graph is not None and eager._graph is None
    assert graph._graph_block() == 16  # (what the docstring's step counters rest on)
    assert torch.equal(graph.state, eager.state)
    for run, what in ((eager, "eager"), (graph, "captured")):
        sxx, sx, count = sums(run)
        assert count == n
        assert_within(sxx, want_xx, bxx, f"{what} sxx")
        assert_within(sx, want_x, bx, f"{what} sx")
    (xa, sa, _), (xb, sb, _) = sums(eager), sums(graph)
    assert_within(xa, xb, bxx, "eager / captured sxx", factor=2.0)
    assert_within(sa, sb, bx, "eager / captured sx", factor=2.0)
    assert graph.covariance_sums()["every"] == every
    graph.reset_covariance()
    assert all(float(v.abs().sum().item()) == 0.0 for k, v in graph.covariance_sums().items() if k != "every")


@gpu
def test_split_steps_of_the_dense_gaussian_through_the_class(device):
    """A dense-covariance Gaussian through the PT class (no fused kernel: split steps), nine ladders, eager (a trace is kept) and
    captured (none).  burn_in = 32 and cov_every = 16: the first 32 steps capture the graph, and each later _advance(16) is ONE
    replayed block whose LAST step is due - the captured ptrwm_covariance takes its due path inside the block - after which the
    state is copied: a trace of the run's own due states.  Both runs give the same count, and each run's sums are within the
    bound of the replay of ITS OWN trace.
    The two are not held against one trace here (test_split_steps_eager_and_captured_share_one_trace does that with a density
    that does not care how it is launched): with this density, a torch GEMM per step, the eager and the captured run of the class
    differ in the last bits of the state with cov= off as well - measured on an MI355X, 9 ladders x 70 steps, states up to 4.8e-7
    apart - so their sums differ by far more than a summation bound, for a reason outside this feature."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized

    dim, burn, every, R, blocks = 4, 32, 16, 9, 4

    def make(**more):
        return ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, dense_target(device), beta_ladder=[1.0, 0.5, 0.2], swap_every=2, burn_in=burn,
                                                  device=device, num_replicas=R, seed=SEED, cov="all", cov_every=every, **more)

    import warnings

    def run(alg):
        """burn-in, then `blocks` times 16 steps; the states after the due steps [snapshots, R, T, dim]"""
        rows = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            alg._advance(burn)
            assert alg.covariance_count == 0
            for _ in range(blocks):
                alg._advance(every)
                rows.append(alg._run.state.clone())
        torch.cuda.synchronize()
        return torch.stack(rows).cpu().numpy()

    eager, graph = make(trace="all", pre_allocate_steps=burn + blocks * every), make(trace="none")
    snaps = {"eager": run(eager), "captured": run(graph)}
    assert graph._run._graph is not None and eager._run._graph is None and graph._run._graph_block() == every
    assert eager.covariance_count == graph.covariance_count == R * blocks  # step counters 48, 64, 80, 96
    for alg, what in ((eager, "eager"), (graph, "captured")):
        want_xx, want_x, n, bxx, bx = replay(snaps[what])
        a = alg._run.covariance_sums()
        assert int(a["count"].item()) == n
        assert_within(np.tril(a["sxx"].cpu().numpy()), want_xx, bxx, f"{what} sxx")
        assert_within(a["sx"].cpu().numpy(), want_x, bx, f"{what} sx")
    print(f"eager and captured states differ by at most {np.abs(snaps['eager'] - snaps['captured']).max():.3e}")
    c = graph.posterior_covariance(2)
    assert c.shape == (dim, dim) and c.dtype == torch.float64 and torch.equal(c, c.T)
    graph.reset()
    assert graph.covariance_count == 0


# ---- 6. combination and shards ------------------------------------------------------------------------------------------
@gpu
def test_all_features_together_equal_the_features_one_at_a_time(device):
    """One PT run with cov='all', acf='cold', hist='cold' and adapt_scale=True equals the same features run one at a time:
    integers equal, doubles within the any-order bounds (tile sums meet in another order from run to run)."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    dim, N, burn, R = 4, 60, 20, 70
    feats = {"cov": dict(cov="all", cov_every=3), "acf": dict(acf="cold", acf_every=2, acf_max_lag=4),
             "hist": dict(hist="cold", hist_range=(-20.0, 20.0), hist_bins=16, hist_every=5), "adapt": dict(adapt_scale=True, adapt_every=5)}

    def run(**more):
        alg = ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0]),
                                                 beta_ladder=[1.0, 0.3, 0.05], swap_every=2, burn_in=burn, device=device, num_replicas=R, seed=5, **more)
        alg.generate_samples(N)
        torch.cuda.synchronize()
        return alg

    both = run(**{k: v for f in feats.values() for k, v in f.items()})
    # the tuning changes the run itself: every single-feature run carries it too
    cov1, acf1, hist1 = (run(**feats[k], **feats["adapt"]) for k in ("cov", "acf", "hist"))
    for other in (cov1, acf1, hist1):
        assert torch.equal(both._run.state, other._run.state) and torch.equal(both._run.n_accept, other._run.n_accept)
        assert torch.equal(both._run.proposal.temp_scale, other._run.proposal.temp_scale)
    a, b = both._run.covariance_sums(), cov1._run.covariance_sums()
    assert int(a["count"].item()) == int(b["count"].item()) == R * 20 == both.covariance_count
    n = R * 20
    # (both sides are any-order sums of the same terms: |x_i x_j| summed is at most sqrt(sxx_ii sxx_jj))
    d = np.sqrt(np.diagonal(a["sxx"].cpu().numpy(), axis1=1, axis2=2))
    assert_within(np.tril(a["sxx"].cpu().numpy()), np.tril(b["sxx"].cpu().numpy()), 2 * n * U * d[:, :, None] * d[:, None, :], "sxx together / alone")
    assert_within(a["sx"].cpu().numpy(), b["sx"].cpu().numpy(), 2 * n * U * np.sqrt(n) * d, "sx together / alone")
    ha, hb = both._run._hist, hist1._run._hist
    assert torch.equal(ha["counts"], hb["counts"]) and torch.equal(ha["count"], hb["count"])
    fa, fb = both._run.autocorr_sums(), acf1._run.autocorr_sums()
    assert torch.equal(fa["pairs"], fb["pairs"])
    for k in ("sxy", "head", "tail"):
        assert np.allclose(fa[k].cpu().numpy(), fb[k].cpu().numpy(), rtol=1e-12, atol=1e-9), k
    info = both.get_diagnostic_info()
    assert info["cov_count"] == n and info["cov_condition"] > 1.0 and "act_max" in info


@gpu
def test_two_shards_add_up_to_the_unsharded_sums(device):
    dim, T, Cn, N = 3, 4, 11, 30
    kw = dict(burn=4, se=2, temps=4, every=5)
    x0 = np.random.default_rng(3).normal(0.0, 1.0, size=(Cn, T, dim))
    whole = Run(device, dim, T, Cn, x0=x0, **kw)
    trace = torch.zeros(N, Cn, 4, dim, device=device)
    whole.launches([N], trace=trace)
    want_xx, want_x, n, bxx, bx = replay(trace.cpu().numpy()[due_rows(0, N, 4, 5)])
    a = Run(device, dim, T, 4, x0=x0[:4], chain_offset=0, **kw).launches([N])
    b = Run(device, dim, T, Cn - 4, x0=x0[4:], chain_offset=4, **kw).launches([N])
    (xa, sa, na), (xb, sb, nb), (xw, sw, nw) = a.acc.np(), b.acc.np(), whole.acc.np()
    assert na + nb == n == nw == 6 * Cn
    assert_within(xa + xb, want_xx, bxx, "two shards sxx")
    assert_within(sa + sb, want_x, bx, "two shards sx")
    assert_within(xw, want_xx, bxx, "unsharded sxx")
    from algorithms.sharding import allreduce_covariance

    out = allreduce_covariance({"sxx": whole.acc.sxx, "sx": whole.acc.sx, "count": whole.acc.count, "every": 5})  # no process group: this shard
    assert torch.equal(out["sxx"], whole.acc.sxx) and torch.equal(out["sx"], whole.acc.sx) and torch.equal(out["count"], whole.acc.count)
    assert out["covariance"].shape == (4, dim, dim)


# ---- 7. it estimates what it should -------------------------------------------------------------------------------------
@gpu
def test_the_dense_gaussian_gives_back_its_covariance(device):
    """8 192 chains start from exact draws of a dense Gaussian in dim 4 (correlations of both signs, condition number 50) and
    take 200 steps, a snapshot every 20.  Every entry of posterior_covariance() lies within 5 standard errors of Sigma, the
    standard error of a Gaussian sample covariance counting ONE independent draw per chain, sqrt((S_ii S_jj + S_ij^2) / 8192) -
    conservative, since later snapshots only add information; the leading eigenvector within that error of Sigma's; the condition
    number within a factor of two of 50."""
    from algorithms import RandomWalkMH_GPU_Optimized

    dim, M = 4, 8192
    sigma = dense_sigma()
    tgt = dense_target(device)
    torch.manual_seed(4)
    x0 = tgt.draw_samples_torch(M).reshape(M, dim)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, tgt, burn_in=0, device=device, num_chains=M, seed=8, initial_states=x0,
                                         cov="cold", cov_every=20)
        alg.generate_samples(200)
    assert alg.covariance_count == M * 10
    c = alg.posterior_covariance().numpy()
    se = np.sqrt((np.outer(np.diag(sigma), np.diag(sigma)) + sigma ** 2) / M)
    print(f"covariance error / standard error:\n{np.abs(c - sigma) / se}")
    assert (np.abs(c - sigma) <= 5 * se).all()
    r = alg.posterior_correlation().numpy()
    assert np.allclose(np.diag(r), 1.0) and (np.sign(r) == np.sign(sigma)).all()
    w, v = alg.principal_axes()
    w0, v0 = np.linalg.eigh(sigma)
    lead, lead0 = v[:, 0].numpy(), v0[:, -1]
    lead = lead * np.sign(lead @ lead0)
    # (first-order perturbation: the leading eigenvector moves by at most |dS| / gap, gap = 5 - 2; 5 |se|_F / 3 is asked for)
    assert (w.numpy()[:-1] >= w.numpy()[1:]).all()
    assert np.linalg.norm(lead - lead0) <= 5 * np.linalg.norm(se) / 3.0
    cond = alg.get_diagnostic_info()["cov_condition"]
    print(f"eigenvalues {w.tolist()}, condition {cond}")
    assert 25.0 <= cond <= 100.0
