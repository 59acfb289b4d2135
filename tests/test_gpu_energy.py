"""Pooled log-density sums along the ladder (include/ptrwm.h ptrwm_energy_args, csrc/energy.h) on the GPU.  Every run goes through
the C ABI.  The yardstick is tests/energy_reference.py: NumPy float64, math.exp per term, math.fsum per element.

Bounds (energy_reference.sum_tolerance), per element with its n terms, in units of 2^-53 times the sum of |term|:
  * count and nonfinite: EQUAL;
  * s1, s2: EQUAL where logp holds small integers, else n (any-order summation; the square of a converted float is exact);
  * colder, hotter: n + 4 - any-order summation, n - 1, plus one ulp for each of the two exp.  glibc's exp is below 1 ulp; the
    device's double exp is 1 ulp by the table "double precision mathematical functions" of ROCm's HIP documentation (HIP math
    API: exp(double x), maximum ULP difference 1).
"""
import math

import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E
from energy_reference import assert_sums_match, due_steps, energy_reference, ref_of, sum_tolerance

gpu = pytest.mark.gpu

SEED = 20261021
SENTINEL = -12345.5
SUMS = ("s1", "s2", "colder", "hotter")


class Acc:
    """The accumulator's arrays on the device, bound to a plan; colder[:, 0] and hotter[:, T - 1] hold a sentinel."""

    def __init__(self, plan, device, T, groups, every, ref=None):
        self.T = T
        self.count = torch.zeros(groups, T, dtype=torch.int64, device=device)
        self.nonfinite = torch.zeros(1, dtype=torch.int64, device=device)
        self.s1, self.s2, self.colder, self.hotter = (torch.zeros(groups, T, dtype=torch.float64, device=device) for _ in range(4))
        self.colder[:, 0] = SENTINEL
        self.hotter[:, T - 1] = SENTINEL
        self.ref = torch.zeros(T, dtype=torch.float64, device=device) if ref is None else torch.tensor(np.asarray(ref, np.float64), device=device)
        self.ref_set = torch.full((1,), 0 if ref is None else 1, dtype=torch.int32, device=device)
        plan.set_energy(self.count, self.s1, self.s2, self.colder, self.hotter, ref=self.ref, ref_set=self.ref_set,
                        nonfinite=self.nonfinite, every=every)

    def np(self):
        """The sums as NumPy arrays, the never-written columns zeroed after checking that nobody wrote there."""
        torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy() for k in ("count", "nonfinite", "ref", "ref_set") + SUMS}
        assert (out["colder"][:, 0] == SENTINEL).all() and (out["hotter"][:, self.T - 1] == SENTINEL).all(), "an unused column was written"
        out["colder"][:, 0] = 0.0
        if self.T > 1:
            out["hotter"][:, self.T - 1] = 0.0
        else:
            out["hotter"][:, 0] = 0.0
        return out


def ladder(T):
    """beta_t = 0.5^t; the longest ladder takes 0.01^(t / 255): 0.5^255 is no float32."""
    if T == 256:
        return (0.01 ** (np.arange(T) / 255.0)).astype(np.float32)
    return (0.5 ** np.arange(T)).astype(np.float32)


# ---- 1. stand-alone snapshots on hand-made logp ---------------------------------------------------------------------------
# tests/test_energy_host.py holds every row against energy_geometry itself.  The last row's chain count is raised until a group
# has two tiles of chains with a partial last one (a tile: 4096 / T = 1024 chains of ONE group, so 16 groups need > 16 384).
STANDALONE_CASES = [dict(name="no_neighbours", T=1, Cn=300, groups=16, offset=0),
                    dict(name="fewer_chains_than_groups", T=2, Cn=3, groups=16, offset=0),
                    dict(name="odd_ladder_offset", T=3, Cn=70, groups=16, offset=5),
                    dict(name="headline_row", T=32, Cn=70, groups=16, offset=0),
                    dict(name="row_longer_than_a_wave", T=65, Cn=40, groups=3, offset=1),
                    dict(name="longest_ladder", T=256, Cn=19, groups=64, offset=7),
                    dict(name="one_chain_one_group", T=8, Cn=1, groups=1, offset=0),
                    dict(name="second_tile", T=4, Cn=20000, groups=16, offset=0)]


@gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["auto_ref", "pinned_ref_integers"])
@pytest.mark.parametrize("case", STANDALONE_CASES, ids=[c["name"] for c in STANDALONE_CASES])
def test_standalone_snapshots_of_hand_made_logp_match_the_reference(device, case, pinned):
    """ptrwm_energy behind steps 0..7 with every = 2 and burn_in = 3: the due step counters are 4, 6 and 8, the other calls add
    nothing.  Automatic ref: floats in [-16, 16], so every |argument| <= 32 under a ref that is their maximum; after the first due
    call ref equals NumPy's per-temperature maximum bit for bit and the flag is 1, and later calls do not move it.  Pinned ref:
    small integers (s1 and s2 must be EQUAL) against a level that is never written.  The odd ladder carries -inf, +inf and NaN:
    they appear in nonfinite and nowhere else.  logp and beta are untouched."""
    T, Cn, G, offset = (case[k] for k in ("T", "Cn", "groups", "offset"))
    every, burn, n_steps = 2, 3, 8
    rng = np.random.default_rng(1000 * T + Cn + (1 if pinned else 0))
    if pinned:
        values = rng.integers(-16, 17, size=(n_steps, Cn, T)).astype(np.float32)
        pin = np.round(rng.uniform(-4.0, 4.0, size=T) * 4) / 4
    else:
        values = rng.uniform(-16.0, 16.0, size=(n_steps, Cn, T)).astype(np.float32)
        pin = None
    if case["name"] == "odd_ladder_offset":
        for s, c, t, v in ((3, 0, 0, -np.inf), (3, 17, 1, np.inf), (5, 33, 2, np.nan), (7, 69, 0, -np.inf), (4, 5, 1, np.nan), (3, 21, 2, np.inf)):
            values[s, c, t] = v
    betas = ladder(T)
    assert (np.diff(betas) < 0).all() if T > 1 else True
    st = torch.zeros(Cn, T, 1, device=device)
    lp = torch.zeros(Cn, T, device=device)
    beta = torch.tensor(betas, device=device)
    plan = E.RunPlan(None, H.proposal_spec("Normal", 1, np.ones(T, np.float32), base_variance_scalar=1.0).engine(device), state=st, logp=lp,
                     beta=beta, burn_in=burn, chain_offset=offset)
    acc = Acc(plan, device, T, G, every, ref=pin)
    dev = torch.tensor(values, device=device)
    refs = []
    for s in range(n_steps):
        lp.copy_(dev[s])
        plan.split_energy(s)  # (logp after step s; the library skips the steps that are not due)
        refs.append((acc.ref.clone(), acc.ref_set.clone()))
    got = acc.np()
    due = due_steps(range(1, n_steps + 1), burn, every)
    assert due == [4, 6, 8]
    snaps = [values[sc - 1] for sc in due]
    if pinned:
        ref = pin
        assert all(np.array_equal(r.cpu().numpy(), pin) and int(f.item()) == 1 for r, f in refs)  # never written
    else:
        ref = ref_of(snaps[0])
        assert all(int(f.item()) == 0 and float(r.abs().sum().item()) == 0.0 for r, f in refs[:3])  # calls that are not due
        assert all(np.array_equal(r.cpu().numpy(), ref) and int(f.item()) == 1 for r, f in refs[3:])  # set once, bit for bit
        # (|l| <= 16 under a ref that is a maximum of such values, and |beta differences| <= 1: every |argument| <= 32)
        assert np.abs(values[np.isfinite(values)]).max() <= 16.0 and betas.max() <= 1.0 and betas.min() > 0.0
    want = energy_reference(snaps, betas, G, offset, ref)
    assert want["count"].sum() + want["nonfinite"] == 3 * Cn * T
    assert want["nonfinite"] == (5 if case["name"] == "odd_ladder_offset" else 0)  # (one of the six sits behind a step that is not due)
    assert_sums_match(got, want, case["name"], integers=pinned)
    assert torch.equal(lp, dev[-1]) and np.array_equal(beta.cpu().numpy(), betas)  # a snapshot only reads
    if T > 1:
        assert np.isfinite(got["colder"]).all() and (got["colder"][:, 1:][want["count"][:, 1:] > 0] > 0).all()


# ---- 2. fused runs replayed from a trace_logp of every step ------------------------------------------------------------------
def carpet(device, dim=5):
    from target_distributions import RoughCarpetDistributionTorch

    return RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0])


class Run:
    """One sampler run through the C ABI (RoughCarpet dim 5, Normal proposals) with every output on the device; the covariance
    every 4 and the histogram every 5 ride along where asked for."""

    def __init__(self, device, T, Cn, *, burn, se, every=0, groups=16, others=True, f64=False, chain_offset=0, x0=None, ref=None, dim=5):
        self.T, self.Cn, self.dim, self.device, self.burn, self.every, self.groups = T, Cn, dim, device, burn, every, groups
        self.betas = np.geomspace(1.0, 0.05, T).astype(np.float32) if T > 1 else np.ones(1, np.float32)
        self.tgt = carpet(device, dim).engine_target()
        prop = H.proposal_spec("Normal", dim, self.betas, base_variance_scalar=2.38 ** 2 / dim).engine(device)
        if x0 is None:
            x0 = np.random.default_rng(1000 * T + Cn).normal(0.0, 1.0, size=(Cn, T, dim))
        self.st = torch.tensor(x0, device=device, dtype=torch.float64 if f64 else torch.float32)
        self.lp = E.logdensity(self.tgt, self.st.view(-1, dim).float().contiguous()).view(Cn, T).contiguous()
        self.stats = {k: torch.zeros(Cn, T, dtype=(torch.float64 if k == "sq_jump" else torch.int64), device=device)
                      for k in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")}
        self.plan = E.RunPlan(self.tgt, prop, state=self.st, logp=self.lp, beta=torch.tensor(self.betas, device=device), burn_in=burn,
                              swap_every=se, seed=SEED, chain_offset=chain_offset, **self.stats)
        if others:
            self.cov = (torch.zeros(T, dim, dim, dtype=torch.float64, device=device), torch.zeros(T, dim, dtype=torch.float64, device=device),
                        torch.zeros(1, dtype=torch.int64, device=device))
            self.plan.set_covariance(*self.cov, every=4)
            self.hist = torch.zeros(T, dim, 10, dtype=torch.int64, device=device)
            self.plan.set_histogram(self.hist, torch.full((dim,), -20.0, device=device), torch.full((dim,), 8 / 40.0, device=device), n_bins=8,
                                    temps=T, every=5)
        self.acc = Acc(self.plan, device, T, groups, every, ref=ref) if every else None

    def launches(self, cuts, step0=0, trace=None, trace_logp=None):
        row = 0
        for n in cuts:
            if trace is None:
                self.plan.launch(step0, n)
            else:
                self.plan.launch(step0, n, trace=trace, trace_logp=trace_logp, trace_row0=row)
                row += n
            step0 += n
        return self

    def rest_np(self):
        torch.cuda.synchronize()
        return {"state": self.st.cpu().numpy(), "logp": self.lp.cpu().numpy(), **{k: v.cpu().numpy() for k, v in self.stats.items()}}


def traced_snapshots(device, T, Cn, N, **kw):
    """(run, the logp of every due step [snapshots, Cn, T]) of a run that traces every step."""
    run = Run(device, T, Cn, **kw)
    trace = torch.zeros(N, Cn, T, run.dim, device=device, dtype=run.st.dtype)
    trace_logp = torch.zeros(N, Cn, T, device=device)
    run.launches([N], trace=trace, trace_logp=trace_logp)
    torch.cuda.synchronize()
    due = due_steps(range(1, N + 1), kw["burn"], kw["every"])
    return run, trace_logp.cpu().numpy()[[sc - 1 for sc in due]]


#              id        T  chains burn swap_every steps
FUSED_RUNS = [("pt_t8", 8, 64, 11, 5, 60),
              ("pt_t3", 3, 200, 11, 5, 60),
              ("rwm", 1, 300, 11, 5, 60)]


def test_every_fused_shape_has_its_step_kernels():
    """No GPU needed: no case below can fail for want of a variant, or of the entry points."""
    assert {"ptrwm_energy", "ptrwm_run_with_energy"} <= set(E.SYMBOLS) and hasattr(E.RunPlan, "split_energy")
    kind = E.TARGET_ROUGH_CARPET
    for _, T, *_ in FUSED_RUNS:
        assert E.has_thread_variant(kind, E.PROPOSAL_NORMAL, 5) and E.has_quad_variant(kind, E.PROPOSAL_NORMAL, 5, T), T
    assert E.has_stream_variant(kind, E.PROPOSAL_NORMAL, 5)


def assert_rest_equal(a, b, what):
    """State, logp, n_accept and swap_accept bit for bit (sq_jump depends on where launches are cut: include/ptrwm.h)."""
    for k in ("state", "logp", "n_accept", "swap_accept", "last_swap_ordinal"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"


@gpu
@pytest.mark.parametrize("shape", FUSED_RUNS, ids=[s[0] for s in FUSED_RUNS])
def test_fused_runs_match_the_replay_of_their_trace(device, shape):
    """energy_every = 7 with the covariance every 4 and the histogram every 5, so launches are cut at all three periods.  The
    thread form, the lane-split form, one-step launches of the streaming form, the same steps in calls of 1, 13 and the rest,
    and double states each stay within the bounds of the replay; the automatic ref is the first due snapshot's maximum bit for
    bit; state, logp and the counters are bit-identical to the same run without the sums, its other blocks kept."""
    _, T, Cn, burn, se, N = shape
    kw = dict(burn=burn, se=se, every=7)
    traced, snaps = traced_snapshots(device, T, Cn, N, **kw)
    assert snaps.shape[0] == 7  # step counters 14 .. 56
    ref = ref_of(snaps[0])
    want = energy_reference(snaps, traced.betas, 16, 0, ref)
    got = traced.acc.np()
    assert np.array_equal(got["ref"], ref) and got["ref_set"].tolist() == [1]
    assert_sums_match(got, want, "traced")
    runs = {}
    with E.kernel_form(E.FORM_THREAD):
        runs["thread"] = Run(device, T, Cn, **kw).launches([N])
        assert E.last_launch_kind() == E.LAUNCH_THREAD
        with E.stream_mode(E.STREAM_ON):
            runs["streaming, one-step launches"] = Run(device, T, Cn, **kw).launches([1] * N)
            # (the streaming kernel itself takes whole waves of ladders: 64 ladders of 8 rungs are 8 waves; 200 of 3 and 300
            # chains are not, and run the classic form one step at a time)
            assert E.last_launch_kind() == (E.LAUNCH_STREAM if T == 8 else E.LAUNCH_THREAD)
    with E.kernel_form(E.FORM_QUAD):
        runs["lane-split"] = Run(device, T, Cn, **kw).launches([N])
        assert E.last_launch_kind() == E.LAUNCH_QUAD
    runs["calls of 1, 13 and the rest"] = Run(device, T, Cn, **kw).launches([1, 13, N - 14])
    for what, r in runs.items():
        g = r.acc.np()
        assert np.array_equal(g["ref"], ref), what
        assert_sums_match(g, want, what)
        assert_rest_equal(r.rest_np(), traced.rest_np(), what)
    # nothing else moves: the same run without the sums, its covariance and histogram kept
    off = Run(device, T, Cn, burn=burn, se=se).launches([N])
    on = runs["thread"]
    assert_rest_equal(on.rest_np(), off.rest_np(), "with and without the sums")
    assert torch.equal(on.cov[2], off.cov[2]) and torch.equal(on.hist, off.hist) and int(on.cov[2].item()) == Cn * 13  # (step counters 12 .. 60)
    if T > 1:
        assert off.rest_np()["swap_accept"].sum() > 0
    # double states: logp stays float32, the same kernels read it
    f64, snaps64 = traced_snapshots(device, T, Cn, N, f64=True, **kw)
    want64 = energy_reference(snaps64, f64.betas, 16, 0, ref_of(snaps64[0]))
    assert_sums_match(f64.acc.np(), want64, "double states, traced")
    assert_sums_match(Run(device, T, Cn, f64=True, **kw).launches([N]).acc.np(), want64, "double states")


# ---- 3. split steps ------------------------------------------------------------------------------------------------------
def _wrapped(device, dim):
    """The library's own density behind a user-defined class without engine_target(): split steps, and a density whose values do
    not depend on whether it runs eagerly or inside a captured graph."""
    from interfaces import TorchTargetDistribution

    tgt = carpet(device, dim).engine_target()

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


def run_sums(run):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in run.energy_sums().items()}


@gpu
def test_split_steps_eager_and_captured_match_one_trace(device):
    """A user-defined density of dim 5, 4 temperatures x 64 ladders, 48 steps, swap events every 2 steps so a captured block
    covers 16 steps: the eager loop against the replay of its own trace_logp, and ONE advance(48) by graph replay - the two
    kernels of ptrwm_energy sit inside the captured block and decide on the device whether the step is due and whether ref is
    set - against the same replay: counts equal, sums within the bounds."""
    from algorithms._engine_core import EngineRun

    dim, T, Cn, N, burn, every = 5, 4, 64, 48, 6, 4
    betas = np.geomspace(1.0, 0.05, T).astype(np.float32)
    x0 = np.random.default_rng(9).normal(0.0, 1.0, size=(Cn, T, dim)).astype(np.float32)

    def make():
        with pytest.warns(UserWarning, match="split steps"):
            return EngineRun(target_dist=_wrapped(device, dim), proposal=H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim).engine(device),
                             beta_ladder=list(betas), dim=dim, device=device, n_replicas=Cn, initial_state=x0, burn_in=burn, swap_every=2,
                             swap_mode="exchange", swap_order="sequential", seed=SEED, energy=True, energy_every=every, energy_groups=16,
                             cov_temps=T, cov_every=3)

    eager = make()
    trace, trace_logp = torch.zeros(N, Cn, T, dim, device=device), torch.zeros(N, Cn, T, device=device)
    eager.advance(N, trace=trace, trace_logp=trace_logp)
    torch.cuda.synchronize()
    due = due_steps(range(1, N + 1), burn, every)
    assert due == list(range(8, 49, 4))
    snaps = trace_logp.cpu().numpy()[[sc - 1 for sc in due]]
    ref = ref_of(snaps[0])
    want = energy_reference(snaps, betas, 16, 0, ref)
    graph = make()
    graph.advance(N)  # no trace: blocks of steps are captured and replayed
    torch.cuda.synchronize()
    assert graph._graph is not None and eager._graph is None and graph._graph_block() == 16
    assert torch.equal(graph.state, eager.state) and torch.equal(graph.logp, eager.logp)
    sums = {"eager": run_sums(eager), "captured": run_sums(graph)}
    for what, g in sums.items():
        assert np.array_equal(g["ref"], ref) and g["ref_set"].tolist() == [1], what
        assert_sums_match(g, want, what)
    assert np.array_equal(sums["eager"]["count"], sums["captured"]["count"])
    tol = sum_tolerance(want)
    for k in SUMS:  # (each within its bound of the reference, so within twice that of each other)
        assert (np.abs(sums["eager"][k] - sums["captured"][k]) <= 2 * tol[k]).all(), k
    graph.reset_energy()
    g = run_sums(graph)
    assert all(float(np.abs(g[k]).sum()) == 0.0 for k in ("count", "nonfinite", "ref", "ref_set") + SUMS) and g["every"] == every


# ---- 4. with the ladder's tuning ------------------------------------------------------------------------------------------
@gpu
def test_the_sums_use_the_adapted_ladder(device):
    """adapt_ladder=True with burn_in 200 and ladder_every 50 over 8 rungs linear in beta: beta is read at the snapshot, so the
    replay that uses the ADAPTED ladder matches and the replay that uses the initial ladder does not."""
    from algorithms._engine_core import EngineRun

    dim, T, Cn, burn, every, N = 5, 8, 64, 200, 7, 221
    betas = np.linspace(1.0, 0.05, T).astype(np.float32)
    x0 = np.random.default_rng(4).normal(0.0, 1.0, size=(Cn, T, dim)).astype(np.float32)
    run = EngineRun(target_dist=carpet(device, dim), proposal=H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim).engine(device),
                    beta_ladder=list(betas), dim=dim, device=device, n_replicas=Cn, initial_state=x0, burn_in=burn, swap_every=5,
                    swap_mode="exchange", swap_order="sequential", seed=SEED, adapt_ladder=True, ladder_every=50, energy=True,
                    energy_every=every)
    trace, trace_logp = torch.zeros(N, Cn, T, dim, device=device), torch.zeros(N, Cn, T, device=device)
    run.advance(N, trace=trace, trace_logp=trace_logp)
    got = run_sums(run)
    due = due_steps(range(1, N + 1), burn, every)
    assert due == [203, 210, 217]
    snaps = trace_logp.cpu().numpy()[[sc - 1 for sc in due]]
    adapted = run.beta.cpu().numpy()
    assert adapted[0] == betas[0] and adapted[-1] == betas[-1] and not np.array_equal(adapted, betas)  # the interior moved
    assert np.array_equal(got["beta"], adapted)
    ref = ref_of(snaps[0])
    assert np.array_equal(got["ref"], ref)
    assert_sums_match(got, energy_reference(snaps, adapted, 16, 0, ref), "the adapted ladder")
    with pytest.raises(AssertionError, match="misses its bound"):
        assert_sums_match(got, energy_reference(snaps, betas, 16, 0, ref), "the initial ladder", show=False)


# ---- 5. the estimates against the closed form --------------------------------------------------------------------------------
def rel_var(a, beta, d):
    """The relative variance of one term exp(a l) under pi^beta for the unit Gaussian in dim d: (1 + 2a/beta)^(-d/2) (1 + a/beta)^d - 1."""
    return (1 + 2 * a / beta) ** (-d / 2) * (1 + a / beta) ** d - 1


@gpu
def test_the_unit_gaussian_gives_back_its_normalising_constants(device):
    """The library's diagonal Gaussian, normalised, unit variances, dim 4: 8 rungs beta_t = 0.1^(t/7), 4 096 ladders started in
    their tempered laws (x = z / sqrt(beta_t)), 40 steps, a snapshot every 10.  The step kernels leave the tempered laws
    invariant and replicas are independent, so the variance of a pooled mean is at most its one-snapshot value over 4 096
    draws.  Truth: log Z(b_a) / Z(b_b) = (b_b - b_a)/2 d log 2 pi - d/2 log(b_a / b_b).  Every rung's forward and reverse within
    6 sqrt(v / 4096) of it (the truths run from -1.69 to -0.80), v the relative variance of one term (rel_var: 0.178 forward, 0.390 reverse on this ladder);
    mean_energy within 6 sqrt(d / (2 beta^2) / 4096) of -d/(2 beta) - d/2 log 2 pi; every se finite and positive; and
    sum forward <= sum reverse + 6 sigma, sigma^2 the sum of all fourteen margins' variances (whatever their correlation, the
    standard deviation of the difference of the sums is at most the sum of the standard deviations, which the root of the sum of
    squares times sqrt 14 bounds; 6 sigma is asked for, the tighter of the two)."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    d, T, R = 4, 8, 4096
    betas = [float(0.1 ** (t / 7)) for t in range(T)]
    b = np.array(betas, dtype=np.float32).astype(np.float64)  # (the ladder as the device holds it)
    z = np.random.default_rng(11).normal(size=(R, T, d))
    x0 = (z / np.sqrt(b)[None, :, None]).astype(np.float32)
    tgt = MultivariateNormalTorch(d, mean=torch.zeros(d), cov=torch.eye(d), device=device)
    alg = ParallelTemperingRWM_GPU_Optimized(d, 2.38 ** 2 / 4, tgt, beta_ladder=betas, swap_every=5, burn_in=0, device=device, num_replicas=R,
                                             seed=SEED, trace="none", initial_states=x0, energy=True, energy_every=10)
    assert not alg._ensure_started() and not alg._run.split  # the fused kernel
    alg._advance(40)
    assert alg.energy_count.tolist() == [4 * R] * T
    truth = np.array([(b[t] - b[t - 1]) / 2 * d * math.log(2 * math.pi) - d / 2 * math.log(b[t - 1] / b[t]) for t in range(1, T)])
    v_f = np.array([rel_var(b[t - 1] - b[t], b[t], d) for t in range(1, T)])
    v_r = np.array([rel_var(b[t] - b[t - 1], b[t - 1], d) for t in range(1, T)])
    assert np.allclose(v_f, 0.178, atol=2e-3) and np.allclose(v_r, 0.390, atol=2e-3) and (truth < -0.8).all() and (truth > -1.7).all()
    fw, fw_se = alg.log_normalizer_ratios("forward")
    rv, rv_se = alg.log_normalizer_ratios("reverse")
    m_f, m_r = 6 * np.sqrt(v_f / R), 6 * np.sqrt(v_r / R)
    print(f"forward error / margin {np.abs(fw.numpy() - truth) / m_f}\nreverse error / margin {np.abs(rv.numpy() - truth) / m_r}")
    assert (np.abs(fw.numpy() - truth) <= m_f).all() and (np.abs(rv.numpy() - truth) <= m_r).all()
    mean, want_mean = alg.mean_energy().numpy(), -d / (2 * b) - d / 2 * math.log(2 * math.pi)
    m_e = 6 * np.sqrt(d / (2 * b * b) / R)
    print(f"mean energy error / margin {np.abs(mean - want_mean) / m_e}")
    assert (np.abs(mean - want_mean) <= m_e).all()
    for method in ("forward", "reverse", "thermodynamic", "thermodynamic_corrected"):
        se = alg.log_normalizer_ratios(method)[1]
        assert torch.isfinite(se).all() and (se > 0).all(), method
        total, tse = alg.log_normalizer_ratio(method)
        assert math.isfinite(total) and math.isfinite(tse) and tse > 0, method
    sigma = math.sqrt(((v_f + v_r) / R).sum())
    assert float(fw.sum()) <= float(rv.sum()) + 6 * sigma
    assert (alg.energy_variance() > 0).all() and (alg.heat_capacity() > 0).all()
    info = alg.get_diagnostic_info()
    assert info["energy_overflow"] is False and info["energy_nonfinite"] == 0
    assert abs(info["log_z_ratio_forward"] - truth.sum()) <= m_f.sum() and abs(info["log_z_ratio_reverse"] - truth.sum()) <= m_r.sum()


# ---- 6. the classes ------------------------------------------------------------------------------------------------------
class Spy:
    """Stands where RunPlan keeps its library handle: every function fetched from it records its name and calls through."""

    def __init__(self, plan):
        self.lib, self.calls = plan._lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


@gpu
def test_the_classes_answer_with_the_shapes_and_keys_of_the_issue(device, monkeypatch):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized

    dim, R, ladder_ = 5, 70, [1.0, 0.5, 0.2, 0.05]
    T = len(ladder_)
    keys = {"log_z_ratio_forward", "log_z_ratio_reverse", "log_z_ratio_se", "energy_nonfinite", "energy_overflow"}

    def pt(**more):
        return ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, carpet(device, dim), beta_ladder=ladder_, swap_every=2, burn_in=4,
                                                  device=device, num_replicas=R, seed=5, trace="none", **more)

    alg = pt(energy=True, energy_every=3)
    alg._advance(40)
    assert alg.energy_count.tolist() == [R * 12] * T  # step counters 6, 9, ..., 39
    for read in (alg.mean_energy, alg.energy_variance, alg.heat_capacity):
        v = read()
        assert v.shape == (T,) and v.dtype == torch.float64 and torch.isfinite(v).all()
    for method in ("forward", "reverse", "thermodynamic", "thermodynamic_corrected"):
        v, se = alg.log_normalizer_ratios(method)
        assert v.shape == se.shape == (T - 1,) and torch.isfinite(v).all() and (se > 0).all(), method
        total, tse = alg.log_normalizer_ratio(method)
        assert isinstance(total, float) and total == pytest.approx(float(v.sum())) and tse > 0
    info = alg.get_diagnostic_info()
    assert keys <= set(info) and info["energy_overflow"] is False and info["energy_nonfinite"] == 0 and info["log_z_ratio_se"] > 0
    run = alg._run
    assert int(run.energy_sums()["ref_set"].item()) == 1 and not run.energy_sums()["pinned"]
    run.reset_energy()  # the sums and, with an automatic ref, the flag
    s = run_sums(run)
    assert all(float(np.abs(s[k]).sum()) == 0.0 for k in ("count", "nonfinite", "ref_set") + SUMS)
    alg.reset()
    assert alg.energy_count.tolist() == [0] * T and torch.isnan(alg.mean_energy()).all()
    # energy_ref= pins the level: it is there from the start and a reset leaves it
    pinned = pt(energy=True, energy_every=3, energy_ref=-7.5, energy_groups=4)
    pinned._advance(10)
    s = run_sums(pinned._run)
    assert s["ref"].tolist() == [-7.5] * T and s["ref_set"].tolist() == [1] and s["pinned"] and s["count"].shape == (4, T)
    assert s["count"].sum() == R * T * 2  # step counters 6 and 9
    pinned._run.reset_energy()
    s = run_sums(pinned._run)
    assert s["ref"].tolist() == [-7.5] * T and s["ref_set"].tolist() == [1] and s["count"].sum() == 0
    # one temperature: only the moments mean something
    rwm = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, carpet(device, dim), burn_in=4, device=device, num_chains=R, seed=5, energy=True,
                                     energy_every=3)
    rwm.generate_samples(20)
    assert rwm.energy_count.tolist() == [R * E.periodic_steps_in(0, rwm._run.steps_done, 3, 4)] and rwm._run.steps_done >= 20 and rwm.mean_energy().shape == (1,) and torch.isfinite(rwm.energy_variance()).all()
    assert rwm.log_normalizer_ratios()[0].shape == (0,) and keys <= set(rwm.get_diagnostic_info())
    # a run without energy= makes no call to the new entry points
    off = pt(cov="all", cov_every=4)
    off._ensure_started()
    spy = Spy(off._run._plan)
    monkeypatch.setattr(off._run._plan, "_lib", spy)
    off._run.advance(12)
    torch.cuda.synchronize()
    assert spy.calls == ["ptrwm_run_with_covariance"] and off._run.energy_sums() is None
    on = pt(energy=True, energy_every=4)
    on._ensure_started()
    spy = Spy(on._run._plan)
    monkeypatch.setattr(on._run._plan, "_lib", spy)
    on._run.advance(12)
    assert spy.calls == ["ptrwm_run_with_energy"]


# ---- 7. two shards ---------------------------------------------------------------------------------------------------------
@gpu
def test_two_shards_add_up_to_the_unsharded_sums(device):
    """The 64-ladder run of test 2 in shards of 37 and 27 chains, chain_offset 0 and 37.  Under a pinned ref the per-group counts
    add up to the unsharded run's exactly and the sums within the bounds; under automatic refs the host-side rescale of
    allreduce_energy, applied by hand to the two dicts, gives the same."""
    from algorithms.sharding import energy_rescale

    T, Cn, burn, se, N = 8, 64, 11, 5, 60
    kw = dict(burn=burn, se=se, every=7)
    x0 = np.random.default_rng(1000 * T + Cn).normal(0.0, 1.0, size=(Cn, T, 5))
    whole, snaps = traced_snapshots(device, T, Cn, N, x0=x0, **kw)
    pin = np.floor(ref_of(snaps[0]))
    want = energy_reference(snaps, whole.betas, 16, 0, pin)
    parts = [(0, 37), (37, 27)]
    unsharded = Run(device, T, Cn, x0=x0, ref=pin, **kw).launches([N]).acc.np()
    assert_sums_match(unsharded, want, "unsharded, pinned")
    shards = [Run(device, T, n, x0=x0[lo:lo + n], chain_offset=lo, ref=pin, **kw).launches([N]).acc.np() for lo, n in parts]
    added = {k: shards[0][k] + shards[1][k] for k in ("count", "nonfinite") + SUMS}
    assert np.array_equal(added["count"], unsharded["count"]) and (shards[0]["count"] > 0).all() and (shards[1]["count"] > 0).all()
    assert_sums_match(added, want, "two shards, pinned")
    # automatic refs: each shard chooses its own; the common one is their maximum
    autos = [Run(device, T, n, x0=x0[lo:lo + n], chain_offset=lo, **kw).launches([N]) for lo, n in parts]
    dicts = []
    for r, (lo, n) in zip(autos, parts):
        g = r.acc.np()
        assert np.array_equal(g["ref"], ref_of(snaps[0][lo:lo + n]))
        dicts.append({k: torch.from_numpy(v) for k, v in g.items()} | {"beta": torch.from_numpy(r.betas)})
    assert not np.array_equal(dicts[0]["ref"].numpy(), dicts[1]["ref"].numpy())
    common = torch.maximum(dicts[0]["ref"], dicts[1]["ref"])
    assert np.array_equal(common.numpy(), ref_of(snaps[0]))
    scaled = [energy_rescale(dct, common) for dct in dicts]
    added = {k: (scaled[0][k] + scaled[1][k]).numpy() for k in ("count", "nonfinite") + SUMS}
    want = energy_reference(snaps, whole.betas, 16, 0, common.numpy())
    # (the rescale is one product more per shard and sum: one unit of 2^-53 of the element's sum each, inside the four the two
    # exp are given - the reference's own stays below one)
    assert_sums_match(added, want, "two shards, automatic refs rescaled")
