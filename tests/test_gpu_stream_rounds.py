"""The streaming form of the step kernel (kernel.h STREAM) where one wave walks SEVERAL exchange groups.  Needs an MI355X:
run with `-m gpu`.

The streaming kernel is a persistent loop: the next group's rows and statistics arrive by LDS-DMA in the other slab and
landing zone (`prefetch`), the finished group's results wait in registers (`pend_*`) and are stored one iteration later
under `pend_group` (`flush_pending`), `cur ^= 1` switches slabs.  None of that runs unless a wave walks more than one
group, and the launcher (variants.h launch_run_stream) sizes the grid to the device: every other streaming test of the
suite has fewer groups than the device holds waves, so its loop body runs once.

How the batches here make several rounds CERTAIN, without reading the occupancy the launcher asked for:
  * a compute unit holds at most 8 waves per SIMD = 32 waves, so the launcher's max_waves = CUs x workgroups per CU x 4
    is at most W = 32 x CUs (CUs: torch's multi_processor_count), whatever the kernel's registers and LDS allow;
  * with n_groups = k W + r, 0 < r < W, rounds = ceil(n_groups / max_waves) >= ceil(n_groups / W) = k + 1;
  * at most W waves are launched and wave w walks groups w, w + stride, ... with stride <= W: every group with index
    >= W is at least the SECOND group of its wave (its rows landed in slab 1, the results before it were flushed inside
    the loop), every group with index >= 2 W at least the THIRD (slab 0 reused behind a flush);
  * the launcher trims the grid to waves = ceil(n_groups / rounds); r is odd (so no multiple of 4, the waves of a
    workgroup), which leaves the last round uneven: some waves walk one group fewer than others;
  * n_chains = n_groups x (64 // T) keeps every group whole, which the streaming form requires (capi.hip
    stream_layout_ok).
Each case asserts the bound k + 1 from n_groups and W alone: arithmetic on the inputs, not on the code under test.  (On a
256-CU device W = 8 192; the kernel's true max_waves at dim 30 is about 2 048, so the real number of rounds is several
times the bound.)

What is compared: the streaming form against the classic kernel, every replica, bit for bit, on the device, after every
launch of chains of 1-, 2- and 3-step launches; blocks of groups of every round against the CPU oracle, every differing
decision proven (helpers.check_production_ladders); and which launches AUTO hands to the streaming form.
"""
import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E

pytestmark = pytest.mark.gpu

RC_NORMAL = dict(base_variance_scalar=2.38**2 / 30)
SCHED = dict(burn_in=4, swap_every=5, seed=91, chain_offset=3)
HORIZON = 26  # two and a half swap periods behind the burn-in: one-step launches with and without a swap event

# (target, proposal, temperatures, k, r, proposal arguments): n_groups = k W + r, see the module docstring
CASES = {
    "rc15_d30-T32-k2": ("rc15_d30", "Normal", 32, 2, 37, RC_NORMAL),   # the headline kernel; groups past 2 W: third iteration or later
    "rc15_d30-T5-k2": ("rc15_d30", "Normal", 5, 2, 37, RC_NORMAL),     # 60 live lanes: idle lanes across iterations, `2 tid < n_live` DMA guards
    "rc15_d30-T1-k2": ("rc15_d30", "Normal", 1, 2, 37, RC_NORMAL),     # plain RWM: 64 chains per wave, no swap bookkeeping
    "tm_d50-T64-k1": ("tm_d50", "UniformRadius", 64, 1, 37, dict(base_radius=2.5)),  # one ladder per wave; far fewer resident waves than W at dim 50
    "beta_d5-T4-k3": ("beta_d5", "UniformRadius", 4, 3, 37, dict(base_radius=0.3)),  # small dim, highest occupancy, bounded support
    "even_d30-T32-k2": ("even_d30", "Laplace", 32, 2, 37, dict(base_variance_vector=np.full(30, 0.02))),
    "rc15_d30-T32-k1-r5": ("rc15_d30", "Normal", 32, 1, 5, RC_NORMAL),  # a last round in which almost every wave has finished
}
ORACLE_CASES = ["rc15_d30-T32-k2", "rc15_d30-T5-k2", "beta_d5-T4-k3"]
# (case, the statistics the launch is NOT given): the pend_*_on flags and the DMA guards branch on exactly these pointers
ABSENT_CASES = [
    ("rc15_d30-T5-k2", ("sq_jump",)),
    ("rc15_d30-T1-k2", ("n_accept",)),
    ("beta_d5-T4-k3", H.STAT_KEYS),  # RunPlan (and ptrwm_run) take a run without any statistics
]


def wave_bound(device):
    """W: no launch of the streaming kernel has more waves than this (32 resident waves per compute unit)."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert cus >= 2
    return 32 * cus


def start_arrays(spec, Cn, T, device, seed):
    """Starting states drawn on the device, distinct per replica, their log-densities by the engine's own kernel, and
    non-zero starting statistics that differ per replica: a value carried over from another group is a wrong value."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    shape = (Cn, T, spec.dim)
    if spec.cls == "IIDBetaTorch":
        st = 0.2 + 0.6 * torch.rand(shape, generator=g, device=device)
    elif "Rosenbrock" in spec.cls:
        st = 0.1 * torch.randn(shape, generator=g, device=device)
    else:
        st = 0.5 * torch.randn(shape, generator=g, device=device)
    lp = E.logdensity(spec.engine(device), st.view(-1, spec.dim)).view(Cn, T).contiguous()
    idx = torch.arange(Cn * T, device=device, dtype=torch.int64).view(Cn, T)
    stats = {"n_accept": idx % 1009 + 1, "sq_jump": (idx % 977).to(torch.float64) * 0.125 + 0.5,
             "swap_accept": idx % 13 + 2, "last_swap_ordinal": idx % 3}
    return st, lp, {k: v.contiguous() for k, v in stats.items()}


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_same_on_device(a, b, what):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), (k, *what)


def group_ranges(n_groups, W):
    """[0, W), [W, 2 W), [2 W, n_groups): first, second, third-or-later group of a wave (the ranges that exist)."""
    edges = [0] + [e for e in (W, 2 * W) if e < n_groups] + [n_groups]
    return list(zip(edges[:-1], edges[1:]))


def assert_active(cur, start, cpw, T, ranges, what):
    """The agreement is not an empty one: every range of groups holds accepted moves and, for a ladder, accepted swaps
    and a raised last-swap ordinal (each as far as the launch was given the statistic that shows it)."""
    for g0, g1 in ranges:
        sl = slice(g0 * cpw, g1 * cpw)
        assert bool((cur["state"][sl] != start["state"][sl]).any()), ("no move", g0, g1, *what)
        if "n_accept" in cur:
            assert int((cur["n_accept"][sl] - start["n_accept"][sl]).sum()) > 0, ("n_accept", g0, g1, *what)
        if "sq_jump" in cur:
            assert bool((cur["sq_jump"][sl] > start["sq_jump"][sl]).any()), ("sq_jump", g0, g1, *what)
        if T > 1 and "swap_accept" in cur:
            assert int((cur["swap_accept"][sl] - start["swap_accept"][sl]).sum()) > 0, ("swap_accept", g0, g1, *what)
        if T > 1 and "last_swap_ordinal" in cur:
            assert bool((cur["last_swap_ordinal"][sl] > start["last_swap_ordinal"][sl]).any()), ("last_swap_ordinal", g0, g1, *what)


def oracle_blocks(n_groups, W):
    """First groups of five blocks of 8 whole groups: the first groups, the groups straddling W and 2 W, a block in the
    middle of the last range, the last 8 groups."""
    last0 = group_ranges(n_groups, W)[-1][0]
    starts = [0, W - 4, 2 * W - 4, (last0 + n_groups) // 2 - 4, n_groups - 8]
    assert all(0 <= a and a + 8 <= b for a, b in zip(starts, starts[1:] + [n_groups + 8])), starts  # in range, disjoint, ascending
    return starts


_blocks_of_case = {}  # case -> what the oracle link needs of the streaming run (a few hundred ladders on the host)


def chained_launches(device, case, absent=()):
    """Launches of 1, 2 and 3 steps chained over HORIZON steps, the classic kernel and the streaming form side by side on
    device tensors: the launch kinds, all outputs bit for bit after every launch, activity in every range of groups.
    Returns the rows of the oracle blocks (start and end of the chain of one-step launches, streaming form)."""
    tkey, pkind, T, k, r, pkw = CASES[case]
    W = wave_bound(device)
    assert 0 < r < W and r % 2 == 1 and r % 4 != 0
    cpw = 64 // T
    n_groups = k * W + r
    assert -(-n_groups // W) == k + 1 >= 2  # the proven lower bound on rounds: ceil(n_groups / W) <= ceil(n_groups / max_waves)
    Cn = n_groups * cpw
    spec = H.target_spec(tkey)
    assert Cn % cpw == 0 and (cpw * T) % 2 == 0 and (cpw * T * spec.dim) % 4 == 0  # stream_layout_ok
    beta = (0.05 ** (np.arange(T) / max(1, T - 1))).astype(np.float32)
    prop = H.proposal_spec(pkind, spec.dim, beta, **pkw)
    assert E.has_stream_variant(spec.kind, prop.kind, spec.dim)
    st0, lp0, stats0 = start_arrays(spec, Cn, T, device, seed=1000 + T)
    stats0 = {s: v for s, v in stats0.items() if s not in absent}
    start = dict(state=st0, logp=lp0, **stats0)
    ranges = group_ranges(n_groups, W)
    assert len(ranges) == min(k + 1, 3)
    target, proposal, beta_d = spec.engine(device), prop.engine(device), H.dev_t(beta, device)
    sides = {}
    for mode in (E.STREAM_OFF, E.STREAM_ON):
        arrays = {s: torch.empty_like(v) for s, v in start.items()}
        sides[mode] = (arrays, E.RunPlan(target, proposal, beta=beta_d, **arrays, **SCHED))
    kind = {E.STREAM_OFF: E.LAUNCH_THREAD, E.STREAM_ON: E.LAUNCH_STREAM}
    blocks = None
    with E.kernel_form(E.FORM_THREAD):
        for n in (1, 2, 3):
            for arrays, _ in sides.values():
                for s, v in arrays.items():
                    v.copy_(start[s])
            for i in range(HORIZON // n):
                for mode, (_, plan) in sides.items():
                    with E.stream_mode(mode):
                        plan.launch(i * n, n)
                        assert E.last_launch_kind() == kind[mode], (mode, n, i)
                assert_same_on_device(sides[E.STREAM_OFF][0], sides[E.STREAM_ON][0], (case, n, i))
            streamed = sides[E.STREAM_ON][0]
            assert_active(streamed, start, cpw, T, ranges, (case, n))
            if n == 1 and not absent and case in ORACLE_CASES:
                blocks = []
                for g0 in oracle_blocks(n_groups, W):
                    sl = slice(g0 * cpw, (g0 + 8) * cpw)  # only these ladders' rows travel to the host
                    blocks.append((g0 * cpw, {s: v[sl].cpu().numpy() for s, v in start.items()},
                                   {s: v[sl].cpu().numpy() for s, v in streamed.items()}))
    return dict(spec=spec, prop=prop, beta=beta, blocks=blocks, n_groups=n_groups, state_bytes=st0.numel() * 4, rounds_bound=k + 1)


@pytest.mark.parametrize("case", list(CASES))
def test_streaming_form_over_several_rounds_equals_the_classic_kernel(device, case):
    """n_groups = k W + r groups, so that every wave of the streaming kernel walks at least k + 1 >= 2 (k = 1) or >= 3
    groups (module docstring): launch by launch the streaming form leaves the bits of the classic kernel in `state`,
    `logp`, `n_accept`, `sq_jump`, `swap_accept` and `last_swap_ordinal` of every replica, compared on the device, over
    chains of 1-, 2- and 3-step launches (one-step launches with and without a swap event, longer ones with an event
    inside), from distinct starting rows and non-zero starting statistics; and every range of groups - first, second,
    third-or-later group of a wave - holds accepted moves, accepted swaps and raised last-swap ordinals."""
    out = chained_launches(device, case)
    print(f"{case}: n_groups {out['n_groups']}, rounds >= {out['rounds_bound']}, state {out['state_bytes'] / 1e6:.1f} MB")
    if case in ORACLE_CASES:
        _blocks_of_case[case] = out


@pytest.mark.parametrize("case,absent", ABSENT_CASES, ids=[f"{c}-without-{'-'.join(a) if len(a) < 4 else 'all'}" for c, a in ABSENT_CASES])
def test_streaming_rounds_without_some_statistics(device, case, absent):
    """The same chains with statistics the launch is not given - no squared-jump sums, no acceptance counts, none of the
    four (RunPlan takes that): their landing zones are not filled and their pending stores not made, iteration after
    iteration, and everything that is given keeps the classic kernel's bits.  (Without `swap_accept` and
    `last_swap_ordinal` accepted swaps show only in the rows: the ranges are then proven active by their moves.)"""
    chained_launches(device, case, absent=tuple(absent))


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_groups_of_every_round_follow_the_oracle(device, case):
    """Bit-equality with the classic twin shares the twin's reading of the rules: five blocks of 8 whole groups of the
    streaming run's result (26 one-step launches) - the first groups, the groups straddling W and 2 W, a block in the
    middle of the last range, the very last groups - are tied to the CPU oracle by helpers.check_production_ladders:
    the fixture twin, run over just these ladders from their own starting rows and statistics, reproduces the streaming
    run's final arrays bit for bit and follows the oracle decision for decision, every flip proven."""
    out = _blocks_of_case.get(case) or chained_launches(device, case)
    assert len(out["blocks"]) == 5
    for l0, begin, end in out["blocks"]:
        H.check_production_ladders(out["spec"], out["prop"], device, end, l0=l0, state=begin["state"], logp=begin["logp"],
                                   stats0=begin, beta=out["beta"], launches=[(i, 1) for i in range(HORIZON)], **SCHED)


def test_auto_takes_the_streaming_form_at_the_headline_shape_only(device):
    """The AUTO rule (capi.hip: launches of kStreamMaxSteps = 1 step whose state, log-densities, acceptance counts and
    squared-jump sums - n_chains x T x (4 dim + 20) bytes - total kStreamMinBytes..kStreamMaxBytes = 192..448 MiB) at
    BASELINE configs[2]'s shape, 65 536 ladders x 32 temperatures x dim 30 (280 MiB by that count), AUTO kernel form:
    25 one-step launches across five swap events each report LAUNCH_STREAM and leave, in every array, the bits the same
    launches leave under STREAM_OFF; the first and the last 64 ladders follow the oracle; a launch of two steps, and
    one-step launches of a batch of 16 384 ladders (70 MiB) and of 262 144 ladders (1 120 MiB), well outside the window
    on either side, run the classic kernel."""
    T, D, Cn, N = 32, 30, 65536, 25
    spec = H.target_spec("rc15_d30")
    beta = (0.05 ** (np.arange(T) / (T - 1))).astype(np.float32)
    prop = H.proposal_spec("Normal", D, beta, **RC_NORMAL)
    target, proposal, beta_d = spec.engine(device), prop.engine(device), H.dev_t(beta, device)
    st0, lp0, stats0 = start_arrays(spec, Cn, T, device, seed=7)
    start = dict(state=st0, logp=lp0, **stats0)
    assert (192 << 20) < Cn * T * (4 * D + 20) < (448 << 20)
    sides = {}
    for mode in (E.STREAM_OFF, E.STREAM_AUTO):
        arrays = {s: v.clone() for s, v in start.items()}
        sides[mode] = (arrays, E.RunPlan(target, proposal, beta=beta_d, **arrays, **SCHED))
    auto = sides[E.STREAM_AUTO][0]
    with E.kernel_form(E.FORM_AUTO):
        for i in range(N):
            for mode, want in ((E.STREAM_OFF, E.LAUNCH_THREAD), (E.STREAM_AUTO, E.LAUNCH_STREAM)):
                with E.stream_mode(mode):
                    sides[mode][1].launch(i, 1)
                    assert E.last_launch_kind() == want, (mode, i)
            assert_same_on_device(sides[E.STREAM_OFF][0], auto, ("auto", i))
    assert_active(auto, start, 64 // T, T, [(0, Cn // 2)], ("auto",))
    assert H.events_upto(N, SCHED["swap_every"], SCHED["burn_in"]) >= 2
    with E.kernel_form(E.FORM_AUTO), E.stream_mode(E.STREAM_AUTO):
        for l0 in (0, Cn - 64):
            sl = slice(l0, l0 + 64)
            H.check_production_ladders(spec, prop, device, {s: v[sl].cpu().numpy() for s, v in auto.items()}, l0=l0,
                                       state=st0[sl].cpu().numpy(), logp=lp0[sl].cpu().numpy(),
                                       stats0={s: v[sl].cpu().numpy() for s, v in stats0.items()}, beta=beta,
                                       launches=[(i, 1) for i in range(N)], **SCHED)
        sides[E.STREAM_AUTO][1].launch(N, 2)  # kStreamMaxSteps
        assert E.last_launch_kind() == E.LAUNCH_THREAD
    del sides, auto, start, st0, lp0, stats0
    torch.cuda.empty_cache()
    for ladders in (16384, 262144):
        total = ladders * T * (4 * D + 20)
        assert total < (192 << 20) // 2 or total > 2 * (448 << 20)  # clearly outside the window, not at its edge
        if torch.cuda.mem_get_info(device)[0] < 2 * total:
            print(f"{ladders} ladders not run: {total >> 20} MiB of arrays do not fit the device's free memory")
            continue
        state = torch.zeros(ladders, T, D, device=device)
        arrays = dict(state=state, logp=E.logdensity(target, state.view(-1, D)).view(ladders, T).contiguous(),
                      n_accept=torch.zeros(ladders, T, dtype=torch.int64, device=device),
                      sq_jump=torch.zeros(ladders, T, dtype=torch.float64, device=device))
        with E.kernel_form(E.FORM_AUTO), E.stream_mode(E.STREAM_AUTO):
            E.RunPlan(target, proposal, beta=beta_d, **arrays, **SCHED).launch(0, 1)
            assert E.last_launch_kind() == E.LAUNCH_THREAD, ladders
            with E.stream_mode(E.STREAM_ON):  # (the shape itself is one the streaming form serves: the window decided)
                E.RunPlan(target, proposal, beta=beta_d, **arrays, **SCHED).launch(1, 1)
                assert E.last_launch_kind() == E.LAUNCH_STREAM, ladders
        torch.cuda.synchronize()
        del state, arrays
        torch.cuda.empty_cache()
