"""Pooled marginal histograms (include/ptrwm.h ptrwm_hist_args, csrc/hist.h) on the GPU.

The yardstick is independent of the code under test: a run with a full trace of the covered temperatures, and a NumPy replay
of the float32 bin rule (tests/test_hist_host.py shows the replay equal to csrc/hist.h) over the traced rows of the due steps.
Everything is integer, so `counts` and `count` must be EQUAL to the replay.  On top: the counts do not depend on where the
caller cuts the run into launches or shards, a run with histograms moves no other output, and split steps (eager and captured)
and the classes give the same.

Every range is narrower than the samples, so the underflow and the overflow bin are non-empty in every case (asserted).
"""
import math

import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E

gpu = pytest.mark.gpu

SEED = 20241019
HIST_TILE = 256  # chains per workgroup of the snapshot kernel (csrc/hist.h kHistChains)
LO, HI = -0.8, 0.9


def numpy_bins(x, lo, scale, n_bins):
    """The rule of csrc/hist.h: float32 arithmetic, truncation."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - np.asarray(lo, np.float32)) * np.asarray(scale, np.float32)
    b = np.zeros(u.shape, np.int64)
    over = u >= np.float32(n_bins)
    mid = (u >= 0) & ~over
    b[over] = n_bins + 1
    b[mid] = 1 + u[mid].astype(np.int64)
    return b


def replay(rows, lo, scale, n_bins):
    """counts [temps, dim, n_bins + 2] and count [temps] of snapshot rows [snapshots, chains, temps, dim]."""
    rows = np.asarray(rows).astype(np.float32)  # (double states: rounded to float first)
    S, Cn, Tc, D = rows.shape
    bins = numpy_bins(rows, lo[None, None, None, :], scale[None, None, None, :], n_bins)
    counts = np.zeros((Tc, D, n_bins + 2), np.int64)
    for t in range(Tc):
        for d in range(D):
            counts[t, d] = np.bincount(bins[:, :, t, d].ravel(), minlength=n_bins + 2)
    return counts, np.full(Tc, S * Cn, np.int64)


def due_rows(step0, n_steps, burn, every):
    """Indices, within a trace of every step of the request, of the steps whose step counter is due."""
    return [i for i in range(n_steps) if step0 + i + 1 > burn and (step0 + i + 1) % every == 0]


def diag_spec(dim):
    return H.TargetSpec(kind=E.TARGET_DIAG_GAUSSIAN, dim=dim, p=(-0.5 * dim * math.log(2 * math.pi),), ip=(1,),
                        vec0=np.ones(dim, np.float32))


class Run:
    """One sampler run through the C ABI with every output on the device."""

    def __init__(self, device, dim, T, Cn, *, burn, se, n_bins=0, temps=0, every=1, f64=False, chain_offset=0, x0=None, target=True,
                 seed=SEED, lo=LO, hi=HI):
        self.dim, self.T, self.Cn, self.device, self.burn, self.every, self.n_bins = dim, T, Cn, device, burn, every, n_bins
        betas = np.geomspace(1.0, 0.3, T).astype(np.float32)
        self.spec, self.prop = diag_spec(dim), H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim)
        self.tgt = self.spec.engine(device)
        if x0 is None:
            x0 = np.random.default_rng(1000 * T + Cn + dim).normal(0.0, 1.0, size=(Cn, T, dim))
        self.st = torch.tensor(x0, device=device, dtype=torch.float64 if f64 else torch.float32)
        self.lp = E.logdensity(self.tgt, self.st.view(-1, dim).float()).view(Cn, T).contiguous()
        self.stats = {k: torch.zeros(Cn, T, dtype=(torch.float64 if k == "sq_jump" else torch.int64), device=device)
                      for k in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")}
        self.plan = E.RunPlan(self.tgt if target else None, self.prop.engine(device), state=self.st, logp=self.lp,
                              beta=torch.tensor(betas, device=device), burn_in=burn, swap_every=se, seed=seed, chain_offset=chain_offset,
                              **self.stats)
        self.temps = temps
        if temps:
            self.lo = np.full(dim, lo, np.float32) + np.arange(dim, dtype=np.float32) * np.float32(0.01)  # (a range per coordinate)
            self.hi = np.full(dim, hi, np.float32)
            self.scale = (np.float32(n_bins) / (self.hi - self.lo)).astype(np.float32)
            self.counts = torch.zeros(temps, dim, n_bins + 2, dtype=torch.int64, device=device)
            self.count = torch.zeros(temps, dtype=torch.int64, device=device)
            self.plan.set_histogram(self.counts, torch.tensor(self.lo, device=device), torch.tensor(self.scale, device=device),
                                    n_bins=n_bins, temps=temps, every=every, count=self.count)

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

    def hist_np(self):
        torch.cuda.synchronize()
        return self.counts.cpu().numpy(), self.count.cpu().numpy()

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


#          id            dim  T   chains        bins  temps  f64
SHAPES = [("rwm70", 5, 1, 70, 7, 1, False),                  # more than a wave; a partial tile
          ("tile_plus_1", 3, 1, HIST_TILE + 1, 1, 1, False),  # a second workgroup with one chain; one bin
          ("pt3x4_cold", 3, 4, 3, 64, 1, False),              # covered and uncovered temperatures in one run
          ("pt3x4_all", 3, 4, 3, 64, 4, False),
          ("pt2x70", 2, 70, 2, 16, 70, False),                # workgroup-wide ladders; temps * dim above 64
          ("dim33", 33, 1, 5, 1024, 1, False),                # odd dim; the kernel's direct (no-LDS) strategy
          ("dim70", 70, 1, 5, 1024, 1, False),                # lane-split step kernel only
          ("bins126", 5, 2, 9, 126, 2, False),                # the last bin count the LDS strategy takes ...
          ("bins127", 5, 2, 9, 127, 2, False),                # ... and the first that goes direct
          ("f64", 3, 4, 3, 64, 4, True),                      # double states
          ("pt32x30_all", 30, 32, 70, 64, 32, False),         # the README shape: 960 columns in 8 groups of the snapshot kernel
          ("quad_d70_t8", 70, 8, 9, 64, 8, False)]            # lane-split only; 560 columns in 5 groups


def test_every_shape_has_a_step_kernel():
    """No GPU needed: no case below can fail for want of a variant."""
    for _, dim, T, *_ in SHAPES:
        spec = diag_spec(dim)
        assert E.has_thread_variant(spec.kind, E.PROPOSAL_NORMAL, dim) or E.has_quad_variant(spec.kind, E.PROPOSAL_NORMAL, dim, T), dim
    assert E.has_quad_variant(diag_spec(3).kind, E.PROPOSAL_NORMAL, 3, 4)  # double states: the lane-split form


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_counts_equal_the_numpy_replay_of_a_full_trace(device, shape):
    _, dim, T, Cn, nb, temps, f64 = shape
    N, burn, every, se = 24, 5, 3, 2
    kw = dict(burn=burn, se=se, n_bins=nb, temps=temps, every=every, f64=f64)
    traced = Run(device, dim, T, Cn, **kw)
    trace = torch.zeros(N, Cn, temps, dim, device=device, dtype=traced.st.dtype)
    traced.launches([N], trace=trace)
    counts, count = traced.hist_np()
    rows = trace.cpu().numpy()[due_rows(0, N, burn, every)]
    assert rows.shape[0] == 7  # step counters 6, 9, ..., 24
    want, want_n = replay(rows, traced.lo, traced.scale, nb)
    assert np.array_equal(counts, want) and np.array_equal(count, want_n)
    assert counts[..., 0].sum() > 0 and counts[..., -1].sum() > 0 and counts[..., 1:-1].sum() > 0  # both end bins are in play
    assert (counts.sum(-1) == count[:, None]).all()
    # the same run without a trace - the production step kernel between the snapshots - counts the same
    plain = Run(device, dim, T, Cn, **kw).launches([N])
    assert np.array_equal(plain.hist_np()[0], want) and np.array_equal(plain.hist_np()[1], want_n)
    assert_rest_equal(plain.rest_np(), traced.rest_np(), "with and without a trace", sq_jump_exact=False)


@gpu
def test_standalone_snapshot_of_a_hand_written_state(device):
    """ptrwm_histogram on a state that holds lo, hi, their neighbours, +-inf and NaN: the answers of csrc/hist.h."""
    lo, hi, nb = np.float32(-1.5), np.float32(2.5), 8
    inf = np.float32(np.inf)
    vals = np.array([lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, -inf), np.nextafter(hi, inf), inf, -inf,
                     np.nan, 0.0, -0.0, 0.5, 2.0, -1.0, 1e30, -1e30], np.float32)
    Cn, T, D = len(vals), 2, 3
    state = np.zeros((Cn, T, D), np.float32)
    state[:, 0, 0], state[:, 0, 1], state[:, 0, 2] = vals, vals[::-1], np.float32(0.25)
    state[:, 1, :] = vals[:, None]
    for f64 in (False, True):
        st = torch.tensor(state, device=device, dtype=torch.float64 if f64 else torch.float32)
        plan = E.RunPlan(None, H.proposal_spec("Normal", D, np.ones(T, np.float32), base_variance_scalar=1.0).engine(device), state=st,
                         logp=torch.zeros(Cn, T, device=device), beta=torch.ones(T, device=device), burn_in=4)
        los, scale = np.full(D, lo, np.float32), np.full(D, np.float32(nb) / (hi - lo), np.float32)
        for temps in (1, 2):
            counts = torch.zeros(temps, D, nb + 2, dtype=torch.int64, device=device)
            count = torch.zeros(temps, dtype=torch.int64, device=device)
            plan.set_histogram(counts, torch.tensor(los, device=device), torch.tensor(scale, device=device), n_bins=nb, temps=temps,
                               every=2, count=count)
            plan.split_histogram(2)  # step counter 3: not a multiple of 2
            plan.split_histogram(3)  # step counter 4: a multiple, but still in burn-in
            torch.cuda.synchronize()
            assert int(counts.sum().item()) == 0 and int(count.sum().item()) == 0
            plan.split_histogram(5)  # step counter 6: due
            plan.split_histogram(7)  # += : twice the counts
            want, want_n = replay(state[None, :, :temps], los, scale, nb)
            torch.cuda.synchronize()
            assert np.array_equal(counts.cpu().numpy(), 2 * want) and np.array_equal(count.cpu().numpy(), 2 * want_n)
            # spelled out for coordinate 0 of the cold temperature: NaN, -inf, below lo and -1e30 are underflow; lo opens bin 1
            c0 = want[0, 0]
            assert c0[0] == 4 and c0[-1] == 4 and c0[1] == 2  # over: hi, above hi, +inf, 1e30; bin 1: lo and just above lo
            assert c0[nb] == 2  # the last bin: just below hi, and 2.0
            st_np = st.cpu().numpy()
            assert np.array_equal(st_np, state.astype(st_np.dtype), equal_nan=True)  # a snapshot only reads


# The snapshot kernel beyond one group of columns (csrc/hist.h hist_geometry: td = temps * dim columns in `groups` groups of
# `cols`, the last of `last`).  tests/test_hist_host.py holds every row against hist_geometry itself, so that no case falls back
# to a single group if a constant of hist.h changes.
#                  id                dim  T   temps bins chains direct cols groups last  f64 as well
GEOMETRY_CASES = [("readme_8_groups", 30, 32, 32, 64, 300, False, 124, 8, 92, True),   # boundaries inside a temperature; a partial second chain tile
                  ("lds_min_cols", 13, 10, 10, 126, 257, False, 64, 3, 2, False),      # a last group of 2 columns: 128 chains in flight; a tile of one chain
                  ("lds_cols_cap", 7, 40, 40, 16, 70, False, 256, 2, 24, False),       # last group of 24: threads 240..255 idle
                  ("cold_5_of_12", 30, 12, 5, 64, 70, False, 124, 2, 26, False),       # temps < n_temps: chain stride 360 against td 150
                  ("direct_2_groups", 30, 10, 10, 127, 300, True, 256, 2, 44, True),
                  ("direct_max_bins", 104, 3, 3, 1024, 5, True, 256, 2, 56, False),    # the bin limit and the largest dim
                  ("widest_state", 104, 256, 256, 126, 3, False, 64, 416, 64, False)]  # td 26 624: the widest state the ABI accepts
GEOMETRY_RUNS = [(c, False) for c in GEOMETRY_CASES] + [(c, True) for c in GEOMETRY_CASES if c[-1]]


def hand_made_state(dim, T, temps, Cn, lo, cols, groups):
    """x[c, t, d] = mu[t, d] + sigma z in float64, mu a ramp over the column index t * dim + d across the histogram's range: no
    two columns hold the same distribution, so a column binned with another column's bounds, flushed to another column's
    counters, skipped or counted twice changes the counts.  +inf, -inf, NaN and lo[d] itself are planted in the second and in
    the last group of columns (under, over and bin 1 are then certain there).  Returns the state and the planted (chain, column)s."""
    rng = np.random.default_rng(dim * 1000 + T * 10 + Cn)
    mu = np.linspace(LO + 0.2, HI - 0.2, T * dim).reshape(T, dim)
    x = mu[None] + 0.45 * rng.standard_normal((Cn, T, dim))
    td, planted = temps * dim, []
    for g in sorted({1, groups - 1}):
        k0 = g * cols
        gcols = min(cols, td - k0)
        slots = [((3 * i + 1) % Cn, k0 + (5 * i) % gcols) for i in range(4)]
        assert len(set(slots)) == 4
        for (c, k), v in zip(slots, (np.inf, -np.inf, np.nan, None)):
            x[c, k // dim, k % dim] = lo[k % dim] if v is None else v
        planted += slots
    return x, planted


@gpu
@pytest.mark.parametrize("case,f64", GEOMETRY_RUNS, ids=[c[0] + ("_f64" if f else "") for c, f in GEOMETRY_RUNS])
def test_standalone_snapshot_at_every_multi_group_geometry(device, case, f64):
    """ptrwm_histogram on a hand-made state, no step kernel in the way, at the geometries of GEOMETRY_CASES: counts and count
    equal the NumPy replay, a second snapshot doubles them."""
    _, dim, T, temps, nb, Cn, _, cols, groups, last, _ = case
    td = temps * dim
    assert groups > 1 and (groups - 1) * cols + last == td
    lo = np.full(dim, LO, np.float32) + np.arange(dim, dtype=np.float32) * np.float32(0.01)  # (a range per coordinate, as Run)
    scale = (np.float32(nb) / (np.full(dim, HI, np.float32) - lo)).astype(np.float32)
    x, planted = hand_made_state(dim, T, temps, Cn, lo, cols, groups)
    st = torch.tensor(x, device=device, dtype=torch.float64 if f64 else torch.float32)
    plan = E.RunPlan(None, H.proposal_spec("Normal", dim, np.ones(T, np.float32), base_variance_scalar=1.0).engine(device), state=st,
                     logp=torch.zeros(Cn, T, device=device), beta=torch.ones(T, device=device), burn_in=0)
    counts = torch.zeros(temps, dim, nb + 2, dtype=torch.int64, device=device)
    count = torch.zeros(temps, dtype=torch.int64, device=device)
    plan.set_histogram(counts, torch.tensor(lo, device=device), torch.tensor(scale, device=device), n_bins=nb, temps=temps, every=1,
                       count=count)
    x_np = st.cpu().numpy()
    want, want_n = replay(x_np[None, :, :temps], lo, scale, nb)
    for times in (1, 2):  # += : the second snapshot doubles the counts
        plan.split_histogram(times - 1)
        torch.cuda.synchronize()
        got, got_n = counts.cpu().numpy(), count.cpu().numpy()
        assert np.array_equal(got_n, times * want_n), f"count after {times} snapshot(s)"
        bad = np.argwhere((got != times * want).any(-1))
        assert bad.size == 0, f"after {times} snapshot(s), {len(bad)} of {td} columns differ; the first (t, d): {bad[:5].tolist()}"
        assert (got.sum(-1) == got_n[:, None]).all()
    assert want_n.tolist() == [Cn] * temps
    # the planted values are where the replay says, and the last group's columns reach both end bins and the bins between
    flat = want.reshape(td, nb + 2)
    for c, k in planted:
        v = x_np[c, k // dim, k % dim]
        assert flat[k, nb + 1 if v == np.inf else (1 if v == lo[k % dim] else 0)] >= 1
    tail = flat[td - last:]
    assert tail[:, 0].sum() > 0 and tail[:, -1].sum() > 0 and tail[:, 1:-1].sum() > 0
    assert np.array_equal(st.cpu().numpy(), x_np, equal_nan=True)  # a snapshot only reads


@gpu
def test_counts_do_not_depend_on_how_the_caller_cuts_the_run(device):
    """One request of 60 steps against the same run as 3 and as 60 launches, and against step0 continued from an earlier call."""
    dim, T, Cn, N = 3, 4, 9, 60
    kw = dict(burn=7, se=3, n_bins=16, temps=4, every=4)
    one = Run(device, dim, T, Cn, **kw).launches([N])
    want, want_n = one.hist_np()
    assert want_n.tolist() == [Cn * 14] * 4  # step counters 8, 12, ..., 60
    assert want[..., 0].sum() > 0 and want[..., -1].sum() > 0
    for cuts in ([20, 20, 20], [1] * N, [25, 35], [7, 1, 3, 49]):
        r = Run(device, dim, T, Cn, **kw).launches(cuts)
        got, got_n = r.hist_np()
        assert np.array_equal(got, want) and np.array_equal(got_n, want_n), cuts
        assert_rest_equal(r.rest_np(), one.rest_np(), f"cuts {cuts}", sq_jump_exact=False)
    # `every` larger than the request: no snapshot is due, the counters stay zero, and the run is the run without histograms
    none = Run(device, dim, T, Cn, burn=7, se=3, n_bins=16, temps=4, every=100).launches([N])
    assert int(none.hist_np()[0].sum()) == 0 and int(none.hist_np()[1].sum()) == 0
    off = Run(device, dim, T, Cn, burn=7, se=3).launches([N])
    assert_rest_equal(none.rest_np(), off.rest_np(), "no due step")  # (the same launches: sq_jump bit-equal too)
    assert_rest_equal(one.rest_np(), off.rest_np(), "histograms on and off", sq_jump_exact=False)


@gpu
def test_histograms_under_the_streaming_form(device):
    """A snapshot ends a launch, and the streaming form of the step kernel (kernel.h STREAM) keeps state in flight across the
    groups of one launch: 12 one-step launches with a snapshot behind each, streaming against classic - every output equal - and
    both against the NumPy replay of a traced twin."""
    from test_gpu_engine_parity import STREAM_CASES

    tkey, pkind, T, Cn, _, streams = STREAM_CASES[0]
    assert (tkey, pkind, streams) == ("rc15_d30", "Normal", True)  # the shape: dim 30, 32 temperatures, 2 x 37 ladders
    dim, N, burn, nb = 30, 12, 3, 32
    assert E.has_stream_variant(diag_spec(dim).kind, E.PROPOSAL_NORMAL, dim)
    kw = dict(burn=burn, se=2, n_bins=nb, temps=T, every=1)
    runs = {}
    with E.kernel_form(E.FORM_THREAD):
        for mode in (E.STREAM_ON, E.STREAM_OFF):
            with E.stream_mode(mode):
                runs[mode] = Run(device, dim, T, Cn, **kw).launches([1] * N)
                assert E.last_launch_kind() == (E.LAUNCH_STREAM if mode == E.STREAM_ON else E.LAUNCH_THREAD)
        traced = Run(device, dim, T, Cn, **kw)
        trace = torch.zeros(N, Cn, T, dim, device=device)
        traced.launches([1] * N, trace=trace)
    on, off = runs[E.STREAM_ON], runs[E.STREAM_OFF]
    assert np.array_equal(on.hist_np()[0], off.hist_np()[0]) and np.array_equal(on.hist_np()[1], off.hist_np()[1])
    assert_rest_equal(on.rest_np(), off.rest_np(), "streaming and classic")  # (the same launches: sq_jump bit-equal too)
    want, want_n = replay(trace.cpu().numpy()[due_rows(0, N, burn, 1)], traced.lo, traced.scale, nb)
    assert want_n.tolist() == [Cn * 9] * T  # step counters 4, 5, ..., 12
    assert np.array_equal(on.hist_np()[0], want) and np.array_equal(on.hist_np()[1], want_n)
    assert want[..., 0].sum() > 0 and want[..., -1].sum() > 0 and want[..., 1:-1].sum() > 0
    assert_rest_equal(on.rest_np(), traced.rest_np(), "streaming and the traced twin", sq_jump_exact=False)
    assert on.rest_np()["n_accept"].sum() > 0 and on.rest_np()["swap_accept"].sum() > 0


@gpu
def test_nothing_else_moves(device):
    """State, logp and every counter of a run with histograms equal the same run without; moments and flow bound in the same
    call are what they are without histograms."""
    dim, T, Cn, N = 3, 4, 70, 40

    def make(hist, kind):
        r = Run(device, dim, T, Cn, burn=5, se=2, **(dict(n_bins=32, temps=2, every=3) if hist else {}))
        lead = (Cn,) if kind == "chain" else ()
        mom = {"sum": torch.zeros(*lead, 2, dim, dtype=torch.float64, device=device), "sum_sq": torch.zeros(*lead, 2, dim, dtype=torch.float64, device=device),
               "sum_logp": torch.zeros(*lead, 2, dtype=torch.float64, device=device), "count": torch.zeros(2, dtype=torch.int64, device=device)}
        (r.plan.set_chain_moments if kind == "chain" else r.plan.set_moments)(mom["sum"], mom["sum_sq"], sum_logp=mom["sum_logp"],
                                                                                count=mom["count"], every=2)
        flow = {"walker": torch.arange(T, device=device, dtype=torch.int32).repeat(Cn, 1).contiguous(),
                **{k: torch.zeros(Cn, T, dtype=torch.int64, device=device) for k in ("round_trips", "n_up", "n_down")}}
        r.plan.set_flow(flow["walker"], flow["round_trips"], flow["n_up"], flow["n_down"])
        r.launches([N])
        torch.cuda.synchronize()
        return r, {k: v.cpu().numpy() for k, v in mom.items()}, {k: v.cpu().numpy() for k, v in flow.items()}

    for kind in ("pooled", "chain"):
        (on, m_on, f_on), (off, m_off, f_off) = make(True, kind), make(False, kind)
        assert_rest_equal(on.rest_np(), off.rest_np(), kind, sq_jump_exact=False)
        for k in f_on:
            assert np.array_equal(f_on[k], f_off[k]), (kind, k)
        assert np.array_equal(m_on["count"], m_off["count"])
        for k in ("sum", "sum_sq", "sum_logp"):
            if kind == "chain":  # sequential sums in step order: bit-equal however the run is cut
                assert np.array_equal(m_on[k], m_off[k]), k
            else:  # atomics: the order of the additions is free, the last bits with it (tests/test_gpu_moments.py)
                assert np.allclose(m_on[k], m_off[k], rtol=1e-12, atol=1e-9), k
        assert on.hist_np()[1].tolist() == [Cn * 12] * 2  # step counters 6, 9, ..., 39
    # histograms alone: the production kernel's run, bit for bit
    on = Run(device, dim, T, Cn, burn=5, se=2, n_bins=32, temps=2, every=3).launches([N])
    off = Run(device, dim, T, Cn, burn=5, se=2).launches([N])
    assert_rest_equal(on.rest_np(), off.rest_np(), "histograms alone", sq_jump_exact=False)


@gpu
def test_two_shards_add_up_to_the_unsharded_counts(device):
    dim, T, Cn, N = 3, 4, 11, 30
    kw = dict(burn=4, se=2, n_bins=16, temps=4, every=5)
    x0 = np.random.default_rng(3).normal(0.0, 1.0, size=(Cn, T, dim))
    whole = Run(device, dim, T, Cn, x0=x0, **kw).launches([N])
    a = Run(device, dim, T, 4, x0=x0[:4], chain_offset=0, **kw).launches([N])
    b = Run(device, dim, T, Cn - 4, x0=x0[4:], chain_offset=4, **kw).launches([N])
    assert np.array_equal(a.hist_np()[0] + b.hist_np()[0], whole.hist_np()[0])
    assert np.array_equal(a.hist_np()[1] + b.hist_np()[1], whole.hist_np()[1])
    assert whole.hist_np()[0][..., 0].sum() > 0 and whole.hist_np()[0][..., -1].sum() > 0
    from algorithms.sharding import allreduce_histogram

    out = allreduce_histogram({"counts": whole.counts, "count": whole.count, "edges": None})  # no process group: this shard
    assert torch.equal(out["counts"], whole.counts) and torch.equal(out["count"], whole.count)


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
def test_split_steps_eager_and_captured_equal_the_replay(device):
    """A user-defined density: the eager loop against the NumPy replay of its own trace, the captured graph against the eager
    loop (the same Philox words, so the same states)."""
    from algorithms._engine_core import EngineRun

    dim, T, Cn, N, burn, every, nb = 3, 4, 9, 70, 6, 4, 16
    betas = np.geomspace(1.0, 0.3, T).astype(np.float32)
    x0 = np.random.default_rng(9).normal(0.0, 1.0, size=(Cn, T, dim)).astype(np.float32)

    def make():
        with pytest.warns(UserWarning, match="split steps"):
            return EngineRun(target_dist=_wrapped(device, dim), proposal=H.proposal_spec("Normal", dim, betas, base_variance_scalar=2.38 ** 2 / dim).engine(device),
                             beta_ladder=list(betas), dim=dim, device=device, n_replicas=Cn, initial_state=x0, burn_in=burn, swap_every=2,
                             swap_mode="exchange", swap_order="sequential", seed=SEED, hist_temps=T, hist_every=every, hist_bins=nb,
                             hist_range=(LO, HI))

    eager = make()
    trace = torch.zeros(N, Cn, T, dim, device=device)
    eager.advance(N, trace=trace)
    torch.cuda.synchronize()
    h = eager.histogram()
    lo = np.full(dim, LO, np.float32)
    scale = (np.float32(nb) / (np.full(dim, HI, np.float32) - lo)).astype(np.float32)
    want, want_n = replay(trace.cpu().numpy()[due_rows(0, N, burn, every)], lo, scale, nb)
    assert np.array_equal(h["counts"].cpu().numpy(), want) and np.array_equal(h["count"].cpu().numpy(), want_n)
    assert want[..., 0].sum() > 0 and want[..., -1].sum() > 0 and want_n[0] == Cn * 16  # step counters 8, 12, ..., 68
    assert h["edges"].shape == (dim, nb + 1) and h["edges"][0, 0].item() == float(np.float32(LO))
    graph = make()
    graph.advance(N)  # no trace: GRAPH_STEPS-step blocks are captured and replayed
    torch.cuda.synchronize()
    assert graph._graph is not None
    assert torch.equal(graph.state, eager.state)
    assert torch.equal(graph.histogram()["counts"], h["counts"]) and torch.equal(graph.histogram()["count"], h["count"])
    graph.reset_histogram()
    assert int(graph.histogram()["counts"].sum().item()) == 0 and int(graph.histogram()["count"].sum().item()) == 0


@gpu
def test_class_mode_weights_equal_the_fractions_of_the_class_trace(device):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    dim, N, burn, every, nb = 4, 300, 20, 3, 40
    kw = dict(swap_every=2, burn_in=burn, device=device, num_replicas=1, seed=11, trace="all", pre_allocate_steps=N)

    def pt(**more):
        return ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0]),
                                                  beta_ladder=[1.0, 0.3, 0.05, 0.01], **kw, **more)

    alg = pt(hist="all", hist_range=(-20.0, 20.0), hist_bins=nb, hist_every=every)
    alg.generate_samples(N)
    # the class's own trace: row i is the state after step i (row 0: the start), one replica, every temperature
    rows = alg._trace[:alg._rows_used].cpu().numpy()
    assert rows.shape[:3] == (burn + N + 1, 1, 4)
    snap = rows[[sc for sc in range(1, burn + N + 1) if sc > burn and sc % every == 0]]
    lo, hi = np.full(dim, -20.0, np.float32), np.full(dim, 20.0, np.float32)
    scale = (np.float32(nb) / (hi - lo)).astype(np.float32)
    want, want_n = replay(snap, lo, scale, nb)
    for t in (0, 3):
        counts, edges = alg.marginal_histogram(t)
        assert np.array_equal(counts.numpy(), want[t]) and edges.shape == (dim, nb + 1)
        bins = numpy_bins(snap[:, 0, t, :], lo, scale, nb)  # [snapshots, dim]
        total = bins.shape[0]
        # boundaries -5 and 5 are edges 15 and 25 (bin width 1): the intervals are bins 0..15, 16..25, 26..41
        w = alg.mode_weights([-5.0, 5.0], temperature=t).numpy()
        frac = np.stack([(bins <= 15).sum(0), ((bins >= 16) & (bins <= 25)).sum(0), (bins >= 26).sum(0)]) / total
        assert np.array_equal(w, frac)
        m = alg.mass_between(-10.0, 12.0, temperature=t).numpy()
        assert np.array_equal(m, ((bins >= 11) & (bins <= 32)).sum(0) / total)
        with pytest.raises(ValueError, match="nearest edges"):
            alg.mass_between(-10.5, 12.0, temperature=t)
        assert np.allclose(alg.marginal_density(t).sum(1).numpy(), alg.mass_between(-20.0, 20.0, temperature=t).numpy())
    info = alg.get_diagnostic_info()
    assert info["hist_out_of_range"] == (want[..., 0].sum() + want[..., -1].sum()) / want.sum()
    # without hist nothing changes: the same run, the same diagnostics but for the one new key
    off = pt()
    off.generate_samples(N)
    assert torch.equal(off._run.state, alg._run.state) and torch.equal(off._run.logp, alg._run.logp)
    assert torch.equal(off._run.n_accept, alg._run.n_accept) and torch.equal(off._run.swap_accept, alg._run.swap_accept)
    assert torch.equal(off._trace, alg._trace)
    assert set(info) - set(off.get_diagnostic_info()) == {"hist_out_of_range"}
    with pytest.raises(RuntimeError, match="hist="):
        off.marginal_histogram()
    # reset(): the arrays read zero, the next run counts from zero
    alg.reset()
    assert int(alg.marginal_histogram()[0].sum()) == 0
    alg.generate_samples(N)
    assert np.array_equal(alg.marginal_histogram(0)[0].numpy(), want[0])
    # the RWM class: one temperature, many chains
    rwm = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, RoughCarpetDistributionTorch(dim, device=device), burn_in=10, device=device,
                                     num_chains=70, seed=5, hist="cold", hist_range=(-20.0, 20.0), hist_bins=8, hist_every=10)
    rwm.generate_samples(50)
    counts, _ = rwm.marginal_histogram()
    assert (counts.sum(1) == 70 * 5).all()  # step counters 20, 30, ..., 60
    assert "hist_out_of_range" in rwm.get_diagnostic_info()
    assert "hist_out_of_range" not in RandomWalkMH_GPU_Optimized(dim, 1.0, RoughCarpetDistributionTorch(dim, device=device), device=device).get_diagnostic_info()


@gpu
def test_quantiles_of_a_standard_normal(device):
    """One test of meaning: 4 096 chains on a standard normal in dim 4, burn-in 500, 1 000 steps, a snapshot every 50 steps,
    240 bins over (-6, 6).  The median and the 97.5 % quantile must be within
        w + 5 sqrt(q (1 - q) / M) / phi(x_q)
    of 0 and 1.960: w the bin width (the interpolation's error), sqrt(q (1 - q) / M) / phi(x_q) the standard error of a sample
    quantile of M independent draws, M = 4 096 - only the chains are taken as independent, the 20 snapshots can only help, so the
    bound is conservative - and 5 of them."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    dim, M = 4, 4096
    alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, MultivariateNormalTorch(dim, device=device), burn_in=500, device=device,
                                     num_chains=M, seed=2024, hist="cold", hist_range=(-6.0, 6.0), hist_bins=240, hist_every=50)
    alg.generate_samples(1000)
    counts, edges = alg.marginal_histogram()
    assert (counts.sum(1) == M * 20).all()  # step counters 550, 600, ..., 1500
    q = alg.quantiles([0.5, 0.975]).numpy()
    w = 12.0 / 240

    def phi(x):
        return math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)

    for i, (qv, xq) in enumerate(((0.5, 0.0), (0.975, 1.959964))):
        bound = w + 5.0 * math.sqrt(qv * (1.0 - qv) / M) / phi(xq)
        print(f"q = {qv}: quantiles {q[i]}, bound {bound:.4f} around {xq}")
        assert np.all(np.abs(q[i] - xq) <= bound), (qv, q[i], bound)
    assert alg.get_diagnostic_info()["hist_out_of_range"] < 1e-3
