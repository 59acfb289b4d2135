"""Device-side state of a sampler run and the calls into the fused HIP kernel.

Shared by `RandomWalkMH_GPU_Optimized` (one temperature) and `ParallelTemperingRWM_GPU_Optimized`
(a ladder).  Layout in HBM (all contiguous, row-major):

    state        float32 [n_replicas, n_temps, dim]   the replicas' current points
    logp         float32 [n_replicas, n_temps]        their log-densities
    n_accept     int64   [n_replicas, n_temps]        MH acceptances after burn-in
    sq_jump      float64 [n_replicas, n_temps]        sum of squared jump distances after burn-in
    swap_accept  int64   [n_replicas, n_temps]        accepted swaps of pair (t, t+1)
    last_ord     int64   [n_replicas, n_temps]        attempt ordinal of the pair's last accepted swap

and, when moments are on (moments_temps > 0), ONE set of accumulators (`_mom`, a dict) with the leading shape L = () -
pooled over every replica of the shard (include/ptrwm.h ptrwm_moments_args) - or, with moments_per_chain, L = (n_replicas,) -
kept apart per replica (ptrwm_chain_moments_args; deterministic sums):

    sum      float64 [*L, moments_temps, dim]         sum of x over the accumulated steps
    sum_sq   float64 [*L, moments_temps, dim]         sum of x^2
    sum_logp float64 [*L, moments_temps]              sum of the log-density
    count    int64   [moments_temps]                  pooled: (replica, step) pairs added; per replica: accumulated steps

and, with flow=True, the replica-flow arrays (`_flow`, a dict; include/ptrwm.h ptrwm_flow_args), updated at every swap event:

    walker       int32   [n_replicas, n_temps]        flow word of every position: walker id | direction << 16
    round_trips  int64   [n_replicas, n_temps]        completed cold -> hot -> cold trips, by walker id
    n_up, n_down int64   [n_replicas, n_temps]        visits by replicas that last touched the cold / the hot end

and, with hist_temps > 0, the pooled marginal histograms (`_hist`, a dict; include/ptrwm.h ptrwm_hist_args), added to by a
snapshot kernel between launches at every hist_every-th step past burn-in (the bin rule's constants lo, scale - float32 [dim],
csrc/hist.h - are the plan's):

    counts       int64   [hist_temps, dim, hist_bins + 2]   bin 0 underflow (and NaN), bin hist_bins + 1 overflow
    count        int64   [hist_temps]                       (replica, step) pairs added per temperature

and, with adapt_scale=True, the arrays of the warm-up tuning of the proposal scale (`_adapt`, a WarmupTuning; include/ptrwm.h
ptrwm_adapt_args), used by two small kernels between launches at the end of every adaptation window of burn-in:

    window_accept  int64   [n_replicas, n_temps]      acceptances of the current window (scratch, zero between windows)
    pooled         int64   [n_temps + 1]              their sum over replicas, and the window's chain-steps (zero between windows)
    scale_history  float32 [K + 1, n_temps]           the scales before the first and after every window (NaN: not run yet)
    accept_history int64   [K, n_temps]               pooled acceptances of every window

and, with adapt_ladder=True, the arrays of the warm-up tuning of the ladder (`_ladder`, a WarmupTuning; include/ptrwm.h
ptrwm_ladder_args), used by two more small kernels between launches - a probe behind every probe step, an update at the end of
every window - which rewrite `beta` (the run's own tensor) and the run's copy of the scales in place:

    pooled         int64   [n_temps]                  quantised swap probabilities per pair, chain-probes last (zero between windows)
    beta_history   float32 [K + 1, n_temps]           the ladder before the first and after every window (NaN: not run yet)
    rate_history   int64   [K, n_temps]               the pooled row of every window
    skipped        int64   [1]                        updates dropped (two rungs would have rounded onto each other)

and, with acf_temps > 0, the pooled lagged autocovariance (`_acf`, a dict; include/ptrwm.h ptrwm_acf_args, csrc/acf.h), added to
by a snapshot kernel between launches at every acf_every-th step past burn-in, with `_acf_ring`, the last acf_max_lag snapshots
(scratch, the state's dtype, [acf_max_lag, n_replicas, acf_temps, dim]):

    sxy, head, tail  float64 [acf_temps, acf_max_lag + 1, dim]   sums of x_j x_{j-k}, of x_j and of x_{j-k} over replicas and snapshots
    pairs            int64   [acf_max_lag + 1]                   (replica, snapshot) pairs added per lag

and, with cov_temps > 0, the pooled posterior covariance sums (`_cov`, a dict; include/ptrwm.h ptrwm_cov_args, csrc/cov.h), added
to by a snapshot kernel between launches at every cov_every-th step past burn-in:

    sxx    float64 [cov_temps, dim, dim]   sums of x_i x_j over replicas and snapshots, the lower triangle (j <= i) only
    sx     float64 [cov_temps, dim]        sums of x_i
    count  int64   [1]                     (replica, snapshot) pairs added

and, with energy=True, the pooled log-density sums along the ladder (`_energy`, a dict; include/ptrwm.h ptrwm_energy_args,
csrc/energy.h), added to by two small kernels between launches at every energy_every-th step past burn-in, per group g of chains
(global replica id mod energy_groups), with `_energy_ref` [n_temps] float64, the level the exponential sums are taken against, and
`_energy_ref_set` [1] int32, its flag:

    count           int64   [groups, n_temps]   finite log-densities added
    s1, s2          float64 [groups, n_temps]   sums of l and of l^2
    colder, hotter  float64 [groups, n_temps]   sums of exp((beta[t -+ 1] - beta[t]) (l - ref[t])); column 0 / n_temps - 1 unused
    nonfinite       int64   [1]                 log-densities that were not finite (added nowhere else)

`n_replicas` is the axis the reference does not have: independent copies of the whole chain /
ladder, one Philox subsequence each (global replica id = chain_offset + local index), so a run is
invariant to how replicas are sharded over GPUs.
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence

import numpy as np
import torch

import ptrwm_hip


def resolve_device(device) -> torch.device:
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    return torch.device(device)


def draw_seed() -> int:
    """A Philox key from torch's global CPU generator: `torch.manual_seed(s)` (which the harness calls
    after constructing the sampler, interfaces/simulation_gpu.py) therefore fixes the whole run."""
    return int(torch.randint(0, 2**62, (1,)).item())


# ---- starting points ------------------------------------------------------------------------------------------
def start_shape(initial_state, dim: int, n_replicas: int, n_temps: int) -> int:
    """Number of axes of a start: 1 for one point [dim] shared by every row, 2 for [n_replicas, dim] (the temperatures of a
    ladder share their replica's row), 3 for [n_replicas, n_temps, dim].  NumPy array, sequence or torch tensor on any
    device; ValueError for any other shape.  Host-only."""
    shape = tuple(initial_state.shape) if torch.is_tensor(initial_state) else np.asarray(initial_state).shape
    for want in ((dim,), (n_replicas, dim), (n_replicas, n_temps, dim)):
        if shape == want:
            return len(want)
    raise ValueError(f"starting states must have shape [{dim}], [{n_replicas}, {dim}] or [{n_replicas}, {n_temps}, {dim}] "
                     f"(dim / replicas, dim / replicas, temperatures, dim), got {list(shape)}")


def check_init_box(init_box, dim: int) -> Optional[tuple]:
    """`init_box` = (lo, hi), each bound a scalar or a [dim] vector, as two float32 [dim] arrays; None stays None.
    ValueError unless both are finite and lo <= hi element-wise.  Host-only."""
    if init_box is None:
        return None
    try:
        lo, hi = init_box
    except (TypeError, ValueError):
        raise ValueError("init_box must be a pair (lo, hi)") from None
    out = []
    for name, b in (("lo", lo), ("hi", hi)):
        b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
        if b.shape not in ((), (dim,)):
            raise ValueError(f"init_box: {name} must be a scalar or a [{dim}] vector, got shape {list(b.shape)}")
        if not np.all(np.isfinite(b)):
            raise ValueError(f"init_box: {name} must be finite")
        out.append(np.ascontiguousarray(np.broadcast_to(b, (dim,)).astype(np.float32)))
    if not np.all(out[0] <= out[1]):
        raise ValueError("init_box: lo <= hi must hold in every coordinate")
    return out[0], out[1]


def check_hist_range(hist_range, dim: int) -> tuple:
    """`hist_range` = (lo, hi), each bound a scalar or a [dim] vector, as two float32 [dim] arrays.  ValueError unless both are
    finite and lo < hi element-wise AFTER rounding to float32 (the bin rule divides by their float32 difference).  Host-only."""
    try:
        lo, hi = hist_range
    except (TypeError, ValueError):
        raise ValueError("hist_range must be a pair (lo, hi)") from None
    out = []
    for name, b in (("lo", lo), ("hi", hi)):
        b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
        if b.shape not in ((), (dim,)):
            raise ValueError(f"hist_range: {name} must be a scalar or a [{dim}] vector, got shape {list(b.shape)}")
        if not np.all(np.isfinite(b)):
            raise ValueError(f"hist_range: {name} must be finite")
        out.append(np.ascontiguousarray(np.broadcast_to(b, (dim,)).astype(np.float32)))
    if not np.all(np.isfinite(out[0])) or not np.all(np.isfinite(out[1])) or not np.all(out[0] < out[1]):
        raise ValueError("hist_range: lo < hi must hold in every coordinate")
    return out[0], out[1]


def hist_scale(lo: np.ndarray, hi: np.ndarray, n_bins: int) -> np.ndarray:
    """scale[d] of the bin rule (csrc/hist.h): float32(n_bins) / (float32(hi) - float32(lo)), every operation in float32."""
    return (np.float32(n_bins) / (hi.astype(np.float32) - lo.astype(np.float32))).astype(np.float32)


def hist_edges(lo: np.ndarray, hi: np.ndarray, n_bins: int) -> torch.Tensor:
    """The n_bins + 1 edges of every coordinate, float64 [dim, n_bins + 1] (CPU): lo + i (hi - lo) / n_bins of the float32 bounds."""
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    i = np.arange(n_bins + 1, dtype=np.float64)
    e = lo64[:, None] + i[None, :] * ((hi64 - lo64) / n_bins)[:, None]
    e[:, -1] = hi64
    return torch.from_numpy(e)


def check_hist_args(hist_temps, hist_every, hist_bins, hist_range, n_temps: int, dim: int):
    """EngineRun's histogram arguments (no GPU needed): None when off, else (lo, hi) as float32 arrays."""
    for name, v in (("hist_temps", hist_temps), ("hist_every", hist_every), ("hist_bins", hist_bins)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 0 <= hist_temps <= n_temps:
        raise ValueError(f"hist_temps must be in 0..{n_temps}, got {hist_temps}")
    if not hist_temps:
        return None
    if hist_every < 1:
        raise ValueError(f"hist_every must be >= 1, got {hist_every}")
    if not 1 <= hist_bins <= ptrwm_hip.HIST_MAX_BINS:
        raise ValueError(f"hist_bins must be in 1..{ptrwm_hip.HIST_MAX_BINS}, got {hist_bins}")
    if hist_range is None:
        raise ValueError("histograms need hist_range=(lo, hi): the range the bins cover (there are no adaptive ranges)")
    return check_hist_range(hist_range, dim)


def _integer(name, v, lo: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def _number(name, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check_warmup_args(flag: str, name: str, burn_in: int, every, until, adapt_sync, synced: str, idle: str, own) -> dict:
    """What the arguments of the three warm-up tunings share (`flag` switches the tuning on, `name` prefixes its keywords): an
    integer period, `until` in 0..burn_in (default: burn_in), adapt_sync None or a callable (applied to `synced`), windows =
    until // every, and a warning when that is none (the tuning is `idle`).  `own(every)` checks the tuning's other arguments
    once the period stands - they are reported after `until` and before adapt_sync - and returns their entries of the dict."""
    every = _integer(f"{name}_every", every, 1)
    if until is None:
        until = burn_in
    if isinstance(until, bool) or not isinstance(until, (int, np.integer)) or not 0 <= until <= burn_in:
        raise ValueError(f"{name}_until must be an integer in 0..burn_in = {burn_in}, got {until!r}")
    rest = own(every)
    if adapt_sync is not None and not callable(adapt_sync):
        raise ValueError(f"adapt_sync must be None or a callable applied to the {synced}")
    windows = int(until) // every
    if windows == 0:
        warnings.warn(f"{flag}=True but no window of {name}_every = {every} steps ends within the first "
                      f"{until} burn-in steps: {idle}")
    return {"every": every, "until": int(until), "sync": adapt_sync, "windows": windows, **rest}


def _gain_decay(name: str, gain, decay) -> dict:
    """... of the scale's and the ladder's tuning: a finite gain > 0, a decay in 0..1"""
    g, d = _number(f"{name}_gain", gain), _number(f"{name}_decay", decay)
    if not g > 0.0:
        raise ValueError(f"{name}_gain must be positive, got {gain!r}")
    if not 0.0 <= d <= 1.0:
        raise ValueError(f"{name}_decay must lie in 0..1, got {decay!r}")
    return {"gain": g, "decay": d}


def _probe_every(name: str, every: int, probe_every) -> dict:
    """... of the ladder's and the factor's tuning: the probe period, an integer >= 1 that divides the window (default: the window)"""
    probe = every if probe_every is None else _integer(f"{name}_probe_every", probe_every, 1)
    if every % probe != 0:
        raise ValueError(f"{name}_probe_every must divide {name}_every = {every}, got {probe_every!r}")
    return {"probe_every": probe}


def check_adapt_args(adapt_scale, burn_in: int, adapt_every=50, adapt_until=None, adapt_target=0.234, adapt_gain=3.0,
                     adapt_decay=0.5, adapt_scale_bounds=(1e-6, 1e6), adapt_sync=None) -> Optional[dict]:
    """The warm-up tuning arguments of EngineRun and the sampler classes (no GPU needed): None when off, else a dict with
    every / until / target / gain / decay / bounds / sync and windows = until // every.  ValueError for anything the library
    would refuse (include/ptrwm.h ptrwm_adapt_args); a warning when no window fits into burn-in."""
    if not isinstance(adapt_scale, (bool, np.bool_)):
        raise ValueError(f"adapt_scale must be True or False, got {adapt_scale!r}")
    if not adapt_scale:
        return None

    def own(every):
        target = _number("adapt_target", adapt_target)
        if not 0.0 < target < 1.0:
            raise ValueError(f"adapt_target must lie in (0, 1), got {adapt_target!r}")
        try:
            lo, hi = adapt_scale_bounds
        except (TypeError, ValueError):
            raise ValueError("adapt_scale_bounds must be a pair (lo, hi) of factors on the initial scales") from None
        lo, hi = _number("adapt_scale_bounds lo", lo), _number("adapt_scale_bounds hi", hi)
        if not 0.0 < lo <= hi:
            raise ValueError(f"adapt_scale_bounds must satisfy 0 < lo <= hi, got {adapt_scale_bounds!r}")
        return {"target": target, "bounds": (lo, hi), **_gain_decay("adapt", adapt_gain, adapt_decay)}

    return check_warmup_args("adapt_scale", "adapt", int(burn_in), adapt_every, adapt_until, adapt_sync,
                             "pooled [n_temps + 1] int64 tensor", "nothing will adapt", own)


def check_ladder_args(adapt_ladder, burn_in: int, beta_ladder=None, ladder_every=100, ladder_until=None, ladder_probe_every=None,
                      ladder_gain=2.0, ladder_decay=0.5, adapt_sync=None) -> Optional[dict]:
    """The arguments of the warm-up tuning of the temperature ladder (None: off), checked on the host so that bad arguments
    fail the same way with and without a GPU - what the library would refuse (include/ptrwm.h ptrwm_ladder_args) plus what it
    cannot see: a ladder of at least 3 temperatures, positive and strictly decreasing in float32.  A warning when no window
    fits into burn-in."""
    if not isinstance(adapt_ladder, (bool, np.bool_)):
        raise ValueError(f"adapt_ladder must be True or False, got {adapt_ladder!r}")
    if not adapt_ladder:
        return None

    def own(every):
        probe = _probe_every("ladder", every, ladder_probe_every)
        if beta_ladder is not None:
            b = np.asarray(list(beta_ladder), np.float32)
            if b.size < 3:
                raise ValueError(f"adapt_ladder=True moves the interior temperatures: beta_ladder needs at least 3, got {b.size}")
            if not (b > 0).all() or not (b[:-1] > b[1:]).all():
                raise ValueError("adapt_ladder=True needs a beta_ladder that is positive and strictly decreasing in float32")
        return {**probe, **_gain_decay("ladder", ladder_gain, ladder_decay)}

    return check_warmup_args("adapt_ladder", "ladder", int(burn_in), ladder_every, ladder_until, adapt_sync,
                             "pooled int64 tensor", "the ladder will not move", own)


def check_proposal_cov(proposal_cov, dim: int) -> Optional[np.ndarray]:
    """`proposal_cov` (None: no factor), a [dim, dim] symmetric positive-definite covariance as a NumPy array or a tensor,
    factored on the host in float64: the lower-triangular float32 factor L, L L^T = proposal_cov, zeros above the diagonal.
    ValueError for a wrong shape, a matrix that is not symmetric (beyond 1e-6 of its largest entry) or not positive definite."""
    if proposal_cov is None:
        return None
    c = proposal_cov.detach().cpu().numpy() if torch.is_tensor(proposal_cov) else np.asarray(proposal_cov)
    if c.shape != (dim, dim):
        raise ValueError(f"proposal_cov must be a [dim, dim] = [{dim}, {dim}] matrix, got shape {tuple(c.shape)}")
    c = np.asarray(c, np.float64)
    if not np.isfinite(c).all() or np.abs(c - c.T).max() > 1e-6 * np.abs(c).max():
        raise ValueError("proposal_cov must be symmetric (and finite)")
    try:
        chol = np.linalg.cholesky((c + c.T) / 2)
    except np.linalg.LinAlgError:
        raise ValueError("proposal_cov must be positive definite") from None
    with np.errstate(over="ignore"):
        out = np.tril(chol).astype(np.float32)
    if not np.isfinite(out).all() or not (np.diagonal(out) > 0).all():
        raise ValueError("proposal_cov must be positive definite in float32")
    return out


def check_proposal_chol(proposal_chol, dim: int) -> Optional[np.ndarray]:
    """EngineRun's `proposal_chol` (None: no factor): a [dim, dim] factor, read on its lower triangle, as float32 with zeros
    above the diagonal.  ValueError for a wrong shape, an entry that is not finite or a diagonal that is not positive."""
    if proposal_chol is None:
        return None
    c = proposal_chol.detach().cpu().numpy() if torch.is_tensor(proposal_chol) else np.asarray(proposal_chol)
    if c.shape != (dim, dim):
        raise ValueError(f"proposal_chol must be a [dim, dim] = [{dim}, {dim}] matrix, got shape {tuple(c.shape)}")
    low = np.tril_indices(dim)
    out = np.zeros((dim, dim), np.float32)
    out[low] = np.asarray(c, np.float32)[low]  # (whatever stands above the diagonal is never read)
    if not np.isfinite(out).all() or not (np.diagonal(out) > 0).all():
        raise ValueError("proposal_chol must be finite on its lower triangle with a positive diagonal")
    return out


def check_cov_adapt_args(adapt_cov, burn_in: int, dim: int, cov_adapt_every=200, cov_adapt_until=None, cov_adapt_probe_every=None,
                         cov_adapt_memory=0.5, cov_adapt_jitter=1e-6, cov_adapt_min_count=None, adapt_sync=None) -> Optional[dict]:
    """The arguments of the warm-up tuning of the proposal factor (None: off), checked on the host so that bad arguments fail the
    same way with and without a GPU - what the library would refuse (include/ptrwm.h ptrwm_precond_update_args) and a probe
    period that does not divide the window.  A warning when no window fits into burn-in."""
    if not isinstance(adapt_cov, (bool, np.bool_)):
        raise ValueError(f"adapt_cov must be True or False, got {adapt_cov!r}")
    if not adapt_cov:
        return None

    def own(every):
        probe = _probe_every("cov_adapt", every, cov_adapt_probe_every)
        memory, jitter = _number("cov_adapt_memory", cov_adapt_memory), _number("cov_adapt_jitter", cov_adapt_jitter)
        if not 0.0 < memory <= 1.0:
            raise ValueError(f"cov_adapt_memory must lie in (0, 1], got {cov_adapt_memory!r}")
        if jitter < 0.0:
            raise ValueError(f"cov_adapt_jitter must be >= 0, got {cov_adapt_jitter!r}")
        min_count = float(4 * dim) if cov_adapt_min_count is None else _number("cov_adapt_min_count", cov_adapt_min_count)
        if not min_count >= 1.0:
            raise ValueError(f"cov_adapt_min_count must be >= 1, got {cov_adapt_min_count!r}")
        return {**probe, "memory": memory, "jitter": jitter, "min_count": min_count}

    return check_warmup_args("adapt_cov", "cov_adapt", burn_in, cov_adapt_every, cov_adapt_until, adapt_sync,
                             "window's covariance sums", "the proposal factor will not move", own)


def check_init_attempts(init_attempts) -> int:
    if isinstance(init_attempts, bool) or not isinstance(init_attempts, (int, np.integer)) or not 1 <= init_attempts <= 65535:
        raise ValueError(f"init_attempts must be an integer in 1..65535, got {init_attempts!r}")
    return int(init_attempts)


def check_class_starts(dim: int, n_replicas: int, n_temps: int, initial_states, init_box, init_attempts,
                       init_per_temperature: bool = False) -> tuple:
    """The constructor checks the sampler classes share (no GPU needed): returns (mode, states, box) with mode "point" /
    "states" / "box", `states` a private copy of `initial_states` (the caller may go on changing the original - e.g. the
    live `current_states` of an earlier sampler) and `box` the float32 bounds."""
    check_init_attempts(init_attempts)
    box = check_init_box(init_box, dim)
    if initial_states is not None and box is not None:
        raise ValueError("initial_states and init_box exclude each other: the starts are given, or drawn from the box")
    if init_per_temperature and box is None:
        raise ValueError("init_per_temperature=True needs init_box (it chooses how the box is drawn from)")
    if initial_states is not None:
        if not torch.is_tensor(initial_states):
            initial_states = np.array(initial_states)
        start_shape(initial_states, dim, n_replicas, n_temps)
        states = initial_states.detach().clone() if torch.is_tensor(initial_states) else initial_states
        return "states", states, None
    return ("box" if box is not None else "point"), None, box


class WarmupTuning:
    """One warm-up tuning of a run, as the host loop sees it: windows of `every` steps that end at or before
    `until`, the last of them at step `end`.  Split steps stop every `cut_every` steps of an adapting window - the window for the
    scale, the probe period for the ladder and the factor - and call `probe(step)` there where the tuning has one; every window
    ends with window_end.  `sync` is the caller's all-reduce (None: the library updates by itself), applied to each tensor of
    `synced`, the window's counts on the device; `reduce` (None: the launch has done it) sums per-replica scratch into them,
    `update(window)` is the plan's stand-alone update kernel, `after_sync(tuning, window)` what only this tuning records of the
    synced counts.  `warm_steps`: the split steps inside its windows follow the warm-up recipe (RunPlan.split_warmup).  The tuning's
    arrays are attributes."""

    def __init__(self, args: dict, update, synced: tuple, *, cut_every: Optional[int] = None, probe=None, reduce=None,
                 after_sync=None, warm_steps: bool = False, **arrays):
        self.every, self.until, self.end, self.sync = args["every"], args["until"], args["windows"] * args["every"], args["sync"]
        self.cut_every = self.every if cut_every is None else cut_every
        self.probe, self.reduce, self.update, self.synced, self.after_sync = probe, reduce, update, synced, after_sync
        self.warm_steps = warm_steps
        self.__dict__.update(arrays)

    def window_end(self, window: int) -> None:
        """What follows the last step of adapting window `window` where the library does not do it itself (split steps; with
        adapt_sync): the reduction, the caller's all-reduce of the window's counts, the update kernel."""
        if self.reduce is not None:
            self.reduce()
        if self.sync is not None:
            for t in self.synced:
                self.sync(t)
            if self.after_sync is not None:
                self.after_sync(self, window)
        self.update(window)


class EngineRun:
    """`initial_state`: one point [dim] for every replica and temperature, or [n_replicas, dim] (the temperatures of a ladder
    share their replica's row), or [n_replicas, n_temps, dim] - a NumPy array or a torch tensor on any device (a device tensor
    is copied on the device); the log-densities are evaluated from the states either way.

    `init_box` = (lo, hi), each a scalar or a [dim] vector: over-dispersed starts drawn by the library (include/ptrwm.h
    ptrwm_init_states: Philox stream 3, keyed by seed and global replica id, so a sharded run starts exactly where the
    unsharded one does).  Attempt 0 draws every row; attempts 1 .. init_attempts - 1 redraw the rows whose log-density is not
    finite (starts outside the target's support); what is still outside after that is put on `initial_state` (the one point).
    Then ONE host synchronisation - at construction, never in the step loop - checks that every log-density is finite and
    raises ValueError otherwise.  `init_per_temperature`: every temperature of a ladder draws its own point instead of sharing
    the ladder's."""

    def __init__(self, *, target_dist, proposal: "ptrwm_hip.Proposal", beta_ladder: Sequence[float], dim: int,
                 device: torch.device, n_replicas: int, initial_state: np.ndarray, burn_in: int, swap_every: int,
                 swap_mode: str, swap_order: str, seed: Optional[int], chain_offset: int = 0,
                 dtype: torch.dtype = torch.float32, moments_temps: int = 0, moments_every: int = 1,
                 moments_per_chain: bool = False, init_box=None, init_per_temperature: bool = False,
                 init_attempts: int = 8, flow: bool = False, hist_temps: int = 0, hist_every: int = 1, hist_bins: int = 64,
                 hist_range=None, adapt_scale: bool = False, adapt_every: int = 50, adapt_until: Optional[int] = None,
                 adapt_target: float = 0.234, adapt_gain: float = 3.0, adapt_decay: float = 0.5,
                 adapt_scale_bounds=(1e-6, 1e6), adapt_sync=None, adapt_ladder: bool = False, ladder_every: int = 100,
                 ladder_until: Optional[int] = None, ladder_probe_every: Optional[int] = None, ladder_gain: float = 2.0,
                 ladder_decay: float = 0.5, acf_temps: int = 0, acf_every: int = 1, acf_max_lag: int = 32,
                 acf_ring_limit: Optional[int] = None, cov_temps: int = 0, cov_every: int = 1, proposal_chol=None,
                 adapt_cov: bool = False, cov_adapt_every: int = 200, cov_adapt_until: Optional[int] = None,
                 cov_adapt_probe_every: Optional[int] = None, cov_adapt_memory: float = 0.5, cov_adapt_jitter: float = 1e-6,
                 cov_adapt_min_count: Optional[float] = None, energy: bool = False, energy_every: int = 1,
                 energy_groups: int = 16, energy_ref=None):
        adapt = check_adapt_args(adapt_scale, max(0, int(burn_in)), adapt_every, adapt_until, adapt_target, adapt_gain,
                                 adapt_decay, adapt_scale_bounds, adapt_sync)
        ladder = check_ladder_args(adapt_ladder, max(0, int(burn_in)), beta_ladder, ladder_every, ladder_until,
                                   ladder_probe_every, ladder_gain, ladder_decay, adapt_sync)
        # preconditioned proposals x + s_t L z (include/ptrwm.h ptrwm_split_propose_precond): `proposal_chol`, the factor
        # [dim, dim] (lower triangle), and with adapt_cov=True its warm-up tuning from the cold chain's covariance - the factor
        # then starts from `proposal_chol`, or from the identity
        chol = check_proposal_chol(proposal_chol, int(dim))
        factor = check_cov_adapt_args(adapt_cov, max(0, int(burn_in)), int(dim), cov_adapt_every, cov_adapt_until,
                                      cov_adapt_probe_every, cov_adapt_memory, cov_adapt_jitter, cov_adapt_min_count, adapt_sync)
        if factor is not None and chol is None:
            chol = np.eye(int(dim), dtype=np.float32)
        if chol is not None:
            if proposal is not None and proposal.kind != ptrwm_hip.PROPOSAL_NORMAL:
                raise ValueError("proposal_chol / adapt_cov precondition the Normal proposal: Laplace and UniformRadius have no "
                                 "preconditioned form")
            if dtype == torch.float64:
                raise NotImplementedError("dtype=torch.float64 needs the fused kernel; preconditioned proposals run in split "
                                          "steps, which carry float32 states")
        if swap_mode not in ptrwm_hip.SWAP_MODES:
            raise ValueError(f"swap_mode must be one of {sorted(ptrwm_hip.SWAP_MODES)}, got {swap_mode!r}")
        if swap_order not in ptrwm_hip.SWAP_ORDERS:
            raise ValueError(f"swap_order must be one of {sorted(ptrwm_hip.SWAP_ORDERS)}, got {swap_order!r}")
        if n_replicas < 1:
            raise ValueError("number of replicas must be >= 1")
        n_temps = len(beta_ladder)
        if flow and n_temps < 2:
            raise ValueError("flow=True tracks replicas through a ladder: it needs at least two temperatures")
        if not 1 <= n_temps <= ptrwm_hip.MAX_TEMPS:
            raise ValueError(f"the fused kernel keeps one ladder inside one workgroup: 1..{ptrwm_hip.MAX_TEMPS} "
                             f"temperatures, got {n_temps}")
        if not 1 <= dim <= ptrwm_hip.MAX_DIM:
            raise ValueError(f"dim must be in 1..{ptrwm_hip.MAX_DIM} for the fused kernel, got {dim}")
        hist_box = check_hist_args(hist_temps, hist_every, hist_bins, hist_range, n_temps, dim)
        acf_on = check_acf_args(acf_temps, acf_every, acf_max_lag, n_temps, dim, n_replicas, acf_ring_limit)
        cov_on = check_cov_args(cov_temps, cov_every, n_temps)
        energy_on = check_energy_args(energy, energy_every, energy_groups, energy_ref, n_temps)
        # the starts (host-side checks, before the device is asked for: bad arguments fail the same way without a GPU)
        axes = start_shape(initial_state, dim, n_replicas, n_temps)
        box = check_init_box(init_box, dim)
        attempts = check_init_attempts(init_attempts)
        if box is not None and axes != 1:
            raise ValueError("init_box draws the starts: initial_state must then be the one point [dim] that rows still "
                             "outside the target's support fall back to, not per-replica states")
        if device.type != "cuda":
            raise RuntimeError(
                "The PT-RWM engine runs only on a ROCm GPU (device='cuda'); there is no CPU fallback. "
                f"Requested device: {device}"
            )
        # Targets the fused kernel knows describe themselves (engine_target).  Any other TorchTargetDistribution - a
        # user-defined density, a dense-covariance Gaussian - runs in split steps: HIP kernels for proposal, accept and
        # swap (same Philox streams, same arithmetic) around one device-side `log_density` call per step
        # (the reference calls target.log_density on the proposals the same way, pt_rwm_gpu_optimized.py:551).
        self.density_fn = None
        try:
            self.target = target_dist.engine_target()
        except (NotImplementedError, AttributeError):
            if not callable(getattr(target_dist, "log_density", None)):
                raise TypeError(f"{type(target_dist).__name__} has neither engine_target() nor log_density()")
            self.target = None
            self.density_fn = target_dist.log_density
            warnings.warn(f"{type(target_dist).__name__} has no fused kernel: running split steps (HIP proposal / "
                          "accept / swap kernels around its log_density, three launches per step).")
        # One flag says how the run steps.  Split steps: a density the library has no kernel for, or a proposal factor - the
        # preconditioned proposal is a split-step kernel, and a target that has engine_target() then runs split steps with
        # ptrwm_hip.logdensity as its density (_density).
        self.split = self.density_fn is not None or chol is not None
        if chol is not None and self.density_fn is None:
            warnings.warn("preconditioned proposals run in split steps (HIP proposal / log-density / accept / swap kernels, "
                          "several launches per step), not in the fused step kernel")
        if self.target is not None and not self.split and not (
                ptrwm_hip.has_thread_variant(self.target.kind, proposal.kind, dim)
                or ptrwm_hip.has_quad_variant(self.target.kind, proposal.kind, dim, n_temps)):
            raise ValueError(f"no fused kernel for dim {dim} with a ladder of {n_temps} temperatures: above dim 64 a ladder "
                             "holds at most 128 temperatures (one 512-thread workgroup of the lane-split kernel)")
        if adapt is not None or ladder is not None:
            # the run rewrites its scales in place: a copy of its own (engine_proposal() may hand out a view of the proposal
            # object's tensors, which a reset() must find as they were)
            proposal = ptrwm_hip.Proposal(proposal.kind, proposal.temp_scale.clone(), proposal.dim_scale, proposal.inv_dim)
        self.proposal = proposal
        self.dim, self.n_temps, self.n_replicas = dim, n_temps, n_replicas
        self.device = device
        self.burn_in, self.swap_every = int(burn_in), int(swap_every)
        self.swap_mode = ptrwm_hip.SWAP_MODES[swap_mode]
        self.swap_order = ptrwm_hip.SWAP_ORDERS[swap_order]
        self.seed = draw_seed() if seed is None else int(seed)
        self.chain_offset = int(chain_offset)
        self.steps_done = 0
        self.manual_sweeps = 0  # stand-alone swap events (swap_sweep) performed so far
        self.use_graph = True   # split steps: replay a captured HIP graph where no per-step trace is asked for
        self._graph, self._graph_key, self._graph_failed, self._dstep = None, None, False, None  # (_advance_split_graph)
        self.beta = torch.tensor(list(beta_ladder), device=device, dtype=torch.float32)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"state dtype must be torch.float32 or torch.float64, got {dtype}")
        if dtype == torch.float64 and self.split:
            raise NotImplementedError("dtype=torch.float64 needs a target with a fused kernel (split steps carry float32 "
                                      "states)")
        self.dtype = dtype  # float64: the engine's state_f64 mode (the reference's dtype=torch.float64)
        self.init_mode = "box" if box is not None else ("point" if axes == 1 else "states")
        if torch.is_tensor(initial_state):
            x0 = initial_state.detach().to(device=device, dtype=dtype)  # (a device tensor never visits the host)
        else:
            x0 = torch.as_tensor(np.asarray(initial_state), dtype=dtype).to(device)
        if box is not None:
            self.state = torch.empty(n_replicas, n_temps, dim, device=device, dtype=dtype)
            self.logp = torch.empty(n_replicas, n_temps, device=device, dtype=torch.float32)
        else:
            if axes == 1:
                # every temperature (and replica) starts from the same point (pt_rwm_gpu_optimized.py:478-484)
                self.state = x0.expand(n_replicas, n_temps, dim).contiguous()
            else:
                # a copy of its own: the caller's tensor (the live states of an earlier run, say) is never stepped in place
                self.state = torch.empty(n_replicas, n_temps, dim, device=device, dtype=dtype)
                self.state.copy_(x0[:, None, :] if axes == 2 else x0)
            # (log-densities are float32 in either mode: the density kernels evaluate the state rounded to float)
            self.logp = self._density(self.state.view(-1, dim).to(torch.float32)).view(n_replicas, n_temps).contiguous()
        shape = (n_replicas, n_temps)
        self.n_accept = torch.zeros(shape, device=device, dtype=torch.int64)
        self.sq_jump = torch.zeros(shape, device=device, dtype=torch.float64)
        self.swap_accept = torch.zeros(shape, device=device, dtype=torch.int64)
        self.last_ord = torch.zeros(shape, device=device, dtype=torch.int64)
        # everything ptrwm_run needs that stays fixed for this run, marshalled once (the tensors above are never
        # re-allocated: the kernel updates them in place)
        self._plan = ptrwm_hip.RunPlan(
            self.target, self.proposal, state=self.state, logp=self.logp, beta=self.beta, burn_in=self.burn_in,
            swap_every=self.swap_every, swap_mode=self.swap_mode, swap_order=self.swap_order, seed=self.seed,
            chain_offset=self.chain_offset, n_accept=self.n_accept, sq_jump=self.sq_jump,
            swap_accept=self.swap_accept, last_swap_ordinal=self.last_ord)
        # posterior moments accumulated inside the step kernels (0: off)
        if not 0 <= int(moments_temps) <= n_temps:
            raise ValueError(f"moments_temps must be in 0..{n_temps}, got {moments_temps}")
        if int(moments_every) < 1:
            raise ValueError(f"moments_every must be >= 1, got {moments_every}")
        self.moments_temps, self.moments_every = int(moments_temps), int(moments_every)
        self.moments_per_chain = bool(moments_per_chain)
        if self.moments_per_chain and not self.moments_temps:
            raise ValueError("moments_per_chain needs moments_temps >= 1")
        self._mom = None
        if self.moments_temps:
            # per chain, the per-chain arrays only: the pooled sums are their sum over the replicas (moments())
            mt, lead = self.moments_temps, ((n_replicas,) if self.moments_per_chain else ())
            self._mom = {"sum": torch.zeros(*lead, mt, dim, device=device, dtype=torch.float64),
                         "sum_sq": torch.zeros(*lead, mt, dim, device=device, dtype=torch.float64),
                         "sum_logp": torch.zeros(*lead, mt, device=device, dtype=torch.float64),
                         "count": torch.zeros(mt, device=device, dtype=torch.int64)}
            bind = self._plan.set_chain_moments if self.moments_per_chain else self._plan.set_moments
            bind(self._mom["sum"], self._mom["sum_sq"], sum_logp=self._mom["sum_logp"], count=self._mom["count"],
                 every=self.moments_every)
        # replica flow through the ladder, exchanged next to the rows in every swap event (off: None)
        self._flow = None
        if flow:
            self._flow = {"walker": torch.empty(shape, device=device, dtype=torch.int32),
                          **{k: torch.empty(shape, device=device, dtype=torch.int64) for k in ("round_trips", "n_up", "n_down")}}
            self.reset_flow()
            self._plan.set_flow(self._flow["walker"], self._flow["round_trips"], self._flow["n_up"], self._flow["n_down"])
        # The snapshot accumulators - pooled marginal histograms, lagged autocovariance, posterior covariance, log-density sums
        # along the ladder - each added to by a snapshot kernel between launches.  One description each: the dict of its sums under the attribute's name, zeroed by
        # _reset_snapshot and read out by _snapshot_sums (off: None); scratch - the bin rule's constants, the ring - stays out of it.
        self.hist_temps, self.hist_every, self.hist_bins = int(hist_temps), int(hist_every), int(hist_bins)
        self.acf_temps, self.acf_every, self.acf_max_lag = int(acf_temps), int(acf_every), int(acf_max_lag)
        self.cov_temps, self.cov_every = int(cov_temps), int(cov_every)

        def zeros(*shape, dtype=torch.float64):
            return torch.zeros(*shape, device=device, dtype=dtype)

        self._hist = self._acf = self._cov = self._energy = None
        if hist_box is not None:
            lo, hi = hist_box
            self._hist_edges = hist_edges(lo, hi, self.hist_bins)
            h = self._hist = {"counts": zeros(self.hist_temps, dim, self.hist_bins + 2, dtype=torch.int64),
                              "count": zeros(self.hist_temps, dtype=torch.int64)}
            self._plan.set_histogram(h["counts"], torch.from_numpy(lo).to(device), torch.from_numpy(hist_scale(lo, hi, self.hist_bins)).to(device),
                                     n_bins=self.hist_bins, temps=self.hist_temps, every=self.hist_every, count=h["count"])
        if acf_on:
            L, at = self.acf_max_lag, self.acf_temps
            a = self._acf = {**{k: zeros(at, L + 1, dim) for k in ("sxy", "head", "tail")}, "pairs": zeros(L + 1, dtype=torch.int64)}
            self._acf_ring = torch.empty(L, n_replicas, at, dim, device=device, dtype=dtype)
            self._plan.set_autocorr(self._acf_ring, a["sxy"], a["head"], a["tail"], a["pairs"], every=self.acf_every)
        if cov_on:
            c = self._cov = {"sxx": zeros(self.cov_temps, dim, dim), "sx": zeros(self.cov_temps, dim), "count": zeros(1, dtype=torch.int64)}
            self._plan.set_covariance(c["sxx"], c["sx"], c["count"], every=self.cov_every)
        if energy_on is not None:
            # (the level and its flag stay out of the dict of sums: a reset leaves a pinned level where it is)
            G = self.energy_groups = energy_on["groups"]
            self.energy_every, self._energy_pinned = energy_on["every"], energy_on["ref"] is not None
            e = self._energy = {"count": zeros(G, n_temps, dtype=torch.int64), **{k: zeros(G, n_temps) for k in ("s1", "s2", "colder", "hotter")},
                                "nonfinite": zeros(1, dtype=torch.int64)}
            self._energy_ref, self._energy_ref_set = zeros(n_temps), zeros(1, dtype=torch.int32)
            if self._energy_pinned:
                self._energy_ref.copy_(torch.from_numpy(energy_on["ref"]))
                self._energy_ref_set.fill_(1)
            self._plan.set_energy(e["count"], e["s1"], e["s2"], e["colder"], e["hotter"], ref=self._energy_ref,
                                  ref_set=self._energy_ref_set, nonfinite=e["nonfinite"], every=self.energy_every)
        # The warm-up tunings (WarmupTuning, each None when off), in the order the host loop serves them - the library's own:
        # the scale's update and the ladder's rescaling both write temp_scale, and the fused loop runs the scale's kernels
        # before the ladder's.  `beta` and `chol` are the run's own tensors: the update kernels rewrite them in place (so
        # captured blocks of split steps keep working).
        self.init_scales = self.proposal.temp_scale.clone()
        self._adapt = self._scale_tuning(adapt)
        self.init_beta = self.beta.clone()
        self._ladder = self._ladder_tuning(ladder)
        self.chol = self.init_chol = None  # the proposal factor (off: None)
        if chol is not None:
            self.chol = torch.from_numpy(chol).to(device)
            self.init_chol = self.chol.clone()
            self._plan.set_preconditioner(self.chol)
        self._factor = self._factor_tuning(factor)
        self._tunings = [tu for tu in (self._adapt, self._ladder, self._factor) if tu is not None]
        if box is not None:
            self._draw_starts(box, x0.to(torch.float32).contiguous(), bool(init_per_temperature), attempts)

    # ---- warm-up tunings: each builder allocates the tuning's arrays, writes row 0 of its history and binds it to the plan --------
    def _scale_tuning(self, adapt: Optional[dict]) -> Optional[WarmupTuning]:
        """... of the proposal scale, per temperature, by two small kernels between launches"""
        if adapt is None:
            return None
        device, n_temps, K, W = self.device, self.n_temps, adapt["windows"], adapt["every"]
        # the bounds are factors on the initial scales; the library clamps every temperature to one range
        tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
        lo = min(max(adapt["bounds"][0] * float(self.init_scales.min().item()), tiny), huge)
        hi = min(max(adapt["bounds"][1] * float(self.init_scales.max().item()), lo), huge)
        pooled = torch.zeros(n_temps + 1, device=device, dtype=torch.int64)

        def record_counts(tu, window):
            tu.count_history[window] = tu.pooled[-1]  # chain-steps of every shard

        tu = WarmupTuning(
            adapt, self._plan.adapt_update, (pooled,), reduce=self._plan.adapt_reduce if self.split else None,
            after_sync=record_counts, warm_steps=True, pooled=pooled,
            window_accept=torch.zeros(self.n_replicas, n_temps, device=device, dtype=torch.int64),
            scale_history=torch.full((K + 1, n_temps), float("nan"), device=device, dtype=torch.float32),
            accept_history=torch.zeros(K, n_temps, device=device, dtype=torch.int64),
            # chain-steps behind every row of accept_history (with adapt_sync: of every shard, recorded)
            count_history=torch.full((K,), 0 if adapt["sync"] is not None else self.n_replicas * W, device=device, dtype=torch.int64))
        tu.scale_history[0] = self.init_scales
        self._plan.set_adaptation(tu.window_accept, pooled, every=W, until=adapt["until"], target=adapt["target"],
                                  gain=adapt["gain"], decay=adapt["decay"], min_scale=lo, max_scale=hi,
                                  defer_update=adapt["sync"] is not None, scale_history=tu.scale_history,
                                  accept_history=tu.accept_history)
        return tu

    def _ladder_tuning(self, ladder: Optional[dict]) -> Optional[WarmupTuning]:
        """... of the temperature ladder, by two more small kernels between launches: a probe and an update"""
        if ladder is None:
            return None
        device, n_temps, K, plan = self.device, self.n_temps, ladder["windows"], self._plan
        pooled = torch.zeros(n_temps, device=device, dtype=torch.int64)
        tu = WarmupTuning(
            ladder, plan.ladder_update, (pooled,), cut_every=ladder["probe_every"], probe=lambda step: plan.ladder_probe(),
            pooled=pooled,
            beta_history=torch.full((K + 1, n_temps), float("nan"), device=device, dtype=torch.float32),
            # row j: the pooled row of window j - pair sums, and chain-probes in the last column
            rate_history=torch.zeros(K, n_temps, device=device, dtype=torch.int64),
            skipped=torch.zeros(1, device=device, dtype=torch.int64))
        tu.beta_history[0] = self.init_beta
        self._plan.set_ladder(pooled, every=ladder["every"], probe_every=ladder["probe_every"], until=ladder["until"],
                              gain=ladder["gain"], decay=ladder["decay"], rescale_scales=True,
                              defer_update=ladder["sync"] is not None, beta_history=tu.beta_history,
                              rate_history=tu.rate_history, skipped=tu.skipped)
        return tu

    def _factor_tuning(self, factor: Optional[dict]) -> Optional[WarmupTuning]:
        """... of the proposal factor, by a covariance probe of temperature 0 and one update kernel between steps.  There is no
        pooled row: the window's counts are the covariance sums sxx, sx, count - the tuning's own, never the user's cov= ones."""
        if factor is None:
            return None
        device, dim, K = self.device, self.dim, factor["windows"]
        f64 = lambda *s: torch.zeros(*s, device=device, dtype=torch.float64)  # noqa: E731
        sums = {"sxx": f64(dim, dim), "sx": f64(dim), "count": torch.zeros(1, device=device, dtype=torch.int64)}
        tu = WarmupTuning(
            factor, self._plan.precond_update, tuple(sums.values()), cut_every=factor["probe_every"],
            probe=self._plan.precond_probe, **sums,
            run_xx=f64(dim, dim), run_x=f64(dim), run_w=f64(1),  # the running triple
            chol_history=torch.full((K + 1, dim, dim), float("nan"), device=device, dtype=torch.float32),
            weight_history=torch.full((K,), float("nan"), device=device, dtype=torch.float64),
            skipped=torch.zeros(1, device=device, dtype=torch.int64))
        tu.chol_history[0] = self.init_chol
        self._plan.set_precond_update(tu.sxx, tu.sx, tu.count, tu.run_xx, tu.run_x, tu.run_w, windows=max(K, 1),
                                      probe_every=factor["probe_every"], memory=factor["memory"], jitter=factor["jitter"],
                                      min_count=factor["min_count"], chol_history=tu.chol_history if K else None,
                                      weight_history=tu.weight_history if K else None, skipped=tu.skipped)
        return tu

    def proposal_factor(self) -> Optional[torch.Tensor]:
        """The current proposal factor: float32 [dim, dim] on the device, zeros above the diagonal (a copy); None without one."""
        return None if self.chol is None else torch.tril(self.chol)

    def preconditioner_history(self) -> Optional[dict]:
        """None when the factor's tuning is off, else "factors" float32 [K + 1, dim, dim] (row 0 the initial factor, row k + 1
        the one in force behind window k; NaN for windows that have not run), "weights" float64 [K] (the running weight w after
        window k; NaN likewise) and "skipped", the updates dropped.  Device tensors."""
        if self._factor is None:
            return None
        fa = self._factor
        return {"factors": fa.chol_history.clone(), "weights": fa.weight_history.clone(), "skipped": int(fa.skipped.item())}

    def _draw_starts(self, box: tuple, point: torch.Tensor, per_temperature: bool, attempts: int) -> None:
        """Starts from the box (class docstring): attempt 0 for every row, a redraw per further attempt for the rows the
        density rejects, `point` for what is left - all enqueued; then the one synchronising check."""
        lo, hi = (torch.from_numpy(b).to(self.device) for b in box)

        def evaluate():
            rows = self.state.view(-1, self.dim).to(torch.float32)
            self.logp.copy_(self._density(rows).view(self.n_replicas, self.n_temps))

        self._plan.init_states(lo, hi, attempt=0, per_temperature=per_temperature)
        evaluate()
        for a in range(1, attempts):
            self._plan.init_states(lo, hi, attempt=a, per_temperature=per_temperature)
            evaluate()
        self._plan.init_states(lo, hi, attempt=attempts, per_temperature=per_temperature, fallback=point)
        evaluate()
        bad = int((~torch.isfinite(self.logp)).sum().item())
        if bad:
            raise ValueError(f"{bad} of {self.logp.numel()} starting rows have no finite log-density after {attempts} "
                             "draw(s) from init_box and the fallback to initial_state: neither the box nor the point "
                             "lies in the target's support")

    def _density(self, rows: torch.Tensor) -> torch.Tensor:
        """log-density of every row [n, dim] -> float32 [n] on the device."""
        if self.density_fn is None:
            return ptrwm_hip.logdensity(self.target, rows)
        out = self.density_fn(rows)
        if not torch.is_tensor(out) or out.shape != (rows.shape[0],):
            raise ValueError("log_density must map a [n, dim] device tensor to a [n] tensor")
        if not out.is_cuda:
            raise RuntimeError("log_density returned a CPU tensor: a split-step target must evaluate on the GPU "
                               "(there is no CPU path)")
        return out.to(torch.float32).contiguous()

    # ---- stepping ---------------------------------------------------------------------------
    def traced_rows(self, n_steps: int, every: int) -> int:
        """Rows a trace with thinning period `every` receives from the next n_steps steps."""
        return ptrwm_hip.periodic_steps_in(self.steps_done, self.steps_done + n_steps, every)

    def advance(self, n_steps: int, trace: Optional[torch.Tensor] = None, trace_logp: Optional[torch.Tensor] = None,
                trace_row0: int = 0, trace_every: int = 1) -> None:
        """Enqueue n_steps fused steps (no host synchronisation)."""
        if n_steps <= 0:
            return
        if self.split:
            self._advance_split(n_steps, trace, trace_logp, trace_row0, max(1, int(trace_every)))
            return
        # adapt_sync: one launch up to the nearest pending window end of any tuning (the library refuses to step past a pending
        # update), the caller's all-reduce of that window's counts and the update in between - in the order of the list where
        # several end at the same step; ordinary launches from the end of warm-up
        while n_steps > 0:
            s, pending = self.steps_done, self._pending_sync()
            if not pending:
                break
            n = min([n_steps] + [tu.every - s % tu.every for tu in pending])
            self._launch(n, trace, trace_logp, trace_row0, trace_every)
            if trace is not None:
                trace_row0 += ptrwm_hip.periodic_steps_in(s, s + n, max(1, int(trace_every)))
            for tu in pending:
                if (s + n) % tu.every == 0:
                    tu.window_end((s + n) // tu.every - 1)
            n_steps -= n
        if n_steps > 0:
            self._launch(n_steps, trace, trace_logp, trace_row0, trace_every)

    def _pending_sync(self) -> list:
        """The tunings that defer their update to the caller and still have a window to end, for fused steps: a proposal factor
        makes every step a split step, so its tuning is never among them."""
        assert not self.split
        return [tu for tu in self._tunings if tu.sync is not None and self.steps_done < tu.end]

    def _launch(self, n_steps, trace, trace_logp, trace_row0, trace_every) -> None:
        if trace is None and trace_logp is None:
            self._plan.launch(self.steps_done, n_steps, swap_event_offset=self.manual_sweeps)
        else:
            self._plan.launch(self.steps_done, n_steps, trace=trace, trace_logp=trace_logp, trace_row0=trace_row0,
                              trace_every=trace_every, swap_event_offset=self.manual_sweeps)
        self.steps_done += n_steps

    def beta_ladder(self) -> torch.Tensor:
        """The current ladder: float32 [n_temps] on the device (a copy)."""
        return self.beta.clone()

    def ladder_history(self) -> Optional[dict]:
        """None when the ladder's tuning is off, else "betas" float32 [K + 1, n_temps] (row 0 the initial ladder, row j + 1 the
        one after window j; NaN for windows that have not run), "rates" float64 [K, n_temps - 1] (every pair's mean swap
        probability over window j, from the integer history; NaN likewise), "probes" int64 [K] (chain-probes behind row j, every
        shard's with adapt_sync), "pooled" the integer rows [K, n_temps] and "skipped" the updates dropped.  Device tensors."""
        if self._ladder is None:
            return None
        ld = self._ladder
        rows = ld.rate_history.clone()
        probes = rows[:, -1]
        return {"betas": ld.beta_history.clone(), "rates": rows[:, :-1].double() / (probes.double()[:, None] * 16777216.0),
                "probes": probes.clone(), "pooled": rows, "skipped": int(ld.skipped.item())}

    # ---- warm-up tuning: read-outs -------------------------------------------------------------------------------
    def proposal_scales(self) -> torch.Tensor:
        """The current per-temperature proposal scales: float32 [n_temps] on the device (a copy)."""
        return self.proposal.temp_scale.clone()

    def adaptation_history(self) -> Optional[dict]:
        """None when adaptation is off, else "scales" float32 [K + 1, n_temps] (row 0 the initial scales, row k + 1 those after
        window k) and "acceptance" float64 [K, n_temps] (the pooled acceptance rate of window k, from the integer history);
        rows of windows that have not run yet are NaN.  Device tensors."""
        if self._adapt is None:
            return None
        ad = self._adapt
        return {"scales": ad.scale_history.clone(),
                "acceptance": ad.accept_history.double() / ad.count_history.double()[:, None],
                "accepted": ad.accept_history.clone()}

    # ---- split steps through a captured HIP graph ------------------------------------------------------------
    # A split step is four launches of this library (proposal, Metropolis rule, swap event, step counter) around the
    # caller's density evaluation.  Issued one by one from Python they cost two ctypes calls plus the density's own torch
    # dispatch per step - tens of microseconds of host time against a few microseconds of kernels for a small batch.  In
    # device-step mode (include/ptrwm.h `device_step`) no argument of those launches depends on the step, so GRAPH_STEPS
    # steps are captured ONCE with torch.cuda.CUDAGraph - the density's kernels included - and replayed.  Same kernels,
    # same Philox words: bit-identical to the eager loop and (with the library's own density) to ptrwm_run.
    GRAPH_STEPS = 16

    def _split_step_on_device_counter(self, offset: int = 0, no_sweep: bool = False, advance: int = 1) -> None:
        """One split step at device step counter + offset; `advance` > 0 adds that much to the counter afterwards."""
        C, T, D = self.n_replicas, self.n_temps, self.dim
        props = self._plan.split_propose(offset)
        lp_new = self._density(props.view(-1, D)).view(C, T)
        self._plan.split_accept(offset, lp_new, swap_event_offset=self.manual_sweeps, no_sweep=no_sweep)
        self._plan.split_snapshots(offset)  # (each bound accumulator decides on the device whether this step counts)
        if advance:
            self._plan.split_advance(advance)

    def _graph_block(self) -> int:
        """Steps per captured block: a multiple of swap_every (>= GRAPH_STEPS) where that is short enough, so that a block
        replayed from a counter that is a multiple of swap_every has its swap steps at FIXED offsets and the swap kernel
        is enqueued only there; GRAPH_STEPS otherwise (the swap kernel then rides with every step and decides on the
        device)."""
        se = int(self.swap_every)
        if self.n_temps < 2 or se > 4 * self.GRAPH_STEPS:
            return self.GRAPH_STEPS
        return se * -(-self.GRAPH_STEPS // se)

    def _advance_split_graph(self, n_steps: int) -> bool:
        """n_steps split steps by graph replay; False if the density cannot be captured (the caller falls back)."""
        if self._graph_failed:
            return False
        if self._dstep is None:
            self._dstep = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._dstep.fill_(self.steps_done)
        self._plan.set_device_step(self._dstep)
        block = self._graph_block()
        aligned = self.n_temps >= 2 and block % int(self.swap_every) == 0  # swap steps sit at fixed offsets of a block
        se = int(self.swap_every)
        try:
            done = 0

            def eager(k):  # k steps, one at a time, on the device counter
                for _ in range(k):
                    self._split_step_on_device_counter()

            key = (self.manual_sweeps, block)  # (baked into the captured launches)
            if self._graph_key != key:
                self._graph = None
            if self._graph is None:
                # one step outside capture first, on a side stream (lazy initialisations of whatever the density calls
                # must not happen while capturing); it is a real step of the run
                cur = torch.cuda.current_stream(self.device)
                side = torch.cuda.Stream(self.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    self._split_step_on_device_counter()
                cur.wait_stream(side)
                done = 1
            if aligned:  # replay only from counters that are multiples of swap_every
                k = min(n_steps - done, (-(self.steps_done + done)) % se)
                eager(k)
                done += k
            if self._graph is None and n_steps - done >= block:
                g = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(g):
                        for j in range(block):
                            # step counter + j has step_counter = counter + j + 1: a swap step iff (j + 1) % swap_every == 0
                            self._split_step_on_device_counter(offset=j, no_sweep=aligned and (j + 1) % se != 0,
                                                               advance=block if j == block - 1 else 0)
                except Exception as e:  # a density that synchronises, allocates outside the pool, ...
                    self._graph_failed = True
                    torch.cuda.synchronize(self.device)
                    warnings.warn(f"split steps: the density could not be captured in a HIP graph ({type(e).__name__}: {e}); "
                                  "running step by step")
                    self._dstep.fill_(self.steps_done + done)
                    eager(n_steps - done)
                    self.steps_done += n_steps
                    return True
                self._graph, self._graph_key = g, key
            while self._graph is not None and n_steps - done >= block:
                self._graph.replay()
                done += block
            eager(n_steps - done)
            self.steps_done += n_steps
            return True
        finally:
            self._plan.set_device_step(None)

    def _advance_split(self, n_steps, trace, trace_logp, trace_row0, trace_every) -> None:
        """n_steps split steps; traced steps (step_counter a multiple of trace_every) are copied with torch."""
        while n_steps > 0:
            # the host loop - and with it every captured block - ends every cut_every steps of an adapting window of each
            # tuning (WarmupTuning); the stand-alone kernels follow in the order of the list, the library's: each tuning's probe
            # and, at a window's end, its reduction and update
            s = self.steps_done
            live = [tu for tu in self._tunings if s < tu.end]
            k = min([n_steps] + [tu.cut_every - s % tu.cut_every for tu in live])
            trace_row0 += (self._split_steps(k, trace, trace_logp, trace_row0, trace_every, warmup=True)
                           if any(tu.warm_steps for tu in live) else
                           self._advance_split_plain(k, trace, trace_logp, trace_row0, trace_every))
            for tu in live:
                if (s + k) % tu.cut_every == 0:
                    if tu.probe is not None:
                        tu.probe(s + k - 1)
                    if (s + k) % tu.every == 0:
                        tu.window_end((s + k) // tu.every - 1)
            n_steps -= k

    def _advance_split_plain(self, n_steps, trace, trace_logp, trace_row0, trace_every) -> int:
        """n_steps ordinary split steps - by graph replay where nothing is traced - and the rows traced."""
        if trace is None and n_steps >= 2 and self.use_graph and self._advance_split_graph(n_steps):
            return 0
        return self._split_steps(n_steps, trace, trace_logp, trace_row0, trace_every)

    def _split_steps(self, n_steps, trace, trace_logp, trace_row0, trace_every, warmup: bool = False) -> int:
        """n_steps eager split steps, and the rows traced.  `warmup`: inside an adapting window of the scale, by the recipe of
        include/ptrwm.h - acceptances counted into the window scratch, no swap event, and nothing for the moments and the
        histograms, which count from the end of burn-in."""
        C, T, D = self.n_replicas, self.n_temps, self.dim
        row = trace_row0
        self._plan.split_warmup(warmup)
        try:
            for _ in range(n_steps):
                s = self.steps_done
                props = self._plan.split_propose(s)
                lp_new = self._density(props.view(-1, D)).view(C, T)
                self._plan.split_accept(s, lp_new, swap_event_offset=self.manual_sweeps)
                if not warmup:
                    self._plan.split_snapshots(s)
                self.steps_done += 1
                if trace is not None and ptrwm_hip.periodic_steps_in(s, s + 1, trace_every):
                    tc, tt = trace.shape[1], trace.shape[2]
                    trace[row] = self.state[:tc, :tt]
                    if trace_logp is not None:
                        trace_logp[row] = self.logp[:tc, :tt]
                    row += 1
        finally:
            self._plan.split_warmup(False)
        return row - trace_row0

    def swap_sweep(self) -> None:
        """One stand-alone swap event over the current states (`_attempt_all_swaps()` called on its own,
        pt_rwm_gpu_optimized.py:594-633; no host synchronisation).  Its uniforms come from Philox stream 2 at
        counter = number of stand-alone sweeps so far, so they never coincide with the fused kernel's."""
        if self.n_temps < 2:
            return
        self._plan.swap_sweep(rng_step=self.manual_sweeps, event_index=self.swap_events(), rng_stream=2)
        self.manual_sweeps += 1

    # ---- summaries (each read synchronises) ---------------------------------------------------
    @property
    def post_burn_steps(self) -> int:
        return ptrwm_hip.periodic_steps_in(0, self.steps_done, 1, self.burn_in)

    def swap_events(self) -> int:
        if self.n_temps < 2:
            return 0
        return ptrwm_hip.periodic_steps_in(0, self.steps_done, self.swap_every, self.burn_in) + self.manual_sweeps

    def swap_attempts_per_replica(self) -> int:
        """Swap attempts one ladder has made so far (deterministic, needs no device read)."""
        ev, T = self.swap_events(), self.n_temps
        if self.swap_order == ptrwm_hip.ORDER_SEQUENTIAL:
            return ev * (T - 1)
        n_even, n_odd = (T - 1 + 1) // 2, (T - 1) // 2  # pairs with even / odd lower index
        # events are numbered from 0: even-numbered events take the even pairs
        return ((ev + 1) // 2) * n_even + (ev // 2) * n_odd

    def moments(self) -> Optional[dict]:
        """The raw moment sums of this shard (device tensors, no synchronisation), or None when moments are off:
        sum / sum_sq [temps, dim] float64, sum_logp [temps] float64, count [temps] int64, every."""
        if not self.moments_temps:
            return None
        m = self._mom
        if self.moments_per_chain:  # pooled = the per-chain sums added over the replicas; count: (replica, step) pairs
            return {"sum": m["sum"].sum(0), "sum_sq": m["sum_sq"].sum(0), "sum_logp": m["sum_logp"].sum(0),
                    "count": m["count"] * self.n_replicas, "every": self.moments_every}
        return {**m, "every": self.moments_every}

    def reset_moments(self) -> None:
        """Zero the moment accumulators (the chains keep their states)."""
        for t in (self._mom or {}).values():
            t.zero_()

    def _snapshot_sums(self, name: str, **extra) -> Optional[dict]:
        """The read-out of the snapshot accumulator under attribute `name`: its sums and `extra`, or None when it is off."""
        sums = getattr(self, name)
        return {**sums, **extra} if sums is not None else None

    def _reset_snapshot(self, name: str) -> None:
        for t in (getattr(self, name) or {}).values():
            t.zero_()

    def histogram(self) -> Optional[dict]:
        """The pooled marginal histograms of this shard, or None when they are off: counts [hist_temps, dim, hist_bins + 2]
        and count [hist_temps] (int64 device tensors, no synchronisation) and edges [dim, hist_bins + 1] (float64, CPU)."""
        return self._snapshot_sums("_hist", edges=getattr(self, "_hist_edges", None))

    def reset_histogram(self) -> None:
        """Zero the histogram counters (the chains keep their states)."""
        self._reset_snapshot("_hist")

    def autocorr_sums(self) -> Optional[dict]:
        """The pooled lagged autocovariance sums of this shard, or None when they are off: sxy / head / tail
        [acf_temps, acf_max_lag + 1, dim] float64 and pairs [acf_max_lag + 1] int64 (device tensors, no synchronisation), and
        every."""
        return self._snapshot_sums("_acf", every=self.acf_every)

    def reset_autocorr(self) -> None:
        """Zero the autocovariance sums (the chains keep their states).  The ring stays valid: snapshots are numbered from the
        step counter, so the next one pairs with the ones before the reset."""
        self._reset_snapshot("_acf")

    def covariance_sums(self) -> Optional[dict]:
        """The pooled covariance sums of this shard, or None when they are off: sxx [cov_temps, dim, dim] (lower triangle) and sx
        [cov_temps, dim] float64, count [1] int64 (device tensors, no synchronisation), and every."""
        return self._snapshot_sums("_cov", every=self.cov_every)

    def reset_covariance(self) -> None:
        """Zero the covariance sums (the chains keep their states)."""
        self._reset_snapshot("_cov")

    def energy_sums(self) -> Optional[dict]:
        """The pooled log-density sums of this shard, or None when they are off: count [groups, n_temps] int64, s1 / s2 / colder /
        hotter [groups, n_temps] float64, nonfinite [1] int64, ref [n_temps] float64, ref_set [1] int32 and beta [n_temps]
        float32 - the ladder as it stands - (device tensors, no synchronisation), and every, pinned."""
        if self._energy is None:
            return None
        return self._snapshot_sums("_energy", ref=self._energy_ref, ref_set=self._energy_ref_set, beta=self.beta,
                                   every=self.energy_every, pinned=self._energy_pinned)

    def reset_energy(self) -> None:
        """Zero the log-density sums (the chains keep their states); a level the run chose itself is chosen anew by the next
        due snapshot, a pinned one (energy_ref=) stays."""
        self._reset_snapshot("_energy")
        if self._energy is not None and not self._energy_pinned:
            self._energy_ref_set.zero_()
            self._energy_ref.zero_()

    def flow(self) -> Optional[dict]:
        """Replica flow of this shard (device tensors, no synchronisation), or None when flow is off: walker (int32 flow
        words), round_trips (by walker id), n_up / n_down (by temperature), all [n_replicas, n_temps], and events - the swap
        events so far that the arrays cover: since the start of the run or the last reset_flow(), stand-alone sweeps included."""
        return {**self._flow, "events": self.swap_events() - self._flow_events0} if self._flow is not None else None

    def reset_flow(self) -> None:
        """Every walker back on its starting position (id = temperature index, no direction), counters zeroed, and the event
        count of flow() restarted: n_up[:, 0] == events and the round-trip rate hold for the arrays as they are."""
        self._flow_events0 = self.swap_events()
        if self._flow is not None:
            self._flow["walker"].copy_(torch.arange(self.n_temps, device=self.device, dtype=torch.int32).expand(self.n_replicas, -1))
            for k in ("round_trips", "n_up", "n_down"):
                self._flow[k].zero_()

    def chain_moments(self) -> Optional[dict]:
        """The raw per-chain moment sums of this shard (device tensors, no synchronisation), or None when
        moments_per_chain is off: sum / sum_sq [n_replicas, temps, dim] float64, sum_logp [n_replicas, temps] float64,
        count [temps] int64 (accumulated steps per replica), every."""
        return {**self._mom, "every": self.moments_every} if self.moments_per_chain else None

    def reset_chain_moments(self) -> None:
        """Zero the per-chain accumulators (the chains keep their states)."""
        if self.moments_per_chain:
            self.reset_moments()

    def summary(self) -> dict:
        """Whole-shard sums, as plain Python numbers / CPU tensors (one device sync)."""
        acc = self.n_accept.sum(0).cpu()
        sq = self.sq_jump.sum(0).cpu()
        sw = self.swap_accept.sum(0).cpu()
        return {
            "n_replicas": self.n_replicas,
            "post_burn_steps": self.post_burn_steps,
            "accept_count": acc,            # [T] int64
            "sq_jump_sum": sq,              # [T] float64
            "swap_accept_count": sw,        # [T] int64 (last entry unused)
            "swap_attempts": self.swap_attempts_per_replica() * self.n_replicas,
        }


# ---- posterior moments of the drop-in classes ------------------------------------------------------------------
MOMENT_MODES = (None, "cold", "all")


def moments_temps(mode, n_temps: int, every) -> int:
    """Temperatures a `moments=` mode covers (0: off); raises on a bad mode or thinning period."""
    if mode not in MOMENT_MODES:
        raise ValueError(f"moments must be None, 'cold' or 'all', got {mode!r}")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"moments_every must be an integer >= 1, got {every!r}")
    return {None: 0, "cold": 1, "all": n_temps}[mode]


def chain_mean_var(sum: torch.Tensor, sum_sq: torch.Tensor, n) -> tuple:
    """Mean and variance (ddof 1) of every chain from its sums over n draws: sum / sum_sq [chains, ...] float64."""
    n = float(n)
    mean = sum / n
    var = (sum_sq - n * mean * mean) / (n - 1.0) if n >= 2 else torch.full_like(mean, float("nan"))
    return mean, var


def rhat_ess_from_chain_summary(m: float, s_mean: torch.Tensor, s_mean_sq: torch.Tensor, s_var: torch.Tensor, n) -> tuple:
    """Gelman-Rubin R-hat and between-chain ESS from what sums over chains: M, sum_c m_c, sum_c m_c^2, sum_c s2_c (m_c / s2_c
    the chain means / variances over n draws each).  See rhat_ess_from_chain_sums."""
    m, n = float(m), float(n)
    if m < 2 or n < 2:
        nan = torch.full_like(s_mean, float("nan"))
        return nan, nan.clone()
    w = s_var / m
    grand = s_mean / m
    b = n * (s_mean_sq - m * grand * grand) / (m - 1.0)
    var_plus = (n - 1.0) / n * w + b / n
    rhat = torch.sqrt(var_plus / w)
    ess = torch.clamp(m * n * var_plus / b, max=m * n)
    return rhat, ess


def rhat_ess_from_chain_sums(sum: torch.Tensor, sum_sq: torch.Tensor, n) -> tuple:
    """(R-hat, ESS) per coordinate from per-chain sums: sum / sum_sq [M, ...] float64 (CPU or GPU), n draws per chain.
    With m_c, s2_c the chain means and variances (ddof 1):  W = mean_c s2_c,  B = n var_c(m_c, ddof 1),
    var+ = (n - 1) / n W + B / n,  R-hat = sqrt(var+ / W),  ESS = min(M n, M n var+ / B).  NaN when M < 2 or n < 2."""
    mean, var = chain_mean_var(sum, sum_sq, n)
    return rhat_ess_from_chain_summary(sum.shape[0], mean.sum(0), (mean * mean).sum(0), var.sum(0), n)


class PosteriorMoments:
    """Estimates from the moments accumulated inside the step kernels (include/ptrwm.h ptrwm_moments_args), pooled over
    every replica of the run.  The host class sets `_moments_mode` / `_moments_every` and owns `_run` (an EngineRun).
    Every read synchronises."""

    def _moment_sums(self) -> dict:
        if getattr(self, "_moments_mode", None) is None:
            raise RuntimeError("posterior moments are off: construct the sampler with moments='cold' or 'all'")
        run = getattr(self, "_run", None)
        if run is None:  # nothing run yet, or reset(): empty sums (the next run starts from zero)
            mt = moments_temps(self._moments_mode, len(getattr(self, "beta_ladder", [1.0])), self._moments_every)
            z = torch.zeros(mt, self.dim, device=self.device, dtype=torch.float64)
            return {"sum": z, "sum_sq": z.clone(), "sum_logp": torch.zeros(mt, device=self.device, dtype=torch.float64),
                    "count": torch.zeros(mt, device=self.device, dtype=torch.int64), "every": self._moments_every}
        return run.moments()

    def _check_temperature(self, temperature: int, m: dict) -> int:
        mt = m["sum"].shape[0]
        if not isinstance(temperature, (int, np.integer)) or not 0 <= temperature < mt:
            raise ValueError(f"temperature must be in 0..{mt - 1} (the moments cover the first {mt}), got {temperature!r}")
        return int(temperature)

    @property
    def moment_count(self) -> torch.Tensor:
        """(replica, step) pairs accumulated per covered temperature: int64 [temps] on the device."""
        return self._moment_sums()["count"]

    def posterior_mean(self, temperature: int = 0) -> torch.Tensor:
        """sum x / n over every replica of `temperature` and every accumulated step: float64 [dim] on the device."""
        m = self._moment_sums()
        t = self._check_temperature(temperature, m)
        return m["sum"][t] / m["count"][t].double()

    def posterior_variance(self, temperature: int = 0) -> torch.Tensor:
        """sum x^2 / n - mean^2 (per coordinate): float64 [dim] on the device."""
        m = self._moment_sums()
        t = self._check_temperature(temperature, m)
        n = m["count"][t].double()
        mean = m["sum"][t] / n
        return m["sum_sq"][t] / n - mean * mean

    def mean_log_density(self) -> torch.Tensor:
        """sum logp / n per covered temperature: float64 [temps] on the device."""
        m = self._moment_sums()
        return m["sum_logp"] / m["count"].double()

    # ---- per-chain estimates (moments_per_chain=True) -----------------------------------------------------------
    def _chain_sums(self, temperature: int) -> tuple:
        """(sum [chains, dim], sum_sq [chains, dim], draws per chain) of one covered temperature."""
        if not getattr(self, "_moments_per_chain", False):
            raise RuntimeError("per-chain moments are off: construct the sampler with moments_per_chain=True")
        run = getattr(self, "_run", None)
        if run is None:
            raise RuntimeError("nothing has run yet: no per-chain moments")
        cm = run.chain_moments()
        t = self._check_temperature(temperature, {"sum": cm["sum"][0]})
        return cm["sum"][:, t], cm["sum_sq"][:, t], int(cm["count"][t].item())

    def chain_means(self, temperature: int = 0) -> torch.Tensor:
        """Every chain's own mean of `temperature`: float64 [chains, dim] on the device."""
        s, q, n = self._chain_sums(temperature)
        return chain_mean_var(s, q, n)[0] if n >= 1 else torch.full_like(s, float("nan"))

    def chain_variances(self, temperature: int = 0) -> torch.Tensor:
        """Every chain's own variance (ddof 1) of `temperature`: float64 [chains, dim] on the device."""
        s, q, n = self._chain_sums(temperature)
        return chain_mean_var(s, q, n)[1] if n >= 1 else torch.full_like(s, float("nan"))

    def rhat(self, temperature: int = 0) -> torch.Tensor:
        """Gelman-Rubin R-hat per coordinate over the chains of `temperature` (rhat_ess_from_chain_sums): float64 [dim]."""
        s, q, n = self._chain_sums(temperature)
        return rhat_ess_from_chain_sums(s, q, n)[0]

    def ess(self, temperature: int = 0) -> torch.Tensor:
        """Between-chain effective sample size per coordinate, all chains together: float64 [dim]."""
        s, q, n = self._chain_sums(temperature)
        return rhat_ess_from_chain_sums(s, q, n)[1]

    def _moments_diagnostics(self) -> dict:
        if getattr(self, "_moments_mode", None) is None:
            return {}
        m = self._moment_sums()
        n = m["count"].double()
        mean = m["sum"] / n[:, None]
        extra = {}
        if getattr(self, "_moments_per_chain", False) and getattr(self, "_run", None) is not None:
            extra = {"rhat_max": float(self.rhat().max().item()), "ess_min": float(self.ess().min().item())}
        return {
            **extra,
            "moments": self._moments_mode,
            "moments_every": self._moments_every,
            "moment_count": m["count"].cpu(),
            "posterior_mean": mean.cpu(),
            "posterior_variance": (m["sum_sq"] / n[:, None] - mean * mean).cpu(),
            "mean_log_density": (m["sum_logp"] / n).cpu(),
        }


# ---- pooled lagged autocovariance: estimators and the drop-in classes' readers -------------------------------------------
ACF_RING_LIMIT = 1 << 31  # elements (8 GiB of float states): what a ring may hold unless the caller says otherwise


def covered_temperature(temperature, temps: int, what: str) -> int:
    """`temperature` as an index into the first `temps` temperatures a snapshot accumulator covers (`what`: "the ... cover(s)")"""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, np.integer)) or not 0 <= temperature < temps:
        raise ValueError(f"temperature must be in 0..{temps - 1} ({what} the first {temps}), got {temperature!r}")
    return int(temperature)


def check_acf_args(acf_temps, acf_every, acf_max_lag, n_temps: int, dim: int, n_replicas: int, ring_limit=None) -> bool:
    """EngineRun's autocovariance arguments (no GPU needed): False when off.  The ring holds acf_max_lag x replicas x acf_temps
    x dim elements of the state's type; above `ring_limit` elements (default ACF_RING_LIMIT = 2^31) that is refused, naming the
    size, because it is rarely what the caller means - thin with acf_every instead of raising acf_max_lag."""
    for name, v in (("acf_temps", acf_temps), ("acf_every", acf_every), ("acf_max_lag", acf_max_lag)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 0 <= acf_temps <= n_temps:
        raise ValueError(f"acf_temps must be in 0..{n_temps}, got {acf_temps}")
    if not acf_temps:
        return False
    if acf_every < 1:
        raise ValueError(f"acf_every must be >= 1, got {acf_every}")
    if not 1 <= acf_max_lag <= ptrwm_hip.ACF_MAX_LAG:
        raise ValueError(f"acf_max_lag must be in 1..{ptrwm_hip.ACF_MAX_LAG}, got {acf_max_lag}")
    limit = ACF_RING_LIMIT if ring_limit is None else int(ring_limit)
    elems = int(acf_max_lag) * int(n_replicas) * int(acf_temps) * int(dim)
    if elems > limit:
        raise ValueError(f"the autocovariance ring would hold acf_max_lag x replicas x temperatures x dim = {acf_max_lag} x "
                         f"{n_replicas} x {acf_temps} x {dim} = {elems} elements ({elems * 4 / 2**30:.1f} GiB of float32 states), "
                         f"above the limit of {limit}: lower acf_max_lag and reach long lags with acf_every, cover acf='cold', "
                         "or raise acf_ring_limit")
    return True


def acf_temps(mode, n_temps: int) -> int:
    """Temperatures an `acf=` mode covers (0: off)."""
    if mode not in (None, "cold", "all"):
        raise ValueError(f"acf must be None, 'cold' or 'all', got {mode!r}")
    return {None: 0, "cold": 1, "all": n_temps}[mode]


def acf_autocovariance(sxy, head, tail, pairs) -> torch.Tensor:
    """c_k = sxy_k / n_k - (head_k / n_k)(tail_k / n_k) from the sums of one temperature: sxy / head / tail [lags, dim], pairs
    [lags]; float64 [lags, dim] on the CPU, NaN at a lag without pairs."""
    sxy, head, tail = (torch.as_tensor(t).detach().cpu().to(torch.float64) for t in (sxy, head, tail))
    n = torch.as_tensor(pairs).detach().cpu().to(torch.float64)[:, None]
    if sxy.dim() != 2 or head.shape != sxy.shape or tail.shape != sxy.shape or n.shape[0] != sxy.shape[0]:
        raise ValueError("sxy, head and tail must be [lags, dim] and pairs [lags]")
    n = torch.where(n > 0, n, torch.full_like(n, float("nan")))
    return sxy / n - (head / n) * (tail / n)


def acf_autocorrelation(sxy, head, tail, pairs) -> torch.Tensor:
    """rho_k = c_k / c_0: float64 [lags, dim]; NaN where c_0 is not positive."""
    c = acf_autocovariance(sxy, head, tail, pairs)
    c0 = torch.where(c[0] > 0, c[0], torch.full_like(c[0], float("nan")))
    return c / c0


def sokal_window(rho, c: float = 5.0) -> tuple:
    """Integrated autocorrelation time by Sokal's automatic window, per coordinate, from rho [lags, dim] (rho[0] = 1):
    tau(M) = 1 + 2 sum_{k=1..M} rho_k and the window is the smallest M >= 1 with M >= c tau(M).  Returns (tau [dim] float64,
    window [dim] int64, reached [dim] bool).  Lags from the first NaN on (no pairs yet: a run shorter than the ring) are not
    there.  Where no M up to the last lag there is qualifies, `reached` is False, window is that last lag and tau is tau(last
    lag): a LOWER BOUND, not an estimate.  A coordinate without any lag: tau NaN, window 0, reached False."""
    rho = torch.as_tensor(rho).detach().cpu().to(torch.float64)
    if rho.dim() != 2 or rho.shape[0] < 2:
        raise ValueError("rho must be [lags >= 2, dim]")
    if not c > 0:
        raise ValueError("c must be positive")
    L = rho.shape[0] - 1
    there = torch.cumprod(torch.isfinite(rho).to(torch.int64), 0)[1:].bool()  # [L, dim]: lag M and every lag below it is finite
    taus = 1.0 + 2.0 * torch.cumsum(torch.where(there, rho[1:], torch.zeros_like(rho[1:])), 0)  # tau(M), M = 1..L
    M = torch.arange(1, L + 1, dtype=torch.float64)[:, None]
    ok = there & (M >= c * taus)
    reached = ok.any(0)
    n_there = there.sum(0)
    at = torch.where(reached, ok.to(torch.int64).argmax(0), (n_there - 1).clamp(min=0))  # index of the window in taus
    tau = torch.where(n_there > 0, taus.gather(0, at[None, :])[0], torch.full((rho.shape[1],), float("nan"), dtype=torch.float64))
    return tau, torch.where(n_there > 0, at + 1, torch.zeros_like(at)), reached


class Autocorrelation:
    """Estimates from the pooled lagged autocovariance (include/ptrwm.h ptrwm_acf_args, csrc/acf.h): how correlated successive
    snapshots of a coordinate are, pooled over every replica of the run.  The host class calls `_check_acf_ctor` in its
    constructor, passes `_acf_kwargs(n_temps)` to EngineRun and owns `_run`.  Every read synchronises; results are CPU tensors.

    The keywords: acf='cold' or 'all' temperatures, a snapshot every acf_every-th step past burn-in, lags 0..acf_max_lag in
    snapshots; acf_ring_limit overrides the largest ring (elements) the constructor accepts."""

    def _check_acf_ctor(self, dim: int, acf, acf_every, acf_max_lag, acf_ring_limit=None) -> None:
        """The constructor's autocovariance arguments, checked before anything is built (no GPU needed; the ring's size is
        checked again where the number of replicas is known)."""
        if acf_temps(acf, 1):
            check_acf_args(1, acf_every, acf_max_lag, 1, dim, 1, acf_ring_limit)
        self._acf_mode, self._acf_every, self._acf_max_lag, self._acf_ring_limit = acf, acf_every, acf_max_lag, acf_ring_limit

    def _acf_kwargs(self, n_temps: int) -> dict:
        """EngineRun's autocovariance arguments."""
        if self._acf_mode is None:
            return {}
        return {"acf_temps": acf_temps(self._acf_mode, n_temps), "acf_every": self._acf_every, "acf_max_lag": self._acf_max_lag,
                "acf_ring_limit": self._acf_ring_limit}

    def _acf_data(self, temperature) -> tuple:
        if getattr(self, "_acf_mode", None) is None:
            raise RuntimeError("the autocovariance is off: construct the sampler with acf='cold' or 'all'")
        temps = acf_temps(self._acf_mode, len(getattr(self, "beta_ladder", [1.0])))
        t = covered_temperature(temperature, temps, "the autocovariance covers")
        run = getattr(self, "_run", None)
        if run is None or run.autocorr_sums() is None:  # nothing run yet, or reset(): empty sums
            z = torch.zeros(self._acf_max_lag + 1, self.dim, dtype=torch.float64)
            return z, z.clone(), z.clone(), torch.zeros(self._acf_max_lag + 1, dtype=torch.int64)
        a = run.autocorr_sums()
        return a["sxy"][t].cpu(), a["head"][t].cpu(), a["tail"][t].cpu(), a["pairs"].cpu()

    def autocovariance(self, temperature: int = 0) -> torch.Tensor:
        """c_k of every coordinate at lags k = 0 .. acf_max_lag (in snapshots: acf_every steps apart), pooled over every replica
        and every snapshot: float64 [acf_max_lag + 1, dim]; NaN at a lag no snapshot has reached yet."""
        return acf_autocovariance(*self._acf_data(temperature))

    def autocorrelation(self, temperature: int = 0) -> torch.Tensor:
        """rho_k = c_k / c_0: float64 [acf_max_lag + 1, dim]."""
        return acf_autocorrelation(*self._acf_data(temperature))

    def integrated_autocorr_time(self, temperature: int = 0, c: float = 5.0) -> tuple:
        """(tau [dim] float64, window [dim] int64, reached [dim] bool): the integrated autocorrelation time of every coordinate
        by Sokal's automatic window - the smallest M with M >= c tau(M), tau(M) = 1 + 2 sum_{k <= M} rho_k.  tau is in units of
        SNAPSHOTS: multiply by acf_every for steps only when acf_every is much shorter than tau (a thinned sequence's tau is
        not the full one's divided by the thinning otherwise).  Where no window up to acf_max_lag qualifies, `reached` is False
        and tau is the value at acf_max_lag - a lower bound on the autocorrelation time, not an estimate of it."""
        return sokal_window(self.autocorrelation(temperature), c)

    def ess_autocorr(self, temperature: int = 0) -> torch.Tensor:
        """Effective sample size of every coordinate: pairs[0] / tau - the (replica, snapshot) pairs so far over the integrated
        autocorrelation time (in snapshots).  Where the window was not reached tau is a lower bound, so this is an UPPER bound;
        check integrated_autocorr_time()[2].  float64 [dim]."""
        tau = self.integrated_autocorr_time(temperature)[0]
        return float(self._acf_data(temperature)[3][0]) / tau

    def _acf_diagnostics(self) -> dict:
        if getattr(self, "_acf_mode", None) is None:
            return {}
        tau, _, reached = self.integrated_autocorr_time(0)
        ok = bool(torch.isfinite(tau).all())
        return {"act_max": float(tau.max()) if ok else float("nan"), "act_window_reached": bool(reached.all())}


# ---- pooled posterior covariance: estimators and the drop-in classes' readers ------------------------------------------------
def check_cov_args(cov_temps, cov_every, n_temps: int) -> bool:
    """EngineRun's covariance arguments (no GPU needed): False when off."""
    for name, v in (("cov_temps", cov_temps), ("cov_every", cov_every)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 0 <= cov_temps <= n_temps:
        raise ValueError(f"cov_temps must be in 0..{n_temps}, got {cov_temps}")
    if not cov_temps:
        return False
    if cov_every < 1:
        raise ValueError(f"cov_every must be >= 1, got {cov_every}")
    return True


def cov_temps(mode, n_temps: int) -> int:
    """Temperatures a `cov=` mode covers (0: off)."""
    if mode not in (None, "cold", "all"):
        raise ValueError(f"cov must be None, 'cold' or 'all', got {mode!r}")
    return {None: 0, "cold": 1, "all": n_temps}[mode]


def cov_covariance(sxx, sx, count) -> torch.Tensor:
    """sxx / n - mean mean^T from the sums of one temperature, mirrored to both triangles: sxx [dim, dim] (only its lower
    triangle, j <= i, is read), sx [dim], count a scalar; float64 [dim, dim] on the CPU, NaN without a snapshot.  It divides by
    n, as the pooled variance does.  Raw sums: about log10(1 + mean^2 / var) digits of a coordinate are lost."""
    sxx = torch.as_tensor(sxx).detach().cpu().to(torch.float64)
    sx = torch.as_tensor(sx).detach().cpu().to(torch.float64)
    n = float(torch.as_tensor(count).reshape(-1)[0]) if not isinstance(count, (int, float)) else float(count)
    if sxx.dim() != 2 or sxx.shape[0] != sxx.shape[1] or sx.shape != sxx.shape[:1]:
        raise ValueError("sxx must be [dim, dim] and sx [dim]")
    if not n > 0:
        return torch.full_like(sxx, float("nan"))
    low = torch.tril(sxx)
    full = low + torch.tril(sxx, -1).T
    m = sx / n
    c = full / n - torch.outer(m, m)
    return (c + c.T) / 2  # (exactly symmetric; halves of equal numbers are exact)


def cov_correlation(cov) -> torch.Tensor:
    """cov[i, j] / sqrt(cov[i, i] cov[j, j]): float64 [dim, dim] with a unit diagonal; a coordinate whose variance is not
    positive gives NaN off its diagonal."""
    cov = torch.as_tensor(cov).detach().cpu().to(torch.float64)
    var = torch.diagonal(cov)
    sd = torch.sqrt(torch.where(var > 0, var, torch.full_like(var, float("nan"))))
    r = cov / torch.outer(sd, sd)
    r.fill_diagonal_(1.0)
    return r


def cov_principal_axes(cov) -> tuple:
    """(eigenvalues descending [dim], eigenvectors as columns [dim, dim]) of the float64 matrix, from torch.linalg.eigh."""
    w, v = torch.linalg.eigh(torch.as_tensor(cov).detach().cpu().to(torch.float64))
    return torch.flip(w, (0,)), torch.flip(v, (1,))


def cov_condition(cov) -> float:
    """Largest over smallest eigenvalue; inf where the smallest is <= 0; NaN for a matrix with a NaN."""
    cov = torch.as_tensor(cov).detach().cpu().to(torch.float64)
    if not bool(torch.isfinite(cov).all()):
        return float("nan")
    w = torch.linalg.eigvalsh(cov)
    lo, hi = float(w[0]), float(w[-1])
    return hi / lo if lo > 0 else float("inf")


class PosteriorCovariance:
    """Estimates from the pooled covariance sums (include/ptrwm.h ptrwm_cov_args, csrc/cov.h): how the coordinates move
    together, pooled over every replica of the run.  The host class calls `_check_cov_ctor` in its constructor, passes
    `_cov_kwargs(n_temps)` to EngineRun and owns `_run`.  Every read synchronises; results are CPU tensors.

    The keywords: cov='cold' or 'all' temperatures, a snapshot every cov_every-th step past burn-in."""

    def _check_cov_ctor(self, cov, cov_every) -> None:
        """The constructor's covariance arguments, checked before anything is built (no GPU needed)."""
        if cov_temps(cov, 1):
            check_cov_args(1, cov_every, 1)
        self._cov_mode, self._cov_every = cov, cov_every

    def _cov_kwargs(self, n_temps: int) -> dict:
        """EngineRun's covariance arguments."""
        if self._cov_mode is None:
            return {}
        return {"cov_temps": cov_temps(self._cov_mode, n_temps), "cov_every": self._cov_every}

    def _cov_data(self, temperature) -> tuple:
        if getattr(self, "_cov_mode", None) is None:
            raise RuntimeError("the covariance is off: construct the sampler with cov='cold' or 'all'")
        temps = cov_temps(self._cov_mode, len(getattr(self, "beta_ladder", [1.0])))
        t = covered_temperature(temperature, temps, "the covariance covers")
        run = getattr(self, "_run", None)
        if run is None or run.covariance_sums() is None:  # nothing run yet, or reset(): empty sums
            return (torch.zeros(self.dim, self.dim, dtype=torch.float64), torch.zeros(self.dim, dtype=torch.float64),
                    torch.zeros(1, dtype=torch.int64))
        a = run.covariance_sums()
        return a["sxx"][t].cpu(), a["sx"][t].cpu(), a["count"].cpu()

    @property
    def covariance_count(self) -> int:
        """(replica, step) pairs accumulated so far."""
        return int(self._cov_data(0)[2][0])

    def posterior_covariance(self, temperature: int = 0) -> torch.Tensor:
        """Covariance of the coordinates, pooled over every replica and every snapshot: sxx / n - mean mean^T, float64
        [dim, dim], symmetric; it divides by n, as posterior_variance does.  NaN before the first snapshot."""
        return cov_covariance(*self._cov_data(temperature))

    def posterior_correlation(self, temperature: int = 0) -> torch.Tensor:
        """Correlation matrix: float64 [dim, dim]; a coordinate of zero variance gives NaN off its diagonal."""
        return cov_correlation(self.posterior_covariance(temperature))

    def principal_axes(self, temperature: int = 0) -> tuple:
        """(eigenvalues descending [dim], eigenvectors as columns [dim, dim]) of posterior_covariance(temperature)."""
        return cov_principal_axes(self.posterior_covariance(temperature))

    def _cov_diagnostics(self) -> dict:
        if getattr(self, "_cov_mode", None) is None:
            return {}
        return {"cov_condition": cov_condition(self.posterior_covariance(0)), "cov_count": self.covariance_count}


# ---- pooled log-density sums along the ladder: estimators and the drop-in classes' readers ---------------------------------------
ENERGY_METHODS = ("forward", "reverse", "thermodynamic", "thermodynamic_corrected")


def check_energy_args(energy, energy_every=1, energy_groups=16, energy_ref=None, n_temps: Optional[int] = None) -> Optional[dict]:
    """EngineRun's arguments of the log-density sums (no GPU needed): None when off, else {"every", "groups", "ref"} - ref None
    (the first due snapshot chooses the level) or float64 [n_temps] (pinned: a scalar stands for every temperature).  With
    n_temps None (a class whose ladder is not built yet) a vector's length is left to EngineRun."""
    if not isinstance(energy, (bool, np.bool_)):
        raise ValueError(f"energy must be True or False, got {energy!r}")
    if not energy:
        if energy_ref is not None:
            raise ValueError("energy_ref pins the level of energy=True: it does nothing without it")
        return None
    every, groups = _integer("energy_every", energy_every, 1), _integer("energy_groups", energy_groups, 1)
    if groups > ptrwm_hip.ENERGY_MAX_GROUPS:
        raise ValueError(f"energy_groups must be in 1..{ptrwm_hip.ENERGY_MAX_GROUPS}, got {energy_groups!r}")
    ref = None
    if energy_ref is not None:
        r = energy_ref.detach().cpu().numpy() if torch.is_tensor(energy_ref) else np.asarray(energy_ref)
        if r.dtype == object or not np.issubdtype(r.dtype, np.number) or np.issubdtype(r.dtype, np.complexfloating):
            raise ValueError(f"energy_ref must be a number or a [n_temps] vector of numbers, got {energy_ref!r}")
        ref = np.asarray(r, dtype=np.float64)
        if ref.ndim > 1 or (ref.ndim == 1 and n_temps is not None and ref.shape[0] != n_temps):
            raise ValueError(f"energy_ref must be a scalar or a [n_temps] = [{n_temps}] vector, got shape {tuple(ref.shape)}")
        if not np.isfinite(ref).all():
            raise ValueError("energy_ref must be finite")
        if n_temps is not None:
            ref = np.ascontiguousarray(np.broadcast_to(ref, (n_temps,)))
    return {"every": every, "groups": groups, "ref": ref}


def _f64(x) -> np.ndarray:
    return torch.as_tensor(x).detach().cpu().to(torch.float64).numpy()


def _energy_jackknife(estimate, used: np.ndarray) -> np.ndarray:
    """The delete-one-group jackknife standard error of estimate(mask), mask a bool [groups] of the groups summed over, over the
    m groups of `used`: se^2 = (m - 1) / m sum_g (theta_(g) - mean theta_(.))^2, NaN for m < 2."""
    idx = np.flatnonzero(used)
    m = len(idx)
    if m < 2:
        return np.full_like(np.asarray(estimate(used), dtype=np.float64), np.nan)
    theta = []
    for g in idx:
        mask = used.copy()
        mask[g] = False
        theta.append(np.asarray(estimate(mask), dtype=np.float64))
    theta = np.stack(theta)
    with np.errstate(invalid="ignore"):
        return np.sqrt((m - 1) / m * ((theta - theta.mean(0)) ** 2).sum(0))


def energy_moments_from_sums(count, s1, s2, beta) -> dict:
    """Per rung, from the sums [groups, n_temps] added over the groups: "mean" = s1 / n, the mean of l = log pi; "variance" =
    s2 / n - mean^2 (divided by n, as posterior_variance is); "heat_capacity" = beta^2 variance, whose shape over the ladder
    says where it needs rungs; "count" = n.  float64 [n_temps] on the CPU (count int64); NaN where n = 0."""
    n = torch.as_tensor(count).detach().cpu().to(torch.int64).sum(0)
    nf, a, b, be = n.to(torch.float64).numpy(), _f64(s1).sum(0), _f64(s2).sum(0), _f64(beta)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(nf > 0, a / nf, np.nan)
        var = np.where(nf > 0, b / nf - mean * mean, np.nan)
    return {"mean": torch.from_numpy(mean), "variance": torch.from_numpy(var), "heat_capacity": torch.from_numpy(be * be * var),
            "count": n}


def stepping_stones_from_sums(count, colder, hotter, ref, beta) -> dict:
    """The stepping-stone estimates of log Z(beta[t-1]) / Z(beta[t]), t = 1 .. n_temps - 1 (entry t - 1 of each array), from the
    sums [groups, n_temps] and the level ref [n_temps] they were taken against:
        forward[t] =   log(colder[t] / n[t])     + (beta[t-1] - beta[t]) ref[t]        (draws of rung t)
        reverse[t] = -(log(hotter[t-1] / n[t-1]) + (beta[t] - beta[t-1]) ref[t-1])     (draws of rung t - 1)
    By Jensen E forward <= truth <= E reverse.  "forward_se" / "reverse_se": the delete-one-group jackknife over the groups that
    have draws at the rung involved (NaN with fewer than two); "forward_total" / "reverse_total" and their "_se": the sum over
    the ladder, log Z(beta[0]) / Z(beta[n_temps-1]), jackknifed as a whole over the groups with draws at every rung;
    "overflow": an exponential sum holds an inf (choose or pin a higher ref).  float64 on the CPU."""
    n, c, h, r, be = _f64(count), _f64(colder), _f64(hotter), _f64(ref), _f64(beta)
    T = n.shape[1]

    def forward(mask, t):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.log(c[mask, t].sum() / n[mask, t].sum()) + (be[t - 1] - be[t]) * r[t]

    def reverse(mask, t):
        with np.errstate(invalid="ignore", divide="ignore"):
            return -(np.log(h[mask, t - 1].sum() / n[mask, t - 1].sum()) + (be[t] - be[t - 1]) * r[t - 1])

    out = {}
    everywhere = (n > 0).all(1)
    for name, fn, rung in (("forward", forward, 0), ("reverse", reverse, -1)):
        used = [n[:, t + rung] > 0 for t in range(1, T)]
        out[name] = torch.tensor([fn(u, t) for t, u in zip(range(1, T), used)], dtype=torch.float64)
        out[name + "_se"] = torch.tensor([float(_energy_jackknife(lambda m, t=t: fn(m, t), u)) for t, u in zip(range(1, T), used)],
                                         dtype=torch.float64)
        out[name + "_total"] = float(out[name].sum())
        out[name + "_total_se"] = float(_energy_jackknife(lambda m: sum(fn(m, t) for t in range(1, T)), everywhere)) if T > 1 else float("nan")
    out["overflow"] = bool(np.isinf(c[:, 1:]).any() or np.isinf(h[:, :-1]).any()) if T > 1 else False
    return out


def thermodynamic_integral_from_sums(count, s1, s2, beta) -> dict:
    """Thermodynamic integration of log Z(beta[t-1]) / Z(beta[t]) = integral of E_beta[l] d beta, t = 1 .. n_temps - 1 (entry
    t - 1), with E[t] and V[t] the mean and variance of l at rung t:
        trapezoid[t] = (beta[t-1] - beta[t]) (E[t-1] + E[t]) / 2
        corrected[t] = trapezoid[t] - (beta[t-1] - beta[t])^2 (V[t-1] - V[t]) / 12       (Friel, Hurn and Wyse 2014)
    with "trapezoid_se" / "corrected_se", the delete-one-group jackknife over the groups that have draws at both rungs, and
    "trapezoid_total" / "corrected_total" with their "_se" (jackknifed as a whole over the groups with draws at every rung).
    float64 on the CPU."""
    n, a, b, be = _f64(count), _f64(s1), _f64(s2), _f64(beta)
    T = n.shape[1]

    def pair(mask, t, corrected):
        with np.errstate(invalid="ignore", divide="ignore"):
            nn = n[mask][:, [t - 1, t]].sum(0)
            e = a[mask][:, [t - 1, t]].sum(0) / nn
            v = b[mask][:, [t - 1, t]].sum(0) / nn - e * e
            d = be[t - 1] - be[t]
            return d * (e[0] + e[1]) / 2 - (d * d * (v[0] - v[1]) / 12 if corrected else 0.0)

    out = {}
    everywhere = (n > 0).all(1)
    for name, corrected in (("trapezoid", False), ("corrected", True)):
        used = [(n[:, t - 1] > 0) & (n[:, t] > 0) for t in range(1, T)]
        out[name] = torch.tensor([pair(u, t, corrected) for t, u in zip(range(1, T), used)], dtype=torch.float64)
        out[name + "_se"] = torch.tensor([float(_energy_jackknife(lambda m, t=t: pair(m, t, corrected), u))
                                          for t, u in zip(range(1, T), used)], dtype=torch.float64)
        out[name + "_total"] = float(out[name].sum())
        out[name + "_total_se"] = (float(_energy_jackknife(lambda m: sum(pair(m, t, corrected) for t in range(1, T)), everywhere))
                                   if T > 1 else float("nan"))
    return out


class LadderEnergies:
    """Estimates from the pooled log-density sums along the ladder (include/ptrwm.h ptrwm_energy_args, csrc/energy.h): the
    normalising-constant ratios log Z(beta_a) / Z(beta_b), Z(beta) = integral of pi(x)^beta dx, by stepping stones in both
    directions and by thermodynamic integration, and the mean, variance and heat capacity of l = log pi per rung.  The host class
    calls `_check_energy_ctor` in its constructor, passes `_energy_kwargs()` to EngineRun and owns `_run`.  Every read
    synchronises; results are CPU tensors.

    The keywords: energy=True; a snapshot every energy_every-th step past burn-in; energy_groups (1..64, default 16) disjoint
    groups of chains, by global replica id, for the jackknife error bars - they hold whatever the chains' autocorrelation in
    time, and need at least two groups with draws; energy_ref, a scalar or [n_temps], pins the level the exponential sums are
    taken against (default: the largest finite log-density of each rung at the first snapshot), which shards must share for
    their sums to add directly.  With one temperature only the moments mean something."""

    def _check_energy_ctor(self, energy, energy_every, energy_groups, energy_ref) -> None:
        """The constructor's arguments, checked before anything is built (no GPU needed)."""
        check_energy_args(energy, energy_every, energy_groups, energy_ref)
        self._energy_on, self._energy_args = bool(energy), (energy_every, energy_groups, energy_ref)

    def _energy_kwargs(self) -> dict:
        """EngineRun's arguments."""
        if not self._energy_on:
            return {}
        every, groups, ref = self._energy_args
        return {"energy": True, "energy_every": every, "energy_groups": groups, "energy_ref": ref}

    def _energy_data(self) -> dict:
        if not getattr(self, "_energy_on", False):
            raise RuntimeError("the log-density sums are off: construct the sampler with energy=True")
        run = getattr(self, "_run", None)
        if run is None or run.energy_sums() is None:  # nothing run yet, or reset(): empty sums
            G, T = int(self._energy_args[1]), len(getattr(self, "beta_ladder", [1.0]))
            z = torch.zeros(G, T, dtype=torch.float64)
            return {"count": torch.zeros(G, T, dtype=torch.int64), "s1": z, "s2": z, "colder": z, "hotter": z,
                    "nonfinite": torch.zeros(1, dtype=torch.int64), "ref": torch.zeros(T, dtype=torch.float64),
                    "ref_set": torch.zeros(1, dtype=torch.int32),
                    "beta": torch.tensor(list(getattr(self, "beta_ladder", [1.0])), dtype=torch.float32)}
        return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in run.energy_sums().items()}

    @property
    def energy_count(self) -> torch.Tensor:
        """Finite log-densities accumulated per rung, over every group: int64 [n_temps]."""
        return self._energy_data()["count"].sum(0)

    def _energy_moments(self) -> dict:
        a = self._energy_data()
        return energy_moments_from_sums(a["count"], a["s1"], a["s2"], a["beta"])

    def mean_energy(self) -> torch.Tensor:
        """The mean of l = log pi per rung, pooled over every replica and snapshot: float64 [n_temps]."""
        return self._energy_moments()["mean"]

    def energy_variance(self) -> torch.Tensor:
        """The variance of l per rung (divided by n): float64 [n_temps]."""
        return self._energy_moments()["variance"]

    def heat_capacity(self) -> torch.Tensor:
        """beta^2 Var_beta(l) per rung: where it peaks, the ladder needs rungs.  float64 [n_temps]."""
        return self._energy_moments()["heat_capacity"]

    def _energy_estimate(self, method: str) -> tuple:
        if method not in ENERGY_METHODS:
            raise ValueError(f"method must be one of {ENERGY_METHODS}, got {method!r}")
        a = self._energy_data()
        if method in ("forward", "reverse"):
            return stepping_stones_from_sums(a["count"], a["colder"], a["hotter"], a["ref"], a["beta"]), method
        return (thermodynamic_integral_from_sums(a["count"], a["s1"], a["s2"], a["beta"]),
                "trapezoid" if method == "thermodynamic" else "corrected")

    def log_normalizer_ratios(self, method: str = "forward") -> tuple:
        """(values, se), float64 [n_temps - 1] each: entry t - 1 estimates log Z(beta[t-1]) / Z(beta[t]) by `method` -
        "forward" / "reverse" (stepping stones from the hotter / the colder rung's draws; in expectation they bracket the
        truth from below / above), "thermodynamic" (trapezoid) or "thermodynamic_corrected" - with its jackknife standard error."""
        est, key = self._energy_estimate(method)
        return est[key], est[key + "_se"]

    def log_normalizer_ratio(self, method: str = "forward") -> tuple:
        """(total, se): log Z(beta[0]) / Z(beta[n_temps-1]) by `method`, the sum over the ladder, with its jackknife standard error."""
        est, key = self._energy_estimate(method)
        return est[key + "_total"], est[key + "_total_se"]

    def _energy_diagnostics(self) -> dict:
        if not getattr(self, "_energy_on", False):
            return {}
        a = self._energy_data()
        st = stepping_stones_from_sums(a["count"], a["colder"], a["hotter"], a["ref"], a["beta"])
        return {"log_z_ratio_forward": st["forward_total"], "log_z_ratio_reverse": st["reverse_total"],
                "log_z_ratio_se": max(st["forward_total_se"], st["reverse_total_se"]) if not (
                    np.isnan(st["forward_total_se"]) or np.isnan(st["reverse_total_se"])) else float("nan"),
                "energy_nonfinite": int(a["nonfinite"][0]), "energy_overflow": st["overflow"]}


# ---- pooled marginal histograms of the drop-in classes -------------------------------------------------------------
HIST_MODES = (None, "cold", "all")


def hist_temps(mode, n_temps: int) -> int:
    """Temperatures a `hist=` mode covers (0: off)."""
    if mode not in HIST_MODES:
        raise ValueError(f"hist must be None, 'cold' or 'all', got {mode!r}")
    return {None: 0, "cold": 1, "all": n_temps}[mode]


def _hist_cpu(counts, edges) -> tuple:
    counts = torch.as_tensor(counts).detach().cpu().to(torch.int64)
    edges = torch.as_tensor(edges).detach().cpu().to(torch.float64)
    if counts.dim() != 2 or edges.shape != (counts.shape[0], counts.shape[1] - 1) or counts.shape[1] < 3:
        raise ValueError("counts must be [dim, bins + 2] and edges [dim, bins + 1]")
    return counts, edges


def hist_density(counts, edges) -> torch.Tensor:
    """counts [dim, bins + 2] / (total x bin width) over the bins proper: float64 [dim, bins].  The total includes the two end
    bins, so the density integrates to the in-range fraction; NaN where nothing has been counted."""
    counts, edges = _hist_cpu(counts, edges)
    total = counts.sum(1).double()
    total[total == 0] = float("nan")
    return counts[:, 1:-1].double() / total[:, None] / (edges[:, 1:] - edges[:, :-1])


def hist_quantiles(counts, edges, q) -> torch.Tensor:
    """Quantiles per coordinate, float64 [len(q), dim]: with target = q x total (end bins included), the first non-empty bin
    whose cumulative count reaches the target, and linear interpolation inside it; NaN where that is the underflow or the
    overflow bin, and where nothing has been counted."""
    counts, edges = _hist_cpu(counts, edges)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or not np.all((qs >= 0.0) & (qs <= 1.0)):
        raise ValueError("quantiles: q must be numbers in [0, 1]")
    dim, nb = counts.shape[0], counts.shape[1] - 2
    cum = torch.cumsum(counts, 1).double()
    total = cum[:, -1]
    out = torch.full((len(qs), dim), float("nan"), dtype=torch.float64)
    for i, qv in enumerate(qs):
        for d in range(dim):
            if total[d] == 0:
                continue
            target = qv * float(total[d])
            hit = torch.nonzero((cum[d] >= target) & (cum[d] > 0))
            j = int(hit[0])
            if j == 0 or j == nb + 1:
                continue
            below = float(cum[d, j - 1])
            out[i, d] = edges[d, j - 1] + (target - below) / float(counts[d, j]) * (edges[d, j] - edges[d, j - 1])
    return out


def _hist_edge_index(edges: torch.Tensor, v, what: str) -> list:
    """Per coordinate, the index of the edge `v` names (a scalar or a [dim] vector; -inf: -1, below the underflow bin;
    +inf: bins + 1, above the overflow bin).  ValueError, naming the nearest edges, where it names none."""
    dim, ne = edges.shape
    vs = np.broadcast_to(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64), (dim,))
    idx = []
    for d in range(dim):
        x = float(vs[d])
        if np.isnan(x):
            raise ValueError(f"mass_between: {what} is NaN")
        if np.isinf(x):
            idx.append(-1 if x < 0 else ne)
            continue
        e = edges[d].numpy()
        j = int(np.argmin(np.abs(e - x)))
        width = (e[-1] - e[0]) / (ne - 1)
        if abs(e[j] - x) > 1e-6 * width:
            lo_j = max(0, min(ne - 2, int(np.searchsorted(e, x)) - 1))
            raise ValueError(f"mass_between: {what} = {x!r} is not a bin edge of coordinate {d}; the nearest edges are "
                             f"{float(e[lo_j])!r} and {float(e[lo_j + 1])!r} (the histogram does not interpolate)")
        idx.append(j)
    return idx


def hist_mass_between(counts, edges, a, b) -> torch.Tensor:
    """Fraction of the total (end bins included) counted in [a, b): float64 [dim].  `a` and `b` must be bin edges (within 1e-6
    of a bin width), or -inf / +inf to take the underflow / overflow bin in; then the answer is a ratio of exact counts.
    NaN where nothing has been counted."""
    counts, edges = _hist_cpu(counts, edges)
    ia, ib = _hist_edge_index(edges, a, "a"), _hist_edge_index(edges, b, "b")
    total = counts.sum(1).double()
    total[total == 0] = float("nan")
    out = torch.zeros(counts.shape[0], dtype=torch.float64)
    for d in range(counts.shape[0]):
        if ib[d] < ia[d]:
            raise ValueError("mass_between: a <= b must hold")
        # edge i is the left end of bin 1 + i; -1 / bins + 1 take the end bins in
        out[d] = counts[d, 1 + ia[d]:1 + ib[d]].sum().double()
    return out / total


def hist_mode_weights(counts, edges, boundaries) -> torch.Tensor:
    """mass_between over (-inf, b_0), [b_0, b_1), ..., [b_last, +inf): float64 [len(boundaries) + 1, dim]; underflow and
    overflow are folded into the end intervals, so the weights of a coordinate add up to 1."""
    bs = [-np.inf] + [float(x) for x in np.atleast_1d(np.asarray(boundaries, dtype=np.float64))] + [np.inf]
    if any(not bs[i] < bs[i + 1] for i in range(len(bs) - 1)):
        raise ValueError("mode_weights: boundaries must be finite and strictly increasing")
    return torch.stack([hist_mass_between(counts, edges, bs[i], bs[i + 1]) for i in range(len(bs) - 1)])


class MarginalHistograms:
    """Estimates from the pooled marginal histograms (include/ptrwm.h ptrwm_hist_args): the marginal distribution of every
    coordinate over every replica of the run.  The host class sets `_hist_mode` / `_hist_every` / `_hist_bins` /
    `_hist_range` and owns `_run` (an EngineRun).  Every read synchronises; results are CPU tensors.

    The keywords: hist='cold' or 'all' temperatures, hist_range=(lo, hi) the range of the hist_bins bins, a snapshot every
    hist_every-th step past burn-in."""

    def _check_hist_ctor(self, dim: int, hist, hist_range, hist_bins, hist_every) -> None:
        """The constructor's histogram arguments, checked before anything is built (no GPU needed)."""
        if hist_temps(hist, 1):
            check_hist_args(1, hist_every, hist_bins, hist_range, 1, dim)
        self._hist_mode, self._hist_every, self._hist_bins, self._hist_range = hist, hist_every, hist_bins, hist_range

    def _hist_kwargs(self, n_temps: int) -> dict:
        """EngineRun's histogram arguments."""
        if self._hist_mode is None:
            return {}
        return {"hist_temps": hist_temps(self._hist_mode, n_temps), "hist_every": self._hist_every, "hist_bins": self._hist_bins,
                "hist_range": self._hist_range}

    def _hist_data(self, temperature: int) -> tuple:
        if getattr(self, "_hist_mode", None) is None:
            raise RuntimeError("histograms are off: construct the sampler with hist='cold' or 'all' and hist_range=(lo, hi)")
        run = getattr(self, "_run", None)
        n_temps = len(getattr(self, "beta_ladder", [1.0]))
        temps = hist_temps(self._hist_mode, n_temps)
        t = covered_temperature(temperature, temps, "the histograms cover")
        if run is None or run.histogram() is None:  # nothing run yet, or reset(): empty counters
            lo, hi = check_hist_range(self._hist_range, self.dim)
            return torch.zeros(self.dim, self._hist_bins + 2, dtype=torch.int64), hist_edges(lo, hi, self._hist_bins)
        h = run.histogram()
        return h["counts"][t].cpu(), h["edges"]

    def marginal_histogram(self, temperature: int = 0) -> tuple:
        """(counts [dim, bins + 2] int64, edges [dim, bins + 1] float64) of `temperature`, pooled over every replica and every
        snapshot: counts[:, 0] below the range (and NaN), counts[:, -1] at or above it."""
        return self._hist_data(temperature)

    def marginal_density(self, temperature: int = 0) -> torch.Tensor:
        """counts normalised by the total and the bin width: float64 [dim, bins].  Out-of-range mass is left out of the density
        but not out of the total, so a coordinate's density integrates to its in-range fraction."""
        return hist_density(*self._hist_data(temperature))

    def quantiles(self, q, temperature: int = 0) -> torch.Tensor:
        """Marginal quantiles, float64 [len(q), dim]: linear interpolation inside the bin where the cumulative count crosses q;
        NaN where it crosses in the underflow or overflow bin."""
        return hist_quantiles(*self._hist_data(temperature), q)

    def mass_between(self, a, b, temperature: int = 0) -> torch.Tensor:
        """Fraction of the mass in [a, b) per coordinate: float64 [dim].  Exact: `a` and `b` must be bin edges (or -inf /
        +inf); anything else raises ValueError naming the nearest edges."""
        return hist_mass_between(*self._hist_data(temperature), a, b)

    def mode_weights(self, boundaries, temperature: int = 0) -> torch.Tensor:
        """mass_between over the consecutive intervals the (bin-edge) boundaries cut the line into, underflow and overflow
        folded into the end intervals: float64 [len(boundaries) + 1, dim]."""
        return hist_mode_weights(*self._hist_data(temperature), boundaries)

    def _hist_diagnostics(self) -> dict:
        if getattr(self, "_hist_mode", None) is None:
            return {}
        run = getattr(self, "_run", None)
        if run is None or run.histogram() is None:
            return {"hist_out_of_range": float("nan")}
        c = run.histogram()["counts"]
        total = int(c.sum().item())
        return {"hist_out_of_range": (int(c[..., 0].sum().item()) + int(c[..., -1].sum().item())) / total if total else float("nan")}


# ---- the warm-up tunings in the drop-in classes ------------------------------------------------------------------------------
class WarmupKeywords:
    """What the mixins of the three warm-up tunings share.  `adapt_sync` is one keyword for all of them - a callable applied to a
    window's counts at every window end, which makes shards of one run tune together (algorithms.sharding.adaptation_sync): the
    host class stores it once, as `_adapt_sync`, before it calls a mixin's `_check_*_ctor`, and passes it to EngineRun once, as
    adapt_sync=, next to the mixins' `_*_kwargs()` (EngineRun ignores it where no tuning is on)."""

    def _check_tuning(self, key: str, flag: str, check, *args, **kw) -> None:
        """One tuning's constructor keywords `kw`, checked before anything is built (no GPU needed) by `check`: its dict (None:
        off) is kept as `_<key>_args`, EngineRun's keywords - `flag` and `kw`; off: none - as `_<key>_kw`."""
        checked = check(*args, **kw, adapt_sync=self._adapt_sync)
        setattr(self, f"_{key}_args", checked)
        setattr(self, f"_{key}_kw", {flag: True, **kw} if checked is not None else {})

    @staticmethod
    def _history_before_run(first: torch.Tensor, windows: int) -> torch.Tensor:
        """A tuning's history where nothing has run yet, or after reset(): float32 [windows + 1, *first.shape] on `first`'s
        device, row 0 `first`, the rows of the windows still to run NaN."""
        rows = torch.full((windows + 1, *first.shape), float("nan"), device=first.device, dtype=torch.float32)
        rows[0] = first
        return rows

    @staticmethod
    def _rows_before_run(windows: int, *shape, device=None) -> torch.Tensor:
        """... and what it records per window: float64 [windows, *shape], NaN."""
        return torch.full((windows, *shape), float("nan"), device=device, dtype=torch.float64)


class ScaleAdaptation(WarmupKeywords):
    """Readers of the per-temperature proposal scales and of their warm-up tuning (include/ptrwm.h ptrwm_adapt_args).  The
    host class calls `_check_adapt_ctor` in its constructor, passes `_adapt_kwargs()` to EngineRun, owns `_run` and defines
    `_initial_proposal()` (the engine proposal a fresh run starts from).  Every read synchronises.

    The keywords: adapt_scale=True tunes the scale of every temperature towards the acceptance rate adapt_target in windows of
    adapt_every steps up to adapt_until (default: all of burn-in), with adapt_gain and adapt_decay; adapt_scale_bounds are
    factors on the initial scales; adapt_sync (WarmupKeywords) is applied to the pooled [T + 1] counts."""

    def _check_adapt_ctor(self, burn_in: int, adapt_scale, **kw) -> None:
        self._check_tuning("adapt", "adapt_scale", check_adapt_args, adapt_scale, max(0, int(burn_in)), **kw)

    def _adapt_kwargs(self) -> dict:
        """EngineRun's adaptation arguments."""
        return dict(self._adapt_kw)

    def _init_scales(self) -> torch.Tensor:
        run = getattr(self, "_run", None)
        return (run.init_scales if run is not None else self._initial_proposal().temp_scale).clone()

    def proposal_scales(self) -> torch.Tensor:
        """The current proposal scale of every temperature: float32 [T] on the device (the initial scales before the first
        step and after reset(); the tuned ones once warm-up has run)."""
        run = getattr(self, "_run", None)
        return run.proposal_scales() if run is not None else self._init_scales()

    def adaptation_history(self) -> dict:
        """{"scales": float32 [K + 1, T], "acceptance": float64 [K, T]} of the K = adapt_until // adapt_every adaptation
        windows: row 0 of scales the initial scales, row k + 1 those after window k; acceptance the pooled acceptance rate of
        window k (from the integer counts).  Rows of windows that have not run yet are NaN.  Device tensors."""
        if getattr(self, "_adapt_args", None) is None:
            raise RuntimeError("adaptation is off: construct the sampler with adapt_scale=True")
        run = getattr(self, "_run", None)
        if run is not None:
            h = run.adaptation_history()
            return {"scales": h["scales"], "acceptance": h["acceptance"]}
        init, K = self._init_scales(), self._adapt_args["windows"]
        return {"scales": self._history_before_run(init, K),
                "acceptance": self._rows_before_run(K, init.numel(), device=init.device)}

    def _adapt_diagnostics(self) -> dict:
        return {"adapted_scales": self.proposal_scales().cpu().tolist(), "init_scales": self._init_scales().cpu().tolist()}


# ---- preconditioned proposals in the drop-in classes ------------------------------------------------------------------------------
class Preconditioning(WarmupKeywords):
    """`proposal_cov=` and `adapt_cov=` of the sampler classes, and the readers of the proposal factor (include/ptrwm.h
    ptrwm_split_propose_precond / ptrwm_precond_update, csrc/precond.h).  The host class calls `_check_precond_ctor` in its
    constructor, passes `_precond_kwargs()` to EngineRun and owns `_run` and `dim`.  Every read synchronises; results are CPU
    tensors.

    The keywords: proposal_cov, a [dim, dim] covariance factored on the host, gives increments N(0, (var / beta_t) proposal_cov);
    adapt_cov=True learns the factor during burn-in from the cold chain's covariance, in windows of cov_adapt_every steps probed
    every cov_adapt_probe_every steps (default: one probe per window), up to cov_adapt_until (default: all of burn-in), with
    cov_adapt_memory, cov_adapt_jitter and cov_adapt_min_count of include/ptrwm.h; adapt_sync (WarmupKeywords) is applied to the
    window's covariance sums.  Such runs are split steps."""

    def _check_precond_ctor(self, dim: int, burn_in: int, proposal_cov, adapt_cov, proposal_distribution, dtype, **kw) -> None:
        """The constructor's arguments, checked before anything is built (no GPU needed).  `proposal_distribution`: the
        proposal object the caller passed (None: the class builds a Normal one)."""
        chol = check_proposal_cov(proposal_cov, int(dim))
        self._check_tuning("factor", "adapt_cov", check_cov_adapt_args, adapt_cov, max(0, int(burn_in)), int(dim), **kw)
        on = chol is not None or self._factor_args is not None
        if on and proposal_distribution is not None and type(proposal_distribution).__name__ != "NormalProposal":
            raise ValueError("proposal_cov / adapt_cov precondition the Normal proposal: "
                             f"{type(proposal_distribution).__name__} has no preconditioned form")
        if on and dtype == torch.float64:
            raise NotImplementedError("dtype=torch.float64 needs the fused kernel; preconditioned proposals run in split "
                                      "steps, which carry float32 states")
        if on and chol is None:
            chol = np.eye(int(dim), dtype=np.float32)
        self._init_chol = chol

    def _precond_kwargs(self) -> dict:
        """EngineRun's arguments: the factor where there is one, and its tuning's."""
        return {"proposal_chol": self._init_chol, **self._factor_kw} if self._init_chol is not None else {}

    def _precond_on(self) -> None:
        if getattr(self, "_init_chol", None) is None:
            raise RuntimeError("proposals are not preconditioned: construct the sampler with proposal_cov= or adapt_cov=True")

    def proposal_factor(self) -> torch.Tensor:
        """The lower-triangular factor L of the proposal, increments s_t L z: float32 [dim, dim], zeros above the diagonal - the
        initial factor before the first step and after reset(), the learned one once warm-up has run."""
        self._precond_on()
        run = getattr(self, "_run", None)
        return run.proposal_factor().cpu() if run is not None else torch.from_numpy(self._init_chol.copy())

    def proposal_covariance(self) -> torch.Tensor:
        """L L^T in float64 [dim, dim]: the covariance of the increments up to the factor (var / beta_t) of every temperature."""
        f = self.proposal_factor().double()
        return f @ f.T

    def preconditioner_history(self) -> dict:
        """{"factors": float32 [K + 1, dim, dim], "weights": float64 [K], "skipped": int} of the K = cov_adapt_until //
        cov_adapt_every windows: row 0 of factors the initial factor, row k + 1 the one in force behind window k; weights the
        running weight w behind window k.  Rows of windows that have not run yet are NaN."""
        self._precond_on()
        if self._factor_args is None:
            raise RuntimeError("the factor's tuning is off: construct the sampler with adapt_cov=True")
        run = getattr(self, "_run", None)
        if run is not None:
            h = run.preconditioner_history()
            return {"factors": h["factors"].cpu(), "weights": h["weights"].cpu(), "skipped": h["skipped"]}
        K = self._factor_args["windows"]
        return {"factors": self._history_before_run(torch.from_numpy(self._init_chol), K), "weights": self._rows_before_run(K),
                "skipped": 0}

    def _precond_diagnostics(self) -> dict:
        if getattr(self, "_init_chol", None) is None:
            return {"preconditioned": False}
        out = {"preconditioned": True, "precond_condition": cov_condition(self.proposal_covariance())}
        if self._factor_args is not None:
            h = self.preconditioner_history()
            done = int((~torch.isnan(h["weights"])).sum())
            out.update(precond_updates=done - h["skipped"], precond_updates_skipped=h["skipped"])
        else:
            out.update(precond_updates=0, precond_updates_skipped=0)
        return out


# ---- warm-up tuning of the temperature ladder in the PT class ---------------------------------------------------------------
class LadderAdaptation(WarmupKeywords):
    """Readers of the temperature ladder and of its warm-up tuning (include/ptrwm.h ptrwm_ladder_args).  The host class calls
    `_check_ladder_ctor` in its constructor once `beta_ladder` stands, passes `_ladder_kwargs()` to EngineRun and owns `_run`
    and `beta_ladder` (a list, refreshed from the run while the ladder moves).  Every read synchronises.

    The keywords: adapt_ladder=True moves the interior betas towards equal swap rates between neighbours in windows of
    ladder_every steps up to ladder_until (default: all of burn-in), with ladder_gain and ladder_decay, from a probe of every
    replica behind every ladder_probe_every-th step (default: one per window); both ends stay, the proposal scales follow their
    temperature, and adapt_sync (WarmupKeywords) is applied to the pooled [T] row."""

    def _check_ladder_ctor(self, burn_in: int, adapt_ladder, beta_ladder, **kw) -> None:
        self._check_tuning("ladder", "adapt_ladder", check_ladder_args, adapt_ladder, max(0, int(burn_in)), beta_ladder, **kw)
        self._init_beta_ladder = list(beta_ladder)

    def _ladder_kwargs(self) -> dict:
        """EngineRun's ladder arguments."""
        return dict(self._ladder_kw)

    def _refresh_beta_ladder(self, steps_before: int) -> None:
        """After an advance that began at `steps_before`: `beta_ladder` follows the run's ladder where it may have moved."""
        la, run = getattr(self, "_ladder_args", None), getattr(self, "_run", None)
        if la is not None and run is not None and steps_before < la["windows"] * la["every"]:
            self.beta_ladder = [float(b) for b in run.beta.cpu().tolist()]
            self.beta_tensor = run.beta.clone()

    def adapted_beta_ladder(self) -> list:
        """The current ladder as a list of floats: the initial one before the first step and after reset(), the tuned one once
        warm-up has run."""
        run = getattr(self, "_run", None)
        return [float(b) for b in run.beta.cpu().tolist()] if run is not None else [float(np.float32(b)) for b in self._init_beta_ladder]

    def ladder_history(self) -> dict:
        """{"betas": float32 [K + 1, T], "rates": float64 [K, T - 1], "probes": int64 [K]} of the K = ladder_until //
        ladder_every windows: row 0 of betas the initial ladder, row j + 1 the one after window j; rates every pair's mean
        swap probability over window j (from the integer counts); probes the chain-probes behind it.  Rows of windows that
        have not run yet are NaN (probes 0).  Device tensors."""
        if getattr(self, "_ladder_args", None) is None:
            raise RuntimeError("the ladder's tuning is off: construct the sampler with adapt_ladder=True")
        run = getattr(self, "_run", None)
        if run is not None:
            h = run.ladder_history()
            return {"betas": h["betas"], "rates": h["rates"], "probes": h["probes"]}
        K, init = self._ladder_args["windows"], torch.tensor(self._init_beta_ladder, dtype=torch.float32)
        return {"betas": self._history_before_run(init, K), "rates": self._rows_before_run(K, init.numel() - 1),
                "probes": torch.zeros(K, dtype=torch.int64)}

    def _ladder_diagnostics(self) -> dict:
        if getattr(self, "_ladder_args", None) is None:
            return {}
        run = getattr(self, "_run", None)
        return {"adapted_beta_ladder": self.adapted_beta_ladder(),
                "init_beta_ladder": [float(np.float32(b)) for b in self._init_beta_ladder],
                "ladder_updates_skipped": int(run._ladder.skipped.item()) if run is not None else 0}
