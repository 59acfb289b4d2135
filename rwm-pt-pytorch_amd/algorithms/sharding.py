"""Multi-GPU layout of a run: independent replicas sharded over ranks, one process per GPU.

The reference has no distributed path at all.  Replicas (chains / whole ladders) are
independent, so the sampling itself needs NO collective: rank r owns a contiguous block of global replica
ids and passes its first id as `chain_offset`, which is the Philox subsequence -- results do not depend on
the number of GPUs.  The only exchange is one tiny all-reduce(SUM) of the summary counters at the end
(RCCL over xGMI with backend "nccl"; latency-bound, a few hundred bytes).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist


def shard_range(n_total: int, rank: int, world_size: int) -> Tuple[int, int]:
    """(offset, count) of rank's contiguous block when n_total replicas are split as evenly as possible
    (the first n_total % world_size ranks get one extra)."""
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError(f"bad rank/world_size {rank}/{world_size}")
    if n_total < 0:
        raise ValueError("n_total must be >= 0")
    base, extra = divmod(n_total, world_size)
    count = base + (1 if rank < extra else 0)
    offset = rank * base + min(rank, extra)
    return offset, count


def pack_summary(summary: dict, device) -> torch.Tensor:
    """EngineRun.summary() -> one float64 vector [4T + 3] (exact for counts < 2^53)."""
    parts = [
        summary["accept_count"].double(),
        summary["sq_jump_sum"].double(),
        summary["swap_accept_count"].double(),
        torch.tensor([summary["n_replicas"], summary["swap_attempts"], summary["post_burn_steps"]], dtype=torch.float64),
    ]
    return torch.cat(parts).to(device)


def unpack_summary(vec: torch.Tensor, n_temps: int, world_size: int) -> dict:
    v = vec.detach().cpu()
    T = n_temps
    post = int(round(v[3 * T + 2].item() / world_size))  # identical on every rank
    n_rep = int(round(v[3 * T].item()))
    acc, sq, sw = v[:T], v[T:2 * T], v[2 * T:3 * T]
    denom = max(1, n_rep * post)
    attempts = int(round(v[3 * T + 1].item()))
    return {
        "n_replicas": n_rep,
        "post_burn_steps": post,
        "accept_count": acc.round().long(),
        "acceptance_rate": acc / denom,                 # per temperature
        "esjd": sq / denom,                             # per temperature
        "swap_accept_count": sw.round().long(),
        "swap_attempts": attempts,
        "swap_acceptance_rate": float(sw.sum() / attempts) if attempts else 0.0,
    }


def allreduce_summary(summary: dict, device, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job acceptance / ESJD / swap statistics from every rank's shard (one all-reduce)."""
    n_temps = summary["accept_count"].numel()
    vec = pack_summary(summary, device)
    world = 1
    if dist.is_available() and dist.is_initialized():
        world = dist.get_world_size(group)
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    return unpack_summary(vec, n_temps, world)


def allreduce_moments(moments: dict, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job moment sums from every rank's shard (EngineRun.moments(): sum / sum_sq [temps, dim], sum_logp and count
    [temps]): one SUM all-reduce of a float64 vector, separate from the summary's (pack_summary keeps its layout).
    Returns new tensors on the shards' device; the inputs are not modified.  Counts are exact below 2^53."""
    s, q, lp, n = moments["sum"], moments["sum_sq"], moments["sum_logp"], moments["count"]
    temps, dim = s.shape
    vec = torch.cat([s.reshape(-1).double(), q.reshape(-1).double(), lp.reshape(-1).double(), n.reshape(-1).double()])
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    td = temps * dim
    out = {
        "sum": vec[:td].view(temps, dim),
        "sum_sq": vec[td:2 * td].view(temps, dim),
        "sum_logp": vec[2 * td:2 * td + temps],
        "count": vec[2 * td + temps:].round().to(torch.int64),
    }
    if "every" in moments:
        out["every"] = moments["every"]
    return out


def chain_summary(chain_moments: dict) -> dict:
    """What of a shard's per-chain moments (EngineRun.chain_moments()) adds over shards, per (temperature, coordinate):
    the number of chains M, sum_c m_c, sum_c m_c^2 and sum_c s2_c of the chain means m_c and variances s2_c (ddof 1).
    `draws` [temps]: accumulated steps per chain (the same on every shard of a run)."""
    from ._engine_core import chain_mean_var

    s, q, n = chain_moments["sum"], chain_moments["sum_sq"], chain_moments["count"]
    draws = [int(v) for v in n.tolist()]
    means, variances = zip(*(chain_mean_var(s[:, t], q[:, t], draws[t]) if draws[t] >= 1 else
                             (torch.full_like(s[:, t], float("nan")),) * 2 for t in range(s.shape[1])))
    mean, var = torch.stack(means, 1), torch.stack(variances, 1)  # [M, temps, dim]
    return {"n_chains": s.shape[0], "sum_mean": mean.sum(0), "sum_mean_sq": (mean * mean).sum(0), "sum_var": var.sum(0),
            "draws": draws}


def allreduce_chain_summary(chain_moments: dict, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job Gelman-Rubin R-hat and between-chain ESS from every rank's per-chain moments: each rank reduces its own
    chains to chain_summary() - (M, sum m_c, sum m_c^2, sum s2_c) per (temperature, coordinate) - and ONE SUM all-reduce of
    that float64 vector combines them; the per-chain arrays never leave their shard.  Returns rhat / ess [temps, dim]
    (new tensors on the shards' device), n_chains (whole job) and draws."""
    from ._engine_core import rhat_ess_from_chain_summary

    cs = chain_summary(chain_moments)
    temps, dim = cs["sum_mean"].shape
    td = temps * dim
    vec = torch.cat([cs["sum_mean"].reshape(-1), cs["sum_mean_sq"].reshape(-1), cs["sum_var"].reshape(-1),
                     torch.tensor([float(cs["n_chains"])], dtype=torch.float64, device=cs["sum_mean"].device)])
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    m = int(round(float(vec[3 * td].item())))
    sm, sq, sv = (vec[i * td:(i + 1) * td].view(temps, dim) for i in range(3))
    pairs = [rhat_ess_from_chain_summary(m, sm[t], sq[t], sv[t], cs["draws"][t]) for t in range(temps)]
    return {"rhat": torch.stack([p[0] for p in pairs]), "ess": torch.stack([p[1] for p in pairs]), "n_chains": m,
            "draws": cs["draws"]}


# ---- replica flow (EngineRun.flow(); include/ptrwm.h ptrwm_flow_args) --------------------------------------------------------
def flow_up_fraction(n_up: torch.Tensor, n_down: torch.Tensor) -> torch.Tensor:
    """f(t) = n_up / (n_up + n_down) per temperature from visit counts already summed over the replicas ([T], any integer or
    float dtype): float64 [T], NaN where no walker that has touched an end has visited yet."""
    up, down = n_up.double(), n_down.double()
    return up / (up + down)  # (0 / 0 = NaN)


def flow_round_trip_rate(trips: int, n_replicas: int, n_temps: int, events: int) -> float:
    """Round trips per walker and swap event: trips / (replicas x temperatures x events); 0.0 before the first event."""
    den = n_replicas * n_temps * events
    return float(trips) / den if den > 0 else 0.0


def allreduce_flow(flow: dict, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job up-fraction and round-trip rate from every rank's flow arrays (EngineRun.flow()): ONE SUM all-reduce of an
    int64 vector - n_up and n_down summed over the local replicas ([T] each), the local trip total and the local replica
    count - separate from the summary's (pack_summary keeps its layout).  `events` is the same on every shard of a run.
    Returns up_fraction (float64 [T], a new tensor on the shards' device), round_trip_rate, round_trips_total, n_up / n_down
    ([T] int64, whole job), n_replicas and events."""
    up, down, trips = flow["n_up"], flow["n_down"], flow["round_trips"]
    n_rep, n_temps = up.shape
    vec = torch.cat([up.sum(0).to(torch.int64), down.sum(0).to(torch.int64), trips.sum().to(torch.int64).reshape(1),
                     torch.tensor([n_rep], dtype=torch.int64, device=up.device)])
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    g_up, g_down = vec[:n_temps], vec[n_temps:2 * n_temps]
    total, reps, events = int(vec[2 * n_temps].item()), int(vec[2 * n_temps + 1].item()), int(flow["events"])
    return {"up_fraction": flow_up_fraction(g_up, g_down), "round_trip_rate": flow_round_trip_rate(total, reps, n_temps, events),
            "round_trips_total": total, "n_up": g_up, "n_down": g_down, "n_replicas": reps, "events": events}


def allreduce_histogram(sampler, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job pooled marginal histograms from every rank's shard: ONE int64 SUM all-reduce of `counts` and `count` packed
    into one vector (integers: exact, whatever the order).  `sampler`: a sampler constructed with hist=, its EngineRun, or the
    dict EngineRun.histogram() returns.  Returns new tensors {"counts", "count"} on the shards' device plus "edges"; the
    shard's own arrays are not modified."""
    h = sampler
    if not isinstance(h, dict):
        run = getattr(sampler, "_run", sampler)
        h = run.histogram() if run is not None and hasattr(run, "histogram") else None
        if h is None:
            raise RuntimeError("allreduce_histogram: histograms are off, or nothing has run yet")
    counts, count = h["counts"], h["count"]
    vec = torch.cat([counts.reshape(-1).to(torch.int64), count.reshape(-1).to(torch.int64)])
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    n = counts.numel()
    return {"counts": vec[:n].view(counts.shape), "count": vec[n:].view(count.shape), "edges": h.get("edges")}


def allreduce_autocorr(sampler, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job pooled lagged autocovariance sums from every rank's shard: ONE float64 SUM all-reduce of `sxy`, `head`, `tail`
    and `pairs` packed into one vector (the pair counts ride as doubles: exact below 2^53).  `sampler`: a sampler constructed
    with acf=, its EngineRun, or the dict EngineRun.autocorr_sums() returns.  Returns new tensors {"sxy", "head", "tail",
    "pairs"} on the shards' device plus "every"; the shard's own arrays are not modified.  The estimators
    (algorithms._engine_core.acf_autocovariance, acf_autocorrelation, sokal_window) take one temperature's rows of them."""
    a = sampler
    if not isinstance(a, dict):
        run = getattr(sampler, "_run", sampler)
        a = run.autocorr_sums() if run is not None and hasattr(run, "autocorr_sums") else None
        if a is None:
            raise RuntimeError("allreduce_autocorr: the autocovariance is off, or nothing has run yet")
    parts = [a[k] for k in ("sxy", "head", "tail", "pairs")]
    vec = torch.cat([p.reshape(-1).to(torch.float64) for p in parts])
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    out, at = {"every": a.get("every")}, 0
    for k, p in zip(("sxy", "head", "tail", "pairs"), parts):
        out[k] = vec[at:at + p.numel()].view(p.shape).to(p.dtype)
        at += p.numel()
    return out


def allreduce_covariance(sampler, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job pooled covariance from every rank's shard: ONE float64 SUM all-reduce of `sxx`, `sx` and `count` packed into
    one vector (the count rides as a double: exact below 2^53).  `sampler`: a sampler constructed with cov=, its EngineRun, or
    the dict EngineRun.covariance_sums() returns.  Returns new tensors {"sxx", "sx", "count"} on the shards' device, "every",
    and "covariance": float64 [temps, dim, dim] on the CPU, the whole job's covariance of every covered temperature
    (algorithms._engine_core.cov_covariance); the shard's own arrays are not modified."""
    from ._engine_core import cov_covariance

    a = sampler
    if not isinstance(a, dict):
        run = getattr(sampler, "_run", sampler)
        a = run.covariance_sums() if run is not None and hasattr(run, "covariance_sums") else None
        if a is None:
            raise RuntimeError("allreduce_covariance: the covariance is off, or nothing has run yet")
    parts = [a[k] for k in ("sxx", "sx", "count")]
    vec = torch.cat([p.reshape(-1).to(torch.float64) for p in parts])
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    out, at = {"every": a.get("every")}, 0
    for k, p in zip(("sxx", "sx", "count"), parts):
        out[k] = vec[at:at + p.numel()].view(p.shape).to(p.dtype)
        at += p.numel()
    out["covariance"] = torch.stack([cov_covariance(out["sxx"][t], out["sx"][t], out["count"]) for t in range(out["sxx"].shape[0])])
    return out


ENERGY_SUMS = ("count", "nonfinite", "s1", "s2", "colder", "hotter")


def energy_rescale(sums: dict, ref_common) -> dict:
    """A shard's log-density sums (EngineRun.energy_sums()) taken to the level `ref_common` [n_temps], on the host in float64:
    colder[:, t] *= exp((beta[t-1] - beta[t]) (ref[t] - ref_common[t])), hotter[:, t] *= exp((beta[t+1] - beta[t]) (ref[t] -
    ref_common[t])); where the two levels agree - a pinned ref - the factor is exactly 1.  A sum that is zero stays zero.
    New CPU tensors; the shard's own arrays are not modified."""
    out = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in sums.items()}
    beta, ref = out["beta"].to(torch.float64), out["ref"].to(torch.float64)
    common = torch.as_tensor(ref_common).detach().cpu().to(torch.float64)
    shift = ref - common
    n_temps = beta.numel()
    if n_temps > 1:
        for name, to, at in (("colder", slice(0, n_temps - 1), slice(1, n_temps)), ("hotter", slice(1, n_temps), slice(0, n_temps - 1))):
            factor = torch.exp((beta[to] - beta[at]) * shift[at])
            cols = out[name][:, at]
            out[name][:, at] = torch.where(cols != 0, cols * factor, cols)
    out["ref"] = common
    return out


def allreduce_energy(sampler, group: Optional[dist.ProcessGroup] = None) -> dict:
    """Whole-job log-density sums along the ladder from every rank's shard.  A tiny MAX all-reduce of `ref` gives the common
    level (a shard that has not chosen one yet stands aside); every shard rescales its two exponential sums to it on the host
    (energy_rescale: the identity under a pinned ref); ONE float64 SUM all-reduce of the sums packed into one vector follows
    (the counts ride as doubles: exact below 2^53).  `sampler`: a sampler constructed with energy=True, its EngineRun, or the
    dict EngineRun.energy_sums() returns.  Returns new tensors {"count", "nonfinite", "s1", "s2", "colder", "hotter", "ref"} on
    the shards' device plus "beta" and "every" - what algorithms._engine_core's energy_moments_from_sums,
    stepping_stones_from_sums and thermodynamic_integral_from_sums take; the shard's own arrays are not modified."""
    a = sampler
    if not isinstance(a, dict):
        run = getattr(sampler, "_run", sampler)
        a = run.energy_sums() if run is not None and hasattr(run, "energy_sums") else None
        if a is None:
            raise RuntimeError("allreduce_energy: the log-density sums are off, or nothing has run yet")
    device = a["count"].device
    chosen = bool(int(torch.as_tensor(a["ref_set"]).reshape(-1)[0]) != 0)
    ref = a["ref"].detach().to(torch.float64).clone() if chosen else torch.full_like(a["ref"], float("-inf"), dtype=torch.float64)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(ref, op=dist.ReduceOp.MAX, group=group)
    ref = torch.where(torch.isinf(ref), torch.zeros_like(ref), ref)  # (no shard has chosen: nothing has been added anywhere)
    mine = energy_rescale(a, ref)
    parts = [mine[k] for k in ENERGY_SUMS]
    vec = torch.cat([p.reshape(-1).to(torch.float64) for p in parts]).to(device)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    out, at = {"ref": ref.to(device), "ref_set": torch.ones(1, dtype=torch.int32, device=device), "beta": a["beta"],
               "every": a.get("every")}, 0
    for k, p in zip(ENERGY_SUMS, parts):
        out[k] = vec[at:at + p.numel()].view(p.shape).to(p.dtype)
        at += p.numel()
    return out


# ---- warm-up tuning of the proposal scale and of the ladder (include/ptrwm.h ptrwm_adapt_args, ptrwm_ladder_args) ---------------
def adaptation_sync(group: Optional[dist.ProcessGroup] = None):
    """The `adapt_sync=` callable of a sharded run, for both tunings: all-reduces (SUM) the pooled int64 counts of a window in
    place, over `group` - [n_temps + 1] for the scale's (adapt_scale=True), [n_temps] for the ladder's (adapt_ladder=True).  Every rank then applies the same update to the same integers, so a sharded run adapts - and samples - exactly
    as the unsharded one.  Without an initialised process group the counts are left as they are (one shard)."""

    def sync(pooled: torch.Tensor) -> torch.Tensor:
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(pooled, op=dist.ReduceOp.SUM, group=group)
        return pooled

    return sync
