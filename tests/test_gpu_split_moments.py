"""The moment kernels of split steps (capi.hip split_moments_kernel, split_chain_moments_kernel; include/ptrwm.h
ptrwm_split_moments, ptrwm_split_chain_moments) on their own, at the sizes user-defined targets reach.

No step kernel in the way: a plan without a target over a hand-made float state and log-density, one call, and plain NumPy
in float64 as the yardstick - sums of x, x * x and logp over the chains, for the first `temps` temperatures.  Every column
(t, d) has a mean of its own, so an element read from, or added to, another column's place changes the sums far beyond the
tolerance.  The shapes: more covered elements than the workgroup's 256 threads (the pooled kernel's stride), temps < n_temps
(the chain stride is not the number of covered elements), a partial last tile of chains, one thread's worth of work, and the
widest state the ABI accepts.

Per chain the sums are sequential in fp64 - the header's contract - so they are compared bit for bit.  Pooled sums are added
by atomics in any order: |got - want| <= RTOL * sum |terms|, the RTOL of tests/test_gpu_moments.py; at most 2 x 600 fp64
additions in any order err by less than 1200 * 2^-53 = 1.4e-13 of the sum of magnitudes.  Counts are exact.
"""
import numpy as np
import pytest
import torch

import helpers as H
import ptrwm_hip as E
from test_gpu_moments import RTOL

pytestmark = pytest.mark.gpu

#         dim  T   temps chains
CASES = [(30, 10, 10, 257),     # 300 elements: the pooled kernel's stride; a second tile of one chain
         (30, 12, 5, 600),      # temps < n_temps: chain stride 360 against 150 elements; three tiles, the last partial
         (104, 256, 256, 300),  # the widest state: 26 624 elements, 104 strides; 31 200 workgroups of the per-chain kernel
         (1, 256, 256, 3),      # one coordinate: every element another temperature
         (3, 2, 1, 1)]          # three live threads
IDS = [f"d{d}_T{T}_t{t}_c{c}" for d, T, t, c in CASES]


def hand_made(dim, T, Cn):
    """x[c, t, d] = mu[t, d] + z and a log-density, float32; mu a ramp over the column index t * dim + d."""
    rng = np.random.default_rng(7 * dim + 3 * T + Cn)
    mu = np.linspace(-3.0, 3.0, T * dim).reshape(T, dim)
    x = (mu[None] + rng.standard_normal((Cn, T, dim))).astype(np.float32)
    lp = (-5.0 + 3.0 * rng.standard_normal((Cn, T)) - np.arange(T)[None, :]).astype(np.float32)
    return x, lp


def make_plan(device, x, lp, burn_in=0):
    Cn, T, dim = x.shape
    st, logp = torch.tensor(x, device=device), torch.tensor(lp, device=device)
    plan = E.RunPlan(None, H.proposal_spec("Normal", dim, np.ones(T, np.float32), base_variance_scalar=1.0).engine(device), state=st,
                     logp=logp, beta=torch.ones(T, device=device), burn_in=burn_in)
    return plan, st, logp


def bind(plan, device, kind, Cn, temps, dim, extras, every=1):
    lead = (Cn,) if kind == "chain" else ()
    acc = {"sum": torch.zeros(*lead, temps, dim, dtype=torch.float64, device=device),
           "sum_sq": torch.zeros(*lead, temps, dim, dtype=torch.float64, device=device),
           "sum_logp": torch.zeros(*lead, temps, dtype=torch.float64, device=device) if extras else None,
           "count": torch.zeros(temps, dtype=torch.int64, device=device) if extras else None}
    (plan.set_chain_moments if kind == "chain" else plan.set_moments)(acc["sum"], acc["sum_sq"], sum_logp=acc["sum_logp"], count=acc["count"],
                                                                      every=every)
    return acc


def fetch(acc):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in acc.items() if v is not None}


def check(got, kind, x, lp, temps, times, what):
    """`got` after `times` calls on the same state against the float64 sums."""
    Cn = x.shape[0]
    x64, lp64 = x[:, :temps].astype(np.float64), lp[:, :temps].astype(np.float64)
    if kind == "chain":  # 0 + v, then + v: sequential, and exact
        assert np.array_equal(got["sum"], times * x64), f"{what}: sum"
        assert np.array_equal(got["sum_sq"], times * (x64 * x64)), f"{what}: sum_sq"
        if "sum_logp" in got:
            assert np.array_equal(got["sum_logp"], times * lp64), f"{what}: sum_logp"
            assert got["count"].tolist() == [times] * temps, f"{what}: count"  # (accumulated steps)
        return
    for k, terms in (("sum", x64), ("sum_sq", x64 * x64), ("sum_logp", lp64)):
        if k not in got:
            continue
        want, mag = times * terms.sum(0), times * np.abs(terms).sum(0)
        err = np.abs(got[k] - want)
        print(f"{what}: {k} worst |got - want| / sum|terms| = {np.max(err / mag):.3e} (bound {RTOL:.0e})")
        bad = np.argwhere(~(err <= RTOL * mag))
        assert bad.size == 0, f"{what}: {k}: {len(bad)} elements differ, the first {bad[:5].tolist()}"
    if "count" in got:
        assert got["count"].tolist() == [times * Cn] * temps, f"{what}: count"  # (accumulated replicas)


@pytest.mark.parametrize("extras", [True, False], ids=["logp_count", "sums_only"])
@pytest.mark.parametrize("kind", ["pooled", "chain"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_call_equals_the_float64_sums_and_a_second_doubles_them(device, case, kind, extras):
    dim, T, temps, Cn = case
    x, lp = hand_made(dim, T, Cn)
    plan, st, logp = make_plan(device, x, lp)
    acc = bind(plan, device, kind, Cn, temps, dim, extras)
    for times in (1, 2):
        plan.split_moments(0)
        check(fetch(acc), kind, x, lp, temps, times, f"{kind} after {times} call(s)")
    assert torch.equal(st.cpu(), torch.tensor(x)) and torch.equal(logp.cpu(), torch.tensor(lp))  # the kernels only read


@pytest.mark.parametrize("kind", ["pooled", "chain"])
def test_a_step_that_is_not_due_leaves_every_accumulator_at_zero(device, kind):
    """Burn-in 4, every 2: step counters 3 (no multiple) and 4 (in burn-in) accumulate nothing, 6 does - decided on the host
    from the step argument, and on the device from a device_step counter."""
    dim, T, temps, Cn = CASES[1]
    x, lp = hand_made(dim, T, Cn)
    plan, _, _ = make_plan(device, x, lp, burn_in=4)

    def all_zero(acc):
        return all(not v.any() for v in fetch(acc).values())

    acc = bind(plan, device, kind, Cn, temps, dim, True, every=2)
    plan.split_moments(2)  # step counter 3
    plan.split_moments(3)  # step counter 4
    assert all_zero(acc)
    plan.split_moments(5)  # step counter 6
    check(fetch(acc), kind, x, lp, temps, 1, f"{kind}, host step")
    acc = bind(plan, device, kind, Cn, temps, dim, True, every=2)
    counter = torch.full((1,), 2, dtype=torch.int64, device=device)
    plan.set_device_step(counter)
    plan.split_moments(0)  # counter + 0: step counter 3
    plan.split_moments(1)  # step counter 4
    assert all_zero(acc)
    counter.fill_(4)
    plan.split_moments(0)  # step counter 5
    assert all_zero(acc)
    plan.split_moments(1)  # step counter 6
    check(fetch(acc), kind, x, lp, temps, 1, f"{kind}, device step")
    plan.split_moments(3)  # step counter 8
    check(fetch(acc), kind, x, lp, temps, 2, f"{kind}, device step")
    plan.set_device_step(None)
