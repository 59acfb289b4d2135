"""Starting points on the GPU (include/ptrwm.h ptrwm_init_states, EngineRun's init_box / per-replica initial_state, the
classes' initial_states / init_box).

The kernel's rows are compared BIT FOR BIT with tests/init_reference.expected_box_starts - a NumPy float32 restatement of
the header's draw on the oracle's Philox - never with the code under test: attempt 0 over shapes chosen for tile tails
(the kernel works on tiles of 64 rows), dim not a multiple of four (one Philox block per four coordinates), ladders longer
than a wave and the widest row; redraws that must touch the rows with a non-finite log-density and nothing else;
support-aware starts through EngineRun; invariance to sharding; the classes; and what the feature is for: R-hat that sees
chains sitting in different modes."""
import warnings

import numpy as np
import pytest
import torch

import ptrwm_hip as E
from init_reference import expected_box_starts

pytestmark = pytest.mark.gpu

GUARD = 8  # sentinel elements on either side of a state array (a multiple of four: `misalign` alone sets the alignment)


def _plan(device, Cn, T, D, *, seed, chain_offset=0, f64=False, misalign=0):
    """A target-less plan over a state array that sits `misalign` elements into its allocation, between sentinels."""
    dt = torch.float64 if f64 else torch.float32
    n = Cn * T * D
    buf = torch.full((GUARD + misalign + n + GUARD,), -777.0, device=device, dtype=dt)
    state = buf[GUARD + misalign:GUARD + misalign + n].view(Cn, T, D)
    logp = torch.zeros(Cn, T, device=device, dtype=torch.float32)
    prop = E.Proposal(E.PROPOSAL_NORMAL, temp_scale=torch.ones(T, device=device))
    plan = E.RunPlan(None, prop, state=state, logp=logp, beta=torch.ones(T, device=device), seed=seed,
                     chain_offset=chain_offset)
    return plan, buf, state, logp


def _guards_intact(buf, misalign, n):
    b = buf.cpu().numpy()
    return np.all(b[:GUARD + misalign] == -777.0) and np.all(b[GUARD + misalign + n:] == -777.0)


def _bounds(device, lo, hi, D):
    f = lambda b: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(b, np.float32), (D,)))).to(device)  # noqa: E731
    return f(lo), f(hi)


SHAPES = [(70, 1, 3), (33, 5, 30), (5, 64, 7), (3, 130, 41), (4, 3, 104)]


@pytest.mark.parametrize("chain_offset", [0, 2**32 + 5], ids=["offset0", "offset2p32"])
@pytest.mark.parametrize("per_temperature", [False, True], ids=["shared", "per_temperature"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_attempt_zero_equals_the_restatement_bit_for_bit(device, shape, per_temperature, chain_offset):
    Cn, T, D = shape
    seed = 0x1234_5678_9ABC_DEF0 + D
    plan, buf, state, _ = _plan(device, Cn, T, D, seed=seed, chain_offset=chain_offset)
    lo, hi = _bounds(device, -20.0, 20.0, D)
    plan.init_states(lo, hi, attempt=0, per_temperature=per_temperature)
    torch.cuda.synchronize()
    want = expected_box_starts(seed, chain_offset, Cn, T, D, -20.0, 20.0, 0, per_temperature)
    got = state.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert _guards_intact(buf, 0, Cn * T * D)


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_a_state_array_off_the_16_byte_grid(device, misalign):
    """The tile leaves through stage_copy: whole aligned vectors plus ragged ends, whatever the array's alignment."""
    Cn, T, D = 33, 5, 30
    plan, buf, state, logp = _plan(device, Cn, T, D, seed=99, misalign=misalign)
    assert state.data_ptr() % 16 == 4 * misalign
    lo, hi = _bounds(device, -1.0, 3.0, D)
    plan.init_states(lo, hi, per_temperature=True)
    torch.cuda.synchronize()
    want = expected_box_starts(99, 0, Cn, T, D, -1.0, 3.0, 0, True)
    assert np.array_equal(state.cpu().numpy(), want) and _guards_intact(buf, misalign, Cn * T * D)
    # ... and a redraw of a few rows of it
    bad = np.zeros((Cn, T), bool)
    bad.reshape(-1)[[0, 63, 64, 100, Cn * T - 1]] = True
    logp.copy_(torch.from_numpy(np.where(bad, -np.inf, 0.0).astype(np.float32)))
    plan.init_states(lo, hi, attempt=2, per_temperature=True)
    torch.cuda.synchronize()
    want2 = np.where(bad[..., None], expected_box_starts(99, 0, Cn, T, D, -1.0, 3.0, 2, True), want)
    assert np.array_equal(state.cpu().numpy(), want2) and _guards_intact(buf, misalign, Cn * T * D)


def test_double_states_hold_the_widened_float(device):
    Cn, T, D = 33, 5, 30
    plan, buf, state, logp = _plan(device, Cn, T, D, seed=4242, chain_offset=2**32 + 5, f64=True)
    lo, hi = _bounds(device, -20.0, 20.0, D)
    plan.init_states(lo, hi, per_temperature=True)
    torch.cuda.synchronize()
    want = expected_box_starts(4242, 2**32 + 5, Cn, T, D, -20.0, 20.0, 0, True)
    got = state.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))
    assert _guards_intact(buf, 0, Cn * T * D)
    # a redraw stores the rewritten rows only
    bad = np.zeros((Cn, T), bool)
    bad.reshape(-1)[[3, 64, 65, 130, 164]] = True
    logp.copy_(torch.from_numpy(np.where(bad, np.nan, -1.0).astype(np.float32)))
    marked = state.clone()
    marked[torch.from_numpy(~bad).to(device)] += 2.0 ** -40  # low bits a float cannot hold: kept rows must keep them
    state.copy_(marked)
    plan.init_states(lo, hi, attempt=1, per_temperature=True)
    torch.cuda.synchronize()
    want1 = expected_box_starts(4242, 2**32 + 5, Cn, T, D, -20.0, 20.0, 1, True).astype(np.float64)
    assert np.array_equal(state.cpu().numpy(), np.where(bad[..., None], want1, marked.cpu().numpy()))
    assert _guards_intact(buf, 0, Cn * T * D)


def test_a_box_with_its_own_bounds_per_coordinate(device):
    Cn, T, D = 70, 2, 7
    rng = np.random.default_rng(5)
    lo = rng.normal(0.0, 5.0, D).astype(np.float32)
    hi = (lo + rng.uniform(0.0, 9.0, D)).astype(np.float32)
    hi[2] = lo[2]  # a coordinate pinned to one value
    plan, buf, state, _ = _plan(device, Cn, T, D, seed=31337)
    plan.init_states(*_bounds(device, lo, hi, D))
    torch.cuda.synchronize()
    want = expected_box_starts(31337, 0, Cn, T, D, lo, hi, 0, False)
    got = state.cpu().numpy()
    assert np.array_equal(got, want) and np.all(got[..., 2] == lo[2])
    assert np.all(got >= lo) and np.all(got <= hi)


def _scattered_logp(rng, Cn, T):
    """Finite values with -inf, +inf and NaN scattered through them: first and last row of the batch, both sides of a
    tile boundary, and one tile (rows 128..191) with nothing to redraw where the batch is long enough."""
    lp = rng.normal(-30.0, 10.0, Cn * T).astype(np.float32)
    kinds = np.array([-np.inf, np.inf, np.nan], np.float32)
    idx = rng.choice(Cn * T, size=max(6, Cn * T // 5), replace=False)
    idx = np.union1d(idx, [0, 63, 64, Cn * T - 1])
    idx = idx[(idx < 128) | (idx >= 192)]
    lp[idx] = kinds[np.arange(idx.size) % 3]
    return lp.reshape(Cn, T)


@pytest.mark.parametrize("fallback", [False, True], ids=["redraw", "fallback"])
@pytest.mark.parametrize("shape", [(70, 1, 3), (33, 5, 30), (3, 130, 41)], ids=["70x1x3", "33x5x30", "3x130x41"])
def test_a_redraw_touches_the_rows_without_a_finite_logp_and_nothing_else(device, shape, fallback):
    Cn, T, D = shape
    rng = np.random.default_rng(Cn * 100 + D)
    seed, off = 2024 + D, 11
    plan, buf, state, logp = _plan(device, Cn, T, D, seed=seed, chain_offset=off)
    lo, hi = _bounds(device, -0.1, 1.1, D)
    before = rng.normal(0.0, 3.0, (Cn, T, D)).astype(np.float32)
    before.reshape(-1)[::17] = np.float32(np.nan)  # kept rows are copied as bits, whatever they hold
    state.copy_(torch.from_numpy(before))
    lp = _scattered_logp(rng, Cn, T)
    logp.copy_(torch.from_numpy(lp))
    bad = ~np.isfinite(lp)
    assert bad.any() and (~bad).any() and np.isnan(lp).any() and np.isposinf(lp).any() and np.isneginf(lp).any()
    point = rng.uniform(0.2, 0.8, D).astype(np.float32)
    plan.init_states(lo, hi, attempt=3, per_temperature=True,
                     fallback=torch.from_numpy(point).to(device) if fallback else None)
    torch.cuda.synchronize()
    new = np.broadcast_to(point, (Cn, T, D)) if fallback else expected_box_starts(seed, off, Cn, T, D, -0.1, 1.1, 3, True)
    want = np.where(bad[..., None], new, before)
    got = state.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert np.array_equal(logp.cpu().numpy().view(np.uint32), lp.view(np.uint32))  # read, never written
    assert _guards_intact(buf, 0, Cn * T * D)


def test_a_batch_of_finite_logp_is_left_alone(device):
    Cn, T, D = 33, 5, 30
    plan, buf, state, logp = _plan(device, Cn, T, D, seed=1)
    before = torch.randn(Cn, T, D, device=device)
    state.copy_(before)
    logp.copy_(torch.randn(Cn, T, device=device) * 1e30)  # huge, negative zero, denormal: all finite
    logp.view(-1)[:3] = torch.tensor([-0.0, 1e-45, 3.4e38], device=device)
    for fb in (None, torch.zeros(D, device=device)):
        plan.init_states(*_bounds(device, 0.0, 1.0, D), attempt=3, fallback=fb)
    torch.cuda.synchronize()
    assert torch.equal(state, before) and _guards_intact(buf, 0, Cn * T * D)


# ---- EngineRun ------------------------------------------------------------------------------------------------------
def _engine_run(device, target, dim, betas, n_replicas, *, point, seed, chain_offset=0, **kw):
    from algorithms._engine_core import EngineRun
    from proposal_distributions import NormalProposal

    prop = NormalProposal(dim, 2.38 ** 2 / dim, 1.0, device, torch.float32, None)
    return EngineRun(target_dist=target, proposal=prop.engine_proposal(list(betas) if len(betas) > 1 else None),
                     beta_ladder=list(betas), dim=dim, device=device, n_replicas=n_replicas, initial_state=point,
                     burn_in=kw.pop("burn_in", 0), swap_every=kw.pop("swap_every", 5), swap_mode="exchange",
                     swap_order="sequential", seed=seed, chain_offset=chain_offset, **kw)


def test_engine_run_redraws_starts_outside_the_support(device):
    """IIDBeta lives on (0, 1)^2; the box (-0.1, 1.1)^2 puts a row inside with probability (1 / 1.2)^2 = 0.69, so all 8
    attempts miss with probability 0.31^8 = 8e-5: every row ends on its first attempt inside, or on the point."""
    from target_distributions import IIDBetaTorch

    Cn, D, seed, attempts = 256, 2, 20260, 8
    target = IIDBetaTorch(D, device=device)
    point = np.full(D, 0.5, np.float32)
    run = _engine_run(device, target, D, [1.0], Cn, point=point, seed=seed, init_box=(-0.1, 1.1), init_attempts=attempts)
    assert run.init_mode == "box"
    state, logp = run.state.cpu().numpy(), run.logp.cpu().numpy()
    assert np.all(np.isfinite(logp))
    et = target.engine_target()
    want = np.broadcast_to(point, (Cn, 1, D)).copy()
    settled = np.zeros((Cn, 1), bool)
    for a in range(attempts):
        rows = expected_box_starts(seed, 0, Cn, 1, D, -0.1, 1.1, a, False)
        ok = np.isfinite(E.logdensity(et, torch.from_numpy(rows.reshape(-1, D)).to(device)).cpu().numpy()).reshape(Cn, 1)
        take = ok & ~settled
        want[take] = rows[take]
        settled |= take
        if a == 0:
            assert 0.55 < ok.mean() < 0.82  # 0.69 of 256 rows: the box does reach outside the support
    assert (~settled).sum() <= Cn // 100  # at most 1 % of the rows fall back to the point (for this seed: see above)
    assert np.array_equal(state, want)
    assert np.array_equal(logp.reshape(-1), E.logdensity(et, run.state.view(-1, D)).cpu().numpy())
    assert np.all(state > 0.0) and np.all(state < 1.0)
    # one attempt only: what misses goes straight to the point
    one = _engine_run(device, target, D, [1.0], Cn, point=point, seed=seed, init_box=(-0.1, 1.1), init_attempts=1)
    rows = expected_box_starts(seed, 0, Cn, 1, D, -0.1, 1.1, 0, False)
    ok = np.isfinite(E.logdensity(et, torch.from_numpy(rows.reshape(-1, D)).to(device)).cpu().numpy()).reshape(Cn, 1, 1)
    assert np.array_equal(one.state.cpu().numpy(), np.where(ok, rows, point))
    # a box wholly outside the support, and a point outside it too: nothing to fall back to
    with pytest.raises(ValueError, match="256 of 256 starting rows"):
        _engine_run(device, target, D, [1.0], Cn, point=np.full(D, 2.0, np.float32), seed=seed, init_box=(1.5, 2.5))
    # ... with a point inside, every row lands on it
    res = _engine_run(device, target, D, [1.0], Cn, point=point, seed=seed, init_box=(1.5, 2.5))
    assert np.all(res.state.cpu().numpy() == 0.5)


def test_starts_and_runs_do_not_depend_on_the_sharding(device):
    from target_distributions import RoughCarpetDistributionTorch

    D, betas, seed = 30, [1.0, 0.5, 0.25, 0.1], 777
    target = RoughCarpetDistributionTorch(D, device=device, mode_centers=[-15.0, 0.0, 15.0])
    kw = dict(point=np.zeros(D), seed=seed, init_box=(-20.0, 20.0), burn_in=10, swap_every=5)
    whole = _engine_run(device, target, D, betas, 40, **kw)
    parts = [_engine_run(device, target, D, betas, 20, chain_offset=off, **kw) for off in (0, 20)]
    assert np.array_equal(whole.state.cpu().numpy(), expected_box_starts(seed, 0, 40, 4, D, -20.0, 20.0, 0, False))

    def same():
        torch.cuda.synchronize()
        for name in ("state", "logp", "n_accept", "swap_accept"):
            a = getattr(whole, name).cpu().numpy()
            b = np.concatenate([getattr(p, name).cpu().numpy() for p in parts])
            assert np.array_equal(a, b), name

    same()
    for r in [whole] + parts:
        r.advance(50)
    same()
    assert not np.array_equal(whole.state[:20].cpu().numpy(), whole.state[20:].cpu().numpy())
    # every temperature its own start: invariant all the same
    kw["init_per_temperature"] = True
    whole = _engine_run(device, target, D, betas, 40, **kw)
    parts = [_engine_run(device, target, D, betas, 20, chain_offset=off, **kw) for off in (0, 20)]
    assert np.array_equal(whole.state.cpu().numpy(), expected_box_starts(seed, 0, 40, 4, D, -20.0, 20.0, 0, True))
    same()


# ---- the classes ----------------------------------------------------------------------------------------------------
def _rc(dim, device):
    from target_distributions import RoughCarpetDistributionTorch

    return RoughCarpetDistributionTorch(dim, device=device, mode_centers=[-15.0, 0.0, 15.0])


def _pt(device, dim, betas, R, **kw):
    from algorithms import ParallelTemperingRWM_GPU_Optimized

    return ParallelTemperingRWM_GPU_Optimized(dim, 2.38 ** 2 / dim, _rc(dim, device), beta_ladder=list(betas), swap_every=5,
                                              burn_in=5, device=device, num_replicas=R, seed=4711, **kw)


def _rwm(device, dim, n, target=None, **kw):
    from algorithms import RandomWalkMH_GPU_Optimized

    return RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim, target if target is not None else _rc(dim, device), burn_in=5,
                                      device=device, num_chains=n, seed=4711, **kw)


def test_given_states_arrive_verbatim(device):
    D, betas, R = 7, [1.0, 0.5, 0.2], 5
    rng = np.random.default_rng(8)
    per_replica = rng.normal(0.0, 10.0, (R, D)).astype(np.float32)
    per_row = rng.normal(0.0, 10.0, (R, 3, D)).astype(np.float32)
    for given, want in ((per_replica, np.repeat(per_replica[:, None], 3, 1)), (per_row, per_row),
                        (torch.from_numpy(per_row).to(device), per_row), (torch.from_numpy(per_replica), np.repeat(per_replica[:, None], 3, 1))):
        alg = _pt(device, D, betas, R, initial_states=given, pre_allocate_steps=10)
        alg._ensure_started()
        run = alg._run
        assert run.init_mode == "states" and alg.get_diagnostic_info()["init"] == "states"
        assert np.array_equal(run.state.cpu().numpy(), want)
        want_lp = E.logdensity(run.target, torch.from_numpy(want.reshape(-1, D)).to(device)).cpu().numpy()
        assert np.array_equal(run.logp.cpu().numpy().reshape(-1), want_lp)
        # the stored chains open with replica 0's actual start
        assert np.array_equal(alg.get_cold_chain_gpu()[0].cpu().numpy(), want[0, 0])
        assert np.array_equal(alg._trace[0, 0].cpu().numpy(), want[0])
        if torch.is_tensor(given) and given.is_cuda:
            assert run.state.data_ptr() != given.data_ptr()  # a copy: the caller's tensor is never stepped in place
    chains = rng.normal(0.0, 10.0, (70, D)).astype(np.float32)
    for pre in (20, None):
        alg = _rwm(device, D, 70, initial_states=chains, pre_allocate_steps=pre)
        alg.step()
        torch.cuda.synchronize()
        first = alg.get_chain_gpu()[0].cpu().numpy()
        assert np.array_equal(first, chains[0]) and alg.get_diagnostic_info()["init"] == "states"
    alg = _rwm(device, D, 70, initial_states=chains)
    alg._ensure_started()
    assert np.array_equal(alg.current_states.cpu().numpy(), chains)
    assert np.array_equal(alg._run.logp.cpu().numpy().reshape(-1),
                          E.logdensity(alg._run.target, torch.from_numpy(chains).to(device)).cpu().numpy())


def test_the_point_given_per_replica_is_the_default_run(device):
    D, betas, R = 30, [1.0, 0.5, 0.2, 0.05], 9
    base = _pt(device, D, betas, R, trace="none")
    point = torch.as_tensor(np.asarray(base._initial_state), dtype=torch.float32)
    runs = [base, _pt(device, D, betas, R, trace="none", initial_states=point.to(device).expand(R, D)),
            _pt(device, D, betas, R, trace="none", initial_states=point.expand(R, 4, D).numpy())]
    for alg in runs:
        alg._advance(40)
    torch.cuda.synchronize()
    assert base.get_diagnostic_info()["init"] == "point" and runs[1].get_diagnostic_info()["init"] == "states"
    for alg in runs[1:]:
        for name in ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_ord"):
            assert np.array_equal(getattr(alg._run, name).cpu().numpy(), getattr(base._run, name).cpu().numpy()), name
    assert base._run.n_accept.sum().item() > 0


def test_a_box_start_opens_the_stored_chain_and_survives_reset(device):
    D = 4
    want = expected_box_starts(4711, 0, 6, 3, D, -20.0, 20.0, 0, False)
    alg = _pt(device, D, [1.0, 0.5, 0.2], 6, init_box=(-20.0, 20.0), pre_allocate_steps=10)
    alg.generate_samples(10)
    assert alg.get_diagnostic_info()["init"] == "box"
    assert np.array_equal(alg._trace[0, 0].cpu().numpy(), want[0])
    end = alg._run.state.clone()
    alg.reset()
    alg.generate_samples(10)
    assert np.array_equal(alg._trace[0, 0].cpu().numpy(), want[0]) and torch.equal(alg._run.state, end)
    # per temperature
    alg = _pt(device, D, [1.0, 0.5, 0.2], 6, init_box=(-20.0, 20.0), init_per_temperature=True)
    alg._ensure_started()
    assert np.array_equal(alg._run.state.cpu().numpy(), expected_box_starts(4711, 0, 6, 3, D, -20.0, 20.0, 0, True))
    # RWM, with and without pre-allocated storage
    want = expected_box_starts(4711, 0, 70, 1, D, -20.0, 20.0, 0, False)[:, 0]
    for pre in (12, None):
        alg = _rwm(device, D, 70, init_box=(-20.0, 20.0), pre_allocate_steps=pre)
        alg._ensure_started()
        assert np.array_equal(alg.current_states.cpu().numpy(), want)
        alg.generate_samples(7)
        assert np.array_equal(alg.get_chain_gpu()[0].cpu().numpy(), want[0])
        end = alg.current_states.clone()
        alg.reset()
        assert alg.current_states is None
        alg.generate_samples(7)
        assert np.array_equal(alg.get_chain_gpu()[0].cpu().numpy(), want[0]) and torch.equal(alg.current_states, end)


def test_a_restart_continues_from_the_previous_states(device):
    D = 6
    for make in (lambda **kw: _rwm(device, D, 70, **kw), lambda **kw: _pt(device, D, [1.0, 0.5, 0.2], 5, trace="none", **kw),
                 lambda **kw: _pt(device, D, [1.0, 0.5, 0.2], 1, trace="none", **kw)):
        prev = make(init_box=(-20.0, 20.0))
        prev._advance(30)
        torch.cuda.synchronize()
        left_at = prev._run.state.cpu().numpy()
        nxt = make(initial_states=prev.current_states)
        prev._advance(5)  # the earlier sampler goes on: the new one keeps what it was given
        nxt._ensure_started()
        torch.cuda.synchronize()
        assert not np.array_equal(prev._run.state.cpu().numpy(), left_at)
        assert np.array_equal(nxt._run.state.cpu().numpy(), left_at)
        lp = E.logdensity(nxt._run.target, torch.from_numpy(left_at.reshape(-1, D)).to(device)).cpu().numpy()
        assert np.array_equal(nxt._run.logp.cpu().numpy().reshape(-1), lp)
        nxt._advance(20)
        torch.cuda.synchronize()
        after = nxt._run.state.cpu().numpy()
        assert np.all(np.isfinite(after)) and not np.array_equal(after, left_at) and nxt._run.n_accept.sum().item() > 0


def test_a_split_step_target_takes_a_box(device):
    from target_distributions import MultivariateNormalTorch

    D, n = 4, 70
    a = np.random.default_rng(3).normal(size=(D, D))
    cov = torch.tensor(a @ a.T + D * np.eye(D), dtype=torch.float32)
    target = MultivariateNormalTorch(D, cov=cov, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ("has no fused kernel: running split steps")
        alg = _rwm(device, D, n, target=target, init_box=(-3.0, 3.0))
        alg._ensure_started()
        assert alg._run.density_fn is not None and alg._run.init_mode == "box"
        want = expected_box_starts(4711, 0, n, 1, D, -3.0, 3.0, 0, False)  # full support: attempt 0 stands everywhere
        assert np.array_equal(alg._run.state.cpu().numpy(), want)
        lp = target.log_density(alg._run.state.view(-1, D)).float()
        assert torch.equal(alg._run.logp.view(-1), lp) and torch.isfinite(lp).all()
        alg._advance(20)
        torch.cuda.synchronize()
    assert torch.isfinite(alg._run.state).all() and alg._run.n_accept.sum().item() > 0


# ---- what it is for -------------------------------------------------------------------------------------------------
def test_rhat_sees_the_modes_only_from_over_dispersed_starts(device):
    """512 RWM chains on a rough carpet with modes at -15, 0, 15 in every coordinate.  From the box (-20, 20) the chains
    settle in the mode whose basin they start in - basins of width 12.5, 15 and 12.5 out of 40 - and cannot cross in 500
    steps: R-hat must say so.  The between-chain spread of three unit-width modes 15 apart predicts R-hat of about 12; 3
    is the project's "far from converged" mark.  From the origin every chain sits in mode 0 and R-hat has nothing to see."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    D, modes = 4, np.array([-15.0, 0.0, 15.0])

    def sampler(**kw):
        target = RoughCarpetDistributionTorch(D, device=device, mode_centers=list(modes))
        alg = RandomWalkMH_GPU_Optimized(D, 2.38 ** 2 / D, target, burn_in=100, device=device, num_chains=512, seed=2027,
                                         moments="cold", moments_every=2, moments_per_chain=True, **kw)
        alg.generate_samples(400)
        return alg

    alg = sampler(init_box=(-20.0, 20.0))
    rhat = alg.rhat().cpu().numpy()
    means = alg.chain_means().cpu().numpy()
    assert means.shape == (512, D)
    print("rhat", rhat)
    assert rhat.min() > 3.0
    dist = np.abs(means[:, :, None] - modes[None, None, :])  # [chain, coordinate, mode]
    print("largest distance of a chain mean from its mode", dist.min(-1).max())
    assert np.all(dist.min(-1) < 2.0)
    share = np.stack([(dist.argmin(-1) == k).mean(0) for k in range(3)])  # [mode, coordinate]
    print("share of the chains per mode and coordinate\n", share)
    assert share.min() >= 0.10
    # the same sampler from the one point: every chain in the mode at the origin
    plain = sampler()
    means0 = plain.chain_means().cpu().numpy()
    print("from the origin: largest |chain mean|", np.abs(means0).max(), "rhat", plain.rhat().cpu().numpy())
    assert np.all(np.abs(means0) < 2.0)
