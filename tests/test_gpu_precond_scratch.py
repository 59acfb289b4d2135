"""Preconditioned proposals where the caller owns more than the suite's other tests let it: a `proposals` scratch that is not
16-byte aligned (the C ABI asks for no alignment; RunPlan's own scratch comes from torch and is always aligned), and a factor
tensor that is rewritten in place between replays of a captured block of steps.  Needs an MI355X: run with `-m gpu`.

The kernel places a tile at prec_x_at(head, ...), head the alignment of the PROPOSALS' run, and copies the states in by vectors
where the state's head is equal and element by element otherwise; 64 dim is a multiple of 4, so the head is the base
pointer's for every tile.  All 16 pairs (state shift, proposals shift) run here, each array in its own sentinel-filled
allocation; tests/precond_test.cpp replays heads 0 and 3 on the CPU."""
import numpy as np
import pytest
import torch

import invariance_reference as R
import precond_reference as PR
import ptrwm_hip as E
import test_gpu_precond_rounds as RD

pytestmark = pytest.mark.gpu

SHIFTS = [(a, b) for a in range(4) for b in range(4)]  # (state, proposals), in floats off a 16-byte boundary
CN, T = 70, 3  # 210 rows: three tiles and a part, tiles straddling chains


@pytest.mark.parametrize("dim", [5, 30, 104])
def test_every_alignment_of_state_and_scratch_on_integers(device, dim):
    """210 rows, every pair of shifts, integer data (RD.integers_on_guarded_arrays): the proposals equal the float64 product,
    the sentinels on both sides of the state, the proposals and accept_u are intact, state and factor are untouched."""
    for a, b in SHIFTS:
        RD.integers_on_guarded_arrays(device, dim, CN, T, seed=8000 + dim, state_shift=a, props_shift=b)


def test_alignment_does_not_change_a_float(device):
    """dim 30, generic floats: the 16 results are bit-equal to the aligned one and to precond_reference's fmaf chain."""
    dim = 30
    rng = np.random.default_rng(8100)
    chol_np = RD.nan_upper(RD.random_factor(rng, dim))
    z = rng.standard_normal((CN, T, dim)).astype(np.float32)
    x = (rng.standard_normal((CN, T, dim)) * 10).astype(np.float32)
    u = rng.random((CN, T)).astype(np.float32)
    scales = np.array([0.7, 1.3, 1.9], np.float32)
    want = PR.propose_rows(x.reshape(-1, dim), chol_np, z.reshape(-1, dim), np.tile(scales, CN)).reshape(CN, T, dim)
    chol, zd, ud = (torch.tensor(v, device=device) for v in (chol_np, z, u))
    first = None
    for a, b in SHIFTS:
        sflat, st = RD.guarded(device, (CN, T, dim), a)
        pflat, props = RD.guarded(device, (CN, T, dim), b)
        aflat, acc = RD.guarded(device, (2, CN, T))
        st.copy_(torch.tensor(x, device=device))
        RD.make_plan(device, st, scales, chol, (props, acc)).split_propose(0, ext_prop=zd, ext_u=ud)
        torch.cuda.synchronize()
        got = props.cpu().numpy()
        first = got if first is None else first
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), (a, b)
        assert np.array_equal(got, want), (a, b, np.argwhere(got != want)[:5])
        assert RD.guards_intact(sflat, st) and RD.guards_intact(pflat, props) and RD.guards_intact(aflat, acc), (a, b)


def test_misaligned_scratch_over_two_rounds(device):
    """State one float and proposals three floats off, at the two-round batch of dim 17 (test_gpu_precond_rounds): every tile of
    either round starts from the same heads."""
    dim, k, Tn, G, Cn, n_rows = RD.shape_of(device, "d17-T1-k1")
    got, x = RD.integers_on_guarded_arrays(device, dim, Cn, Tn, seed=8200, state_shift=1, props_shift=3)
    for a, b in RD.row_ranges(n_rows, G):
        assert (got[a:b] != x[a:b]).any(axis=1).mean() > 0.9, (a, b)


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _gauss(device, dim):
    fam = R.family("gauss", dim)
    return fam, fam.spec().engine(device)


def test_whole_split_steps_do_not_depend_on_the_alignment(device):
    """6 whole split steps - the preconditioned proposal (Philox), the library's ptrwm_logdensity on a diagonal Gaussian, and
    split_accept with swap_every = 2, so that the Metropolis kernel and, on swap steps, the swap kernel read and rewrite the
    caller's `proposals` too - at shifts (0, 0), (0, 3) and (2, 1): states, log-densities, n_accept, swap_accept and the
    squared-jump sums are bit-equal across the three, the sentinels intact, and moves and swaps were accepted."""
    dim, n_steps = 30, 6
    fam, tgt = _gauss(device, dim)
    rng = np.random.default_rng(8300)
    betas = np.array([1.0, 0.5, 0.25], np.float32)
    x0 = R.exact_starts(fam, rng, betas, CN)
    chol = torch.tensor(RD.nan_upper(RD.random_factor(rng, dim, 10.0) * 0.3), device=device)
    scales = (2.38 / np.sqrt(dim) / np.sqrt(betas)).astype(np.float32)
    runs = []
    for a, b in [(0, 0), (0, 3), (2, 1)]:
        sflat, st = RD.guarded(device, (CN, T, dim), a)
        pflat, props = RD.guarded(device, (CN, T, dim), b)
        aflat, acc = RD.guarded(device, (2, CN, T))
        st.copy_(torch.tensor(x0, device=device))
        lp = E.logdensity(tgt, st.view(-1, dim)).view(CN, T).contiguous()
        stats = {s: torch.zeros(CN, T, dtype=torch.int64, device=device) for s in ("n_accept", "swap_accept")}
        stats["sq_jump"] = torch.zeros(CN, T, dtype=torch.float64, device=device)  # (a swap step's: |final - proposals' pre-step rows|^2)
        plan = RD.make_plan(device, st, scales, chol, (props, acc), seed=99, chain_offset=7, logp=lp,
                            beta=torch.tensor(betas, device=device), swap_every=2, **stats)
        for s in range(n_steps):
            out = plan.split_propose(s)
            assert out.data_ptr() == props.data_ptr()
            plan.split_accept(s, E.logdensity(tgt, out.view(-1, dim)).view(CN, T))
        torch.cuda.synchronize()
        assert RD.guards_intact(sflat, st) and RD.guards_intact(pflat, props) and RD.guards_intact(aflat, acc), (a, b)
        runs.append(dict(state=st.clone(), logp=lp.clone(), **{s: v.clone() for s, v in stats.items()}))
    for other in runs[1:]:
        for key, v in runs[0].items():
            assert torch.equal(_bits(v), _bits(other[key])), key
    assert int(runs[0]["n_accept"].sum()) > CN and int(runs[0]["swap_accept"].sum()) > 0


def test_a_captured_block_reads_the_factor_at_replay(device):
    """set_preconditioner binds the tensor's memory: a block of 8 split steps captured ONCE in device-step mode with factor tensor
    F bound is replayed, F is rewritten in place - by copy_ from another factor, then by plan.precond_update on prepared sums -
    and the block is replayed after each.  dim 5, T = 3, 70 chains (210 rows: no multiple of 64), the library's density.  An
    eager plan driven step by step in host-step mode with the same factors at the same steps has the same bits in state,
    log-densities, n_accept and swap_accept after every block; the factor the update wrote is precond_reference's, bit for bit;
    and a control plan that keeps the first factor through the second block ends it elsewhere, so nothing passes on a no-op."""
    dim, se, s0, K = 5, 4, 3, 8
    fam, tgt = _gauss(device, dim)
    rng = np.random.default_rng(8400)
    betas = np.array([1.0, 0.5, 0.25], np.float32)
    x0 = torch.tensor(R.exact_starts(fam, rng, betas, CN), device=device)
    scales = (2.38 / np.sqrt(dim) / np.sqrt(betas)).astype(np.float32)
    f1 = RD.nan_upper(RD.random_factor(rng, dim, 10.0) * 0.5)
    f2 = RD.nan_upper(RD.random_factor(rng, dim, 100.0) * 0.2)
    n = 6 * dim + 7
    draws = (rng.standard_normal((n, dim)) @ RD.random_factor(rng, dim, 30.0).T * 0.4).astype(np.float32).astype(np.float64)
    sxx, sx = np.tril(draws.T @ draws), draws.sum(0)
    upd = dict(memory=1.0, jitter=1e-6, min_count=4.0 * dim)
    outcome, f3, _, _, _ = PR.update(sxx, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, chol=f2, **upd)
    assert outcome == PR.UPDATED

    def side(factor):
        st = x0.clone()
        lp = E.logdensity(tgt, st.view(-1, dim)).view(CN, T).contiguous()
        stats = {s: torch.zeros(CN, T, dtype=torch.int64, device=device) for s in ("n_accept", "swap_accept")}
        F = torch.tensor(factor, device=device)
        plan = RD.make_plan(device, st, scales, F, seed=321, chain_offset=2, logp=lp, beta=torch.tensor(betas, device=device),
                            swap_every=se, **stats)
        return dict(plan=plan, F=F, arrays=dict(state=st, logp=lp, **stats))

    def eager(sd, first, count):  # host-step mode, one step at a time
        for s in range(first, first + count):
            props = sd["plan"].split_propose(s)
            sd["plan"].split_accept(s, E.logdensity(tgt, props.view(-1, dim)).view(CN, T))

    def same(a, b, what):
        for key, v in a["arrays"].items():
            assert torch.equal(_bits(v), _bits(b["arrays"][key])), (key, what)

    cap, ref, ctl = side(f1), side(f1), side(f1)
    d = lambda a, dt=torch.float64: torch.tensor(np.asarray(a), dtype=dt, device=device)  # noqa: E731
    cap["plan"].set_precond_update(d(sxx), d(sx), d([n], torch.int64), d(np.zeros((dim, dim))), d(np.zeros(dim)), d([0.0]), windows=1, **upd)
    counter = torch.full((1,), s0, dtype=torch.int64, device=device)
    plan = cap["plan"]
    plan.set_device_step(counter)

    def step(offset=0, no_sweep=False, advance=1):
        props = plan.split_propose(offset)
        plan.split_accept(offset, E.logdensity(tgt, props.view(-1, dim)).view(CN, T), no_sweep=no_sweep)
        if advance:
            plan.split_advance(advance)

    cur = torch.cuda.current_stream(device)
    side_stream = torch.cuda.Stream(device)
    side_stream.wait_stream(cur)
    with torch.cuda.stream(side_stream):
        step()  # one step outside capture
    cur.wait_stream(side_stream)
    assert (s0 + 1) % se == 0  # the block starts at a multiple of swap_every: its swap steps sit at fixed offsets
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for j in range(K):
            step(offset=j, no_sweep=(j + 1) % se != 0, advance=K if j == K - 1 else 0)
    for sd in (ref, ctl):
        eager(sd, s0, 1)
    at = s0 + 1
    # block 1: the factor the block was captured with
    g.replay()
    eager(ref, at, K)
    eager(ctl, at, K)
    torch.cuda.synchronize()
    same(cap, ref, "block 1")
    same(cap, ctl, "block 1, control")
    at += K
    # block 2: rewritten by copy_
    cap["F"].copy_(torch.tensor(f2, device=device))
    ref["F"].copy_(torch.tensor(f2, device=device))
    g.replay()
    eager(ref, at, K)
    eager(ctl, at, K)  # (keeps f1)
    torch.cuda.synchronize()
    same(cap, ref, "block 2")
    assert not torch.equal(cap["arrays"]["state"], ctl["arrays"]["state"])  # the second factor was read
    at += K
    # block 3: rewritten by the update kernel
    plan.precond_update(0)
    torch.cuda.synchronize()
    assert np.array_equal(cap["F"].cpu().numpy().view(np.uint32), f3.view(np.uint32))
    assert not np.array_equal(np.tril(f3), np.tril(np.nan_to_num(f2)))
    ref["F"].copy_(torch.tensor(f3, device=device))
    for key, v in ctl["arrays"].items():  # the control goes on from where the others stand, with the factor before the update
        v.copy_(ref["arrays"][key])
    ctl["F"].copy_(torch.tensor(f2, device=device))
    g.replay()
    eager(ref, at, K)
    eager(ctl, at, K)
    torch.cuda.synchronize()
    same(cap, ref, "block 3")
    assert not torch.equal(cap["arrays"]["state"], ctl["arrays"]["state"])  # the updated factor was read
    assert int(counter.item()) == s0 + 1 + 3 * K
    assert int(cap["arrays"]["n_accept"].sum()) > CN and int(cap["arrays"]["swap_accept"].sum()) > 0
