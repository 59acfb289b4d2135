"""Preconditioned Gaussian proposals on the device (include/ptrwm.h ptrwm_split_propose_precond / ptrwm_precond_update,
csrc/precond.h), through the C ABI: the kernel's layout on integers, where every order of the sums gives the same floats; the
rule bit for bit against tests/precond_reference.py; the Philox path against the Normal kernel's own normals; the update kernel
against the reference's Python floats."""
import numpy as np
import pytest
import torch

import precond_reference as PR
import ptrwm_hip as E

DIMS = [1, 3, 4, 5, 16, 17, 30, 33, 64, 104]


def _plan(device, x, scales, *, seed=0, chain_offset=0, burn_in=0, swap_every=1):
    Cn, T, D = x.shape
    st = x if torch.is_tensor(x) else torch.tensor(x, device=device)
    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(np.asarray(scales, np.float32), device=device))
    plan = E.RunPlan(None, prop, state=st, logp=torch.zeros(Cn, T, device=device), beta=torch.ones(T, device=device), seed=seed,
                     chain_offset=chain_offset, burn_in=burn_in, swap_every=swap_every)
    return plan, st


def _nan_upper(L):
    return (np.tril(L) + np.triu(np.full(L.shape, np.nan), 1)).astype(np.float32)


# ---- 1. the layout, on integers -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_exact_layout_on_integers(device, dim):
    """External randoms; integer z in [-4, 4], an integer asymmetric lower-triangular L in [-3, 3], integer x, scales that are
    powers of two and differ per temperature: every product and partial sum is exact in float32 whatever the order.  The strict
    upper triangle of the caller's chol is NaN: it must never be read.  T = 1 with 5, 64, 65 and 210 rows (part of a tile, a
    tile, a tile and a row, three tiles and a part); T = 3 with 5, 64, 65 and 70 chains (15, 192, 195 and 210 rows); and once
    with the states one float off the proposals' alignment (the element-wise staging)."""
    rng = np.random.default_rng(1000 + dim)
    L = rng.integers(-3, 4, (dim, dim)).astype(np.float64)
    L[np.arange(dim), np.arange(dim)] = rng.integers(1, 4, dim)
    chol_np = _nan_upper(L)
    chol = torch.tensor(chol_np, device=device)
    for T, Cn, shift in [(1, 5, 0), (1, 64, 0), (1, 65, 0), (1, 210, 0), (3, 5, 0), (3, 64, 0), (3, 65, 0), (3, 70, 0), (3, 70, 1)]:
        z = rng.integers(-4, 5, (Cn, T, dim)).astype(np.float32)
        x = rng.integers(-50, 51, (Cn, T, dim)).astype(np.float32)
        u = rng.random((Cn, T)).astype(np.float32)
        scales = np.float32(2.0) ** -np.arange(1, T + 1, dtype=np.float32)
        flat = torch.zeros(Cn * T * dim + 4, device=device)
        st = flat[shift:shift + Cn * T * dim].view(Cn, T, dim)
        st.copy_(torch.tensor(x, device=device))
        assert st.is_contiguous() and (st.data_ptr() // 4) % 4 == shift
        plan, st = _plan(device, st, scales)
        plan.set_preconditioner(chol)
        props = plan.split_propose(0, ext_prop=torch.tensor(z, device=device), ext_u=torch.tensor(u, device=device))
        torch.cuda.synchronize()
        want = (x.astype(np.float64) + scales[None, :, None].astype(np.float64) * (z.astype(np.float64) @ np.tril(L).T)).astype(np.float32)
        got = props.cpu().numpy()
        assert not np.isnan(got).any(), (T, Cn)
        assert np.array_equal(got, want), (T, Cn, shift, np.argwhere(got != want)[:5])
        acc = plan._split_buffers()[1].cpu().numpy()
        assert np.array_equal(acc[0], u) and np.all(acc[1] == -1.0), (T, Cn)
        assert np.array_equal(st.cpu().numpy(), x)  # the state is only read
        assert np.array_equal(chol.cpu().numpy().view(np.uint32), chol_np.view(np.uint32))  # ... and so is the factor
        assert float(flat[shift + Cn * T * dim:].abs().sum()) == 0.0 and float(flat[:shift].abs().sum()) == 0.0


# ---- 2. the rule, bit for bit ---------------------------------------------------------------------------------------------------------
def _random_factor(rng, dim, cond=100.0):
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    cov = (q * np.exp(np.linspace(0.0, np.log(cond), dim))) @ q.T
    return np.linalg.cholesky((cov + cov.T) / 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [5, 30, 104])
def test_the_rule_bit_for_bit(device, dim):
    """Gaussian z, a random L of condition about 100, random x: the proposals equal precond_reference's fmaf chain as floats
    (==, so -0 equals +0).  130 rows: two tiles and two rows."""
    rng = np.random.default_rng(2000 + dim)
    Cn, T = 65, 2
    chol_np = _nan_upper(_random_factor(rng, dim))
    z = rng.standard_normal((Cn, T, dim)).astype(np.float32)
    x = (rng.standard_normal((Cn, T, dim)) * 10).astype(np.float32)
    u = rng.random((Cn, T)).astype(np.float32)
    scales = np.array([0.7, 1.9], np.float32)
    plan, st = _plan(device, x, scales)
    plan.set_preconditioner(torch.tensor(chol_np, device=device))
    got = plan.split_propose(0, ext_prop=torch.tensor(z, device=device), ext_u=torch.tensor(u, device=device)).cpu().numpy()
    want = PR.propose_rows(x.reshape(-1, dim), chol_np, z.reshape(-1, dim), np.tile(scales, Cn)).reshape(Cn, T, dim)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ---- 3. the Philox path, without touching the oracle ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,device_step", [(5, False), (30, False), (33, False), (30, True)], ids=["d5", "d30", "d33", "d30-device-step"])
def test_philox_path_against_the_normal_kernels_own_normals(device, dim, device_step):
    """ptrwm_split_propose with NormalProposal, all scales 1 and a zero state returns z itself (fmaf(rad, sin, 0) is rad sin).
    For the same seed, step, chain_offset and T the new kernel's proposals equal the reference chain on that z, and plane 0 of
    accept_u equals the Normal kernel's accept uniforms.  dim 5: half a pair; chain_offset and step are not zero."""
    rng = np.random.default_rng(3000 + dim)
    Cn, T, seed, step, offset = 70, 3, 0x1234567890ABCDEF, 41, (1 << 33) + 5
    zero = np.zeros((Cn, T, dim), np.float32)
    counter = torch.tensor([step - 2], dtype=torch.int64, device=device) if device_step else None
    arg = 2 if device_step else step  # (device-step mode: the counter plus this call's offset)
    ref_plan, _ = _plan(device, zero, np.ones(T, np.float32), seed=seed, chain_offset=offset)
    ref_plan.set_device_step(counter)
    z = ref_plan.split_propose(arg).cpu().numpy()
    u = ref_plan._split_buffers()[1][0].cpu().numpy()
    assert np.isfinite(z).all() and z.std() > 0.8 and z.std() < 1.2
    chol_np = _nan_upper(_random_factor(rng, dim))
    x = (rng.standard_normal((Cn, T, dim)) * 10).astype(np.float32)
    scales = np.array([0.5, 1.3, 2.9], np.float32)
    plan, st = _plan(device, x, scales, seed=seed, chain_offset=offset)
    plan.set_device_step(counter)
    plan.set_preconditioner(torch.tensor(chol_np, device=device))
    got = plan.split_propose(arg).cpu().numpy()
    acc = plan._split_buffers()[1].cpu().numpy()
    want = PR.propose_rows(x.reshape(-1, dim), chol_np, z.reshape(-1, dim), np.tile(scales, Cn)).reshape(Cn, T, dim)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(acc[0], u) and np.all(acc[1] == -1.0)
    if device_step:
        assert int(counter.item()) == step - 2  # the proposal does not advance the counter


# ---- 4. the update kernel ------------------------------------------------------------------------------------------------------------
def _sums(rng, dim, n, integer):
    if integer:
        x = rng.integers(-6, 7, (n, dim)).astype(np.float64)
    else:
        f = _random_factor(rng, dim, 1e4)
        x = (rng.standard_normal((n, dim)) @ f.T + rng.standard_normal(dim)).astype(np.float32).astype(np.float64)
    return np.tril(x.T @ x) + np.triu(np.full((dim, dim), 123.0), 1), x.sum(0)


def _run_update(device, dim, sxx, sx, n, run_xx, run_x, run_w, chol, *, memory, jitter, min_count, window=1, K=3):
    d = lambda a, dt=torch.float64: torch.tensor(np.asarray(a), dtype=dt, device=device)  # noqa: E731
    t = dict(sxx=d(sxx), sx=d(sx), count=d([n], torch.int64), run_xx=d(run_xx), run_x=d(run_x), run_w=d([run_w]))
    rec = dict(chol_history=torch.full((K + 1, dim, dim), float("nan"), device=device),
               weight_history=torch.full((K,), float("nan"), dtype=torch.float64, device=device),
               skipped=torch.zeros(1, dtype=torch.int64, device=device))
    chol_t = torch.tensor(chol, device=device)
    plan, _ = _plan(device, np.zeros((1, 1, dim), np.float32), [1.0])
    plan.set_preconditioner(chol_t)
    plan.set_precond_update(**t, windows=K, memory=memory, jitter=jitter, min_count=min_count, **rec)
    plan.precond_update(window)
    torch.cuda.synchronize()
    return chol_t.cpu().numpy(), {k: v.cpu().numpy() for k, v in {**t, **rec}.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 5, 30, 63, 64, 65, 104])
def test_update_kernel_against_python_floats_bitwise(device, dim):
    """Integer-valued sums, then generic ones with a running triple and memory 0.5, then the skips: the kernel's factor, history
    row, weight, running triple, zeroed window sums and skip count equal precond_reference, bit for bit.  The kernel runs one
    thread per row with barriers inside the column loop: dims 63, 64 and 65 put the last row in front of, on and behind a wave
    boundary.  Among the skips: a factor whose entries are finite as doubles and infinite as floats (sums scaled to entries of
    about 1e40), a running weight that is not a number, and a pivot that fails at column 0 (coordinate 0 identically zero, no
    jitter).  Last, K = 1 with window 0: both history rows are written by the one call."""
    rng = np.random.default_rng(4000 + dim)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64)  # noqa: E731
    n = 6 * dim + 7
    cases = []
    sxx, sx = _sums(rng, dim, n, integer=True)
    cases.append(("integer", sxx, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, dict(memory=1.0, jitter=1e-6, min_count=4.0 * dim), PR.UPDATED))
    sxx, sx = _sums(rng, dim, n, integer=False)
    rxx, rx = _sums(rng, dim, n, integer=False)
    cases.append(("generic", sxx, sx, n, rxx, rx, float(n), dict(memory=0.5, jitter=1e-6, min_count=4.0 * dim), PR.UPDATED))
    cases.append(("few draws", sxx, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, dict(memory=0.5, jitter=1e-6, min_count=100.0 * dim), PR.FEW_DRAWS))
    bad = sxx.copy()
    bad[dim - 1, dim - 1] = -abs(bad[dim - 1, dim - 1])
    cases.append(("negative variance", bad, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, dict(memory=1.0, jitter=0.0, min_count=4.0 * dim), PR.NOT_POSITIVE))
    bad = sxx.copy()
    bad[dim // 2, 0] = np.inf
    cases.append(("infinite sum", bad, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, dict(memory=1.0, jitter=1e-6, min_count=4.0 * dim), PR.NOT_POSITIVE))
    cases.append(("float overflow", sxx * 1e80, sx * 1e40, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, dict(memory=1.0, jitter=1e-6, min_count=4.0 * dim), PR.NOT_POSITIVE))
    cases.append(("weight not a number", sxx, sx, n, rxx, rx, float("nan"), dict(memory=0.5, jitter=1e-6, min_count=4.0 * dim), PR.FEW_DRAWS))
    bad = sxx.copy()
    bad[:, 0] = 0.0
    bad[0, 1:] = 123.0  # (above the diagonal: never read)
    bad_x = sx.copy()
    bad_x[0] = 0.0
    cases.append(("pivot 0", bad, bad_x, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, dict(memory=1.0, jitter=0.0, min_count=4.0 * dim), PR.NOT_POSITIVE))
    for name, sxx, sx, n, rxx, rx, rw, kw, expect in cases:
        chol0 = _nan_upper(rng.standard_normal((dim, dim)))
        outcome, want, want_xx, want_x, want_w = PR.update(sxx, sx, n, rxx, rx, rw, chol=chol0, **kw)
        assert outcome == expect, (name, outcome)
        got, t = _run_update(device, dim, sxx, sx, n, rxx, rx, rw, chol0, **kw)
        assert np.array_equal(bits(got), bits(want)), name  # (the NaNs above the diagonal: not touched)
        if outcome != PR.UPDATED:
            assert np.array_equal(bits(got), bits(chol0)), name
        assert t["skipped"].tolist() == [0 if outcome == PR.UPDATED else 1], name
        assert np.array_equal(bits(t["run_xx"]), bits(want_xx)) and np.array_equal(bits(t["run_x"]), bits(want_x)), name
        assert bits(t["run_w"])[0] == bits(np.array([want_w]))[0] and bits(t["weight_history"])[1] == bits(np.array([want_w]))[0], name
        assert np.isnan(t["weight_history"][[0, 2]]).all(), name
        assert t["count"].tolist() == [0] and not t["sx"].any() and not np.tril(t["sxx"]).any(), name
        assert np.array_equal(np.triu(t["sxx"], 1), np.triu(sxx, 1)), name  # (above the diagonal: not touched)
        hist = t["chol_history"]
        assert np.array_equal(bits(hist[2]), bits(np.tril(np.nan_to_num(want, nan=0.0)))), name  # row window + 1: zeros above
        assert np.isnan(hist[[0, 1, 3]]).all(), name  # (row 0 is written by window 0 only)
    # window 0 also records the factor it ran with
    chol0 = _nan_upper(rng.standard_normal((dim, dim)))
    sxx, sx = _sums(rng, dim, n, integer=False)
    got, t = _run_update(device, dim, sxx, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, chol0, memory=1.0, jitter=1e-6,
                         min_count=4.0 * dim, window=0)
    assert np.array_equal(bits(t["chol_history"][0]), bits(np.tril(np.nan_to_num(chol0, nan=0.0))))
    assert np.array_equal(bits(t["chol_history"][1]), bits(np.tril(np.nan_to_num(got, nan=0.0))))
    # ... and with K = 1 that call writes the whole record: both history rows and the one weight
    chol0 = _nan_upper(rng.standard_normal((dim, dim)))
    sxx, sx = _sums(rng, dim, n, integer=False)
    kw = dict(memory=1.0, jitter=1e-6, min_count=4.0 * dim)
    outcome, want, want_xx, want_x, want_w = PR.update(sxx, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, chol=chol0, **kw)
    assert outcome == PR.UPDATED
    got, t = _run_update(device, dim, sxx, sx, n, np.zeros((dim, dim)), np.zeros(dim), 0.0, chol0, **kw, window=0, K=1)
    assert np.array_equal(bits(got), bits(want)) and t["skipped"].tolist() == [0]
    assert t["chol_history"].shape == (2, dim, dim) and t["weight_history"].shape == (1,)
    assert np.array_equal(bits(t["chol_history"][0]), bits(np.tril(np.nan_to_num(chol0, nan=0.0))))
    assert np.array_equal(bits(t["chol_history"][1]), bits(np.tril(np.nan_to_num(want, nan=0.0))))
    assert bits(t["weight_history"])[0] == bits(np.array([want_w]))[0] == bits(t["run_w"])[0]
    assert np.array_equal(bits(t["run_xx"]), bits(want_xx)) and np.array_equal(bits(t["run_x"]), bits(want_x))
    assert t["count"].tolist() == [0] and not t["sx"].any() and not np.tril(t["sxx"]).any()


# ---- 5. invariance with a fixed factor --------------------------------------------------------------------------------------------
import invariance_reference as R  # noqa: E402

N_STEPS = 300


class _EngineTarget:
    """A target the library has a kernel for, as EngineRun sees one (engine_target())"""

    def __init__(self, target):
        self._target = target

    def engine_target(self):
        return self._target


class _UserTarget:
    """A user-defined density: log_density only"""

    def __init__(self, fn):
        self.log_density = fn


def _fixed_factor(dim, seed, lo=0.25, hi=2.5):
    """A dense factor whose covariance has eigenvalues lo .. hi (condition hi / lo <= 10)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    cov = (q * np.exp(np.linspace(np.log(lo), np.log(hi), dim))) @ q.T
    assert np.linalg.cond(cov) <= 10.0 + 1e-9
    return np.linalg.cholesky((cov + cov.T) / 2).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("fkey", ["sgauss", "rc15", "user", "sgauss-rounds"])
def test_fixed_factor_leaves_the_tempered_laws_invariant(device, fkey):
    """tests/invariance_reference.py as it stands, with its own P_MIN / Z_MAX: a fixed dense factor of condition 10, a ladder of 4
    with swaps, every replica from an exact draw, the final states hold the tempered law at every rung.  sgauss and rc15 are
    targets with a fused kernel - the split route with the library's density - and `user` a density in plain torch.  The steps
    run as captured blocks.  32 768 ladders x 4 are 2 048 tiles of the proposal kernel, one per workgroup on 256 compute units;
    sgauss-rounds has 65 536 ladders, so that every workgroup walks at least two tiles in every one of the 300 steps
    (precond_reference.grid; tests/test_gpu_precond_rounds.py)."""
    from algorithms._engine_core import EngineRun

    case, rounds = f"gpu-precond-{fkey}", fkey.endswith("-rounds")  # (the seed comes from the case's name)
    fkey = fkey.split("-")[0]
    dim, T, Cn, se = 4, 4, 65536 if rounds else 32768, 2
    if rounds:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        assert cus >= 2 and -(-PR.tiles(Cn * T) // PR.grid(PR.tiles(Cn * T), cus)) >= 2
    fam = R.family("gauss" if fkey == "user" else fkey, dim)
    s = R.setup_case(case, fam, "Normal", T, 0.1, Cn)
    if fkey == "user":
        mu = torch.tensor(fam.mu, device=device, dtype=torch.float32)
        prec = torch.tensor(1.0 / fam.var, device=device, dtype=torch.float32)
        target = _UserTarget(lambda x: -0.5 * (((x - mu) ** 2) * prec).sum(-1))
    else:
        target = _EngineTarget(s["spec"].engine(device))
    chol = _fixed_factor(dim, s["seed"])
    with pytest.warns(UserWarning, match="split steps"):
        run = EngineRun(target_dist=target, proposal=s["prop"].engine(device), beta_ladder=[float(b) for b in s["engine_betas"]], dim=dim,
                        device=device, n_replicas=Cn, initial_state=s["x0"], burn_in=0, swap_every=se, swap_mode="exchange",
                        swap_order="sequential", seed=s["seed"], proposal_chol=chol)
    assert run.split and (run.density_fn is None) == (fkey != "user")
    run.advance(N_STEPS)
    torch.cuda.synchronize()
    assert run._graph is not None  # captured blocks, with the factor bound
    out = {"state": run.state.cpu().numpy(), "n_accept": run.n_accept.cpu().numpy(), "swap_accept": run.swap_accept.cpu().numpy()}
    rates = R.power_conditions(out, fam, N_STEPS, se)
    r = R.check(out["state"], s["betas"], fam)
    print(f"READINGS {case[4:]}: {R.describe(r)}; acceptance {rates['accept'].min():.2f}..{rates['accept'].max():.2f}, "
          f"swaps {rates['swap'].min():.2f}..{rates['swap'].max():.2f}")
    assert R.inside(r), R.describe(r)
    assert np.array_equal(run.proposal_factor().cpu().numpy(), chol)  # a fixed factor stays what it was


# ---- 6. affine equivariance, end to end through the RWM class --------------------------------------------------------------
@pytest.mark.gpu
def test_affine_equivariance_through_the_rwm_class(device):
    """Sigma = Q diag(1 .. 10^4) Q^T in dim 8.  Run A: the density -1/2 |L^-1 x|^2 with proposal_cov = Sigma, from L w0.  Run B:
    the standard Gaussian with no factor, from w0.  Same seed, 4096 chains, 200 steps: in exact arithmetic both make the same
    decisions, so the accepted counts agree within 4 sqrt(N p (1 - p)), N the number of decisions - a bound that holds even for
    independent runs, so rounding flips cannot break it, while a transposed or mis-indexed factor collapses A's acceptance."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from interfaces import TorchTargetDistribution
    from target_distributions import MultivariateNormalTorch

    dim, Cn, n_steps, seed = 8, 4096, 200, 20261021
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    sigma = (q * np.exp(np.linspace(0.0, np.log(1e4), dim))) @ q.T
    sigma = (sigma + sigma.T) / 2
    L = np.linalg.cholesky(sigma)
    w0 = rng.standard_normal((Cn, dim))
    linv_t = torch.tensor(np.linalg.inv(L).T, device=device, dtype=torch.float64)

    class Whitened(TorchTargetDistribution):
        def get_name(self):
            return "Whitened"

        def log_density(self, x):
            y = torch.as_tensor(x, device=self.device).double() @ linv_t
            return (-0.5 * (y * y).sum(-1)).float()

        def density(self, x):
            return torch.exp(self.log_density(x))

    var = 2.38 ** 2 / dim
    with pytest.warns(UserWarning, match="no fused kernel"):
        a = RandomWalkMH_GPU_Optimized(dim, var, Whitened(dim, device), device=device, num_chains=Cn, seed=seed,
                                       initial_states=(w0 @ L.T).astype(np.float32), proposal_cov=sigma)
        a._advance(n_steps)
    b = RandomWalkMH_GPU_Optimized(dim, var, MultivariateNormalTorch(dim, mean=[0.0] * dim, cov=np.eye(dim).tolist(), device=device),
                                   device=device, num_chains=Cn, seed=seed, initial_states=w0.astype(np.float32))
    b._advance(n_steps)
    torch.cuda.synchronize()
    acc_a, acc_b, N = a.num_acceptances, b.num_acceptances, Cn * n_steps
    p = (acc_a + acc_b) / (2 * N)
    print(f"READINGS affine equivariance: accepted {acc_a} with the factor, {acc_b} whitened, of {N}; bound {4 * np.sqrt(N * p * (1 - p)):.0f}")
    assert 0.1 < p < 0.5
    assert abs(acc_a - acc_b) <= 4 * np.sqrt(N * p * (1 - p))
    assert a.get_diagnostic_info()["preconditioned"] is True and b.get_diagnostic_info()["preconditioned"] is False
    assert a.get_diagnostic_info()["precond_condition"] == pytest.approx(1e4, rel=1e-3)


# ---- 7. adaptation, at EngineRun level ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adaptation_follows_the_reference_window_by_window(device):
    """A dense Gaussian of condition 100 in dim 5, 4096 replicas from exact draws, two windows of 50 steps probed every 10, a
    full trace of temperature 0 at the probe steps.  After each window the weight is probes x replicas as the schedule implies
    (memory 0.5: 20 480, then 30 720), nothing is skipped, and the factor is within one float32 unit in the last place of
    precond_reference run on the trace's sums (math.fsum).  The device's sums differ from fsum's by the order of n = 20 480 fp64
    additions: to first order the factor moves by (n + dim) 2^-53 kappa(A) < 3e-10 relative, far below half a float32 ulp
    (6e-8), so one ulp covers a rounding that falls the other way.  After window 0 - the factor was the identity, the chain
    exactly invariant - L0 L0^T lies within 5.5 sqrt((S_ii S_jj + S_ij^2) / 4096) of Sigma, element by element: the Wishart
    error of 4096 independent draws (more probes only shrink it).  adapt_sync, a recording callable, is called once per window
    on each of the three sum tensors, before the update."""
    import math

    from algorithms._engine_core import EngineRun

    dim, Cn, W, P = 5, 4096, 50, 10
    rng = np.random.default_rng(77)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    sigma = (q * np.exp(np.linspace(np.log(0.1), np.log(10.0), dim))) @ q.T
    sigma = (sigma + sigma.T) / 2
    x0 = (rng.standard_normal((Cn, dim)) @ np.linalg.cholesky(sigma).T).astype(np.float32)
    prec = torch.tensor(np.linalg.inv(sigma), device=device, dtype=torch.float64)
    target = _UserTarget(lambda x: (-0.5 * ((x.double() @ prec) * x.double()).sum(-1)).float())
    calls = []

    def sync(t):
        calls.append((tuple(t.shape), t.dtype, run.proposal_factor().cpu().numpy()))
        return t

    prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor([2.38 / math.sqrt(dim) * 0.4], device=device))
    with pytest.warns(UserWarning, match="no fused kernel"):
        run = EngineRun(target_dist=target, proposal=prop, beta_ladder=[1.0], dim=dim, device=device, n_replicas=Cn, initial_state=x0,
                        burn_in=2 * W, swap_every=1, swap_mode="exchange", swap_order="sequential", seed=5, adapt_cov=True,
                        cov_adapt_every=W, cov_adapt_probe_every=P, adapt_sync=sync)
    assert np.array_equal(run.proposal_factor().cpu().numpy(), np.eye(dim, dtype=np.float32))
    ulps = lambda a, b: np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))  # noqa: E731
    rxx, rx, rw, factor = np.zeros((dim, dim)), np.zeros(dim), 0.0, np.eye(dim, dtype=np.float32)
    for window in range(2):
        tr = torch.empty(W // P, Cn, 1, dim, device=device)
        run.advance(W, trace=tr, trace_every=P)
        torch.cuda.synchronize()
        rows = tr.cpu().numpy().reshape(-1, dim).astype(np.float64)
        n = rows.shape[0]
        assert n == (W // P) * Cn
        sxx = np.array([[math.fsum(rows[:, i] * rows[:, j]) if j <= i else 0.0 for j in range(dim)] for i in range(dim)])
        sx = np.array([math.fsum(rows[:, i]) for i in range(dim)])
        outcome, want, rxx, rx, rw = PR.update(sxx, sx, n, rxx, rx, rw, 0.5, 1e-6, 4.0 * dim, factor)
        assert outcome == PR.UPDATED
        h = run.preconditioner_history()
        assert h["skipped"] == 0
        assert float(h["weights"][window]) == rw == (20480.0 if window == 0 else 30720.0)
        got = run.proposal_factor().cpu().numpy()
        worst = int(ulps(got[np.tril_indices(dim)], want[np.tril_indices(dim)]).max())
        print(f"READINGS adaptation window {window}: factor within {worst} float32 ulp(s) of the reference, weight {rw:.0f}")
        assert worst <= 1
        assert np.array_equal(h["factors"][window + 1].cpu().numpy(), got) and not np.triu(got, 1).any()
        # the recording callable: the three sum tensors, while the factor was still the window's own
        assert [(c[0], c[1]) for c in calls[3 * window:]] == [((dim, dim), torch.float64), ((dim,), torch.float64), ((1,), torch.int64)]
        assert all(np.array_equal(c[2], factor) for c in calls[3 * window:])
        if window == 0:
            g = got.astype(np.float64)
            err = np.abs(g @ g.T - sigma)
            bound = 5.5 * np.sqrt((np.outer(np.diag(sigma), np.diag(sigma)) + sigma ** 2) / Cn)
            print(f"READINGS adaptation window 0: L0 L0^T off Sigma by at most {(err / bound).max() * 5.5:.2f} Wishart standard errors")
            assert (err <= bound).all()
        factor = got  # (the next window ran with the device's own factor)
    assert len(calls) == 6
    # past the last window nothing adapts
    run.advance(20)
    torch.cuda.synchronize()
    assert np.array_equal(run.proposal_factor().cpu().numpy(), factor) and len(calls) == 6


@pytest.mark.gpu
def test_adaptation_with_a_ladder_learns_from_temperature_0_only(device):
    """The window-by-window test with a ladder [1, 0.5, 0.25] (the probe is then ptrwm_covariance with temps = 1 on a [C, T, D]
    state): the library's diagonal Gaussian in dim 5 - so that eager and captured densities are the same bits - 4096 ladders,
    every replica from an exact draw of its own tempered law, two windows of 80 steps probed every 40 (all inside burn-in: no
    swap event), a trace whose second extent is 1: temperature 0 at the probe steps.
      * After each window the factor is within one float32 ulp of precond_reference on the math.fsum sums of that trace, the
        weight is probes x ladders as the schedule implies (memory 0.5: 8 192, then 12 288) and nothing is skipped.  The device's
        sums differ from fsum's by the order of n = 8 192 fp64 additions: to first order the factor moves by
        (n + dim) 2^-53 kappa(A) relative, with kappa(A) < 8 here (variances 0.5 .. 2) below 8e-12 - asserted, from the reference's
        own A, to lie below half a float32 ulp, 2^-25 = 3e-8 - so one ulp covers a rounding that falls the other way.
      * The control that gives the test its point: a twin run with a full trace has the same temperature-0 rows bit for bit, and
        the same sums taken from its rung 1 (variance Sigma / 0.5) give a factor sqrt 2 larger, far more than one ulp away.  A
        probe that read another rung, or all rungs, fails the first check.
      * A third run, same seed, use_graph left on and no trace: every chunk of 40 steps replays captured blocks.  At the end of
        window 0 its states equal the eager run's bit for bit - the factor was the identity for both - and its window-0 factor
        is within one ulp of the same reference.  Nothing is claimed about window 1 between the two runs: their factors may
        differ by an ulp."""
    import math

    from algorithms._engine_core import EngineRun

    dim, Cn, T, W, P = 5, 4096, 3, 80, 40
    fam = R.family("gauss", dim)
    betas = np.array([1.0, 0.5, 0.25], np.float32)
    x0 = R.exact_starts(fam, np.random.default_rng(78), betas, Cn)
    scales = (2.38 / math.sqrt(dim) * 0.8 / np.sqrt(betas)).astype(np.float32)

    def make():
        prop = E.Proposal(E.PROPOSAL_NORMAL, torch.tensor(scales, device=device))
        with pytest.warns(UserWarning, match="split steps"):
            return EngineRun(target_dist=_EngineTarget(fam.spec().engine(device)), proposal=prop, beta_ladder=[float(b) for b in betas],
                             dim=dim, device=device, n_replicas=Cn, initial_state=x0, burn_in=2 * W, swap_every=1, swap_mode="exchange",
                             swap_order="sequential", seed=6, adapt_cov=True, cov_adapt_every=W, cov_adapt_probe_every=P)

    def sums_of(rows):
        sxx = np.array([[math.fsum(rows[:, i] * rows[:, j]) if j <= i else 0.0 for j in range(dim)] for i in range(dim)])
        return sxx, np.array([math.fsum(rows[:, i]) for i in range(dim)])

    ulps = lambda a, b: np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))  # noqa: E731
    tri = np.tril_indices(dim)
    run = make()
    assert run.split and run.density_fn is None
    assert np.array_equal(run.proposal_factor().cpu().numpy(), np.eye(dim, dtype=np.float32))
    rxx, rx, rw, factor = np.zeros((dim, dim)), np.zeros(dim), 0.0, np.eye(dim, dtype=np.float32)
    wants, cold0, state0, logp0 = [], None, None, None
    for window in range(2):
        tr = torch.empty(W // P, Cn, 1, dim, device=device)
        run.advance(W, trace=tr, trace_every=P)
        torch.cuda.synchronize()
        assert run._graph is None  # (a traced chunk runs step by step)
        rows = tr.cpu().numpy().reshape(-1, dim).astype(np.float64)
        n = rows.shape[0]
        assert n == (W // P) * Cn
        sxx, sx = sums_of(rows)
        outcome, want, rxx, rx, rw = PR.update(sxx, sx, n, rxx, rx, rw, 0.5, 1e-6, 4.0 * dim, factor)
        assert outcome == PR.UPDATED
        m = rx / rw
        kappa = np.linalg.cond(np.tril(rxx) / rw + np.tril(rxx, -1).T / rw - np.outer(m, m))
        bound = (n + dim) * 2.0 ** -53 * kappa
        assert kappa < 8.0 and bound < 2.0 ** -25
        h = run.preconditioner_history()
        assert h["skipped"] == 0
        assert float(h["weights"][window]) == rw == (8192.0 if window == 0 else 12288.0)
        got = run.proposal_factor().cpu().numpy()
        worst = int(ulps(got[tri], want[tri]).max())
        print(f"READINGS ladder adaptation window {window}: factor within {worst} float32 ulp(s) of the reference, weight {rw:.0f}, "
              f"kappa {kappa:.2f}, bound {bound:.2e} against half an ulp {2.0 ** -25:.2e}")
        assert worst <= 1
        assert np.array_equal(h["factors"][window + 1].cpu().numpy(), got) and not np.triu(got, 1).any()
        wants.append(want)
        if window == 0:
            cold0, state0, logp0 = tr.clone(), run.state.clone(), run.logp.clone()
        factor = got  # (the next window ran with the device's own factor)
    # the control: rung 1 of a full trace
    twin = make()
    full = torch.empty(W // P, Cn, T, dim, device=device)
    twin.advance(W, trace=full, trace_every=P)
    torch.cuda.synchronize()
    assert torch.equal(full[:, :, :1], cold0)
    got0 = twin.proposal_factor().cpu().numpy()
    assert int(ulps(got0[tri], wants[0][tri]).max()) <= 1
    sxx, sx = sums_of(full[:, :, 1].cpu().numpy().reshape(-1, dim).astype(np.float64))
    outcome, hot, _, _, _ = PR.update(sxx, sx, (W // P) * Cn, np.zeros((dim, dim)), np.zeros(dim), 0.0, 0.5, 1e-6, 4.0 * dim,
                                      np.eye(dim, dtype=np.float32))
    ratio = np.diag(hot) / np.diag(got0)
    print(f"READINGS ladder adaptation control: the factor of rung 1's sums is {ratio.min():.3f}..{ratio.max():.3f} times the device's, "
          f"{int(ulps(got0[tri], hot[tri]).max())} ulps away")
    assert outcome == PR.UPDATED and int(ulps(got0[tri], hot[tri]).max()) > 1
    assert np.all((ratio > 1.3) & (ratio < 1.55))  # sqrt 2, within the sampling error of 8 192 draws (1 %) many times over
    # captured blocks
    graph = make()
    assert graph.use_graph
    graph.advance(W)
    torch.cuda.synchronize()
    assert graph._graph is not None
    assert torch.equal(graph.state.view(torch.int32), state0.view(torch.int32)) and torch.equal(graph.logp.view(torch.int32), logp0.view(torch.int32))
    g0 = graph.proposal_factor().cpu().numpy()
    assert int(ulps(g0[tri], wants[0][tri]).max()) <= 1
    h = graph.preconditioner_history()
    assert h["skipped"] == 0 and float(h["weights"][0]) == 8192.0
    graph.advance(W)
    torch.cuda.synchronize()
    h = graph.preconditioner_history()
    assert h["skipped"] == 0 and float(h["weights"][1]) == 12288.0 and not bool(torch.isnan(h["factors"]).any())


@pytest.mark.gpu
def test_class_learns_a_factor_and_reset_restores_the_initial_one(device):
    """adapt_cov=True through the RWM class on a target with a fused kernel (split steps with the library's density, with the
    warning that says so): two windows update the factor towards the target's scales, the read-outs say so, and reset()
    returns to the initial factor and an empty history."""
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    dim, Cn = 4, 4096
    var = np.array([0.25, 1.0, 4.0, 16.0])
    rng = np.random.default_rng(3)
    x0 = (rng.standard_normal((Cn, dim)) * np.sqrt(var)).astype(np.float32)
    target = MultivariateNormalTorch(dim, mean=[0.0] * dim, cov=np.diag(var).tolist(), device=device)
    alg = RandomWalkMH_GPU_Optimized(dim, 2.38 ** 2 / dim * 0.25, target, device=device, num_chains=Cn, seed=11, burn_in=100,
                                     initial_states=x0, adapt_cov=True, cov_adapt_every=50, cov_adapt_probe_every=10)
    with pytest.warns(UserWarning, match="preconditioned proposals run in split steps"):
        alg._advance(120)
    torch.cuda.synchronize()
    f = alg.proposal_factor().numpy().astype(np.float64)
    assert np.allclose(np.diag(f @ f.T), var, rtol=0.15) and not np.triu(f, 1).any()
    h = alg.preconditioner_history()
    assert not bool(torch.isnan(h["factors"]).any()) and h["weights"].tolist() == [5.0 * Cn, 7.5 * Cn] and h["skipped"] == 0
    info = alg.get_diagnostic_info()
    assert info["preconditioned"] is True and info["precond_updates"] == 2 and info["precond_updates_skipped"] == 0
    assert info["precond_condition"] == pytest.approx(64.0, rel=0.3)
    alg.reset()
    assert np.array_equal(alg.proposal_factor().numpy(), np.eye(dim, dtype=np.float32))
    assert bool(torch.isnan(alg.preconditioner_history()["weights"]).all())
    with pytest.warns(UserWarning, match="preconditioned proposals run in split steps"):
        alg._advance(10)
    torch.cuda.synchronize()
    assert np.array_equal(alg.proposal_factor().numpy(), np.eye(dim, dtype=np.float32))  # (a fresh run: no window has ended)


# ---- 8. nothing else moved --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_runs_without_the_new_keywords_never_reach_the_new_entry_points(device, monkeypatch):
    """A spy on the binding: a run of each class without the new keywords - fused steps, and split steps around a user-defined
    density - issues no call to ptrwm_split_propose_precond or ptrwm_precond_update, and binds no factor; with proposal_cov
    the same spy sees the calls (so it can see)."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from interfaces import TorchTargetDistribution
    from target_distributions import RoughCarpetDistributionTorch

    lib = E.load_library()
    seen = []
    for name in ("ptrwm_split_propose_precond", "ptrwm_precond_update"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (seen.append(_n), _f(*a))[1])
    for name in ("set_preconditioner", "set_precond_update", "precond_probe", "precond_update"):
        real = getattr(E.RunPlan, name)
        monkeypatch.setattr(E.RunPlan, name, lambda self, *a, _n=name, _f=real, **k: (seen.append(_n), _f(self, *a, **k))[1])

    class User(TorchTargetDistribution):
        def get_name(self):
            return "User"

        def log_density(self, x):
            return -0.5 * (torch.as_tensor(x, device=self.device) ** 2).sum(-1)

        def density(self, x):
            return torch.exp(self.log_density(x))

    rwm = RandomWalkMH_GPU_Optimized(4, 1.0, RoughCarpetDistributionTorch(4, device=device), device=device, num_chains=64, seed=1, burn_in=4,
                                     adapt_scale=True, adapt_every=2)
    rwm._advance(40)
    with pytest.warns(UserWarning, match="no fused kernel"):
        pt = ParallelTemperingRWM_GPU_Optimized(4, 1.0, User(4, device), beta_ladder=[1.0, 0.5, 0.2], swap_every=2, device=device,
                                                num_replicas=64, seed=1, trace="none", cov="cold")
        pt._advance(40)
    torch.cuda.synchronize()
    assert seen == [] and rwm._run.chol is None and pt._run.chol is None and not rwm._run.split and pt._run.split
    with pytest.warns(UserWarning, match="split steps"):
        on = RandomWalkMH_GPU_Optimized(4, 1.0, RoughCarpetDistributionTorch(4, device=device), device=device, num_chains=64, seed=1,
                                        proposal_cov=np.diag([1.0, 2.0, 3.0, 4.0]))
        on._advance(3)
    torch.cuda.synchronize()
    assert seen.count("ptrwm_split_propose_precond") >= 3 and "set_preconditioner" in seen and "ptrwm_precond_update" not in seen
