"""Per-chain posterior moments (include/ptrwm.h ptrwm_chain_moments_args) without a GPU: the R-hat / ESS estimators against
a direct NumPy evaluation of their formulas, the new symbols and the C layout of the ctypes mirror, every refusal of the
two entry points before the first HIP call, the classes' argument check, and allreduce_chain_summary over a gloo world of
two against the single-process estimate.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from host_harness import ROOT, assert_layout, c_layout, gloo_world, valid_args


@pytest.fixture(scope="module")
def engine():
    import ptrwm_hip

    if not os.path.exists(ptrwm_hip.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__

        __graft_entry__.build()
    return ptrwm_hip


def numpy_rhat_ess(x):
    """The formulas of the estimators, evaluated directly on draws x [M chains, N draws, ...]."""
    M, N = x.shape[:2]
    m_c = x.mean(1)
    s2_c = x.var(1, ddof=1)
    W = s2_c.mean(0)
    B = N * m_c.var(0, ddof=1)
    var_plus = (N - 1) / N * W + B / N
    return np.sqrt(var_plus / W), np.minimum(M * N, M * N * var_plus / B)


def _synthetic(M, N, dim, seed):
    """AR(1) chains with chain-specific offsets: correlated draws, unequal chain means and variances."""
    rng = np.random.default_rng(seed)
    x = np.empty((M, N, dim))
    x[:, 0] = rng.normal(size=(M, dim))
    for i in range(1, N):
        x[:, i] = 0.8 * x[:, i - 1] + rng.normal(size=(M, dim)) * np.linspace(0.5, 1.5, dim)
    return x + rng.normal(scale=0.3, size=(M, 1, dim))


@pytest.mark.parametrize("M,N,dim", [(2, 2, 3), (7, 50, 4), (64, 200, 30), (1000, 17, 2)])
def test_rhat_and_ess_equal_the_formulas_on_synthetic_chains(M, N, dim):
    from algorithms._engine_core import rhat_ess_from_chain_sums

    x = _synthetic(M, N, dim, seed=M * 1000 + N)
    want_r, want_e = numpy_rhat_ess(x)
    rhat, ess = rhat_ess_from_chain_sums(torch.from_numpy(x.sum(1)), torch.from_numpy((x * x).sum(1)), N)
    assert rhat.shape == (dim,) and ess.shape == (dim,) and rhat.dtype == torch.float64
    np.testing.assert_allclose(rhat.numpy(), want_r, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ess.numpy(), want_e, rtol=1e-12, atol=0)
    assert np.all(ess.numpy() <= M * N)


def test_ess_is_capped_at_the_number_of_draws():
    """Chain means closer together than independent draws would put them: M N var+ / B exceeds M N, the estimate does not."""
    from algorithms._engine_core import rhat_ess_from_chain_sums

    rng = np.random.default_rng(3)
    x = rng.normal(size=(8, 40, 2))
    x -= x.mean(1, keepdims=True) * 0.999  # (nearly) equal chain means
    want_r, want_e = numpy_rhat_ess(x)
    rhat, ess = rhat_ess_from_chain_sums(torch.from_numpy(x.sum(1)), torch.from_numpy((x * x).sum(1)), 40)
    assert np.all(want_e == 8 * 40) and np.array_equal(ess.numpy(), want_e)
    np.testing.assert_allclose(rhat.numpy(), want_r, rtol=1e-12, atol=0)


@pytest.mark.parametrize("M,N", [(1, 50), (5, 1), (1, 1)])
def test_rhat_and_ess_are_nan_without_two_chains_of_two_draws(M, N):
    from algorithms._engine_core import rhat_ess_from_chain_sums

    x = _synthetic(M, N, 3, seed=1)
    rhat, ess = rhat_ess_from_chain_sums(torch.from_numpy(x.sum(1)), torch.from_numpy((x * x).sum(1)), N)
    assert rhat.shape == (3,) and torch.isnan(rhat).all() and torch.isnan(ess).all()


def test_new_symbols_exist_and_the_mirror_has_the_c_layout(engine, tmp_path):
    lib = engine.load_library()
    for name in ("ptrwm_run_with_chain_moments", "ptrwm_split_chain_moments"):
        assert name in engine.SYMBOLS and getattr(lib, name) is not None
    fs = [f[0] for f in engine.ChainMomentsArgs._fields_]
    assert_layout(engine.ChainMomentsArgs, "ptrwm_chain_moments_args", fs, c_layout(tmp_path, {"ptrwm_chain_moments_args": fs}))
    assert fs == ["struct_size", "temps", "every", "sum", "sum_sq", "sum_logp", "count"]


def test_the_two_accumulator_structs_are_one_layout(engine):
    """MomentsArgs and ChainMomentsArgs: the same size and the same fields - names, offsets, types (the library checks and
    reads both through one view, csrc/capi.hip)."""
    a, b = engine.MomentsArgs, engine.ChainMomentsArgs
    assert a is not b and C.sizeof(a) == C.sizeof(b)
    assert [f[0] for f in a._fields_] == [f[0] for f in b._fields_]
    for (name, ta), (_, tb) in zip(a._fields_, b._fields_):
        assert ta is tb, name
        assert getattr(a, name).offset == getattr(b, name).offset and getattr(a, name).size == getattr(b, name).size, name


def _cm(temps, every=1, sums=True):
    """A fresh accumulator block (no pointer of these tests is ever dereferenced: every case is refused, or has nothing to
    do, before anything is enqueued)."""
    m = valid_args("cmom")["cmom"]
    m.temps, m.every = temps, every
    if not sums:
        m.sum = m.sum_sq = None
    return m


def test_chain_moments_refusals_need_no_gpu(engine):
    lib = engine.load_library()
    v = valid_args(n_temps=8)
    td, pd, ra = v["td"], v["pd"], v["ra"]
    td.p[0], td.p[1], td.p[2] = -15.0, 0.0, 15.0
    run = lambda m: lib.ptrwm_run_with_chain_moments(C.byref(td), C.byref(pd), C.byref(ra), m, None)  # noqa: E731
    m = _cm(1)
    m.struct_size = 8
    assert run(C.byref(m)) == -6  # PTRWM_E_STRUCT
    for temps, every in ((0, 1), (9, 1), (-1, 1), (1, 0), (8, -3)):
        assert run(C.byref(_cm(temps, every))) == -5, (temps, every)  # PTRWM_E_ARG
    assert run(C.byref(_cm(1, sums=False))) == -1  # PTRWM_E_NULL
    m = _cm(1)
    m.sum_sq = None
    assert run(C.byref(m)) == -1
    # the run's own checks come first, as in ptrwm_run
    ra.swap_every = 0
    assert run(C.byref(_cm(1))) == -5
    ra.swap_every = 1
    ra.n_steps = 0
    assert run(C.byref(_cm(1))) == 0  # empty: nothing to do
    # the LDS limit.  RWM (one temperature) at dim 32: 4 waves x 64 chains x 65 doubles on top of the thread form's own
    # 40 960 bytes are more than 160 KiB, 4 x 16 x 65 in the lane-split form are not - a pinned thread form is refused, and
    # so is a shape neither form holds
    td.dim = 32
    ra = valid_args(n_temps=1)["ra"]
    assert engine.has_thread_variant(td.kind, pd.kind, 32) and engine.has_quad_variant(td.kind, pd.kind, 32, 1)
    with engine.kernel_form(engine.FORM_THREAD):
        assert run(C.byref(_cm(1))) == -5
    td.dim = 60
    ra = valid_args(n_temps=256)["ra"]  # thread form only; 256 x 121 doubles on top of 256 rows
    assert not engine.has_quad_variant(td.kind, pd.kind, 60, 256)
    assert run(C.byref(_cm(256))) == -5

    # split steps: the same argument checks
    sp = valid_args(n_temps=8)["ra"]
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, None, None) == -1
    assert lib.ptrwm_split_chain_moments(None, 30, C.byref(_cm(1)), None) == -1
    m = _cm(1)
    m.struct_size = 0
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(m), None) == -6
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(9)), None) == -5
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(0)), None) == -5
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(1, every=0)), None) == -5
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(1, sums=False)), None) == -1
    m = _cm(1)
    m.sum_sq = None
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(m), None) == -1
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 0, C.byref(_cm(1)), None) == -2
    sp.n_chains = 0
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(1)), None) == 0  # empty batch
    # a step that does not count is known on the host: nothing is enqueued
    sp = valid_args(n_temps=8)["ra"]
    sp.burn_in, sp.step0 = 10, 3
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(1)), None) == 0
    sp.burn_in, sp.step0 = 0, 4  # step_counter 5, every 2
    assert lib.ptrwm_split_chain_moments(C.byref(sp), 30, C.byref(_cm(1, every=2)), None) == 0


def test_the_classes_want_a_moments_mode_for_per_chain_moments(engine):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    target = RoughCarpetDistributionTorch(5, device="cpu")
    with pytest.raises(ValueError, match="moments_per_chain"):
        RandomWalkMH_GPU_Optimized(5, 0.5, target, moments=None, moments_per_chain=True)
    with pytest.raises(ValueError, match="moments_per_chain"):
        ParallelTemperingRWM_GPU_Optimized(5, 0.5, target, beta_ladder=[1.0, 0.5], moments_per_chain=True)
    # with a mode it is accepted (nothing runs before the first step: no GPU needed), and off by default
    a = RandomWalkMH_GPU_Optimized(5, 0.5, target, moments="cold", moments_per_chain=True)
    b = ParallelTemperingRWM_GPU_Optimized(5, 0.5, target, beta_ladder=[1.0, 0.5], moments="all", moments_per_chain=True)
    c = RandomWalkMH_GPU_Optimized(5, 0.5, target, moments="cold")
    assert a._moments_per_chain and b._moments_per_chain and not c._moments_per_chain
    with pytest.raises(RuntimeError, match="per-chain"):
        c.rhat()


TEMPS, DIM, DRAWS = 2, 3, 25


def _shard(rank, chains):
    """Per-chain sums of `chains` synthetic chains (what EngineRun.chain_moments() returns), and the draws behind them."""
    x = np.stack([_synthetic(chains, DRAWS, DIM, seed=50 + 7 * rank + t) for t in range(TEMPS)], 2)  # [M, N, temps, dim]
    cm = {"sum": torch.from_numpy(x.sum(1)), "sum_sq": torch.from_numpy((x * x).sum(1)),
          "sum_logp": torch.zeros(chains, TEMPS, dtype=torch.float64),
          "count": torch.full((TEMPS,), DRAWS, dtype=torch.int64), "every": 2}
    return cm, x


def _worker(rank):
    from algorithms.sharding import allreduce_chain_summary

    cm, _ = _shard(rank, 5 + 3 * rank)
    kept = {k: v.clone() for k, v in cm.items() if torch.is_tensor(v)}
    out = allreduce_chain_summary(cm)
    assert all(torch.equal(cm[k], v) for k, v in kept.items())  # inputs untouched
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def test_allreduce_chain_summary_over_two_ranks_equals_one_process():
    from algorithms._engine_core import rhat_ess_from_chain_sums
    from algorithms.sharding import allreduce_chain_summary

    got = gloo_world(_worker)
    (a, xa), (b, xb) = _shard(0, 5), _shard(1, 8)
    whole = {k: torch.cat([a[k], b[k]]) for k in ("sum", "sum_sq")}
    x = np.concatenate([xa, xb])
    for _, out in got:
        assert out["n_chains"] == 13 and out["draws"] == [DRAWS] * TEMPS
        assert out["rhat"].shape == (TEMPS, DIM) and out["ess"].shape == (TEMPS, DIM)
        for t in range(TEMPS):
            rhat, ess = rhat_ess_from_chain_sums(whole["sum"][:, t], whole["sum_sq"][:, t], DRAWS)
            np.testing.assert_allclose(out["rhat"][t], rhat.numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(out["ess"][t], ess.numpy(), rtol=1e-12, atol=0)
            want_r, want_e = numpy_rhat_ess(x[:, :, t])
            np.testing.assert_allclose(out["rhat"][t], want_r, rtol=1e-12, atol=0)
            np.testing.assert_allclose(out["ess"][t], want_e, rtol=1e-12, atol=0)
    # no process group: the shard's own estimate
    one = allreduce_chain_summary(a)
    rhat, ess = rhat_ess_from_chain_sums(a["sum"][:, 0], a["sum_sq"][:, 0], DRAWS)
    assert one["n_chains"] == 5
    np.testing.assert_allclose(one["rhat"][0].numpy(), rhat.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(one["ess"][0].numpy(), ess.numpy(), rtol=1e-13, atol=0)
