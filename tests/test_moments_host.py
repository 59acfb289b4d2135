"""Posterior moments (include/ptrwm.h ptrwm_moments_args) without a GPU: the ctypes mirror has the C layout, every refusal
of the two entry points returns before the first HIP call, the drop-in classes reject bad `moments` arguments, and
allreduce_moments over a gloo world of two equals the sum of the shards.  CPU only."""
import ctypes as C
import os
import sys

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


def test_moments_args_mirror_has_the_c_layout(engine, tmp_path):
    fs = [f[0] for f in engine.MomentsArgs._fields_]
    assert_layout(engine.MomentsArgs, "ptrwm_moments_args", fs, c_layout(tmp_path, {"ptrwm_moments_args": fs}))
    assert fs == ["struct_size", "temps", "every", "sum", "sum_sq", "sum_logp", "count"]


def _moments(temps, every=1, sums=True):
    """A fresh accumulator block (no pointer of these tests is ever dereferenced: every case is refused, or has nothing to
    do, before anything is enqueued)."""
    m = valid_args("mom")["mom"]
    m.temps, m.every = temps, every
    if not sums:
        m.sum = m.sum_sq = None
    return m


def test_moments_refusals_need_no_gpu(engine):
    lib = engine.load_library()
    v = valid_args(n_temps=8)
    td, pd, ra = v["td"], v["pd"], v["ra"]
    td.p[0], td.p[1], td.p[2] = -15.0, 0.0, 15.0
    run = lambda m: lib.ptrwm_run_with_moments(C.byref(td), C.byref(pd), C.byref(ra), m, None)  # noqa: E731
    m = _moments(1)
    m.struct_size = 8
    assert run(C.byref(m)) == -6  # PTRWM_E_STRUCT
    for temps, every in ((0, 1), (9, 1), (-1, 1), (1, 0), (8, -3)):
        assert run(C.byref(_moments(temps, every))) == -5, (temps, every)  # PTRWM_E_ARG
    assert run(C.byref(_moments(1, sums=False))) == -1  # PTRWM_E_NULL
    m = _moments(1)
    m.sum_sq = None
    assert run(C.byref(m)) == -1
    # the run's own checks come first, as in ptrwm_run
    ra.swap_every = 0
    assert run(C.byref(_moments(1))) == -5
    ra.swap_every = 1
    ra.n_steps = 0
    assert run(C.byref(_moments(1))) == 0  # empty: nothing to do
    # an accumulator too big for the kernel's LDS: every temperature of a 256-rung ladder at dim 60 (thread form)
    td.dim = 60
    ra = valid_args(n_temps=256)["ra"]
    assert engine.has_thread_variant(td.kind, pd.kind, 60) and not engine.has_quad_variant(td.kind, pd.kind, 60, 256)
    with engine.kernel_form(engine.FORM_THREAD):
        assert run(C.byref(_moments(256))) == -5

    # split steps: the same argument checks
    sp = valid_args(n_temps=8)["ra"]
    assert lib.ptrwm_split_moments(C.byref(sp), 30, None, None) == -1
    assert lib.ptrwm_split_moments(None, 30, C.byref(_moments(1)), None) == -1
    m = _moments(1)
    m.struct_size = 0
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(m), None) == -6
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(_moments(9)), None) == -5
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(_moments(1, every=0)), None) == -5
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(_moments(1, sums=False)), None) == -1
    assert lib.ptrwm_split_moments(C.byref(sp), 0, C.byref(_moments(1)), None) == -2
    sp.n_chains = 0
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(_moments(1)), None) == 0  # empty batch
    # a step that does not count is known on the host: nothing is enqueued
    sp = valid_args(n_temps=8)["ra"]
    sp.burn_in, sp.step0 = 10, 3
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(_moments(1)), None) == 0
    sp.burn_in, sp.step0 = 0, 4  # step_counter 5, every 2
    assert lib.ptrwm_split_moments(C.byref(sp), 30, C.byref(_moments(1, every=2)), None) == 0


def test_the_classes_reject_bad_moments_arguments(engine):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import moments_temps
    from target_distributions import RoughCarpetDistributionTorch

    assert moments_temps(None, 8, 1) == 0 and moments_temps("cold", 8, 1) == 1 and moments_temps("all", 8, 3) == 8
    target = RoughCarpetDistributionTorch(5, device="cpu")
    for bad in ("warm", "COLD", 1, True, "every"):
        with pytest.raises(ValueError, match="moments"):
            RandomWalkMH_GPU_Optimized(5, 0.5, target, moments=bad)
        with pytest.raises(ValueError, match="moments"):
            ParallelTemperingRWM_GPU_Optimized(5, 0.5, target, beta_ladder=[1.0, 0.5], moments=bad)
    for bad in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="moments_every"):
            RandomWalkMH_GPU_Optimized(5, 0.5, target, moments="cold", moments_every=bad)
        with pytest.raises(ValueError, match="moments_every"):
            ParallelTemperingRWM_GPU_Optimized(5, 0.5, target, beta_ladder=[1.0, 0.5], moments="all", moments_every=bad)


TEMPS, DIM = 3, 4


def _shard(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return {"sum": torch.randn(TEMPS, DIM, generator=g, dtype=torch.float64),
            "sum_sq": torch.rand(TEMPS, DIM, generator=g, dtype=torch.float64),
            "sum_logp": torch.randn(TEMPS, generator=g, dtype=torch.float64),
            "count": torch.randint(0, 1 << 40, (TEMPS,), generator=g, dtype=torch.int64), "every": 5}


def _worker(rank):
    from algorithms.sharding import allreduce_moments

    shard = _shard(rank)
    kept = {k: v.clone() for k, v in shard.items() if torch.is_tensor(v)}
    total = allreduce_moments(shard)
    assert all(torch.equal(shard[k], v) for k, v in kept.items())  # inputs untouched
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in total.items()}


def test_allreduce_moments_over_two_ranks_is_the_sum_of_the_shards():
    from algorithms.sharding import allreduce_moments

    got = gloo_world(_worker)
    a, b = _shard(0), _shard(1)
    for _, total in got:
        for k in ("sum", "sum_sq", "sum_logp"):
            assert torch.allclose(torch.from_numpy(total[k]), a[k] + b[k], rtol=0, atol=1e-15)
        assert torch.equal(torch.from_numpy(total["count"]), a["count"] + b["count"])
        assert total["every"] == 5
    # no process group: the identity
    one = allreduce_moments(a)
    assert torch.equal(one["sum"], a["sum"]) and torch.equal(one["count"], a["count"])
