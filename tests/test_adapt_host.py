"""Warm-up tuning of the proposal scale (include/ptrwm.h ptrwm_adapt_args, csrc/adapt.h) without a GPU: the window helpers
and the launch / reduce / update sequence against brute force, the update rule against NumPy float64, the struct's C layout,
every validation code of the three entry points that returns before a HIP call, the classes' constructor checks, and
adaptation_sync over two gloo ranks."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import ptrwm_hip as E
from host_harness import assert_layout, c_layout, gloo_world, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def adapt_exe(tmp_path_factory):
    """tests/adapt_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    return sanitized_exe(tmp_path_factory.mktemp("adapt"), "adapt_test.cpp")


def test_window_helpers_and_cuts_against_brute_force(adapt_exe):
    """W in {1, 7, 50}, until in {0, W - 1, W, 3 W + 7, burn_in}: the launches csrc/schedule.h's warmup_launch_at - what
    ptrwm_run_with_adaptation's loop asks - cuts a run into, uncut, cut into two requests at every position of a 4-window run
    and cut into single steps, against a loop over the windows - each step covered once, no adapting launch across a window
    end, the same (reduce, update) sequence whatever the cut.  (The window helpers themselves: schedule_test.cpp,
    test_host_logic.py.)"""
    run_exe(adapt_exe, ok="adapt ok:")


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_update_rule_against_numpy_float64(adapt_exe):
    """10^4 random (s_old, pooled, gain_k), both clamps and pooled[T] = 0 among them: the header's update within one float32 ulp
    of the NumPy float64 restatement (the only difference is the double exp, a couple of double ulps at most, which moves the
    final rounding to float at a tie only), and exact wherever a clamp binds or nothing was counted."""
    rng = np.random.default_rng(20261019)
    n = 10_000
    s_old = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), n)).astype(np.float32)
    counted = rng.integers(1, 1 << 40, n)
    counted[rng.random(n) < 0.05] = 0
    accepted = (rng.random(n) * counted).astype(np.int64)
    accepted[rng.random(n) < 0.05] = 0
    full = rng.random(n) < 0.05
    accepted[full] = counted[full]
    gain_k = 3.0 / np.sqrt(rng.integers(1, 200, n).astype(np.float64))
    gain_k[rng.random(n) < 0.1] *= 40.0  # far past both clamps
    target = np.where(rng.random(n) < 0.8, 0.234, rng.uniform(0.05, 0.95, n))
    lo = (s_old.astype(np.float64) * np.exp(-rng.uniform(0.0, 3.0, n))).astype(np.float32)
    hi = (s_old.astype(np.float64) * np.exp(rng.uniform(0.0, 3.0, n))).astype(np.float32)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    lines = "".join(f"{sb} {a} {c} {g!r} {t!r} {l} {h}\n" for sb, a, c, g, t, l, h in
                    zip(_bits(s_old), accepted, counted, gain_k.tolist(), target.tolist(), _bits(lo), _bits(hi)))
    out = run_exe(adapt_exe, "update", input=lines, timeout=120)
    got = np.array([int(v) for v in out.split()], np.uint32).view(np.float32)
    assert got.shape == (n,)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rate = accepted.astype(np.float64) / counted.astype(np.float64)
        raw = s_old.astype(np.float64) * np.exp(gain_k * (rate - target))
    want = np.clip(raw, lo.astype(np.float64), hi.astype(np.float64)).astype(np.float32)
    none = counted == 0
    want[none] = s_old[none]
    clamped = ~none & ((raw <= lo) | (raw >= hi))
    assert none.sum() > 100 and (~none & (raw <= lo)).sum() > 100 and (~none & (raw >= hi)).sum() > 100
    assert np.array_equal(got[none], s_old[none])
    assert np.array_equal(got[clamped], want[clamped])
    ulp = np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64))
    assert ulp.max() <= 1, (ulp.max(), int(np.argmax(ulp)))
    assert (ulp == 0).mean() > 0.99  # a tie of the float rounding is rare


FIELDS = ["struct_size", "every", "until", "target", "gain", "decay", "min_scale", "max_scale", "defer_update", "temp_scale",
          "window_accept", "pooled", "scale_history", "accept_history"]


def test_adapt_struct_layout_matches_the_c_header(tmp_path):
    assert [f[0] for f in E.AdaptArgs._fields_] == FIELDS
    got = c_layout(tmp_path, {"ptrwm_adapt_args": FIELDS}, macros=("PTRWM_ABI_VERSION",))
    assert_layout(E.AdaptArgs, "ptrwm_adapt_args", FIELDS, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays


def _valid(n_temps=4):
    """Arguments the three entry points accept up to their first HIP call."""
    # burn_in 100, so ad.until == 100 in windows of ad.every == 10: "until = 101 past burn_in", "window 9 ends after step 99"
    # and the update's K = 10 windows below
    return valid_args("ad", n_temps=n_temps, burn_in=100)


def test_adapt_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v):
        return lib.ptrwm_run_with_adaptation(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, None,
                                             C.byref(v["ad"]), None)

    def reduce(v):
        return lib.ptrwm_adapt_reduce(C.byref(v["ra"]), C.byref(v["ad"]), None)

    def update(v):
        return lib.ptrwm_adapt_update(C.byref(v["ad"]), v["ra"].n_temps, 0, None)

    inf, nan = float("inf"), float("nan")
    shared = [("struct_size", 4, -6), ("temp_scale", None, -1), ("window_accept", None, -1), ("pooled", None, -1),
              ("every", 0, -5), ("every", -3, -5), ("until", -1, -5), ("target", 0.0, -5), ("target", 1.0, -5), ("target", nan, -5),
              ("gain", 0.0, -5), ("gain", -1.0, -5), ("gain", inf, -5), ("gain", nan, -5), ("decay", -0.1, -5), ("decay", 1.5, -5),
              ("decay", nan, -5), ("min_scale", 0.0, -5), ("min_scale", 2e6, -5), ("min_scale", nan, -5), ("max_scale", inf, -5),
              ("max_scale", nan, -5), ("defer_update", 2, -5), ("defer_update", -1, -5)]
    for call in (run, reduce, update):
        for field, bad, code in shared:
            v = _valid()
            setattr(v["ad"], field, bad)
            assert call(v) == code, (call.__name__, field, bad)
    # what needs the run
    v = _valid()
    v["ad"].until = 101  # past burn_in
    assert run(v) == -5
    v = _valid()
    other = C.create_string_buffer(64)
    v["ad"].temp_scale = C.cast(other, C.c_void_p)  # not the memory the proposal points to
    assert run(v) == -5
    # the existing checks come first
    v = _valid()
    v["ad"].every, v["ra"].swap_every = 0, 0
    assert run(v) == -5
    v["ra"].swap_every, v["ra"].n_temps = 1, 257
    assert run(v) == -3
    v = _valid()
    v["ad"].struct_size, v["ra"].struct_size = 4, 4
    assert run(v) == -6 and reduce(v) == -6
    # defer_update: a request may not step past the end of the adapting window it starts in - refused before anything is
    # enqueued (the NULL stream and host pointers of this test would not survive a launch)
    v = _valid()
    v["ad"].defer_update = 1
    v["ra"].step0, v["ra"].n_steps = 3, 8  # window 0 ends after step 9: 3 + 7 steps
    assert run(v) == -5
    v["ra"].step0, v["ra"].n_steps = 95, 20  # window 9 ends after step 99
    assert run(v) == -5
    # an empty request is fine wherever it starts; NULL adapt arguments of the stand-alone calls are not
    v["ra"].n_steps = 0
    assert run(v) == 0
    v = _valid()
    v["ra"].n_chains = 0
    assert reduce(v) == 0 and run(v) == 0
    assert lib.ptrwm_adapt_reduce(None, None, None) == -1 and lib.ptrwm_adapt_update(None, 4, 0, None) == -1
    assert lib.ptrwm_adapt_reduce(C.byref(v["ra"]), None, None) == -1
    # the update's window must be one of the K = until / every the histories have rows for
    v = _valid()
    assert lib.ptrwm_adapt_update(C.byref(v["ad"]), 4, 10, None) == -5 and lib.ptrwm_adapt_update(C.byref(v["ad"]), 4, -1, None) == -5
    assert lib.ptrwm_adapt_update(C.byref(v["ad"]), 0, 0, None) == -3 and lib.ptrwm_adapt_update(C.byref(v["ad"]), 257, 0, None) == -3
    v["ad"].until = 9  # no window fits
    assert lib.ptrwm_adapt_update(C.byref(v["ad"]), 4, 0, None) == -5


BAD_CTOR = [(dict(adapt_scale=1), "adapt_scale"), (dict(adapt_every=0), "adapt_every"), (dict(adapt_every=2.5), "adapt_every"),
            (dict(adapt_until=-1), "adapt_until"), (dict(adapt_until=201), "adapt_until"), (dict(adapt_target=0.0), "adapt_target"),
            (dict(adapt_target=1.0), "adapt_target"), (dict(adapt_gain=0.0), "adapt_gain"), (dict(adapt_gain=float("inf")), "adapt_gain"),
            (dict(adapt_decay=-0.5), "adapt_decay"), (dict(adapt_decay=1.5), "adapt_decay"), (dict(adapt_scale_bounds=(0.0, 1.0)), "adapt_scale_bounds"),
            (dict(adapt_scale_bounds=(2.0, 1.0)), "adapt_scale_bounds"), (dict(adapt_scale_bounds=3.0), "adapt_scale_bounds"),
            (dict(adapt_sync=7), "adapt_sync")]


def test_class_adapt_checks_need_no_gpu():
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import EngineRun
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    for bad, msg in BAD_CTOR:
        kw = {"adapt_scale": True, **bad}
        with pytest.raises(ValueError, match=msg):
            ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], burn_in=200, device="cpu", **kw)
        with pytest.raises(ValueError, match=msg):
            RandomWalkMH_GPU_Optimized(3, 1.0, tgt, burn_in=200, device="cpu", **kw)
        with pytest.raises(ValueError, match=msg):
            EngineRun(target_dist=tgt, proposal=None, beta_ladder=[1.0, 0.5], dim=3, device=torch.device("cpu"), n_replicas=1,
                      initial_state=np.zeros(3, np.float32), burn_in=200, swap_every=1, swap_mode="exchange",
                      swap_order="sequential", seed=1, **kw)
    with pytest.warns(UserWarning, match="nothing will adapt"):
        RandomWalkMH_GPU_Optimized(3, 1.0, tgt, burn_in=49, device="cpu", adapt_scale=True)
    with pytest.warns(UserWarning, match="nothing will adapt"):
        ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], burn_in=0, device="cpu", adapt_scale=True)
    # off: the other arguments are not looked at, nothing warns, and the readers say so
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], burn_in=0, device="cpu", adapt_every=0)
    with pytest.raises(RuntimeError, match="adaptation is off"):
        off.adaptation_history()
    # before the first step: the initial scales sqrt(var / beta_t), a history of K = adapt_until // adapt_every empty windows
    pt = ParallelTemperingRWM_GPU_Optimized(3, 4.0, tgt, beta_ladder=[1.0, 0.25], burn_in=200, device="cpu", adapt_scale=True,
                                            adapt_every=30, adapt_until=100)
    assert pt.proposal_scales().tolist() == [2.0, 4.0]
    h = pt.adaptation_history()
    assert tuple(h["scales"].shape) == (4, 2) and tuple(h["acceptance"].shape) == (3, 2)
    assert h["scales"][0].tolist() == [2.0, 4.0] and bool(torch.isnan(h["scales"][1:]).all()) and bool(torch.isnan(h["acceptance"]).all())
    info = pt.get_diagnostic_info()
    assert info["init_scales"] == [2.0, 4.0] and info["adapted_scales"] == [2.0, 4.0]
    rw = RandomWalkMH_GPU_Optimized(3, 9.0, tgt, burn_in=100, device="cpu", adapt_scale=True)
    assert rw.proposal_scales().tolist() == [3.0] and tuple(rw.adaptation_history()["scales"].shape) == (3, 1)
    assert rw.get_diagnostic_info()["init_scales"] == [3.0]


POOLED = 5  # n_temps + 1


def _pooled_shard(rank):
    g = torch.Generator().manual_seed(40 + rank)
    p = torch.randint(0, 1 << 20, (POOLED,), generator=g, dtype=torch.int64)
    p[1] = (1 << 31) + 3 + rank  # above 2^31: a narrowing conversion anywhere would show
    return p


def _sync_worker(rank):
    from algorithms.sharding import adaptation_sync

    p = _pooled_shard(rank)
    out = adaptation_sync()(p)
    assert out is p and p.dtype == torch.int64  # in place
    return p.numpy()


def test_adaptation_sync_over_two_ranks_is_the_sum_of_the_shards():
    """gloo, two spawned ranks, CPU tensors: every rank ends with the same integers, the sum of the shards' pooled counts; without
    a process group the counts are left alone."""
    from algorithms.sharding import adaptation_sync

    alone = _pooled_shard(0)
    assert torch.equal(adaptation_sync()(alone), _pooled_shard(0))
    got = gloo_world(_sync_worker)
    want = (_pooled_shard(0) + _pooled_shard(1)).numpy()
    assert int(want[1]) == (1 << 32) + 7
    assert sorted(r for r, _ in got) == [0, 1]
    for _, total in got:
        assert np.array_equal(total, want)
