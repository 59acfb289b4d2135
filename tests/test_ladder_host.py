"""Warm-up tuning of the temperature ladder (include/ptrwm.h ptrwm_ladder_args, csrc/ladder.h) without a GPU: the window and
probe helpers and the launch / probe / update sequence against brute force, the update rule against the NumPy float64
restatement of tests/ladder_reference.py, the struct's C layout, every validation code of the three entry points that returns
before a HIP call, the classes' constructor checks, and adaptation_sync over two gloo ranks on a [n_temps] tensor."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import ladder_reference as LR
import ptrwm_hip as E
from host_harness import assert_layout, c_layout, gloo_world, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def ladder_exe(tmp_path_factory):
    """tests/ladder_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    return sanitized_exe(tmp_path_factory.mktemp("ladder"), "ladder_test.cpp")


def test_window_helpers_and_cuts_against_brute_force(ladder_exe):
    """V in {1, 6, 50}, probe_every in {1, V / 2, V}, until in {0, V - 1, V, 3 V + 5, burn_in}: the launches
    csrc/schedule.h's warmup_launch_at - what ptrwm_run_with_ladder's loop asks - cuts a run into, uncut, cut in two at every
    step of a 4-window run and cut into single steps, against a loop over the windows - each step covered once, no launch
    across a probe step, the same (probe, update) sequence whatever the cut; with the scale's adaptation at W = 7 next to V = 6
    the order scale reduce, scale update, ladder probe, ladder update at shared ends.  (The window helpers themselves:
    schedule_test.cpp, test_host_logic.py.)"""
    run_exe(ladder_exe, ok="ladder ok:")


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _random_ladder(rng, T):
    """A positive, strictly decreasing float32 ladder from 1 (or near it) down to a random hot end, unevenly spaced."""
    lo = np.exp(rng.uniform(np.log(1e-4), np.log(0.5)))
    gaps = rng.random(T - 1) ** rng.choice([1.0, 3.0]) + 1e-3
    logb = -np.cumsum(gaps) / gaps.sum() * -np.log(lo)
    b = np.concatenate([[1.0], np.exp(logb)]).astype(np.float32) * np.float32(rng.choice([1.0, 0.7]))
    return b


def test_update_rule_against_numpy_float64(ladder_exe):
    """10^4 random ladders, T in 3..256, random integer pooled rows, zero counts among them: beta_new within one float32 ulp of
    the restatement (the only differences are the double exp and log, a few double ulps, which move the rounding to float at a
    tie only), the ends bit-identical, a zero count leaves every bit unchanged, a ladder with gaps of one float ulp near 1 takes
    the skip path, and the rescaled scales match s sqrt(b_old / b_new) within one ulp."""
    rng = np.random.default_rng(20261020)
    n = 10_000
    cases = []
    for i in range(n):
        T = int(rng.integers(3, 257)) if i % 4 else int(rng.integers(3, 9))
        beta = _random_ladder(rng, T)
        if i % 500 == 7:  # gaps of one ulp next to 1
            beta = (np.float32(1.0).view(np.uint32) - np.arange(T, dtype=np.uint32)).view(np.float32)
        assert (beta[:-1] > beta[1:]).all() and beta[-1] > 0
        probes = int(rng.integers(1, 1 << 22)) if rng.random() > 0.05 else 0
        pooled = (rng.random(T) ** rng.choice([1.0, 4.0]) * max(probes, 3) * LR.Q).astype(np.int64)
        if rng.random() < 0.05:
            pooled[rng.integers(0, T - 1)] = 0
        pooled[T - 1] = probes
        gain_j = float(2.0 / np.sqrt(float(rng.integers(1, 200))))
        scale = np.exp(rng.uniform(-3, 3, T)).astype(np.float32)
        cases.append((T, gain_j, beta, pooled, scale))
    lines = "".join(f"{T} {g!r} {' '.join(map(str, _bits(b)))} {' '.join(map(str, p))} {' '.join(map(str, _bits(s)))}\n"
                    for T, g, b, p, s in cases)
    rows = run_exe(ladder_exe, "update", input=lines).splitlines()
    assert len(rows) == n
    outcomes, worst, worst_s, exact = [0, 0, 0], 0, 0, 0
    for (T, g, beta, pooled, scale), row in zip(cases, rows):
        v = np.array(row.split(), np.int64)
        got_outcome, got = int(v[0]), v[1:1 + T].astype(np.uint32).view(np.float32)
        got_s = v[1 + T:].astype(np.uint32).view(np.float32)
        want, outcome = LR.update(beta, pooled, g)
        assert got_outcome == outcome, (T, outcome, got_outcome)
        outcomes[outcome] += 1
        assert _bits(got)[0] == _bits(beta)[0] and _bits(got)[-1] == _bits(beta)[-1]  # the ends keep their bits
        if outcome != 0:
            assert np.array_equal(_bits(got), _bits(beta)) and np.array_equal(_bits(got_s), _bits(scale))
            continue
        d = LR.ulps(got, want)
        worst, exact = max(worst, int(d.max())), exact + int((d == 0).all())
        assert (got[:-1] > got[1:]).all()
        # the scales: against the restatement applied to the header's own new ladder (one ulp: the double sqrt is exact)
        worst_s = max(worst_s, int(LR.ulps(got_s, LR.rescale(scale, beta, got)).max()))
        assert _bits(got_s)[0] == _bits(scale)[0] and _bits(got_s)[-1] == _bits(scale)[-1]
    assert worst <= 1 and worst_s <= 1, (worst, worst_s)
    assert outcomes[1] > 100 and outcomes[2] >= 10 and outcomes[0] > 9000, outcomes
    assert exact > 0.9 * outcomes[0]  # a tie of the float rounding is rare


FIELDS = ["struct_size", "every", "probe_every", "until", "gain", "decay", "rescale_scales", "defer_update", "beta", "temp_scale",
          "pooled", "beta_history", "rate_history", "skipped"]


def test_ladder_struct_layout_matches_the_c_header(tmp_path):
    assert [f[0] for f in E.LadderArgs._fields_] == FIELDS
    got = c_layout(tmp_path, {"ptrwm_ladder_args": FIELDS}, macros=("PTRWM_ABI_VERSION",))
    assert_layout(E.LadderArgs, "ptrwm_ladder_args", FIELDS, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays


def _valid(n_temps=4):
    """Arguments the three entry points accept up to their first HIP call."""
    # burn_in 100, so ld.until == 100 in windows of ld.every == 10: "until = 101 past burn_in", "window 9 ends after step 99"
    # and the update's K = 10 windows below
    return valid_args("ld", n_temps=n_temps, burn_in=100)


def test_ladder_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v):
        return lib.ptrwm_run_with_ladder(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, None, None,
                                         C.byref(v["ld"]), None)

    def probe(v):
        return lib.ptrwm_ladder_probe(C.byref(v["ra"]), C.byref(v["ld"]), None)

    def update(v):
        return lib.ptrwm_ladder_update(C.byref(v["ld"]), v["ra"].n_temps, 0, None)

    inf, nan = float("inf"), float("nan")
    shared = [("struct_size", 4, -6), ("beta", None, -1), ("pooled", None, -1), ("temp_scale", None, -1),
              ("every", 0, -5), ("every", -3, -5), ("probe_every", 0, -5), ("probe_every", 3, -5), ("probe_every", 20, -5),
              ("until", -1, -5), ("gain", 0.0, -5), ("gain", -1.0, -5), ("gain", inf, -5), ("gain", nan, -5), ("decay", -0.1, -5),
              ("decay", 1.5, -5), ("decay", nan, -5), ("rescale_scales", 2, -5), ("rescale_scales", -1, -5),
              ("defer_update", 2, -5), ("defer_update", -1, -5)]
    for call in (run, probe, update):
        for field, bad, code in shared:
            v = _valid()
            setattr(v["ld"], field, bad)
            assert call(v) == code, (call.__name__, field, bad)
    # a NULL temp_scale is fine where nothing is rescaled: the stand-alone update's window check is then what refuses
    v = _valid()
    v["ld"].temp_scale, v["ld"].rescale_scales = None, 0
    assert lib.ptrwm_ladder_update(C.byref(v["ld"]), 4, 10, None) == -5
    # fewer than three temperatures: nothing to move
    for call in (run, probe, update):
        v = _valid(n_temps=2)
        assert call(v) == -5, call.__name__
    # what needs the run
    v = _valid()
    v["ld"].until = 101  # past burn_in
    assert run(v) == -5
    other = C.create_string_buffer(64)
    v = _valid()
    v["ld"].beta = C.cast(other, C.c_void_p)  # not the memory the run's beta points to
    assert run(v) == -5 and probe(v) == -5
    v = _valid()
    v["ld"].temp_scale = C.cast(other, C.c_void_p)  # not the memory the proposal points to
    assert run(v) == -5
    # the existing checks come first
    v = _valid()
    v["ld"].every, v["ra"].swap_every = 0, 0
    assert run(v) == -5
    v["ra"].swap_every, v["ra"].n_temps = 1, 257
    assert run(v) == -3 and probe(v) == -3
    v = _valid()
    v["ld"].struct_size, v["ra"].struct_size = 4, 4
    assert run(v) == -6 and probe(v) == -6
    # defer_update: a request may not step past the end of the adapting window it starts in - refused before anything is
    # enqueued (the NULL stream and host pointers of this test would not survive a launch)
    v = _valid()
    v["ld"].defer_update = 1
    v["ra"].step0, v["ra"].n_steps = 3, 8  # window 0 ends after step 9: 3 + 7 steps
    assert run(v) == -5
    v["ra"].step0, v["ra"].n_steps = 95, 20  # window 9 ends after step 99
    assert run(v) == -5
    # an empty request is fine wherever it starts; NULL arguments of the stand-alone calls are not
    v["ra"].n_steps = 0
    assert run(v) == 0
    v = _valid()
    v["ra"].n_chains = 0
    assert probe(v) == 0 and run(v) == 0
    assert lib.ptrwm_ladder_probe(None, None, None) == -1 and lib.ptrwm_ladder_update(None, 4, 0, None) == -1
    assert lib.ptrwm_ladder_probe(C.byref(v["ra"]), None, None) == -1
    # the update's window must be one of the K = until / every the histories have rows for
    v = _valid()
    assert lib.ptrwm_ladder_update(C.byref(v["ld"]), 4, 10, None) == -5 and lib.ptrwm_ladder_update(C.byref(v["ld"]), 4, -1, None) == -5
    assert lib.ptrwm_ladder_update(C.byref(v["ld"]), 0, 0, None) == -3 and lib.ptrwm_ladder_update(C.byref(v["ld"]), 257, 0, None) == -3
    v["ld"].until = 9  # no window fits
    assert lib.ptrwm_ladder_update(C.byref(v["ld"]), 4, 0, None) == -5
    # ladder == NULL is ptrwm_run_with_adaptation: the same refusals
    v = _valid()
    v["ra"].swap_every = 0
    assert lib.ptrwm_run_with_ladder(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, None, None, None, None) == -5


GOOD = [1.0, 0.5, 0.25]
BAD_CTOR = [(dict(adapt_ladder=1), "adapt_ladder"), (dict(ladder_every=0), "ladder_every"), (dict(ladder_every=2.5), "ladder_every"),
            (dict(ladder_until=-1), "ladder_until"), (dict(ladder_until=201), "ladder_until"), (dict(ladder_probe_every=0), "ladder_probe_every"),
            (dict(ladder_probe_every=7), "ladder_probe_every"), (dict(ladder_probe_every=200), "ladder_probe_every"),
            (dict(ladder_gain=0.0), "ladder_gain"), (dict(ladder_gain=float("inf")), "ladder_gain"), (dict(ladder_decay=-0.5), "ladder_decay"),
            (dict(ladder_decay=1.5), "ladder_decay"), (dict(adapt_sync=7), "adapt_sync"),
            (dict(beta_ladder=[1.0, 0.5]), "at least 3"), (dict(beta_ladder=[1.0, 0.5, 0.0]), "strictly decreasing"),
            (dict(beta_ladder=[1.0, 0.5, -0.1]), "strictly decreasing"), (dict(beta_ladder=[1.0, 0.5, 0.5]), "strictly decreasing"),
            (dict(beta_ladder=[0.5, 1.0, 0.25]), "strictly decreasing"),
            (dict(beta_ladder=[1.0, 1.0 - 1e-9, 0.25]), "strictly decreasing")]  # (equal once rounded to float32)


def test_class_ladder_checks_need_no_gpu():
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import EngineRun

    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    for bad, msg in BAD_CTOR:
        kw = {"adapt_ladder": True, "beta_ladder": GOOD, **bad}
        with pytest.raises(ValueError, match=msg):
            ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, burn_in=200, device="cpu", **kw)
        with pytest.raises(ValueError, match=msg):
            EngineRun(target_dist=tgt, proposal=None, dim=3, device=torch.device("cpu"), n_replicas=1,
                      initial_state=np.zeros(3, np.float32), burn_in=200, swap_every=1, swap_mode="exchange",
                      swap_order="sequential", seed=1, **kw)
    with pytest.raises(ValueError, match="adapt_ladder"):
        RandomWalkMH_GPU_Optimized(3, 1.0, tgt, burn_in=200, device="cpu", adapt_ladder=True)
    with pytest.warns(UserWarning, match="will not move"):
        ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=GOOD, burn_in=99, device="cpu", adapt_ladder=True)
    # off: the other arguments are not looked at, nothing warns, and the readers say so
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], burn_in=0, device="cpu", ladder_every=0)
        RandomWalkMH_GPU_Optimized(3, 1.0, tgt, burn_in=0, device="cpu", adapt_ladder=False)
    with pytest.raises(RuntimeError, match="tuning is off"):
        off.ladder_history()
    assert "adapted_beta_ladder" not in off.get_diagnostic_info()
    # before the first step: the initial ladder, a history of K = ladder_until // ladder_every empty windows
    pt = ParallelTemperingRWM_GPU_Optimized(3, 4.0, tgt, beta_ladder=GOOD, burn_in=200, device="cpu", adapt_ladder=True,
                                            ladder_every=30, ladder_until=100, ladder_probe_every=10)
    assert pt.adapted_beta_ladder() == GOOD and pt.beta_ladder == GOOD
    h = pt.ladder_history()
    assert tuple(h["betas"].shape) == (4, 3) and tuple(h["rates"].shape) == (3, 2) and h["probes"].tolist() == [0, 0, 0]
    assert h["betas"][0].tolist() == GOOD and bool(torch.isnan(h["betas"][1:]).all()) and bool(torch.isnan(h["rates"]).all())
    info = pt.get_diagnostic_info()
    assert info["init_beta_ladder"] == GOOD and info["adapted_beta_ladder"] == GOOD and info["ladder_updates_skipped"] == 0
    pt.reset()
    assert pt.beta_ladder == GOOD


POOLED = 4  # n_temps


def _pooled_shard(rank):
    g = torch.Generator().manual_seed(60 + rank)
    p = torch.randint(0, 1 << 40, (POOLED,), generator=g, dtype=torch.int64)
    p[1] = (1 << 52) + 3 + rank  # far above 2^31, and above 2^53 once summed with 2^24 quanta: no float on the way
    return p


def _sync_worker(rank):
    from algorithms.sharding import adaptation_sync

    p = _pooled_shard(rank)
    out = adaptation_sync()(p)
    assert out is p and p.dtype == torch.int64  # in place
    return p.numpy()


def test_adaptation_sync_over_two_ranks_on_a_ladder_row():
    """gloo, two spawned ranks, CPU tensors of the ladder's [n_temps] shape: every rank ends with the same integers, the sum of
    the shards' pooled rows."""
    got = gloo_world(_sync_worker)
    want = (_pooled_shard(0) + _pooled_shard(1)).numpy()
    assert int(want[1]) == (1 << 53) + 7
    assert sorted(r for r, _ in got) == [0, 1]
    for _, total in got:
        assert np.array_equal(total, want)
