"""Pooled lagged autocovariance (include/ptrwm.h ptrwm_acf_args, csrc/acf.h) without a GPU: snapshot numbers, ring slots, the
launch cuts and the kernel geometry against brute force, the struct's C layout, every validation code of the two entry points
that returns before a HIP call, the estimators on hand-made sums, and Sokal's window on the exact AR(1) sequence."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ptrwm_hip as E
from host_harness import assert_layout, c_layout, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def acf_exe(tmp_path_factory):
    """tests/acf_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    return sanitized_exe(tmp_path_factory.mktemp("acf"), "acf_test.cpp")


def test_rule_cuts_and_geometry_against_brute_force(acf_exe):
    """csrc/acf.h and the cut of csrc/schedule.h in tests/acf_test.cpp: snapshot numbers and ring slots against a replay that
    counts, for burn_in that is and is not a multiple of every; the lags before and after the ring fills; the cuts with a
    histogram at another period; acf_geometry for every temps * dim in 1..26 624."""
    run_exe(acf_exe, ok="acf ok:")


def test_gpu_cases_have_the_geometry_they_are_named_for(acf_exe):
    """The shapes of tests/test_gpu_acf.py through acf_geometry itself: a change of a constant of csrc/acf.h cannot quietly
    turn the narrowest, widest and several-group cases into something else."""
    from test_gpu_acf import EQUALITY_CASES

    lines = "".join(f"{c['temps'] * c['dim']}\n" for c in EQUALITY_CASES)
    out = run_exe(acf_exe, "geometry", input=lines, timeout=60)
    geo = {c["name"]: dict(zip(("cols", "groups", "per", "chains", "last"), map(int, ln.split())), **c)
           for c, ln in zip(EQUALITY_CASES, out.splitlines())}
    assert len(geo) == len(EQUALITY_CASES)
    g = geo["partial_tile"]  # 70 chains: one tile, not full
    assert g["groups"] == 1 and g["per"] > 1 and g["Cn"] == 70 < g["chains"]
    g = geo["second_workgroup"]  # 300 chains: a second tile, partial
    assert g["chains"] < g["Cn"] == 300 < 2 * g["chains"] and g["temps"] < g["T"]
    g = geo["narrowest"]
    assert g["cols"] == 1 and g["per"] == 256
    g = geo["widest"]
    assert g["cols"] == 256 and g["per"] == 1 and g["groups"] == 1 and g["Cn"] > g["chains"]
    g = geo["t32_d30"]
    assert g["groups"] == 4 and g["cols"] == 240 and g["cols"] % g["dim"] == 0 and g["T"] == 32
    g = geo["d70_t8"]
    assert g["groups"] == 3 and g["cols"] % g["dim"] != 0 and g["last"] < g["cols"]


def test_launch_cuts_with_a_histogram_at_another_period(acf_exe):
    """The launches of ptrwm_run_with_autocorr replayed step by step in Python: acf every 7, histogram every 5, burn_in 11."""
    step0, n, burn, ae, he, cap = 3, 60, 11, 7, 5, 1000
    out = run_exe(acf_exe, "cuts", step0, n, burn, ae, he, cap, timeout=60)
    got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    want, start = [], step0
    for s in range(step0, step0 + n):  # step s has step counter s + 1
        sc = s + 1
        a, h = sc > burn and sc % ae == 0, sc > burn and sc % he == 0
        if a or h or s == step0 + n - 1:
            want.append((start, s + 1 - start, int(a), int(h)))
            start = s + 1
    assert got == want and sum(c[2] for c in got) == 8 and sum(c[3] for c in got) == 10  # step counters 14 .. 63; 15 .. 60
    assert any(c[2] and c[3] for c in got)  # step counter 35: both
    # no histogram, nothing due: one launch
    assert run_exe(acf_exe, "cuts", 0, 10, 10, 3, 0, 1000, timeout=60).split() == ["0", "10", "0", "0"]


def test_acf_struct_layout_matches_the_c_header(tmp_path):
    fields = [f[0] for f in E.AcfArgs._fields_]
    assert fields == ["struct_size", "temps", "every", "max_lag", "ring", "sxy", "head", "tail", "pairs"]
    got = c_layout(tmp_path, {"ptrwm_acf_args": fields}, macros=("PTRWM_ABI_VERSION", "PTRWM_ACF_MAX_LAG"))
    assert_layout(E.AcfArgs, "ptrwm_acf_args", fields, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays
    assert got["PTRWM_ACF_MAX_LAG"] == E.ACF_MAX_LAG == 1024
    assert "ptrwm_autocorr" in E.SYMBOLS and "ptrwm_run_with_autocorr" in E.SYMBOLS


def _valid(n_temps=4):
    """Arguments both entry points accept up to their first HIP call, with every block that check_acf comes after."""
    return valid_args("ac", "hi", "ad", "ld", n_temps=n_temps)  # ld.every == 10: "3 does not divide 10" below


def test_acf_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v, acf="ac", hist=None, adapt=None, ladder=None):
        ref = lambda k: C.byref(v[k]) if k else None  # noqa: E731
        return lib.ptrwm_run_with_autocorr(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, ref(hist), ref(adapt),
                                           ref(ladder), ref(acf), None)

    def snap(v, acf="ac", dim=30):
        return lib.ptrwm_autocorr(C.byref(v["ra"]), dim, C.byref(v[acf]) if acf else None, None)

    for call in (run, snap):
        v = _valid()
        v["ac"].struct_size = 4
        assert call(v) == -6, call.__name__  # PTRWM_E_STRUCT
        for field, bad in (("temps", 0), ("temps", 5), ("every", 0), ("max_lag", 0), ("max_lag", 1025)):
            v = _valid()
            setattr(v["ac"], field, bad)
            assert call(v) == -5, (call.__name__, field, bad)  # PTRWM_E_ARG
        for field in ("ring", "sxy", "head", "tail", "pairs"):
            v = _valid()
            setattr(v["ac"], field, None)
            assert call(v) == -1, (call.__name__, field)  # PTRWM_E_NULL
        v = _valid()
        v["ac"].temps, v["ac"].max_lag = 4, 1024  # the limits themselves pass
        v["ra"].n_chains = 0
        assert call(v) == 0
        # the order: struct size, then the arguments, then the pointers
        v = _valid()
        v["ac"].struct_size, v["ac"].every, v["ac"].ring = 4, 0, None
        assert call(v) == -6
        v = _valid()
        v["ac"].every, v["ac"].ring = 0, None
        assert call(v) == -5
        # the entry point's own checks come first: the argument block's size, the ladder's length
        v = _valid()
        v["ra"].struct_size, v["ac"].struct_size = 4, 4
        assert call(v) == -6
        v = _valid(n_temps=257)
        v["ac"].ring = None
        assert call(v) == -3
        # an empty batch with a valid block: nothing to do; with a bad block: still refused
        v = _valid()
        v["ra"].n_chains = 0
        assert call(v) == 0
        v["ac"].max_lag = 2000
        assert call(v) == -5
    # ptrwm_autocorr alone: NULL arguments, dim, the flags it reads; a NULL state after the block and the empty-batch return
    v = _valid()
    assert snap(v, acf=None) == -1
    assert lib.ptrwm_autocorr(None, 30, C.byref(v["ac"]), None) == -1
    assert snap(v, dim=0) == -2 and snap(v, dim=105) == -2
    v["ra"].state_f64 = 2
    assert snap(v) == -5
    v = _valid()
    v["ra"].step0 = -1
    assert snap(v) == -5
    v = _valid()
    v["ra"].state, v["ac"].max_lag = None, 0
    assert snap(v) == -5
    v["ac"].max_lag = 8
    assert snap(v) == -1
    # a step that is not due is known on the host: nothing is enqueued, so the fake pointers are never read
    v = _valid()
    v["ra"].step0, v["ra"].burn_in, v["ac"].every = 4, 0, 10  # step counter 5
    assert snap(v) == 0
    v["ra"].step0, v["ra"].burn_in = 9, 10  # step counter 10, still in burn-in
    assert snap(v) == 0
    # ptrwm_run_with_autocorr: check_acf runs after EVERY other block's checks - the run's own arguments, the histogram's, the
    # scale tuning's, the ladder's - and before anything is enqueued
    v = _valid()
    v["ra"].swap_mode, v["ac"].struct_size = 7, 4
    assert run(v) == -5
    v = _valid()
    v["hi"].n_bins, v["ac"].struct_size = 0, 4
    assert run(v, hist="hi") == -5
    v = _valid()
    v["ad"].window_accept, v["ac"].struct_size = None, 4
    assert run(v, adapt="ad") == -1
    v = _valid()
    v["ld"].probe_every, v["ac"].ring = 3, None  # (3 does not divide 10)
    assert run(v, ladder="ld") == -5
    v = _valid()
    v["ld"].struct_size, v["ac"].every = 4, 0
    assert run(v, ladder="ld") == -6
    v = _valid()
    v["td"].dim, v["ac"].ring = 105, None
    assert run(v) == -2
    # acf == NULL: ptrwm_run_with_ladder's codes
    v = _valid()
    v["ra"].state = None
    assert run(v, acf=None) == -1 == lib.ptrwm_run_with_ladder(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, None,
                                                               None, None, None)
    v = _valid()
    v["ra"].n_chains = 0
    assert run(v, acf=None) == 0
    # a request that passes every check goes on to the launch, which a machine without a GPU cannot make
    if not torch.cuda.is_available():
        v = _valid()
        assert run(v) == -7 and run(v, acf=None) == -7


def test_estimators_on_hand_made_sums():
    from algorithms._engine_core import acf_autocorrelation, acf_autocovariance

    # two coordinates, lags 0..2.  Coordinate 0: four pairs (1, 1), (2, 2), (3, 3), (4, 4) at lag 0 - variance 1.25 - and three
    # pairs (2, 1), (3, 2), (4, 3) at lag 1; nothing at lag 2.  Coordinate 1: a constant 2.
    pairs = torch.tensor([4, 3, 0])
    sxy = torch.tensor([[30.0, 16.0], [20.0, 12.0], [0.0, 0.0]])
    head = torch.tensor([[10.0, 8.0], [9.0, 6.0], [0.0, 0.0]])
    tail = torch.tensor([[10.0, 8.0], [6.0, 6.0], [0.0, 0.0]])
    c = acf_autocovariance(sxy, head, tail, pairs)
    assert c.dtype == torch.float64 and c.shape == (3, 2)
    assert c[0].tolist() == [1.25, 0.0]
    assert c[1, 0].item() == pytest.approx(20.0 / 3 - 3.0 * 2.0) and c[1, 1].item() == 0.0
    assert torch.isnan(c[2]).all()  # a lag nobody has reached yet
    rho = acf_autocorrelation(sxy, head, tail, pairs)
    assert rho[0, 0].item() == 1.0 and rho[1, 0].item() == pytest.approx((20.0 / 3 - 6.0) / 1.25)
    assert torch.isnan(rho[:, 1]).all()  # c_0 = 0: no correlation to speak of
    with pytest.raises(ValueError, match="lags, dim"):
        acf_autocovariance(sxy, head[:2], tail, pairs)


@pytest.mark.parametrize("phi", [0.0, 0.3, 0.5, 0.8, 0.9])
def test_sokal_window_on_the_exact_ar1_sequence(phi):
    """rho_k = phi^k: tau = (1 + phi) / (1 - phi), and a window M leaves out 2 phi^(M + 1) / (1 - phi) of it."""
    from algorithms._engine_core import sokal_window

    L, c = 256, 5.0
    rho = torch.tensor([[phi**k, (-phi) ** k] for k in range(L + 1)], dtype=torch.float64)
    tau, window, reached = sokal_window(rho, c)
    assert tau.dtype == torch.float64 and window.dtype == torch.int64 and reached.dtype == torch.bool
    assert reached.tolist() == [True, True]
    exact = (1 + phi) / (1 - phi)
    M = int(window[0])
    # the window is the smallest M with M >= c tau(M)
    tau_of = lambda m: 1 + 2 * sum(phi**k for k in range(1, m + 1))  # noqa: E731
    assert M >= c * tau_of(M) and all(m < c * tau_of(m) for m in range(1, M))
    trunc = 2 * phi ** (M + 1) / (1 - phi)
    # (tau(M) is a float64 running sum of M <= L terms, each partial sum below `exact`: its rounding stays under L 2^-53 exact,
    # and as much again for the powers and the expressions here)
    fp = 2 * L * 2.0 ** -53 * exact
    assert -fp <= exact - float(tau[0]) <= trunc + fp
    assert abs(float(tau[0]) - (exact - trunc)) <= fp
    # the alternating sequence: tau = (1 - phi) / (1 + phi), within its own truncation term
    M1 = int(window[1])
    assert abs(float(tau[1]) - (1 - phi) / (1 + phi)) <= 2 * phi ** (M1 + 1) / (1 + phi) + fp


def test_sokal_window_not_reached_is_a_lower_bound_and_says_so():
    from algorithms._engine_core import sokal_window

    phi, L = 0.95, 32  # tau = 39: no window up to 32 can hold five of them
    rho = torch.tensor([[phi**k, 0.5**k] for k in range(L + 1)], dtype=torch.float64)
    tau, window, reached = sokal_window(rho, 5.0)
    assert reached.tolist() == [False, True]
    assert int(window[0]) == L
    exact = (1 + phi) / (1 - phi)
    assert float(tau[0]) == pytest.approx(exact - 2 * phi ** (L + 1) / (1 - phi), rel=1e-12)
    assert float(tau[0]) < exact  # a lower bound, flagged - never the answer
    assert float(tau[1]) == pytest.approx(3.0, abs=2 * 0.5 ** (int(window[1]) + 1) / 0.5)
    # the same sequence with room: reached
    rho = torch.tensor([[phi**k] for k in range(1025)], dtype=torch.float64)
    tau, window, reached = sokal_window(rho, 5.0)
    assert bool(reached[0]) and abs(float(tau[0]) - exact) <= 2 * phi ** (int(window[0]) + 1) / (1 - phi) + 2 * 1024 * 2.0 ** -53 * exact
    # NaN (nothing accumulated): not reached, tau NaN
    tau, _, reached = sokal_window(torch.full((9, 2), float("nan")), 5.0)
    assert torch.isnan(tau).all() and not reached.any()
    with pytest.raises(ValueError):
        sokal_window(torch.ones(1, 2))


def test_class_acf_checks_need_no_gpu():
    """What the classes and the run refuse before a device is asked for, and what they answer before anything has run."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import ACF_RING_LIMIT, EngineRun, check_acf_args
    from algorithms.sharding import allreduce_autocorr
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    for bad, msg in ((dict(acf="warm"), "'cold' or 'all'"), (dict(acf="cold", acf_every=0), "acf_every"),
                     (dict(acf="all", acf_max_lag=0), "acf_max_lag"), (dict(acf="all", acf_max_lag=1025), "acf_max_lag"),
                     (dict(acf="cold", acf_max_lag=2.5), "integer")):
        with pytest.raises(ValueError, match=msg):
            ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu", **bad)
        with pytest.raises(ValueError, match=msg):
            RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", **bad)
    # the ring's size: refused with the size named, overridable
    assert ACF_RING_LIMIT == 2**31
    assert check_acf_args(32, 100, 32, 32, 30, 65536) is True  # the headline shape, every temperature: 2.01e9 elements
    with pytest.raises(ValueError, match=r"64 x 65536 x 32 x 30 = 4026531840 elements \(15\.0 GiB"):
        check_acf_args(32, 1, 64, 32, 30, 65536)
    assert check_acf_args(32, 1, 64, 32, 30, 65536, ring_limit=2**33) is True
    with pytest.raises(ValueError, match="acf_ring_limit"):
        check_acf_args(1, 1, 8, 1, 3, 100, ring_limit=1000)
    assert check_acf_args(0, 0, 0, 4, 3, 1) is False  # off: nothing else is looked at
    with pytest.raises(ValueError, match="acf_temps"):
        EngineRun(target_dist=tgt, proposal=None, beta_ladder=[1.0, 0.5], dim=3, device=torch.device("cpu"), n_replicas=1,
                  initial_state=np.zeros(3, np.float32), burn_in=0, swap_every=1, swap_mode="exchange", swap_order="sequential",
                  seed=1, acf_temps=3)
    alg = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5, 0.1], device="cpu", acf="all", acf_every=5, acf_max_lag=8)
    assert alg.autocovariance(2).shape == (9, 3) and torch.isnan(alg.autocorrelation()).all()
    tau, window, reached = alg.integrated_autocorr_time()
    assert torch.isnan(tau).all() and not reached.any()
    info = alg.get_diagnostic_info()
    assert math.isnan(info["act_max"]) and info["act_window_reached"] is False
    with pytest.raises(ValueError, match="temperature"):
        alg.autocovariance(3)
    cold = RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", acf="cold")
    assert cold.autocovariance().shape == (33, 3)
    with pytest.raises(ValueError, match="temperature"):
        cold.ess_autocorr(temperature=1)
    off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu")
    with pytest.raises(RuntimeError, match="acf="):
        off.autocorrelation()
    assert "act_max" not in off.get_diagnostic_info()
    with pytest.raises(RuntimeError, match="autocovariance is off"):
        allreduce_autocorr(off)
    # the shards' all-reduce on a hand-made dict (single process, no process group: the job is this shard)
    a = {"sxy": torch.arange(12, dtype=torch.float64).view(1, 4, 3), "head": torch.ones(1, 4, 3, dtype=torch.float64),
         "tail": torch.full((1, 4, 3), 0.1, dtype=torch.float64), "pairs": torch.tensor([2**40 + 1, 3, 2, 1]), "every": 7}
    out = allreduce_autocorr(a)
    assert all(torch.equal(out[k], a[k]) and out[k] is not a[k] and out[k].dtype == a[k].dtype for k in ("sxy", "head", "tail", "pairs"))
    assert out["every"] == 7
