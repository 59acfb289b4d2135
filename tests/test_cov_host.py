"""Pooled posterior covariance (include/ptrwm.h ptrwm_cov_args, csrc/cov.h) without a GPU: the kernel's geometry, a CPU replay
of its staging, block products and flush, and the launch cuts against brute force; the struct's C layout; every validation code
of the two entry points that returns before a HIP call; the estimators on hand-made sums; allreduce_covariance over a gloo world
of two."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ptrwm_hip as E
from host_harness import assert_layout, c_layout, gloo_world, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def cov_exe(tmp_path_factory):
    """tests/cov_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    return sanitized_exe(tmp_path_factory.mktemp("cov"), "cov_test.cpp")


def test_geometry_replay_and_cuts_against_brute_force(cov_exe):
    """csrc/cov.h and the cut of csrc/schedule.h in tests/cov_test.cpp: one owner per (i, j), j <= i < dim, and no pad element
    flushed, for every dim in 1..104; the CPU replay of the kernel on integer states; the cuts with a histogram and an
    autocovariance at other periods."""
    run_exe(cov_exe, ok="cov ok:")


def test_gpu_cases_have_the_geometry_they_are_named_for(cov_exe):
    """The shapes of tests/test_gpu_cov.py through cov_geometry itself: a change of a tile constant of csrc/cov.h cannot quietly
    turn one case into another."""
    from test_gpu_cov import EQUALITY_CASES

    lines = "".join(f"{c['dim']}\n" for c in EQUALITY_CASES)
    out = run_exe(cov_exe, "geometry", input=lines, timeout=60)
    keys = ("blocks", "pairs", "stride", "lds_bytes", "chains", "sub_tile", "k", "waves")
    geo = {c["name"]: dict(zip(keys, map(int, ln.split())), **c) for c, ln in zip(EQUALITY_CASES, out.splitlines())}
    assert len(geo) == len(EQUALITY_CASES) == 9
    # the issue's table, row by row
    assert [(c["dim"], c["T"], c["temps"], c["Cn"]) for c in EQUALITY_CASES[:8]] == [
        (1, 1, 1, 300), (5, 1, 1, 3), (16, 4, 2, 70), (17, 4, 4, 70), (30, 32, 32, 70), (64, 4, 4, 70), (70, 8, 8, 40), (104, 2, 2, 40)]
    g = geo["one_block"]
    assert g["blocks"] == 1 and 16 * g["blocks"] - g["dim"] == 15 and g["Cn"] > g["chains"]  # 15 pad columns (and a second tile)
    g = geo["below_k"]
    assert g["Cn"] < g["k"] and g["blocks"] == 1
    g = geo["exact_block"]
    assert g["dim"] == 16 * g["blocks"] and g["blocks"] == 1 and g["temps"] < g["T"] and g["Cn"] % g["k"] != 0 and g["Cn"] < g["chains"]
    assert g["Cn"] % g["sub_tile"] != 0  # (a partial sub-tile too: rows past the last chain)
    g = geo["second_block"]
    assert g["blocks"] == 2 and g["dim"] - 16 == 1 and g["pairs"] == 3
    g = geo["headline_row"]
    assert g["dim"] == 30 and g["T"] == g["temps"] == 32 and g["pairs"] == 3 and g["pairs"] < g["waves"]
    g = geo["ten_pairs"]
    assert g["pairs"] == 10 and g["dim"] == 16 * g["blocks"]
    g = geo["pairs_over_waves"]
    assert g["pairs"] == 15 > g["waves"]
    g = geo["largest_dim"]
    assert g["dim"] == E.MAX_DIM == 104 and g["pairs"] == 28 and g["lds_bytes"] <= 64 * 1024
    g = geo["second_tile"]  # a second tile of chains, itself partial: one full sub-tile and three chains of another
    assert g["chains"] < g["Cn"] < 2 * g["chains"] and g["Cn"] == g["chains"] + g["sub_tile"] + 3 and (g["Cn"] - g["chains"]) % g["k"] != 0


def test_launch_cuts_with_a_histogram_and_an_autocovariance_at_other_periods(cov_exe):
    """The launches of ptrwm_run_with_covariance replayed step by step in Python: covariance every 7, autocovariance every 4,
    histogram every 5, burn_in 11."""
    step0, n, burn, ce, ae, he, cap = 3, 60, 11, 7, 4, 5, 1000
    out = run_exe(cov_exe, "cuts", step0, n, burn, ce, ae, he, cap, timeout=60)
    got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    want, start = [], step0
    for s in range(step0, step0 + n):  # step s has step counter s + 1
        sc = s + 1
        c, a, h = (sc > burn and sc % e == 0 for e in (ce, ae, he))
        if c or a or h or s == step0 + n - 1:
            want.append((start, s + 1 - start, int(c), int(a), int(h)))
            start = s + 1
    assert got == want and sum(c[2] for c in got) == 8  # step counters 14 .. 63
    assert any(c[2] and c[3] for c in got) and any(c[2] and c[4] for c in got)  # step counters 28 and 35: two kernels behind one launch
    # nothing else bound, nothing due: one launch
    assert run_exe(cov_exe, "cuts", 0, 10, 10, 3, 0, 0, 1000, timeout=60).split() == ["0", "10", "0", "0", "0"]


def test_cov_struct_layout_matches_the_c_header(tmp_path):
    fields = [f[0] for f in E.CovArgs._fields_]
    assert fields == ["struct_size", "temps", "every", "sxx", "sx", "count"]
    got = c_layout(tmp_path, {"ptrwm_cov_args": fields}, macros=("PTRWM_ABI_VERSION",))
    assert_layout(E.CovArgs, "ptrwm_cov_args", fields, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays
    assert "ptrwm_covariance" in E.SYMBOLS and "ptrwm_run_with_covariance" in E.SYMBOLS


def _valid(n_temps=4):
    """Arguments both entry points accept up to their first HIP call, with every block that check_cov comes after."""
    return valid_args("cv", "ac", "hi", "ad", "ld", n_temps=n_temps)  # ld.every == 10: "3 does not divide 10" below


def test_cov_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v, cov="cv", hist=None, adapt=None, ladder=None, acf=None):
        ref = lambda k: C.byref(v[k]) if k else None  # noqa: E731
        return lib.ptrwm_run_with_covariance(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, ref(hist), ref(adapt),
                                             ref(ladder), ref(acf), ref(cov), None)

    def snap(v, cov="cv", dim=30):
        return lib.ptrwm_covariance(C.byref(v["ra"]), dim, C.byref(v[cov]) if cov else None, None)

    for call in (run, snap):
        v = _valid()
        v["cv"].struct_size = 4
        assert call(v) == -6, call.__name__  # PTRWM_E_STRUCT
        for field, bad in (("temps", 0), ("temps", 5), ("every", 0), ("every", -3)):
            v = _valid()
            setattr(v["cv"], field, bad)
            assert call(v) == -5, (call.__name__, field, bad)  # PTRWM_E_ARG
        for field in ("sxx", "sx", "count"):
            v = _valid()
            setattr(v["cv"], field, None)
            assert call(v) == -1, (call.__name__, field)  # PTRWM_E_NULL
        v = _valid()
        v["cv"].temps = 4  # the limit itself passes
        v["ra"].n_chains = 0
        assert call(v) == 0
        # the order: struct size, then the arguments, then the pointers
        v = _valid()
        v["cv"].struct_size, v["cv"].every, v["cv"].sxx = 4, 0, None
        assert call(v) == -6
        v = _valid()
        v["cv"].every, v["cv"].sxx = 0, None
        assert call(v) == -5
        # the entry point's own checks come first: the argument block's size, the ladder's length
        v = _valid()
        v["ra"].struct_size, v["cv"].struct_size = 4, 4
        assert call(v) == -6
        v = _valid(n_temps=257)
        v["cv"].sxx = None
        assert call(v) == -3
        # an empty batch with a valid block: nothing to do; with a bad block: still refused
        v = _valid()
        v["ra"].n_chains = 0
        assert call(v) == 0
        v["cv"].every = 0
        assert call(v) == -5
    # ptrwm_covariance alone, in ptrwm_autocorr's order: NULL arguments, the argument block's size, dim, the ladder's length, the
    # flags it reads, the block, the empty batch, a NULL state
    v = _valid()
    assert snap(v, cov=None) == -1
    assert lib.ptrwm_covariance(None, 30, C.byref(v["cv"]), None) == -1
    assert snap(v, dim=0) == -2 and snap(v, dim=105) == -2
    v["ra"].struct_size = 4
    assert snap(v, dim=0) == -6
    v = _valid(n_temps=0)
    assert snap(v, dim=105) == -2 and snap(v) == -3
    v = _valid()
    v["ra"].state_f64 = 2
    assert snap(v) == -5
    v = _valid(n_temps=257)
    v["ra"].state_f64 = 2
    assert snap(v) == -3
    for field in ("step0", "burn_in", "n_chains"):
        v = _valid()
        setattr(v["ra"], field, -1)
        v["cv"].struct_size = 4
        assert snap(v) == -5, field
    v = _valid()
    v["ra"].state, v["cv"].every = None, 0
    assert snap(v) == -5
    v["cv"].every = 1
    assert snap(v) == -1
    v["ra"].n_chains = 0
    assert snap(v) == 0  # (an empty batch never looks at the state)
    # a step that is not due is known on the host: nothing is enqueued, so the fake pointers are never read
    v = _valid()
    v["ra"].step0, v["ra"].burn_in, v["cv"].every = 4, 0, 10  # step counter 5
    assert snap(v) == 0
    v["ra"].step0, v["ra"].burn_in = 9, 10  # step counter 10, still in burn-in
    assert snap(v) == 0
    # ptrwm_run_with_covariance: check_cov runs after EVERY other block's checks - the run's own arguments, the histogram's, the
    # scale tuning's, the ladder's, the autocovariance's - and before anything is enqueued
    v = _valid()
    v["ra"].swap_mode, v["cv"].struct_size = 7, 4
    assert run(v) == -5
    v = _valid()
    v["hi"].n_bins, v["cv"].struct_size = 0, 4
    assert run(v, hist="hi") == -5
    v = _valid()
    v["ad"].window_accept, v["cv"].struct_size = None, 4
    assert run(v, adapt="ad") == -1
    v = _valid()
    v["ld"].probe_every, v["cv"].sxx = 3, None  # (3 does not divide 10)
    assert run(v, ladder="ld") == -5
    v = _valid()
    v["ac"].max_lag, v["cv"].struct_size = 0, 4
    assert run(v, acf="ac") == -5
    v = _valid()
    v["ac"].ring, v["cv"].every = None, 0
    assert run(v, acf="ac") == -1
    v = _valid()
    v["td"].dim, v["cv"].sxx = 105, None
    assert run(v) == -2
    # cov == NULL: ptrwm_run_with_autocorr's codes
    v = _valid()
    v["ra"].state = None
    assert run(v, cov=None) == -1 == lib.ptrwm_run_with_autocorr(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, None,
                                                                 None, None, None, None)
    v = _valid()
    v["ra"].n_chains = 0
    assert run(v, cov=None) == 0
    # a request that passes every check goes on to the launch, which a machine without a GPU cannot make
    if not torch.cuda.is_available():
        v = _valid()
        assert run(v) == -7 and run(v, cov=None) == -7


def test_estimators_on_hand_made_sums():
    from algorithms._engine_core import cov_condition, cov_correlation, cov_covariance, cov_principal_axes

    # four draws of three coordinates: x = (1, 2, 3, 4), y = 2 x - 1 = (1, 3, 5, 7), z = 2 throughout.  var x = 1.25, var y = 5,
    # cov(x, y) = 2.5, z constant.  The strict upper triangle of sxx holds rubbish: it is never read.
    x, y, z = np.array([1.0, 2, 3, 4]), np.array([1.0, 3, 5, 7]), np.full(4, 2.0)
    d = np.stack([x, y, z], 1)
    sxx = np.tril(d.T @ d) + np.triu(np.full((3, 3), 777.0), 1)
    c = cov_covariance(torch.tensor(sxx), torch.tensor(d.sum(0)), torch.tensor([4]))
    assert c.dtype == torch.float64 and c.shape == (3, 3)
    assert c.tolist() == [[1.25, 2.5, 0.0], [2.5, 5.0, 0.0], [0.0, 0.0, 0.0]]
    assert torch.equal(c, c.T)
    r = cov_correlation(c)
    assert r[0, 1].item() == pytest.approx(1.0) and r[1, 0].item() == r[0, 1].item() and torch.diagonal(r).tolist() == [1.0, 1.0, 1.0]
    assert torch.isnan(r[2, :2]).all() and torch.isnan(r[:2, 2]).all()  # a coordinate of zero variance: NaN off its diagonal
    assert torch.isnan(cov_covariance(torch.zeros(3, 3), torch.zeros(3), torch.tensor([0]))).all()  # nothing accumulated
    with pytest.raises(ValueError, match="dim, dim"):
        cov_covariance(torch.zeros(3, 2), torch.zeros(3), 4)
    # principal axes of a known 3 x 3: eigenvalues 4, 2, 1 - (1, 1, 0) / sqrt 2, (1, -1, 0) / sqrt 2 and (0, 0, 1)
    m = torch.tensor([[3.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    w, v = cov_principal_axes(m)
    assert w.dtype == torch.float64 and w.tolist() == pytest.approx([4.0, 2.0, 1.0])
    h = 1 / math.sqrt(2)
    for col, want in enumerate(([h, h, 0.0], [h, -h, 0.0], [0.0, 0.0, 1.0])):  # (columns; the sign is free)
        assert abs(float(v[:, col] @ torch.tensor(want, dtype=torch.float64))) == pytest.approx(1.0, abs=1e-12), col
    assert torch.allclose(v @ torch.diag(w) @ v.T, m, atol=1e-12)
    assert cov_condition(m) == pytest.approx(4.0)
    assert cov_condition(c) == float("inf")  # the smallest eigenvalue is <= 0 (y = 2 x - 1, z constant)
    assert math.isnan(cov_condition(torch.full((2, 2), float("nan"))))


def test_class_cov_checks_need_no_gpu():
    """What the classes and the run refuse before a device is asked for, and what they answer before anything has run."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import EngineRun, check_cov_args
    from algorithms.sharding import allreduce_covariance
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    for bad, msg in ((dict(cov="warm"), "'cold' or 'all'"), (dict(cov="cold", cov_every=0), "cov_every"),
                     (dict(cov="all", cov_every=2.5), "integer"), (dict(cov="all", cov_every=True), "integer")):
        with pytest.raises(ValueError, match=msg):
            ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu", **bad)
        with pytest.raises(ValueError, match=msg):
            RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", **bad)
    assert check_cov_args(32, 100, 32) is True
    assert check_cov_args(0, 0, 4) is False  # off: nothing else is looked at
    with pytest.raises(ValueError, match="cov_temps"):
        EngineRun(target_dist=tgt, proposal=None, beta_ladder=[1.0, 0.5], dim=3, device=torch.device("cpu"), n_replicas=1,
                  initial_state=np.zeros(3, np.float32), burn_in=0, swap_every=1, swap_mode="exchange", swap_order="sequential",
                  seed=1, cov_temps=3)
    alg = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5, 0.1], device="cpu", cov="all", cov_every=5)
    assert alg.covariance_count == 0
    assert alg.posterior_covariance(2).shape == (3, 3) and torch.isnan(alg.posterior_covariance()).all()  # empty sums
    assert torch.isnan(alg.posterior_correlation()[0, 1])
    info = alg.get_diagnostic_info()
    assert math.isnan(info["cov_condition"]) and info["cov_count"] == 0
    with pytest.raises(ValueError, match="temperature"):
        alg.posterior_covariance(3)
    cold = RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", cov="cold")
    assert cold.posterior_covariance().shape == (3, 3) and cold.covariance_count == 0
    with pytest.raises(ValueError, match="temperature"):
        cold.principal_axes(temperature=1)
    off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu")
    for read in (off.posterior_covariance, off.posterior_correlation, off.principal_axes, lambda: off.covariance_count):
        with pytest.raises(RuntimeError, match="cov="):
            read()
    assert "cov_condition" not in off.get_diagnostic_info() and "cov_count" not in off.get_diagnostic_info()
    with pytest.raises(RuntimeError, match="covariance is off"):
        allreduce_covariance(off)


TEMPS, DIM = 2, 3


def _shard(rank):
    g = torch.Generator().manual_seed(100 + rank)
    x = torch.randn(5 + rank, TEMPS, DIM, generator=g, dtype=torch.float64)
    sxx = torch.tril(torch.einsum("cti,ctj->tij", x, x)) + torch.triu(torch.full((DIM, DIM), 7.0, dtype=torch.float64), 1)
    return {"sxx": sxx, "sx": x.sum(0), "count": torch.tensor([5 + rank]), "every": 5, "x": x}


def _worker(rank):
    from algorithms.sharding import allreduce_covariance

    shard = _shard(rank)
    shard.pop("x")
    kept = {k: v.clone() for k, v in shard.items() if torch.is_tensor(v)}
    total = allreduce_covariance(shard)
    assert all(torch.equal(shard[k], v) for k, v in kept.items())  # inputs untouched
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in total.items()}


def test_allreduce_covariance_over_two_ranks_is_the_covariance_of_the_whole_job():
    from algorithms.sharding import allreduce_covariance

    got = gloo_world(_worker)
    a, b = _shard(0), _shard(1)
    x = torch.cat([a["x"], b["x"]]).numpy()  # the whole job's draws
    for _, total in got:
        for k in ("sxx", "sx"):
            assert torch.allclose(torch.from_numpy(total[k]), a[k] + b[k], rtol=0, atol=1e-14)
        assert total["count"].tolist() == [11] and total["count"].dtype == np.int64 and total["every"] == 5
        assert total["covariance"].shape == (TEMPS, DIM, DIM)
        for t in range(TEMPS):
            assert np.allclose(total["covariance"][t], np.cov(x[:, t].T, bias=True), rtol=0, atol=1e-12)
    # no process group: the identity
    one = {k: v for k, v in a.items() if k != "x"}
    out = allreduce_covariance(one)
    assert torch.equal(out["sxx"], a["sxx"]) and torch.equal(out["count"], a["count"]) and out["sxx"] is not a["sxx"]
