"""Pooled log-density sums along the ladder (include/ptrwm.h ptrwm_energy_args, csrc/energy.h) without a GPU: the kernel's tiling
replayed on the CPU against brute force and the launch cuts; the struct's C layout; every validation code of the two entry points
that returns before a HIP call; the three estimators on hand-made sums; allreduce_energy over a gloo world of two."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ptrwm_hip as E
from energy_reference import energy_reference, ref_of
from host_harness import assert_layout, c_layout, gloo_world, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def energy_exe(tmp_path_factory):
    """tests/energy_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    return sanitized_exe(tmp_path_factory.mktemp("energy"), "energy_test.cpp")


def test_tiling_replay_and_cuts_against_brute_force(energy_exe):
    """csrc/energy.h and the cut of csrc/schedule.h in tests/energy_test.cpp: one owner per (c, t), no pad lane, every chain in
    the group of its global id and equal integer sums, for every n_temps in 1..256 and 1, 3, 16 and 64 groups; the cuts with a
    covariance and a histogram at other periods."""
    run_exe(energy_exe, ok="energy ok:")


def test_gpu_cases_have_the_geometry_they_are_named_for(energy_exe):
    """The shapes of tests/test_gpu_energy.py through energy_geometry itself: a change of a tile constant of csrc/energy.h cannot
    quietly turn one case into another."""
    from test_gpu_energy import STANDALONE_CASES

    lines = "".join(f"{c['T']} {c['Cn']} {c['groups']} {c['offset']}\n" for c in STANDALONE_CASES)
    out = run_exe(energy_exe, "geometry", input=lines, timeout=60)
    keys = ("tile_chains", "tiles", "max_members", "min_members", "last_tile_chains", "lds_doubles", "threads", "tile_elems")
    geo = {c["name"]: dict(zip(keys, map(int, ln.split())), **c) for c, ln in zip(STANDALONE_CASES, out.splitlines())}
    assert len(geo) == len(STANDALONE_CASES) == 8
    # the issue's table, row by row (the last row's chain count is the builder's: see below)
    assert [(c["T"], c["Cn"], c["groups"], c["offset"]) for c in STANDALONE_CASES[:7]] == [
        (1, 300, 16, 0), (2, 3, 16, 0), (3, 70, 16, 5), (32, 70, 16, 0), (65, 40, 3, 1), (256, 19, 64, 7), (8, 1, 1, 0)]
    assert (STANDALONE_CASES[7]["T"], STANDALONE_CASES[7]["groups"], STANDALONE_CASES[7]["offset"]) == (4, 16, 0)
    g = geo["no_neighbours"]
    assert g["T"] == 1 and g["tiles"] == 1 and g["min_members"] >= 18
    g = geo["fewer_chains_than_groups"]
    assert g["Cn"] < g["groups"] and g["min_members"] == 0 and g["max_members"] == 1
    g = geo["odd_ladder_offset"]
    assert g["T"] % 2 == 1 and g["threads"] % g["T"] != 0 and g["offset"] % g["groups"] != 0 and g["min_members"] < g["max_members"]
    g = geo["headline_row"]
    assert g["T"] == 32 and g["threads"] % g["T"] == 0 and g["lds_doubles"] == 128
    g = geo["row_longer_than_a_wave"]
    assert g["T"] > 64 and g["threads"] % g["T"] != 0 and g["Cn"] % g["groups"] != 0 and g["T"] % g["groups"] != 0
    g = geo["longest_ladder"]
    assert g["T"] == E.MAX_TEMPS == 256 and g["groups"] == E.ENERGY_MAX_GROUPS == 64 and g["min_members"] == 0 and g["tile_chains"] == 16
    g = geo["one_chain_one_group"]
    assert g["Cn"] == g["groups"] == g["max_members"] == 1
    g = geo["second_tile"]  # at least two tiles per group, the last one partial
    assert g["tiles"] >= 2 and g["min_members"] > g["tile_chains"] and 0 < g["last_tile_chains"] < g["tile_chains"]
    assert g["min_members"] - (g["tiles"] - 1) * g["tile_chains"] < g["tile_chains"]


def test_launch_cuts_with_a_covariance_and_a_histogram_at_other_periods(energy_exe):
    """The launches of ptrwm_run_with_energy replayed step by step in Python: log-density sums every 7, covariance every 4,
    histogram every 5, burn_in 11."""
    step0, n, burn, ee, ce, he, cap = 3, 60, 11, 7, 4, 5, 1000
    out = run_exe(energy_exe, "cuts", step0, n, burn, ee, ce, he, cap, timeout=60)
    got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    want, start = [], step0
    for s in range(step0, step0 + n):  # step s has step counter s + 1
        sc = s + 1
        e, c, h = (sc > burn and sc % p == 0 for p in (ee, ce, he))
        if e or c or h or s == step0 + n - 1:
            want.append((start, s + 1 - start, int(e), int(c), int(h)))
            start = s + 1
    assert got == want and sum(c[2] for c in got) == 8  # step counters 14 .. 63
    assert any(c[2] and c[3] for c in got) and any(c[2] and c[4] for c in got)  # step counters 28 and 35: more kernels behind one launch
    # nothing else bound, nothing due: one launch
    assert run_exe(energy_exe, "cuts", 0, 10, 10, 3, 0, 0, 1000, timeout=60).split() == ["0", "10", "0", "0", "0"]


FIELDS = ["struct_size", "groups", "every", "ref", "ref_set", "count", "nonfinite", "s1", "s2", "colder", "hotter"]


def test_energy_struct_layout_matches_the_c_header(tmp_path):
    assert [f[0] for f in E.EnergyArgs._fields_] == FIELDS
    got = c_layout(tmp_path, {"ptrwm_energy_args": FIELDS}, macros=("PTRWM_ABI_VERSION", "PTRWM_ENERGY_MAX_GROUPS"))
    assert_layout(E.EnergyArgs, "ptrwm_energy_args", FIELDS, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays
    assert got["PTRWM_ENERGY_MAX_GROUPS"] == E.ENERGY_MAX_GROUPS == 64
    assert "ptrwm_energy" in E.SYMBOLS and "ptrwm_run_with_energy" in E.SYMBOLS
    assert E.RunPlan._RUN_WITH[-1] == "ptrwm_run_with_energy"


def _valid(n_temps=4):
    """Arguments both entry points accept up to their first HIP call, with every block that check_energy comes after, and the
    block itself: 16 groups, every step, every pointer at the harness's host buffer (a refused call never reads it)."""
    v = valid_args("cv", "ac", "hi", "ad", "ld", n_temps=n_temps)
    en = v["en"] = E.EnergyArgs()
    en.struct_size, en.groups, en.every = C.sizeof(E.EnergyArgs), 16, 1
    en.ref = en.ref_set = en.count = en.nonfinite = en.s1 = en.s2 = en.colder = en.hotter = v["ptr"]
    return v


def test_energy_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v, energy="en", hist=None, adapt=None, ladder=None, acf=None, cov=None):
        ref = lambda k: C.byref(v[k]) if k else None  # noqa: E731
        return lib.ptrwm_run_with_energy(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, ref(hist), ref(adapt),
                                         ref(ladder), ref(acf), ref(cov), ref(energy), None)

    def snap(v, energy="en"):
        return lib.ptrwm_energy(C.byref(v["ra"]), C.byref(v[energy]) if energy else None, None)

    for call in (run, snap):
        v = _valid()
        v["en"].struct_size = 4
        assert call(v) == -6, call.__name__  # PTRWM_E_STRUCT
        for field, bad in (("groups", 0), ("groups", 65), ("groups", -1), ("every", 0), ("every", -3)):
            v = _valid()
            setattr(v["en"], field, bad)
            assert call(v) == -5, (call.__name__, field, bad)  # PTRWM_E_ARG
        for field in ("ref", "ref_set", "count", "s1", "s2", "colder", "hotter"):
            v = _valid()
            setattr(v["en"], field, None)
            assert call(v) == -1, (call.__name__, field)  # PTRWM_E_NULL
        for groups in (1, 64):  # the limits themselves pass
            v = _valid()
            v["en"].groups = groups
            v["ra"].n_chains = 0
            assert call(v) == 0
        # nonfinite may be NULL; so may colder and hotter with one temperature, which has no neighbours
        v = _valid()
        v["en"].nonfinite = None
        v["ra"].n_chains = 0
        assert call(v) == 0
        v = _valid(n_temps=1)
        v["en"].colder = v["en"].hotter = None
        v["ra"].n_chains = 0
        assert call(v) == 0
        v = _valid(n_temps=2)
        v["en"].hotter = None
        v["ra"].n_chains = 0
        assert call(v) == -1
        # the order: struct size, then the arguments, then the pointers
        v = _valid()
        v["en"].struct_size, v["en"].every, v["en"].s1 = 4, 0, None
        assert call(v) == -6
        v = _valid()
        v["en"].every, v["en"].s1 = 0, None
        assert call(v) == -5
        # the entry point's own checks come first: the argument block's size, the ladder's length
        v = _valid()
        v["ra"].struct_size, v["en"].struct_size = 4, 4
        assert call(v) == -6
        v = _valid(n_temps=257)
        v["en"].s1 = None
        assert call(v) == -3
        # an empty batch with a valid block: nothing to do; with a bad block: still refused
        v = _valid()
        v["ra"].n_chains = 0
        assert call(v) == 0
        v["en"].every = 0
        assert call(v) == -5
    # ptrwm_energy alone: NULL arguments, the argument block's size, the ladder's length, the numbers it reads, the block, the
    # empty batch, a NULL logp or beta.  It takes no dim.
    v = _valid()
    assert snap(v, energy=None) == -1
    assert lib.ptrwm_energy(None, C.byref(v["en"]), None) == -1
    v = _valid(n_temps=0)
    assert snap(v) == -3
    for field in ("step0", "burn_in", "n_chains"):
        v = _valid()
        setattr(v["ra"], field, -1)
        v["en"].struct_size = 4
        assert snap(v) == -5, field
    for field in ("logp", "beta"):
        v = _valid()
        setattr(v["ra"], field, None)
        v["en"].every = 0
        assert snap(v) == -5, field
        v["en"].every = 1
        assert snap(v) == -1, field
        v["ra"].n_chains = 0
        assert snap(v) == 0, field  # (an empty batch never looks at them)
    # a step that is not due is known on the host: nothing is enqueued, so the fake pointers are never read
    v = _valid()
    v["ra"].step0, v["ra"].burn_in, v["en"].every = 4, 0, 10  # step counter 5
    assert snap(v) == 0
    v["ra"].step0, v["ra"].burn_in = 9, 10  # step counter 10, still in burn-in
    assert snap(v) == 0
    # ptrwm_run_with_energy: check_energy runs after EVERY other block's checks - the run's own arguments, the histogram's, the
    # scale tuning's, the ladder's, the autocovariance's, the covariance's - and before anything is enqueued
    v = _valid()
    v["ra"].swap_mode, v["en"].struct_size = 7, 4
    assert run(v) == -5
    v = _valid()
    v["hi"].n_bins, v["en"].struct_size = 0, 4
    assert run(v, hist="hi") == -5
    v = _valid()
    v["ad"].window_accept, v["en"].struct_size = None, 4
    assert run(v, adapt="ad") == -1
    v = _valid()
    v["ld"].probe_every, v["en"].s1 = 3, None  # (3 does not divide 10)
    assert run(v, ladder="ld") == -5
    v = _valid()
    v["ac"].max_lag, v["en"].struct_size = 0, 4
    assert run(v, acf="ac") == -5
    v = _valid()
    v["cv"].sxx, v["en"].every = None, 0
    assert run(v, cov="cv") == -1
    v = _valid()
    v["cv"].every, v["en"].s1 = 0, None
    assert run(v, cov="cv") == -5
    v = _valid()
    v["td"].dim, v["en"].s1 = 105, None
    assert run(v) == -2
    for field in ("logp", "beta"):  # (the run's own check)
        v = _valid()
        setattr(v["ra"], field, None)
        assert run(v) == -1, field
    # energy == NULL: ptrwm_run_with_covariance's codes
    v = _valid()
    v["ra"].state = None
    assert run(v, energy=None) == -1 == lib.ptrwm_run_with_covariance(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None,
                                                                      None, None, None, None, None, None)
    v = _valid()
    v["ra"].n_chains = 0
    assert run(v, energy=None) == 0
    # a request that passes every check goes on to the launch, which a machine without a GPU cannot make
    if not torch.cuda.is_available():
        v = _valid()
        assert run(v) == -7 and run(v, energy=None) == -7


# ---- the estimators on hand-made sums ------------------------------------------------------------------------------------------
def _hand_made(seed=3, groups=4, T=3, per_group=(5, 0, 7, 6)):
    """Sums of a few draws per group and rung (group 1 is empty), by energy_reference, under a level that is not zero."""
    rng = np.random.default_rng(seed)
    beta = np.array([1.0, 0.5, 0.125], dtype=np.float32)[:T]
    ref = np.array([-2.0, -3.5, -6.0])[:T]
    # one "snapshot" whose chains are laid out so that chain c sits in group c % groups: per_group[g] chains of group g
    chains = [g for g in range(groups) for _ in range(per_group[g])]
    order = sorted(range(len(chains)), key=lambda i: chains[i])
    logp = rng.normal(-4.0, 2.0, size=(len(chains), T)).astype(np.float32)
    sums = {k: np.zeros((groups, T)) for k in ("s1", "s2", "colder", "hotter")}
    count = np.zeros((groups, T), dtype=np.int64)
    for i in order:
        g = chains[i]
        one = energy_reference([logp[i:i + 1]], beta, 1, 0, ref)
        count[g] += one["count"][0]
        for k in sums:
            sums[k][g] += one[k][0]
    return {"count": count, **sums, "ref": ref, "beta": beta, "logp": logp, "chains": np.array(chains)}


def _loops(h, keep):
    """forward, reverse, trapezoid, corrected [T - 1] by explicit loops over the draws of the groups in `keep`."""
    beta, ref, T = h["beta"].astype(np.float64), h["ref"], h["beta"].shape[0]
    rows = [i for i, g in enumerate(h["chains"]) if g in keep]
    x = h["logp"][rows].astype(np.float64)
    E_, V_ = x.mean(0), (x * x).mean(0) - x.mean(0) ** 2
    fw, rv, tz, tc = [], [], [], []
    for t in range(1, T):
        c = sum(math.exp((beta[t - 1] - beta[t]) * (v - ref[t])) for v in x[:, t])
        hh = sum(math.exp((beta[t] - beta[t - 1]) * (v - ref[t - 1])) for v in x[:, t - 1])
        fw.append(math.log(c / len(rows)) + (beta[t - 1] - beta[t]) * ref[t])
        rv.append(-(math.log(hh / len(rows)) + (beta[t] - beta[t - 1]) * ref[t - 1]))
        d = beta[t - 1] - beta[t]
        tz.append(d * (E_[t - 1] + E_[t]) / 2)
        tc.append(tz[-1] - d * d * (V_[t - 1] - V_[t]) / 12)
    return {"forward": np.array(fw), "reverse": np.array(rv), "trapezoid": np.array(tz), "corrected": np.array(tc)}


def _delete_one(h, key, used):
    m = len(used)
    theta = np.stack([_loops(h, [g for g in used if g != out])[key] for out in used])
    return np.sqrt((m - 1) / m * ((theta - theta.mean(0)) ** 2).sum(0)), theta


def test_estimators_on_hand_made_sums():
    from algorithms._engine_core import energy_moments_from_sums, stepping_stones_from_sums, thermodynamic_integral_from_sums

    h = _hand_made()
    used = [0, 2, 3]  # group 1 is empty: it is left out
    full = _loops(h, used)
    x = h["logp"].astype(np.float64)
    mo = energy_moments_from_sums(h["count"], h["s1"], h["s2"], h["beta"])
    assert all(mo[k].dtype == torch.float64 and mo[k].shape == (3,) for k in ("mean", "variance", "heat_capacity"))
    assert mo["count"].tolist() == [18, 18, 18] and mo["count"].dtype == torch.int64
    assert np.allclose(mo["mean"].numpy(), x.mean(0), rtol=1e-13, atol=0)
    assert np.allclose(mo["variance"].numpy(), x.var(0), rtol=1e-11, atol=0)  # (divided by n)
    assert np.allclose(mo["heat_capacity"].numpy(), h["beta"].astype(np.float64) ** 2 * x.var(0), rtol=1e-11, atol=0)
    st = stepping_stones_from_sums(h["count"], h["colder"], h["hotter"], h["ref"], h["beta"])
    ti = thermodynamic_integral_from_sums(h["count"], h["s1"], h["s2"], h["beta"])
    for est, keys in ((st, ("forward", "reverse")), (ti, ("trapezoid", "corrected"))):
        for key in keys:
            assert est[key].dtype == torch.float64 and est[key].shape == (2,)
            assert np.allclose(est[key].numpy(), full[key], rtol=1e-12, atol=1e-13), key
            se, theta = _delete_one(h, key, used)  # the jackknife against an explicit delete-one recomputation
            assert np.allclose(est[key + "_se"].numpy(), se, rtol=1e-9, atol=1e-14), key
            assert (est[key + "_se"] > 0).all()
            assert est[key + "_total"] == pytest.approx(full[key].sum(), rel=1e-12)
            tot = theta.sum(1)
            assert est[key + "_total_se"] == pytest.approx(math.sqrt(2 / 3 * ((tot - tot.mean()) ** 2).sum()), rel=1e-9)
    assert st["overflow"] is False
    # the level does not matter: the same draws summed against another ref give the same estimates
    other = dict(h, ref=h["ref"] + np.array([1.5, -2.0, 0.25]))
    again = {k: np.zeros_like(h[k]) for k in ("colder", "hotter")}
    for i, g in enumerate(h["chains"]):
        one = energy_reference([h["logp"][i:i + 1]], h["beta"], 1, 0, other["ref"])
        for k in again:
            again[k][g] += one[k][0]
    st2 = stepping_stones_from_sums(h["count"], again["colder"], again["hotter"], other["ref"], h["beta"])
    assert np.allclose(st2["forward"].numpy(), st["forward"].numpy(), rtol=1e-12) and np.allclose(st2["reverse"].numpy(), st["reverse"].numpy(), rtol=1e-12)
    # fewer than two groups with draws: no error bar
    one_group = {k: (v[:1] if k in ("count", "s1", "s2", "colder", "hotter") else v) for k, v in h.items()}
    st1 = stepping_stones_from_sums(one_group["count"], one_group["colder"], one_group["hotter"], h["ref"], h["beta"])
    ti1 = thermodynamic_integral_from_sums(one_group["count"], one_group["s1"], one_group["s2"], h["beta"])
    assert np.allclose(st1["forward"].numpy(), _loops(h, [0])["forward"], rtol=1e-12) and torch.isnan(st1["forward_se"]).all()
    assert torch.isnan(st1["reverse_se"]).all() and math.isnan(st1["forward_total_se"])
    assert torch.isnan(ti1["trapezoid_se"]).all() and torch.isnan(ti1["corrected_se"]).all() and math.isnan(ti1["corrected_total_se"])
    two = {k: np.where(np.arange(4)[:, None] >= 2, 0, h[k]) for k in ("count", "s1", "s2", "colder", "hotter")}  # groups 0 and 1: one has draws
    assert torch.isnan(stepping_stones_from_sums(two["count"], two["colder"], two["hotter"], h["ref"], h["beta"])["forward_se"]).all()
    # an inf in an exponential sum surfaces as overflow
    c = h["colder"].copy()
    c[2, 1] = np.inf
    bad = stepping_stones_from_sums(h["count"], c, h["hotter"], h["ref"], h["beta"])
    assert bad["overflow"] is True and math.isinf(float(bad["forward"][0])) and math.isfinite(float(bad["forward"][1]))
    # nothing accumulated: NaN, not an exception
    z = np.zeros((4, 3))
    empty = stepping_stones_from_sums(z.astype(np.int64), z, z, np.zeros(3), h["beta"])
    assert torch.isnan(empty["forward"]).all() and torch.isnan(empty["forward_se"]).all() and empty["overflow"] is False
    assert torch.isnan(energy_moments_from_sums(z.astype(np.int64), z, z, h["beta"])["mean"]).all()
    # one temperature: only the moments mean something - empty ratio arrays
    h1 = _hand_made(T=1)
    st = stepping_stones_from_sums(h1["count"], h1["colder"], h1["hotter"], h1["ref"], h1["beta"])
    ti = thermodynamic_integral_from_sums(h1["count"], h1["s1"], h1["s2"], h1["beta"])
    assert st["forward"].shape == st["reverse"].shape == st["forward_se"].shape == (0,) and st["forward_total"] == 0.0
    assert ti["trapezoid"].shape == ti["corrected_se"].shape == (0,) and st["overflow"] is False
    assert energy_moments_from_sums(h1["count"], h1["s1"], h1["s2"], h1["beta"])["mean"].shape == (1,)


def test_class_energy_checks_need_no_gpu():
    """What the classes and the run refuse before a device is asked for, and what they answer before anything has run."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import EngineRun, check_energy_args
    from algorithms.sharding import allreduce_energy
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    for bad, msg in ((dict(energy="yes"), "True or False"), (dict(energy=True, energy_every=0), "energy_every"),
                     (dict(energy=True, energy_every=2.5), "integer"), (dict(energy=True, energy_groups=0), "energy_groups"),
                     (dict(energy=True, energy_groups=65), "energy_groups"), (dict(energy=True, energy_groups=True), "integer"),
                     (dict(energy=True, energy_ref="high"), "energy_ref"), (dict(energy=True, energy_ref=float("nan")), "finite"),
                     (dict(energy=True, energy_ref=np.zeros((2, 2))), "energy_ref"), (dict(energy_ref=1.0), "energy=True")):
        with pytest.raises(ValueError, match=msg):
            ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu", **bad)
        with pytest.raises(ValueError, match=msg):
            RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", **bad)
    assert check_energy_args(False) is None
    got = check_energy_args(True, 10, 16, -5.0, n_temps=3)
    assert got["every"] == 10 and got["groups"] == 16 and got["ref"].tolist() == [-5.0] * 3 and got["ref"].dtype == np.float64
    assert check_energy_args(True, 1, 64, [1.0, 2.0], n_temps=2)["ref"].tolist() == [1.0, 2.0]
    assert check_energy_args(True)["ref"] is None
    with pytest.raises(ValueError, match="n_temps"):
        check_energy_args(True, 1, 16, [1.0, 2.0, 3.0], n_temps=2)
    with pytest.raises(ValueError, match="n_temps"):  # a vector of the wrong length, caught by the run before the device is asked for
        EngineRun(target_dist=tgt, proposal=None, beta_ladder=[1.0, 0.5], dim=3, device=torch.device("cpu"), n_replicas=1,
                  initial_state=np.zeros(3, np.float32), burn_in=0, swap_every=1, swap_mode="exchange", swap_order="sequential",
                  seed=1, energy=True, energy_ref=[1.0, 2.0, 3.0])
    alg = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5, 0.1], device="cpu", energy=True, energy_every=5)
    assert alg.energy_count.tolist() == [0, 0, 0]
    assert alg.mean_energy().shape == (3,) and torch.isnan(alg.mean_energy()).all() and torch.isnan(alg.heat_capacity()).all()
    for method in ("forward", "reverse", "thermodynamic", "thermodynamic_corrected"):
        v, se = alg.log_normalizer_ratios(method)
        assert v.shape == se.shape == (2,) and torch.isnan(v).all() and torch.isnan(se).all()
        total, tse = alg.log_normalizer_ratio(method)
        assert math.isnan(total) and math.isnan(tse)
    with pytest.raises(ValueError, match="method"):
        alg.log_normalizer_ratios("bennett")
    info = alg.get_diagnostic_info()
    assert math.isnan(info["log_z_ratio_forward"]) and math.isnan(info["log_z_ratio_reverse"]) and math.isnan(info["log_z_ratio_se"])
    assert info["energy_nonfinite"] == 0 and info["energy_overflow"] is False
    one = RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", energy=True, energy_groups=4)
    assert one.energy_variance().shape == (1,) and one.log_normalizer_ratios()[0].shape == (0,) and one.energy_count.tolist() == [0]
    off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu")
    for read in (off.mean_energy, off.energy_variance, off.heat_capacity, off.log_normalizer_ratios, off.log_normalizer_ratio,
                 lambda: off.energy_count):
        with pytest.raises(RuntimeError, match="energy=True"):
            read()
    assert not any(k.startswith(("log_z", "energy_")) for k in off.get_diagnostic_info())
    with pytest.raises(RuntimeError, match="sums are off"):
        allreduce_energy(off)


# ---- allreduce_energy over two ranks ---------------------------------------------------------------------------------------------
GROUPS, OFFSETS, CHAINS = 4, (0, 5), (5, 6)
BETA = np.array([1.0, 0.5, 0.2], dtype=np.float32)


def _job():
    """Two snapshots of the whole job's log-densities [11, 3], far from zero so that the level matters."""
    rng = np.random.default_rng(77)
    return [(-1.0e6 + rng.normal(0.0, 3.0, size=(11, 3))).astype(np.float32) for _ in range(2)]


def _shard(rank):
    lo, n = OFFSETS[rank], CHAINS[rank]
    snaps = [s[lo:lo + n] for s in _job()]
    ref = ref_of(snaps[0])  # the automatic level: this shard's own maxima at its first snapshot
    r = energy_reference(snaps, BETA, GROUPS, lo, ref)
    return {"count": torch.from_numpy(r["count"]), "nonfinite": torch.tensor([r["nonfinite"]]),
            **{k: torch.from_numpy(r[k]) for k in ("s1", "s2", "colder", "hotter")}, "ref": torch.from_numpy(ref),
            "ref_set": torch.ones(1, dtype=torch.int32), "beta": torch.from_numpy(BETA), "every": 7, "pinned": False}


def _worker(rank):
    from algorithms.sharding import allreduce_energy

    shard = _shard(rank)
    kept = {k: v.clone() for k, v in shard.items() if torch.is_tensor(v)}
    total = allreduce_energy(shard)
    assert all(torch.equal(shard[k], v) for k, v in kept.items())  # inputs untouched
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in total.items()}


def test_allreduce_energy_over_two_ranks_is_the_sums_of_the_whole_job_under_the_common_level():
    from algorithms.sharding import allreduce_energy, energy_rescale

    a, b = _shard(0), _shard(1)
    assert not torch.equal(a["ref"], b["ref"])  # the two shards chose different levels
    common = torch.maximum(a["ref"], b["ref"])
    want = energy_reference(_job(), BETA, GROUPS, 0, common.numpy())  # the joined data under the common level
    for _, total in gloo_world(_worker):
        assert np.array_equal(total["ref"], common.numpy()) and total["every"] == 7
        assert np.array_equal(total["count"], want["count"]) and total["count"].dtype == np.int64 and total["nonfinite"].tolist() == [0]
        for k in ("s1", "s2", "colder", "hotter"):
            # (two rescales and one addition more than the reference's one rounding: a few ulp of sums of positive terms)
            assert np.allclose(total[k], want[k], rtol=1e-13, atol=0), k
        assert (total["colder"][:, 1:] > 0).all() and np.isfinite(total["colder"]).all() and np.isfinite(total["hotter"]).all()
    # a pinned level shared by both shards: the rescale is the identity, bit for bit
    same = energy_rescale(a, a["ref"])
    assert all(torch.equal(same[k], a[k]) for k in ("count", "s1", "s2", "colder", "hotter", "ref"))
    # a shard that has not chosen a level yet stands aside in the MAX; no process group: the identity
    out = allreduce_energy(a)
    assert all(torch.equal(out[k], a[k]) for k in ("count", "s1", "s2", "colder", "hotter", "ref")) and out["colder"] is not a["colder"]
    fresh = dict(a, ref=torch.zeros(3, dtype=torch.float64), ref_set=torch.zeros(1, dtype=torch.int32),
                 **{k: torch.zeros_like(a[k]) for k in ("count", "s1", "s2", "colder", "hotter")})
    out = allreduce_energy(fresh)
    assert out["ref"].tolist() == [0.0, 0.0, 0.0] and float(out["colder"].abs().sum()) == 0.0
