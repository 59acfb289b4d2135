"""Replica flow (include/ptrwm.h ptrwm_flow_args, csrc/flow.h) without a GPU: the rule's header against a literal
restatement, the struct's C layout, every validation code of the three entry points that returns before a HIP call, and the
arithmetic of the class accessors and of the shards' all-reduce on hand-made tensors."""
import ctypes as C
import math

import pytest
import torch

import ptrwm_hip as E
from host_harness import assert_layout, c_layout, gloo_world, run_exe, sanitized_exe, valid_args


def test_flow_header_against_a_literal_restatement(tmp_path):
    """csrc/flow.h compiled as plain C++ under AddressSanitizer and UBSan into tests/flow_test.cpp, a program of its own:
    random accept patterns for T in {2, 3, 5, 8, 64, 70, 256}, both modes and both orders; flow words moved through src[t] as
    the kernels move them against explicit id / direction arrays and sequential transpositions or copies, after every event."""
    run_exe(sanitized_exe(tmp_path, "flow_test.cpp"),
            ok="flow ok: 62400 events, 7 ladder lengths x 2 modes x 2 orders x 3 acceptance rates")


def test_flow_struct_layout_matches_the_c_header(tmp_path):
    fields = [f[0] for f in E.FlowArgs._fields_]
    assert fields == ["struct_size", "reserved", "walker", "round_trips", "n_up", "n_down"]
    got = c_layout(tmp_path, {"ptrwm_flow_args": fields}, macros=("PTRWM_ABI_VERSION",))
    assert_layout(E.FlowArgs, "ptrwm_flow_args", fields, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays


def _valid(n_temps=4):
    """Arguments every entry point accepts up to its first HIP call, with both accumulators, whose checks come before flow's."""
    return valid_args("fl", "mom", "cmom", n_temps=n_temps)


def test_flow_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v, mom=None, cmom=None, flow="fl"):
        return lib.ptrwm_run_with_diagnostics(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]),
                                              C.byref(v[mom]) if mom else None, C.byref(v[cmom]) if cmom else None,
                                              C.byref(v[flow]) if flow else None, None)

    def sweep(v, flow="fl", dim=30):
        return lib.ptrwm_swap_sweep_with_flow(C.byref(v["ra"]), dim, 0, 1, C.byref(v[flow]) if flow else None, None)

    def accept(v, flow="fl", dim=30):
        p = v["ptr"]
        return lib.ptrwm_split_accept_with_flow(C.byref(v["ra"]), dim, p, p, p, C.byref(v[flow]) if flow else None, None)

    for call in (run, sweep, accept):
        v = _valid()
        v["fl"].struct_size = 4
        assert call(v) == -6, call.__name__  # PTRWM_E_STRUCT
        v = _valid()
        v["fl"].walker = None
        assert call(v) == -1, call.__name__  # PTRWM_E_NULL
        v = _valid()
        v["fl"].reserved = 1
        assert call(v) == -5, call.__name__  # PTRWM_E_ARG
        v = _valid(n_temps=1)
        assert call(v) == -5, call.__name__  # a ladder of one temperature has no flow
        # the struct size is looked at first, then the walker, then the arguments
        v = _valid(n_temps=1)
        v["fl"].struct_size, v["fl"].walker = 4, None
        assert call(v) == -6
        v = _valid(n_temps=1)
        v["fl"].walker = None
        assert call(v) == -1
        # the entry point's own checks come first: the argument block's size, the ladder's length
        v = _valid()
        v["ra"].struct_size, v["fl"].struct_size = 4, 4
        assert call(v) == -6
        v = _valid(n_temps=257)
        v["fl"].walker = None
        assert call(v) == -3
        # ptrwm_run looks at its diagnostics before its remaining arguments (as it does for the moments), the other two after
        v = _valid()
        v["ra"].swap_mode, v["fl"].walker = 7, None
        assert call(v) == (-1 if call is run else -5)
        # an empty batch with valid flow: nothing to do; with a bad flow block: still refused
        v = _valid()
        v["ra"].n_chains = 0
        assert call(v) == 0
        v["fl"].reserved = 2
        assert call(v) == -5
    # ptrwm_run_with_diagnostics: at most one accumulator; its checks come before flow's
    v = _valid()
    assert run(v, mom="mom", cmom="cmom") == -5
    assert run(v, mom="mom", cmom="cmom", flow=None) == -5
    v["mom"].struct_size, v["fl"].walker = 4, None
    assert run(v, mom="mom") == -6
    v = _valid()
    v["cmom"].temps, v["fl"].struct_size = 9, 4
    assert run(v, cmom="cmom") == -5
    v = _valid(n_temps=257)
    assert run(v) == -3 and sweep(v) == -3 and accept(v) == -3
    v = _valid()
    assert sweep(v, dim=105) == -2 and accept(v, dim=105) == -2
    v["td"].dim = 105
    assert run(v) == -2
    # flow == NULL: the existing entry points' codes (tests/test_capi_library.py TWO_DEFECT_CODES)
    v = _valid()
    v["ra"].n_temps, v["ra"].state_f64 = 257, 2
    assert run(v, flow=None) == -3 and sweep(v, flow=None) == -5 and accept(v, flow=None) == -5
    v = _valid()
    v["ra"].state = None
    assert run(v, flow=None) == -1 and sweep(v, flow=None) == -1 and accept(v, flow=None) == -1
    # the LDS budget, refused before anything is enqueued: per-chain moments of every temperature that fill the workgroup's
    # 160 KiB to the last byte (include/ptrwm.h: RWM-like shape, here 2 temperatures x 32 ladders per wave, dim 30) leave no
    # room for the flow regions; the same request without flow passes this check and goes on to the launch, which a machine
    # without a GPU cannot make (PTRWM_E_LAUNCH or, with one, success - never PTRWM_E_ARG)
    prev = E.set_kernel_form(E.FORM_THREAD)
    try:
        v = _valid(n_temps=2)
        v["ra"].n_chains = 0  # (validated, nothing enqueued)
        v["cmom"].temps = 2
        assert run(v, cmom="cmom") == 0
        v["ra"].n_chains = 64
        # thread form: 38 912 bytes + 4 waves x 32 ladders x 2 temps x 61 doubles x 8 = 38 912 + 124 928 = 163 840 = 160 KiB
        assert run(v, cmom="cmom") == -5  # + 4 096 bytes of flow regions: does not fit
        # the controls - that this -5 is the budget and nothing else - are requests that PASS every check and go on to the
        # launch.  Their pointers are fakes, so they are made only where no launch can happen: without a device the first HIP
        # call fails and the entry point says PTRWM_E_LAUNCH, which it can only say once every argument check lies behind it
        if not torch.cuda.is_available():
            assert run(v, cmom="cmom", flow=None) == -7  # the same request without flow: exactly 160 KiB, fits
            v["cmom"].temps = 1
            assert run(v, cmom="cmom") == -7  # with flow, one moments temperature less: 38 912 + 62 464 + 4 096 bytes, fits
    finally:
        E.set_kernel_form(prev)


def test_up_fraction_round_trip_rate_and_allreduce_on_hand_made_tensors():
    from algorithms.sharding import allreduce_flow, flow_round_trip_rate, flow_up_fraction

    n_up = torch.tensor([[5, 3, 0, 0], [5, 1, 2, 0]])
    n_down = torch.tensor([[0, 1, 0, 5], [0, 3, 0, 5]])
    f = flow_up_fraction(n_up.sum(0), n_down.sum(0))
    assert f.dtype == torch.float64 and f.shape == (4,)
    assert f[0] == 1.0 and f[3] == 0.0 and f[1] == 0.5 and f[2] == 1.0
    f = flow_up_fraction(torch.tensor([5, 0]), torch.tensor([0, 0]))
    assert f[0] == 1.0 and math.isnan(f[1])  # nothing has visited: NaN, not 0
    assert flow_round_trip_rate(6, 2, 4, 5) == 6 / 40
    assert flow_round_trip_rate(0, 2, 4, 0) == 0.0
    trips = torch.tensor([[1, 0, 2, 0], [0, 3, 0, 0]])
    out = allreduce_flow({"walker": torch.zeros(2, 4, dtype=torch.int32), "round_trips": trips, "n_up": n_up, "n_down": n_down,
                          "events": 5})  # single process, no process group: the job is this shard
    assert out["round_trips_total"] == 6 and out["n_replicas"] == 2 and out["events"] == 5
    assert out["round_trip_rate"] == 6 / (2 * 4 * 5)
    assert out["n_up"].tolist() == [10, 4, 2, 0] and out["n_down"].tolist() == [0, 4, 0, 10]
    assert out["up_fraction"].tolist() == [1.0, 0.5, 1.0, 0.0]


FLOW_TEMPS, FLOW_EVENTS = 4, 7


def _flow_shard(rank):
    """Hand-made flow arrays of a shard of 3 (rank 0) or 5 (rank 1) replicas of an 8-replica run."""
    n = (3, 5)[rank]
    g = torch.Generator().manual_seed(40 + rank)
    return {"walker": torch.arange(FLOW_TEMPS, dtype=torch.int32).repeat(n, 1),
            "round_trips": torch.randint(0, 6, (n, FLOW_TEMPS), generator=g, dtype=torch.int64),
            "n_up": torch.randint(0, 50, (n, FLOW_TEMPS), generator=g, dtype=torch.int64),
            "n_down": torch.randint(0, 50, (n, FLOW_TEMPS), generator=g, dtype=torch.int64), "events": FLOW_EVENTS}


def _flow_worker(rank):
    from algorithms.sharding import allreduce_flow

    shard = _flow_shard(rank)
    kept = {k: v.clone() for k, v in shard.items() if torch.is_tensor(v)}
    total = allreduce_flow(shard)
    assert all(torch.equal(shard[k], v) for k, v in kept.items())  # inputs untouched
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in total.items()}


def test_allreduce_flow_over_two_ranks_is_the_flow_of_the_whole():
    """gloo, two spawned ranks holding 3 and 5 replicas, CPU tensors: both ranks return the arrays of the 8-replica whole, and
    the up-fraction and round-trip rate computed from those."""
    from algorithms.sharding import flow_round_trip_rate, flow_up_fraction

    got = gloo_world(_flow_worker)
    a, b = _flow_shard(0), _flow_shard(1)
    whole = {k: torch.cat([a[k], b[k]]) for k in ("round_trips", "n_up", "n_down")}
    assert whole["n_up"].shape == (8, FLOW_TEMPS)
    up, down, trips = whole["n_up"].sum(0), whole["n_down"].sum(0), int(whole["round_trips"].sum())
    assert trips > 0 and not torch.equal(a["n_up"].sum(0), b["n_up"].sum(0))
    assert sorted(r for r, _ in got) == [0, 1]
    for _, total in got:
        assert total["n_up"].tolist() == up.tolist() and total["n_down"].tolist() == down.tolist()
        assert total["round_trips_total"] == trips and total["n_replicas"] == 8 and total["events"] == FLOW_EVENTS
        assert total["up_fraction"].tolist() == flow_up_fraction(up, down).tolist()
        assert total["round_trip_rate"] == flow_round_trip_rate(trips, 8, FLOW_TEMPS, FLOW_EVENTS) == trips / (8 * FLOW_TEMPS * FLOW_EVENTS)


def test_class_flow_checks_need_no_gpu():
    """What the class and the run refuse before a device is asked for."""
    import numpy as np

    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from algorithms._engine_core import EngineRun
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    with pytest.raises(ValueError, match="two temperatures"):
        ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0], device="cpu", flow=True)
    alg = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5, 0.1], device="cpu", flow=True, num_replicas=2)
    assert alg.walker_positions().tolist() == [[0, 1, 2], [0, 1, 2]] and alg.walker_positions().dtype == torch.int32
    assert alg.round_trips().shape == (2, 3) and alg.round_trips().dtype == torch.int64 and alg.round_trip_rate() == 0.0
    assert torch.isnan(alg.up_fraction()).all() and alg.up_fraction().dtype == torch.float64
    off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu")
    with pytest.raises(RuntimeError, match="flow=True"):
        off.round_trips()
    assert "round_trips_total" not in off.get_diagnostic_info()
    with pytest.raises(ValueError, match="two temperatures"):
        EngineRun(target_dist=tgt, proposal=None, beta_ladder=[1.0], dim=3, device=torch.device("cpu"), n_replicas=1,
                  initial_state=np.zeros(3, np.float32), burn_in=0, swap_every=1, swap_mode="exchange", swap_order="sequential",
                  seed=1, flow=True)
