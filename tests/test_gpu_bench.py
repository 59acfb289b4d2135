"""bench.py's own launch paths on the GPU box, before the driver runs it at N = 1, 2, 4, 8: the N > 1 re-launch under
torch.distributed.run (two ranks sharing the one GPU of the test box, collectives over gloo) and the RCCL path of the
script itself (backend "nccl": init_process_group with device_id, barrier, MAX all-reduce of the clock, summary
all-reduce, destroy) with a world of one rank.  Run with `-m gpu`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --full: the summary and roofline objects these tests read are not part of a plain run
ARGS = ["--steps", "3", "--warmup", "1", "--full", "--cpu-seconds", "0", "--no-extras", "--inner", "300"]


def _bench(cmd, env_extra, timeout=600):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line, got {len(lines)}: {r.stdout[-1000:]}"
    return json.loads(lines[0])


def test_bench_two_ranks_share_the_gpu_over_gloo():
    """`python bench.py --gpus 2`: the script's own re-launch under torch.distributed.run, one process per rank, both on
    cuda:0 (PTRWM_BENCH_BACKEND=gloo: the rehearsal mode for a box with fewer GPUs than ranks).  One JSON line from rank
    0, weak scaling (each rank its own 65 536 ladders with its own global ladder ids), the whole-job value within 2x of
    the one-rank reading on the same GPU (two processes time-share it)."""
    one = _bench([sys.executable, "bench.py", "--gpus", "1"] + ARGS, {})
    two = _bench([sys.executable, "bench.py", "--gpus", "2"] + ARGS, {"PTRWM_BENCH_BACKEND": "gloo", "MASTER_PORT": "29641"})
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["scaling"] == "weak"
    assert two["config"]["sharding"].startswith("2 x 65536 independent ladders")
    assert two["config"]["collective_backend"] == "gloo" and one["config"]["collective_backend"] is None
    assert two["summary"]["replicas"] == 2 * one["summary"]["replicas"] == 2 * 65536
    assert 0.5 < two["value"] / one["value"] < 2.0, (one["value"], two["value"])
    # the ranks sample different ladders (global ids 65536.. on rank 1): same statistics, not the same numbers
    assert two["summary"]["acceptance_rate_cold"] == pytest.approx(one["summary"]["acceptance_rate_cold"], rel=2e-2)
    assert two["summary"]["acceptance_rate_cold"] != one["summary"]["acceptance_rate_cold"]
    # the line diagnoses itself: one record per rank (device identity, its own launch times), the world size it saw
    assert one["config"]["world_size"] == 1 and two["config"]["world_size"] == 2
    assert [r["rank"] for r in two["ranks"]] == [0, 1] and len(one["ranks"]) == 1
    for r in two["ranks"]:
        assert r["pci"] and r["device_name"] and 0 < r["kernel_ms_min"] <= r["kernel_ms_median"] <= r["kernel_ms_max"]
        assert r["wall_s"] > 0
    assert two["distinct_devices"] == 1  # the rehearsal mode: both ranks on the test box's one GPU (RCCL would refuse)


def test_bench_under_torchrun_over_rccl():
    """The exact launch line the driver uses for N > 1, at one rank: python -m torch.distributed.run --nnodes=1
    --nproc-per-node 1 --master-addr 127.0.0.1 --master-port P bench.py --gpus 1 ...  Backend "nccl" (RCCL):
    init_process_group(device_id=...), barriers, the MAX all-reduce of the clock and the summary all-reduce on device
    tensors, destroy_process_group - all executed by bench.py itself."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29643", "bench.py", "--gpus", "1"] + ARGS
    out = _bench(cmd, {})
    assert out["n_gpus"] == 1 and out["config"]["collective_backend"] == "nccl"
    assert out["summary"]["replicas"] == 65536 and out["value"] > 1e9
    assert out["roofline"]["kernel_ms"] > 0 and out["ms_per_step"] >= out["roofline"]["kernel_ms"] * 0.99
    assert out["config"]["world_size"] == 1 and out["distinct_devices"] == 1 and len(out["ranks"]) == 1
    r0 = out["ranks"][0]
    assert r0["rank"] == 0 and r0["pci"] and r0["kernel_ms_mean"] == pytest.approx(out["roofline"]["kernel_ms"], rel=1e-6)


def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    """A plain run (no --full): the headline line without the --full objects, `--steps` timed launches, and with
    --dump-outputs the arrays of the last timed step - float32 / float64, within 64 MB - identical in a second run
    with the same arguments."""
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--inner", "200"]
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        line = _bench([sys.executable, "bench.py"] + args + ["--dump-outputs", str(d)], {})
        names = {p.stem for p in d.glob("*.npy")}
        runs.append((line, {n: np.load(d / f"{n}.npy") for n in names}))
    line, a = runs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config", "ranks"):
        assert k in line, k
    for k in ("roofline", "summary", "other_single_gpu_readings", "cpu_baseline"):
        assert k not in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 1e9
    units = line["config"]["ladders_per_gpu"] * line["config"]["temps"] * line["config"]["mh_steps_per_launch"]
    assert line["value"] == pytest.approx(units / (line["ms_per_step"] * 1e-3), rel=1e-6)
    C, T, D = line["config"]["ladders_per_gpu"], line["config"]["temps"], line["config"]["dim"]
    assert set(a) == {"state", "logp", "n_accept", "sq_jump", "swap_accept", "last_swap_ordinal", "ladder_index"}
    L = len(a["ladder_index"])
    assert 0 < L <= C and a["state"].shape == (L, T, D) and a["state"].dtype == np.float32
    assert a["logp"].shape == (L, T) and a["logp"].dtype == np.float32
    for n in ("n_accept", "sq_jump", "swap_accept", "last_swap_ordinal"):
        assert a[n].shape == (L, T) and a[n].dtype == np.float64, n
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    # warm-up and timed launches: 3 x 200 Metropolis steps per replica, burn-in 0
    assert np.isfinite(a["state"]).all() and np.isfinite(a["logp"]).all()
    assert 0 < a["n_accept"].sum() and a["n_accept"].max() <= 3 * 200
    for n, x in runs[1][1].items():
        assert np.array_equal(x, a[n]), n
