"""Pooled marginal histograms (include/ptrwm.h ptrwm_hist_args, csrc/hist.h) without a GPU: the bin rule and the launch cut
against brute force, the struct's C layout, every validation code of the two entry points that returns before a HIP call, the
NumPy replay of the rule that the GPU tests rely on, and the arithmetic of the class accessors on hand-made counts."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
import torch

import ptrwm_hip as E
from host_harness import ROOT, assert_layout, c_layout, gloo_world, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def hist_exe(tmp_path_factory):
    """tests/hist_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    return sanitized_exe(tmp_path_factory.mktemp("hist"), "hist_test.cpp")


def test_bin_rule_and_cuts_against_brute_force(hist_exe):
    """csrc/hist.h and the histogram helper of csrc/schedule.h in tests/hist_test.cpp: the rule against a double-precision
    restatement (lo, hi, their neighbours, +-inf, NaN, denormals; 1, 2, 7, 64 and 1024 bins), the cuts of
    ptrwm_run_with_histogram replayed step by step, and hist_geometry - the snapshot kernel's tiling of the covered columns -
    for every n_bins in 1..1024 and every temps * dim in 1..26 624."""
    run_exe(hist_exe, ok="hist ok:")


def test_gpu_geometry_cases_force_the_geometry_they_are_named_for(hist_exe):
    """The table of tests/test_gpu_hist.py through hist_geometry itself (the program's "geometry" mode): every case has more
    than one group of columns and the strategy, group width, group count and last group its row states - so a change of a
    constant of csrc/hist.h cannot quietly turn the GPU cases back into single-group ones - and, case by case, the property
    it is there for."""
    from test_gpu_hist import GEOMETRY_CASES

    lines = "".join(f"{c[4]} {c[3] * c[1]}\n" for c in GEOMETRY_CASES)
    out = run_exe(hist_exe, "geometry", input=lines, timeout=60)
    got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    assert len(got) == len(GEOMETRY_CASES) == 7
    geo = {}
    for (name, dim, T, temps, _, Cn, direct, cols, groups, last, _), g in zip(GEOMETRY_CASES, got):
        assert g == (int(direct), cols, groups, last), (name, g)
        assert groups > 1 and 1 <= temps <= T and Cn >= 1, name
        geo[name] = dict(dim=dim, T=T, temps=temps, Cn=Cn, direct=direct, cols=cols, groups=groups, last=last)
    g = geo["readme_8_groups"]  # group boundaries inside a temperature's run; two chain tiles, the second partial
    assert not g["direct"] and g["groups"] == 8 and g["cols"] % g["dim"] != 0 and g["last"] < g["cols"] and 256 < g["Cn"] < 512
    g = geo["lds_min_cols"]  # the narrowest LDS group; a last group of 2 columns; the second chain tile holds one chain
    assert not g["direct"] and g["cols"] == 64 and g["groups"] == 3 and g["last"] == 2 and g["Cn"] == 257
    g = geo["lds_cols_cap"]  # the widest group; the last one does not divide the workgroup: idle threads
    assert not g["direct"] and g["cols"] == 256 and g["last"] < g["cols"] and 256 % g["last"] != 0
    g = geo["cold_5_of_12"]  # the chain stride is not the number of covered columns
    assert g["temps"] < g["T"] and g["cols"] % g["dim"] != 0 and g["last"] < g["cols"]
    g = geo["direct_2_groups"]
    assert g["direct"] and g["groups"] == 2 and g["last"] < g["cols"] and g["cols"] % g["dim"] != 0
    g = geo["direct_max_bins"]
    assert g["direct"] and g["dim"] == 104 and g["last"] < g["cols"] and GEOMETRY_CASES[5][4] == E.HIST_MAX_BINS
    g = geo["widest_state"]
    assert not g["direct"] and g["dim"] * g["temps"] == 104 * 256 and g["groups"] == 416


def numpy_bins(x, lo, scale, n_bins):
    """The rule of csrc/hist.h in NumPy: float32 arithmetic, truncation (the replay the GPU tests compare with)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - np.float32(lo)) * np.float32(scale)
    b = np.zeros(u.shape, np.int64)
    over = u >= np.float32(n_bins)
    mid = (u >= 0) & ~over
    b[over] = n_bins + 1
    b[mid] = 1 + u[mid].astype(np.int64)
    return b


def test_numpy_replay_agrees_with_the_header(tmp_path):
    """The same values through hist_bin (compiled here) and through the NumPy replay."""
    src = tmp_path / "dump.cpp"
    src.write_text(f'#include <cstdio>\n#include <cstring>\n#include "{ROOT}/rwm-pt-pytorch_amd/csrc/hist.h"\n'
                   "int main(){ unsigned xb, lb, sb; int nb; while (std::scanf(\"%x %x %x %d\", &xb, &lb, &sb, &nb) == 4) {"
                   " float x, lo, sc; std::memcpy(&x, &xb, 4); std::memcpy(&lo, &lb, 4); std::memcpy(&sc, &sb, 4);"
                   " std::printf(\"%d\\n\", ptrwm::hist_bin(x, lo, sc, nb)); } return 0; }\n")
    exe = tmp_path / "dump"
    subprocess.check_call(["g++", "-std=c++17", "-O2", str(src), "-o", str(exe)])
    rng = np.random.default_rng(5)
    lines, want = [], []
    for lo, hi, nb in ((-6.0, 6.0, 240), (-1.0, 1.0, 7), (0.1, 0.7, 64), (-20.0, 20.0, 1024), (-0.5, 0.25, 1)):
        lo32, hi32 = np.float32(lo), np.float32(hi)
        scale = np.float32(nb) / (hi32 - lo32)
        xs = np.concatenate([rng.normal(0.0, 3.0, 300).astype(np.float32),
                             np.array([lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)), np.nextafter(hi32, np.float32(-np.inf)),
                                       np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45], np.float32),
                             (lo32 + (hi32 - lo32) * np.arange(nb + 1, dtype=np.float32) / np.float32(nb)).astype(np.float32)])
        want.append(numpy_bins(xs, lo32, scale, nb))
        for x in xs:
            lines.append(f"{x.view(np.uint32):x} {lo32.view(np.uint32):x} {scale.view(np.uint32):x} {nb}")
    got = np.array([int(v) for v in run_exe(exe, input="\n".join(lines), timeout=60).split()], np.int64)
    assert np.array_equal(got, np.concatenate(want))


def test_hist_struct_layout_matches_the_c_header(tmp_path):
    fields = [f[0] for f in E.HistArgs._fields_]
    assert fields == ["struct_size", "temps", "every", "n_bins", "lo", "scale", "counts", "count"]
    got = c_layout(tmp_path, {"ptrwm_hist_args": fields}, macros=("PTRWM_ABI_VERSION", "PTRWM_HIST_MAX_BINS"))
    assert_layout(E.HistArgs, "ptrwm_hist_args", fields, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays
    assert got["PTRWM_HIST_MAX_BINS"] == E.HIST_MAX_BINS == 1024


def _valid(n_temps=4):
    """Arguments both entry points accept up to their first HIP call, with the blocks whose checks come before check_hist."""
    return valid_args("hi", "fl", "mom", n_temps=n_temps)


def test_hist_validation_needs_no_gpu():
    lib = E.load_library()

    def run(v, hist="hi", mom=None, flow=None):
        return lib.ptrwm_run_with_histogram(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), C.byref(v[mom]) if mom else None,
                                            None, C.byref(v[flow]) if flow else None, C.byref(v[hist]) if hist else None, None)

    def snap(v, hist="hi", dim=30):
        return lib.ptrwm_histogram(C.byref(v["ra"]), dim, C.byref(v[hist]) if hist else None, None)

    for call in (run, snap):
        v = _valid()
        v["hi"].struct_size = 4
        assert call(v) == -6, call.__name__  # PTRWM_E_STRUCT
        for field, bad in (("temps", 0), ("temps", 5), ("every", 0), ("n_bins", 0), ("n_bins", 1025)):
            v = _valid()
            setattr(v["hi"], field, bad)
            assert call(v) == -5, (call.__name__, field, bad)  # PTRWM_E_ARG
        for field in ("lo", "scale", "counts"):
            v = _valid()
            setattr(v["hi"], field, None)
            assert call(v) == -1, (call.__name__, field)  # PTRWM_E_NULL
        v = _valid()
        v["hi"].temps, v["hi"].n_bins = 4, 1024  # the limits themselves pass; count may be NULL
        v["ra"].n_chains = 0
        assert call(v) == 0
        # the order: struct size, then the arguments, then the pointers
        v = _valid()
        v["hi"].struct_size, v["hi"].every, v["hi"].lo = 4, 0, None
        assert call(v) == -6
        v = _valid()
        v["hi"].every, v["hi"].lo = 0, None
        assert call(v) == -5
        # the entry point's own checks come first: the argument block's size, the ladder's length
        v = _valid()
        v["ra"].struct_size, v["hi"].struct_size = 4, 4
        assert call(v) == -6
        v = _valid(n_temps=257)
        v["hi"].lo = None
        assert call(v) == -3
        # an empty batch with a valid block: nothing to do; with a bad block: still refused
        v = _valid()
        v["ra"].n_chains = 0
        assert call(v) == 0
        v["hi"].n_bins = 2000
        assert call(v) == -5
        # a NULL state is looked at after the block and after the empty-batch return
        v = _valid()
        v["ra"].state, v["hi"].counts = None, None
        assert call(v) == -1
        v["hi"].counts = v["ptr"]
        assert call(v) == -1
    # ptrwm_histogram alone: NULL arguments, dim, the flags it reads
    v = _valid()
    assert snap(v, hist=None) == -1
    assert lib.ptrwm_histogram(None, 30, C.byref(v["hi"]), None) == -1
    assert snap(v, dim=0) == -2 and snap(v, dim=105) == -2
    v["ra"].state_f64 = 2
    assert snap(v) == -5
    v = _valid()
    v["ra"].step0 = -1
    assert snap(v) == -5
    # a step that is not due is known on the host: nothing is enqueued, so the fake pointers are never read
    v = _valid()
    v["ra"].step0, v["ra"].burn_in, v["hi"].every = 4, 0, 10  # step counter 5
    assert snap(v) == 0
    v["ra"].step0, v["ra"].burn_in = 9, 10  # step counter 10, still in burn-in
    assert snap(v) == 0
    # ptrwm_run_with_histogram: the accumulators' and flow's checks come before the histogram's, its own arguments after
    v = _valid()
    v["mom"].struct_size, v["hi"].every = 4, 0
    assert run(v, mom="mom") == -6
    v = _valid()
    v["fl"].walker, v["hi"].struct_size = None, 4
    assert run(v, flow="fl") == -1
    v = _valid()
    v["ra"].swap_mode, v["hi"].lo = 7, None
    assert run(v) == -1
    v = _valid()
    v["ra"].swap_mode = 7
    assert run(v) == -5
    v = _valid()
    v["td"].dim = 105
    assert run(v) == -2
    # hist == NULL: ptrwm_run_with_diagnostics' codes
    v = _valid()
    v["ra"].state = None
    assert run(v, hist=None) == -1 == lib.ptrwm_run_with_diagnostics(C.byref(v["td"]), C.byref(v["pd"]), C.byref(v["ra"]), None, None, None, None)
    v = _valid()
    v["ra"].n_chains = 0
    assert run(v, hist=None) == 0
    # a request that passes every check goes on to the launch, which a machine without a GPU cannot make
    if not torch.cuda.is_available():
        v = _valid()
        assert run(v) == -7 and run(v, hist=None) == -7


def _counts(rows):
    return torch.tensor(rows, dtype=torch.int64)


def test_quantiles_mass_and_mode_weights_on_hand_made_counts():
    from algorithms._engine_core import hist_density, hist_edges, hist_mass_between, hist_mode_weights, hist_quantiles, hist_scale

    lo, hi = np.array([0.0, -2.0], np.float32), np.array([4.0, 2.0], np.float32)
    edges = hist_edges(lo, hi, 4)
    assert edges.dtype == torch.float64 and edges.tolist() == [[0, 1, 2, 3, 4], [-2, -1, 0, 1, 2]]
    assert hist_scale(lo, hi, 4).dtype == np.float32 and hist_scale(lo, hi, 4).tolist() == [1.0, 1.0]
    #                 under  b1  b2  b3  b4  over
    counts = _counts([[0, 10, 20, 30, 40, 0],
                      [10, 0, 40, 40, 0, 10]])
    # density: counts / total / width; the out-of-range mass stays in the total
    dens = hist_density(counts, edges)
    assert dens.shape == (2, 4) and dens[0].tolist() == [0.1, 0.2, 0.3, 0.4] and dens[1].tolist() == [0.0, 0.4, 0.4, 0.0]
    assert float(dens[1].sum()) == pytest.approx(0.8)
    # quantiles: linear inside the crossing bin
    q = hist_quantiles(counts, edges, [0.0, 0.1, 0.25, 0.5, 1.0])
    assert q.shape == (5, 2)
    assert q[:, 0].tolist() == pytest.approx([0.0, 1.0, 1.75, 2.0 + 20.0 / 30.0, 4.0])
    # coordinate 1: the lowest and the highest tenth sit in the end bins - NaN up to and including q = 0.1 (the cumulative count
    # reaches the target inside the underflow bin) and from above 0.9 on, numbers in between
    assert math.isnan(q[0, 1]) and math.isnan(q[1, 1]) and math.isnan(q[4, 1])
    assert q[2, 1] == pytest.approx(-1.0 + 15.0 / 40.0) and q[3, 1] == pytest.approx(0.0)
    assert hist_quantiles(counts, edges, [0.9])[0, 1] == pytest.approx(1.0)
    assert math.isnan(hist_quantiles(counts, edges, [0.05])[0, 1]) and math.isnan(hist_quantiles(counts, edges, [0.95])[0, 1])
    assert torch.isnan(hist_quantiles(_counts([[0] * 6, [0] * 6]), edges, [0.5])).all()  # nothing counted
    with pytest.raises(ValueError):
        hist_quantiles(counts, edges, [1.5])
    # mass between edges: exact ratios of counts
    assert hist_mass_between(counts, edges, [1.0, -1.0], [3.0, 1.0]).tolist() == [0.5, 0.8]
    assert hist_mass_between(counts, edges, 1.0, 2.0).tolist() == [0.2, 0.0]
    assert hist_mass_between(counts, edges, -np.inf, np.inf).tolist() == [1.0, 1.0]
    assert hist_mass_between(counts, edges, -np.inf, [0.0, -2.0]).tolist() == [0.0, 0.1]  # the underflow bin alone
    assert hist_mass_between(counts, edges, [4.0, 2.0], np.inf).tolist() == [0.0, 0.1]  # the overflow bin alone
    assert hist_mass_between(counts, edges, 1.0, 1.0).tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match=r"not a bin edge of coordinate 0; the nearest edges are 1\.0 and 2\.0"):
        hist_mass_between(counts, edges, 1.5, 3.0)
    with pytest.raises(ValueError, match="not a bin edge of coordinate 1"):
        hist_mass_between(counts, edges, 1.0, 3.0)  # an edge of coordinate 0, outside coordinate 1's range
    with pytest.raises(ValueError, match="a <= b"):
        hist_mass_between(counts, edges, 2.0, 1.0)
    assert torch.isnan(hist_mass_between(_counts([[0] * 6, [0] * 6]), edges, 1.0, 2.0)).all()
    # mode weights: the end bins folded into the end intervals, every column adds up to one
    w = hist_mode_weights(counts, edges, [1.0, 2.0])
    assert w.shape == (3, 2) and w[:, 0].tolist() == [0.1, 0.2, 0.7] and w[:, 1].tolist() == pytest.approx([0.9, 0.0, 0.1])
    assert w.sum(0).tolist() == pytest.approx([1.0, 1.0])
    assert hist_mode_weights(counts, edges, [])[0].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="strictly increasing"):
        hist_mode_weights(counts, edges, [2.0, 1.0])
    # an edge that is no short binary fraction is still found: -6 + 159 * 0.05
    e240 = hist_edges(np.array([-6.0], np.float32), np.array([6.0], np.float32), 240)
    c240 = torch.ones(1, 242, dtype=torch.int64)
    assert hist_mass_between(c240, e240, -6.0, 1.95).tolist() == [159 / 242]


def test_class_hist_checks_need_no_gpu():
    """What the classes and the run refuse before a device is asked for, and what they answer before anything has run."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import EngineRun, check_hist_range
    from algorithms.sharding import allreduce_histogram
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    for bad, msg in ((dict(hist="warm", hist_range=(-1, 1)), "'cold' or 'all'"), (dict(hist="cold"), "hist_range"),
                     (dict(hist="cold", hist_range=(1.0, 1.0)), "lo < hi"), (dict(hist="cold", hist_range=(0.0, float("inf"))), "finite"),
                     (dict(hist="cold", hist_range=([0, 0], 1)), "scalar or a"), (dict(hist="all", hist_range=(-1, 1), hist_bins=0), "hist_bins"),
                     (dict(hist="all", hist_range=(-1, 1), hist_bins=1025), "hist_bins"),
                     (dict(hist="all", hist_range=(-1, 1), hist_every=0), "hist_every"), (dict(hist="cold", hist_range=3.0), "pair")):
        with pytest.raises(ValueError, match=msg):
            ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu", **bad)
        with pytest.raises(ValueError, match=msg):
            RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", **bad)
    lo, hi = check_hist_range((-1, [1, 2, 3]), 3)
    assert lo.dtype == np.float32 and lo.tolist() == [-1, -1, -1] and hi.tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="lo < hi"):
        check_hist_range((1.0, 1.0 + 1e-12), 1)  # equal once rounded to float32
    alg = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5, 0.1], device="cpu", hist="all", hist_range=(-20, 20),
                                             hist_bins=8, hist_every=5)
    counts, edges = alg.marginal_histogram(2)
    assert counts.shape == (3, 10) and counts.dtype == torch.int64 and int(counts.sum()) == 0
    assert edges.shape == (3, 9) and edges[0].tolist() == [-20, -15, -10, -5, 0, 5, 10, 15, 20]
    assert torch.isnan(alg.quantiles([0.5])).all() and torch.isnan(alg.mode_weights([-5.0, 5.0])).all()
    assert math.isnan(alg.get_diagnostic_info()["hist_out_of_range"])
    with pytest.raises(ValueError, match="temperature"):
        alg.marginal_histogram(3)
    cold = RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", hist="cold", hist_range=(-20, 20))
    assert cold.marginal_histogram()[0].shape == (3, 66)
    with pytest.raises(ValueError, match="temperature"):
        cold.mass_between(-20, 20, temperature=1)
    off = ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu")
    with pytest.raises(RuntimeError, match="hist="):
        off.marginal_histogram()
    assert "hist_out_of_range" not in off.get_diagnostic_info()
    assert "hist_out_of_range" not in RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu").get_diagnostic_info()
    with pytest.raises(RuntimeError, match="histograms are off"):
        allreduce_histogram(off)
    for bad, msg in ((dict(hist_temps=3, hist_range=(-1, 1)), "hist_temps"), (dict(hist_temps=1), "hist_range"),
                     (dict(hist_temps=1, hist_range=(-1, 1), hist_bins=2000), "hist_bins")):
        with pytest.raises(ValueError, match=msg):
            EngineRun(target_dist=tgt, proposal=None, beta_ladder=[1.0, 0.5], dim=3, device=torch.device("cpu"), n_replicas=1,
                      initial_state=np.zeros(3, np.float32), burn_in=0, swap_every=1, swap_mode="exchange", swap_order="sequential",
                      seed=1, **bad)
    # the shards' all-reduce on a hand-made dict (single process, no process group: the job is this shard)
    h = {"counts": torch.arange(12, dtype=torch.int64).view(1, 2, 6), "count": torch.tensor([7]), "edges": None}
    out = allreduce_histogram(h)
    assert torch.equal(out["counts"], h["counts"]) and out["counts"] is not h["counts"] and out["count"].tolist() == [7]


HIST_SHAPE = (2, 3, 6)  # temps, dim, n_bins + 2


def _hist_shard(rank):
    g = torch.Generator().manual_seed(70 + rank)
    counts = torch.randint(0, 1 << 20, HIST_SHAPE, generator=g, dtype=torch.int64)
    counts[1, 2, 3] = (1 << 31) + 5 + rank  # above 2^31: a narrowing conversion anywhere in the packing would show
    count = counts[:, 0, :].sum(-1)
    edges = torch.linspace(-2.0, 2.0, HIST_SHAPE[2] - 1, dtype=torch.float64).repeat(HIST_SHAPE[1], 1)
    return {"counts": counts, "count": count, "edges": edges}


def _hist_worker(rank):
    from algorithms.sharding import allreduce_histogram

    shard = _hist_shard(rank)
    kept = {k: v.clone() for k, v in shard.items()}
    total = allreduce_histogram(shard)
    assert all(torch.equal(shard[k], v) for k, v in kept.items())  # inputs untouched
    assert total["counts"].dtype == torch.int64 and total["count"].dtype == torch.int64
    return {k: v.numpy() for k, v in total.items()}


def test_allreduce_histogram_over_two_ranks_is_the_sum_of_the_shards():
    """gloo, two spawned ranks, CPU tensors: counts and count add up exactly on both ranks, the edges pass through."""
    got = gloo_world(_hist_worker)
    a, b = _hist_shard(0), _hist_shard(1)
    assert int((a["counts"] + b["counts"])[1, 2, 3]) == (1 << 32) + 11 and int((a["count"] + b["count"]).min()) > 0
    assert sorted(r for r, _ in got) == [0, 1]
    for _, total in got:
        assert total["counts"].shape == HIST_SHAPE and np.array_equal(total["counts"], (a["counts"] + b["counts"]).numpy())
        assert np.array_equal(total["count"], (a["count"] + b["count"]).numpy())
        assert np.array_equal(total["edges"], a["edges"].numpy())
