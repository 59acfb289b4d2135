"""Preconditioned Gaussian proposals (include/ptrwm.h ptrwm_split_propose_precond / ptrwm_precond_update, csrc/precond.h) without a
GPU: the proposal kernel's index maps and a CPU replay of it against the rule's direct chain, the update rule's error bound and
skips (tests/precond_test.cpp under ASan and UBSan); the header held to tests/precond_reference.py bit for bit; the structs'
C layout; every validation code of the two entry points that returns before a HIP call."""
import ctypes as C

import numpy as np
import pytest

import precond_reference as PR
import ptrwm_hip as E
from host_harness import assert_layout, c_layout, run_exe, sanitized_exe, valid_args


@pytest.fixture(scope="module")
def precond_exe(tmp_path_factory):
    """tests/precond_test.cpp, a program of its own, compiled as plain C++ under AddressSanitizer and UBSan."""
    # -ffp-contract=off: the header's operations are rounded one by one (the bitwise tests below hold it to Python floats)
    return sanitized_exe(tmp_path_factory.mktemp("precond"), "precond_test.cpp", "-ffp-contract=off")


def test_maps_replay_and_update_rule(precond_exe):
    """(a) dims 1, 3, 4, 5, 16, 17, 30, 33, 64, 104 x rows 1, 5, 64: one accumulator element per (row, coordinate), every operand
    read inside the slabs on a written element, the LDS byte count what the maps touch; (b) the replay of staging, K-steps and
    epilogue equals the direct chain; (c) L L^T within (2^-23 + 2^-48 + (dim + 1) 2^-52) (|L| |L^T|)_ij of A, and a non-positive
    pivot, a sum that is not finite and w < min_count each leave the factor's bits alone; `memory` applied as stated."""
    run_exe(precond_exe, ok="precond ok:")


def test_geometry_of_the_gpu_shapes(precond_exe):
    dims = [1, 3, 4, 5, 16, 17, 30, 33, 64, 104]
    out = run_exe(precond_exe, "geometry", input="".join(f"{d}\n" for d in dims), timeout=60)
    rows = [tuple(map(int, ln.split())) for ln in out.splitlines()]
    assert len(rows) == len(dims)
    geo = dict(zip(dims, rows))
    assert [geo[d][0] for d in dims] == [1, 1, 1, 1, 1, 2, 2, 3, 4, 7]  # blocks: 17 and 33 open a block with one coordinate
    assert geo[104][3] > 64 * 1024 and geo[104][3] <= 160 * 1024  # above the default allowance, inside the CU's LDS
    assert geo[30][3] < 48 * 1024
    assert geo[16][4] == 64 * 5 and geo[17][4] == 64 * 8  # dim 16: the accept uniform's block lies behind the slab's columns
    assert geo[104][5] == 28


def test_launch_grid_mirror_is_the_headers(precond_exe):
    """precond_reference.grid, from which the GPU tests prove that their batches take a second and a third round, against
    precond.h prec_grid (what ptrwm_split_propose_precond launches with): 256 compute units with every tile count the GPU tests
    use - the round cases of tests/test_gpu_precond_rounds.py, the 4 tiles of the alignment tests, the 2 048 and 4 096 tiles of
    the invariance cases - the same for other device sizes, an unknown count, and the cap's neighbours."""
    import test_gpu_precond_rounds as RD

    pairs = []
    for cus in (2, 64, 256, 304):
        G = PR.grid(RD.HUGE, cus)
        assert G == 8 * cus
        tiles = {1, 4, 2048, 4096, G - 1, G, G + 1, 2 * G, RD.HUGE}
        for dim, k, T in RD.CASES.values():
            G2, r, n_tiles, Cn = RD.plan_rounds(k, T, cus)
            assert G2 == G and 0 < r < G and r % 4 != 0 and n_tiles == k * G + r
            assert Cn * T == 64 * (n_tiles - 1) + 5 and PR.tiles(Cn * T) == n_tiles  # the last tile holds 5 rows
            assert -(-n_tiles // PR.grid(n_tiles, cus)) == k + 1
            tiles.add(n_tiles)
        pairs += [(t, cus) for t in sorted(tiles)]
    pairs += [(t, cus) for cus in (0, -1) for t in (1, 2047, 2048, 2049, 4134)]  # (unknown: 256 compute units)
    assert (PR.tiles(210), PR.tiles(32768 * 4), PR.tiles(65536 * 4), PR.tiles(64), PR.tiles(65)) == (4, 2048, 4096, 1, 2)
    out = run_exe(precond_exe, "grid", input="".join(f"{t} {c}\n" for t, c in pairs), timeout=60)
    got = [int(ln) for ln in out.splitlines()]
    assert got == [PR.grid(t, c) for t, c in pairs]
    assert PR.grid(4134, 256) == 2048 == PR.grid(4134, 0) and PR.grid(5, 256) == 5 and PR.grid(RD.HUGE, 2) == 16


def test_fmaf_vec_is_libm_fmaf():
    """The array form of the reference's fused multiply-add against libm's, on random triples, on products that cancel against
    the addend and on sums constructed to lie next to a float32 rounding tie (where rounding twice would go wrong)."""
    rng = np.random.default_rng(20261021)
    n = 20_000
    a = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
    c[::3] = (-a[::3].astype(np.float64) * b[::3]).astype(np.float32)  # cancellation: the result is the product's rounding error
    # ties: c = m 2^24 with m odd-ish, a b = 0.5 +- tiny  ->  the exact sum lies a hair off the midpoint of two floats
    k = n // 4
    a[:k] = np.float32(0.5) + rng.choice([-1, 1], k).astype(np.float32) * np.float32(2.0 ** -24)
    b[:k] = np.float32(1.0) + rng.integers(-3, 4, k).astype(np.float32) * np.float32(2.0 ** -23)
    c[:k] = rng.integers(1 << 23, 1 << 24, k).astype(np.float32)
    a[-5:], b[-5:], c[-5:] = [0, -0.0, 1, np.inf, 3e38], [5, 0.0, 0, 1, 3e38], [-0.0, 0.0, -0.0, 1, 1]
    got = PR.fmaf_vec(a, b, c)
    want = np.array([PR.fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with np.errstate(over="ignore"):
        twice = (a.astype(np.float64) * b + c).astype(np.float32)  # what rounding twice gives: the tie cases must tell the two apart
    assert (twice[:k].view(np.uint32) != want[:k].view(np.uint32)).any()


def _bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32).ravel()


def _bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).ravel()


def _random_sums(rng, dim, cond):
    """Covariance sums of n draws of a Gaussian whose covariance has condition `cond`, as float states give them"""
    n = int(rng.integers(4 * dim + 1, 8 * dim + 20))
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    sd = np.sqrt(np.exp(np.linspace(0.0, np.log(cond), dim)))
    x = ((rng.standard_normal((n, dim)) * sd) @ q.T + rng.standard_normal(dim) * 3).astype(np.float32).astype(np.float64)
    sxx = np.tril(x.T @ x) + np.triu(np.full((dim, dim), 555.0), 1)  # (rubbish above the diagonal: never read)
    return n, sxx, x.sum(0)


def test_update_rule_against_python_floats_bitwise(precond_exe):
    """200 random sums, dims 1 to 104, condition up to 10^6, with and without a running triple, the three skips among them: the
    header's outcome, factor, running triple and zeroed sums against precond_reference, bit for bit."""
    rng = np.random.default_rng(20261022)
    cases = []
    for i in range(200):
        dim = int(rng.integers(1, 105)) if i % 4 == 0 else int(rng.integers(1, 25))
        if i == 0:
            dim = 104
        cond = float(np.exp(rng.uniform(0.0, np.log(1e6))))
        n, sxx, sx = _random_sums(rng, dim, cond)
        memory = float(rng.choice([1.0, 0.5, 0.3]))
        jitter = float(rng.choice([0.0, 1e-6, 1e-3]))
        min_count = float(4 * dim)
        chol = np.tril(rng.standard_normal((dim, dim))).astype(np.float32)
        if i % 3 == 0:  # a running triple from an earlier window
            n2, run_xx, run_x = _random_sums(rng, dim, cond)
            run_w = float(n2) * 0.7
        else:
            run_xx, run_x, run_w = np.zeros((dim, dim)), np.zeros(dim), 0.0
        kind = i % 20
        if kind == 5:
            min_count = float(100 * dim)  # too few draws
        elif kind == 9:
            sxx[dim - 1, dim - 1] = -abs(sxx[dim - 1, dim - 1])  # a negative variance
            jitter = 0.0
        elif kind == 13:
            sxx[dim // 2, 0] = np.nan if i % 40 == 13 else np.inf
        cases.append((dim, memory, jitter, min_count, n, sxx, sx, run_xx, run_x, run_w, chol))
    lines = []
    for dim, memory, jitter, min_count, n, sxx, sx, run_xx, run_x, run_w, chol in cases:
        nums = [*_bits64(sxx), *_bits64(sx), *_bits64(run_xx), *_bits64(run_x), *_bits64([run_w]), *_bits32(chol)]
        lines.append(f"{dim} {memory!r} {jitter!r} {min_count!r} {n} " + " ".join(map(str, nums)) + "\n")
    rows = run_exe(precond_exe, "update", input="".join(lines), timeout=600).splitlines()
    assert len(rows) == len(cases)
    outcomes = [0, 0, 0]
    for (dim, memory, jitter, min_count, n, sxx, sx, run_xx, run_x, run_w, chol), row in zip(cases, rows):
        v = row.split()
        got_outcome, zeroed = int(v[0]), int(v[1])
        d2 = dim * dim
        got_chol = np.array(v[2:2 + d2], np.uint32)
        got_xx = np.array(v[2 + d2:2 + 2 * d2], np.uint64)
        got_x = np.array(v[2 + 2 * d2:2 + 2 * d2 + dim], np.uint64)
        got_w = np.uint64(v[2 + 2 * d2 + dim])
        outcome, want_chol, want_xx, want_x, want_w = PR.update(sxx, sx, n, run_xx, run_x, run_w, memory, jitter, min_count, chol)
        assert got_outcome == outcome and zeroed == 1, (dim, outcome, got_outcome)
        outcomes[outcome] += 1
        assert np.array_equal(got_chol, _bits32(want_chol)), (dim, outcome)
        assert np.array_equal(got_xx, _bits64(want_xx)) and np.array_equal(got_x, _bits64(want_x)) and got_w == _bits64([want_w])[0]
        if outcome != PR.UPDATED:
            assert np.array_equal(got_chol, _bits32(chol))
    assert outcomes[PR.FEW_DRAWS] >= 10 and outcomes[PR.NOT_POSITIVE] >= 15 and outcomes[PR.UPDATED] >= 150, outcomes


def test_proposal_rule_against_libm_fmaf_bitwise(precond_exe):
    """200 random proposal rows: the header's direct chain AND the replay of the kernel against the reference's chain, every fmaf
    through libm, and the reference's array form against that."""
    rng = np.random.default_rng(20261023)
    cases, lines = [], []
    for i in range(50):  # 50 tiles of 4 rows
        dim = int(rng.choice([1, 3, 4, 5, 16, 17, 30, 33])) if i % 5 else int(rng.choice([64, 104]))
        n = 4
        x = rng.standard_normal((n, dim)).astype(np.float32) * np.float32(10)
        z = rng.standard_normal((n, dim)).astype(np.float32)
        chol = np.tril(rng.standard_normal((dim, dim))).astype(np.float32) + np.triu(np.full((dim, dim), np.nan, np.float32), 1)
        scale = np.exp(rng.uniform(-3, 1, n)).astype(np.float32)
        cases.append((dim, n, x, z, chol, scale))
        chol_in = np.where(np.isnan(chol), np.float32(777), chol)  # (text cannot carry the NaN's payload; the maps never read it)
        nums = [*_bits32(scale), *_bits32(x), *_bits32(chol_in), *_bits32(z)]
        lines.append(f"{dim} {n} " + " ".join(map(str, nums)) + "\n")
    rows = run_exe(precond_exe, "propose", input="".join(lines)).splitlines()
    assert len(rows) == len(cases)
    for (dim, n, x, z, chol, scale), row in zip(cases, rows):
        v = np.array(row.split(), np.uint32)
        replay, chain = v[:n * dim], v[n * dim:]
        want = PR.propose_rows(x, chol, z, scale, exact_libm=True)
        assert not np.isnan(want).any()
        assert np.array_equal(chain, _bits32(want)), dim
        assert np.array_equal(replay, _bits32(want)), dim
        assert np.array_equal(_bits32(PR.propose_rows(x, chol, z, scale)), _bits32(want)), dim


def test_class_precond_checks_need_no_gpu():
    """Every ValueError, NotImplementedError and warning of the new keywords, raised before a device is asked for, and what the
    readers answer before anything has run."""
    import warnings

    import torch

    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from algorithms._engine_core import EngineRun, check_proposal_cov
    from proposal_distributions import LaplaceProposal, UniformRadiusProposal
    from target_distributions import RoughCarpetDistributionTorch

    tgt = RoughCarpetDistributionTorch(3, device="cpu")
    good = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.5], [0.0, 0.5, 2.0]])
    rwm = lambda **kw: RandomWalkMH_GPU_Optimized(3, 1.0, tgt, device="cpu", **kw)  # noqa: E731
    pt = lambda **kw: ParallelTemperingRWM_GPU_Optimized(3, 1.0, tgt, beta_ladder=[1.0, 0.5], device="cpu", **kw)  # noqa: E731
    run = lambda proposal=None, **kw: EngineRun(target_dist=tgt, proposal=proposal, beta_ladder=[1.0, 0.5], dim=3,  # noqa: E731
                                                device=torch.device("cpu"), n_replicas=1, initial_state=np.zeros(3, np.float32),
                                                burn_in=400, swap_every=1, swap_mode="exchange", swap_order="sequential", seed=1, **kw)
    asym = good.copy()
    asym[0, 1] = 1.5
    bad_cov = [(np.eye(4), "dim, dim"), (np.ones(3), "dim, dim"), (asym, "symmetric"), (np.full((3, 3), np.nan), "symmetric"),
               (np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), "positive definite"), (np.zeros((3, 3)), "positive definite"),
               (-np.eye(3), "positive definite")]
    for cov, msg in bad_cov:
        for make in (rwm, pt):
            with pytest.raises(ValueError, match=msg):
                make(proposal_cov=cov)
        with pytest.raises(ValueError, match=msg):
            make(proposal_cov=torch.tensor(cov))
    bad_kw = [(dict(adapt_cov=1), "adapt_cov"), (dict(cov_adapt_every=0), "cov_adapt_every"), (dict(cov_adapt_every=2.5), "cov_adapt_every"),
              (dict(cov_adapt_until=-1), "cov_adapt_until"), (dict(cov_adapt_until=401), "cov_adapt_until"),
              (dict(cov_adapt_probe_every=0), "cov_adapt_probe_every"), (dict(cov_adapt_probe_every=7), "cov_adapt_probe_every"),
              (dict(cov_adapt_probe_every=400), "cov_adapt_probe_every"), (dict(cov_adapt_memory=0.0), "cov_adapt_memory"),
              (dict(cov_adapt_memory=1.5), "cov_adapt_memory"), (dict(cov_adapt_memory=float("nan")), "cov_adapt_memory"),
              (dict(cov_adapt_jitter=-1e-9), "cov_adapt_jitter"), (dict(cov_adapt_min_count=0.5), "cov_adapt_min_count"),
              (dict(adapt_sync=7), "adapt_sync")]
    for bad, msg in bad_kw:
        kw = {"adapt_cov": True, **bad}
        for make in (rwm, pt, run):
            with pytest.raises(ValueError, match=msg):
                make(burn_in=400, **kw) if make is not run else make(**kw)
    # any proposal family but Normal
    for prop in (LaplaceProposal(3, torch.ones(3), 1.0, torch.device("cpu"), torch.float32, None),
                 UniformRadiusProposal(3, 1.0, 1.0, torch.device("cpu"), torch.float32, None)):
        for kw in (dict(proposal_cov=good), dict(adapt_cov=True, burn_in=400)):
            with pytest.raises(ValueError, match="Normal"):
                rwm(proposal_distribution=prop, **kw)
            with pytest.raises(ValueError, match="Normal"):
                pt(proposal_distribution=prop, **kw)
    with pytest.raises(ValueError, match="Normal"):
        run(proposal=E.Proposal(E.PROPOSAL_LAPLACE, torch.ones(2)), proposal_chol=np.eye(3))
    with pytest.raises(ValueError, match="proposal_chol"):
        run(proposal_chol=np.eye(4))
    with pytest.raises(ValueError, match="positive diagonal"):
        run(proposal_chol=np.zeros((3, 3)))
    # float64 states: split steps carry float32
    with pytest.raises(NotImplementedError, match="float64"):
        pt(proposal_cov=good, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float64"):
        pt(adapt_cov=True, burn_in=400, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float64"):
        run(proposal_chol=np.eye(3), dtype=torch.float64)
    # no window fits into burn-in
    with pytest.warns(UserWarning, match="will not move"):
        rwm(adapt_cov=True, burn_in=199)
    with pytest.warns(UserWarning, match="will not move"):
        pt(adapt_cov=True, burn_in=400, cov_adapt_until=150)
    # off: the other arguments are not looked at, nothing warns, and the readers say so
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off = rwm(cov_adapt_every=0, cov_adapt_memory=7.0)
        on = pt(proposal_cov=good, adapt_cov=True, burn_in=400, cov_adapt_every=100, cov_adapt_probe_every=25)
        fixed = rwm(proposal_cov=torch.tensor(good))
    for read in (off.proposal_factor, off.proposal_covariance, off.preconditioner_history):
        with pytest.raises(RuntimeError, match="not preconditioned"):
            read()
    assert off.get_diagnostic_info()["preconditioned"] is False
    with pytest.raises(RuntimeError, match="tuning is off"):
        fixed.preconditioner_history()
    # before the first step: the factor of proposal_cov, factored in float64
    want = np.linalg.cholesky(good).astype(np.float32)
    assert np.array_equal(check_proposal_cov(good, 3), want)
    for alg in (on, fixed):
        f = alg.proposal_factor()
        assert f.dtype == torch.float32 and np.array_equal(f.numpy(), want) and float(f[0, 1]) == 0.0 and float(f[0, 2]) == 0.0
        c = alg.proposal_covariance()
        assert c.dtype == torch.float64 and np.allclose(c.numpy(), good, rtol=1e-6)
        alg.reset()
        assert np.array_equal(alg.proposal_factor().numpy(), want)
    h = on.preconditioner_history()
    assert tuple(h["factors"].shape) == (5, 3, 3) and tuple(h["weights"].shape) == (4,) and h["skipped"] == 0
    assert np.array_equal(h["factors"][0].numpy(), want) and bool(torch.isnan(h["factors"][1:]).all()) and bool(torch.isnan(h["weights"]).all())
    info = on.get_diagnostic_info()
    assert info["preconditioned"] is True and info["precond_updates"] == 0 and info["precond_updates_skipped"] == 0
    assert info["precond_condition"] == pytest.approx(np.linalg.cond(good), rel=1e-4)
    ident = rwm(adapt_cov=True, burn_in=400)  # no proposal_cov: the adaptation starts from the identity
    assert np.array_equal(ident.proposal_factor().numpy(), np.eye(3, dtype=np.float32))


PRECOND_FIELDS = ["struct_size", "reserved", "chol"]
UPDATE_FIELDS = ["struct_size", "reserved", "chol", "sxx", "sx", "count", "run_xx", "run_x", "run_w", "memory", "jitter", "min_count",
                 "windows", "chol_history", "weight_history", "skipped"]


def test_struct_layouts_match_the_c_header(tmp_path):
    assert [f[0] for f in E.PrecondArgs._fields_] == PRECOND_FIELDS and [f[0] for f in E.PrecondUpdateArgs._fields_] == UPDATE_FIELDS
    got = c_layout(tmp_path, {"ptrwm_precond_args": PRECOND_FIELDS, "ptrwm_precond_update_args": UPDATE_FIELDS},
                   macros=("PTRWM_ABI_VERSION",))
    assert_layout(E.PrecondArgs, "ptrwm_precond_args", PRECOND_FIELDS, got)
    assert_layout(E.PrecondUpdateArgs, "ptrwm_precond_update_args", UPDATE_FIELDS, got)
    assert got["PTRWM_ABI_VERSION"] == E.ABI_VERSION == 3  # additive: the version stays
    assert "ptrwm_split_propose_precond" in E.SYMBOLS and "ptrwm_precond_update" in E.SYMBOLS


def _valid(n_temps=4):
    return valid_args("pa", "up", n_temps=n_temps)


def test_validation_needs_no_gpu():
    lib = E.load_library()

    def propose(v, dim=5, pd="pd", pa="pa", props=True, acc=True):
        ref = lambda k: C.byref(v[k]) if k else None  # noqa: E731
        return lib.ptrwm_split_propose_precond(ref(pd), C.byref(v["ra"]), dim, ref(pa), v["ptr"] if props else None,
                                               v["ptr"] if acc else None, None)

    def update(v, dim=5, window=0):
        return lib.ptrwm_precond_update(C.byref(v["up"]), dim, window, None)

    # the proposal, in the documented order: NULL proposal / precond; ptrwm_split_propose's checks; the kind; the struct; the
    # empty batch; the pointers
    v = _valid()
    assert propose(v, pd=None) == -1 and propose(v, pa=None) == -1
    assert lib.ptrwm_split_propose_precond(C.byref(v["pd"]), None, 5, C.byref(v["pa"]), v["ptr"], v["ptr"], None) == -1
    v["ra"].struct_size = 4
    v["pd"].kind = E.PROPOSAL_LAPLACE
    assert propose(v) == -6
    v = _valid()
    v["ra"].state_f64, v["pd"].kind = 1, E.PROPOSAL_LAPLACE
    assert propose(v) == -5  # float states only
    v = _valid()
    assert propose(v, dim=0) == -2 and propose(v, dim=105) == -2
    v = _valid(n_temps=257)
    assert propose(v) == -3
    for kind in (E.PROPOSAL_LAPLACE, E.PROPOSAL_UNIFORM_RADIUS, 7, -1):
        v = _valid()
        v["pd"].kind, v["pa"].struct_size = kind, 4
        assert propose(v) == -4, kind
    v = _valid()
    v["pa"].struct_size, v["pa"].chol = 4, None
    assert propose(v) == -6
    v = _valid()
    v["ra"].n_chains, v["pa"].chol = 0, None
    assert propose(v) == 0  # an empty batch never looks at the pointers
    v = _valid()
    v["pa"].chol = None
    assert propose(v) == -1
    v = _valid()
    v["pd"].temp_scale = None
    assert propose(v) == -1
    v = _valid()
    assert propose(v, props=False) == -1 and propose(v, acc=False) == -1
    v["ra"].ext_prop = v["ptr"]
    assert propose(v) == -1  # ext_prop without ext_u
    v = _valid()
    v["ra"].device_step, v["ra"].ext_prop, v["ra"].ext_u = v["ptr"], v["ptr"], v["ptr"]
    assert propose(v) == -5  # device-step mode draws from Philox only
    # the update: NULL; the struct; dim; the arguments; the pointers
    assert lib.ptrwm_precond_update(None, 5, 0, None) == -1
    v = _valid()
    v["up"].struct_size = 4
    assert update(v, dim=0) == -6
    v = _valid()
    v["up"].memory = 0.0
    assert update(v, dim=0) == -2 and update(v, dim=105) == -2
    nan, inf = float("nan"), float("inf")
    for field, bad in (("memory", 0.0), ("memory", 1.5), ("memory", -0.5), ("memory", nan), ("jitter", -1e-9), ("jitter", inf),
                       ("jitter", nan), ("min_count", 0.5), ("min_count", nan), ("windows", 0)):
        v = _valid()
        setattr(v["up"], field, bad)
        v["up"].chol = None
        assert update(v) == -5, (field, bad)
    v = _valid()
    assert update(v, window=-1) == -5 and update(v, window=3) == -5
    for field in ("chol", "sxx", "sx", "count", "run_xx", "run_x", "run_w"):
        v = _valid()
        setattr(v["up"], field, None)
        assert update(v, window=2) == -1, field
    # what passes every check goes on to the launch, which a machine without a GPU cannot make
    import torch
    if not torch.cuda.is_available():
        v = _valid()
        assert propose(v) == -7 and update(v) == -7
