"""Starting points (include/ptrwm.h ptrwm_init_states) without a GPU: the new symbol and the C layout of its ctypes mirror,
every refusal of the entry point before the first HIP call, every constructor ValueError of EngineRun and the two sampler
classes on device="cpu", and the properties of the NumPy restatement (tests/init_reference.py) the GPU tests compare
against.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from host_harness import ROOT, assert_layout, c_layout, valid_args
from init_reference import expected_box_starts

E_NULL, E_DIM, E_TEMPS, E_ARG, E_STRUCT = -1, -2, -3, -5, -6


@pytest.fixture(scope="module")
def engine():
    import ptrwm_hip

    if not os.path.exists(ptrwm_hip.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__

        __graft_entry__.build()
    return ptrwm_hip


def test_the_symbol_exists_and_the_mirror_has_the_c_layout(engine, tmp_path):
    lib = engine.load_library()
    assert "ptrwm_init_states" in engine.SYMBOLS and lib.ptrwm_init_states is not None
    assert lib.ptrwm_abi_version() == 3  # a new symbol, no change to anything that existed
    fs = [f[0] for f in engine.InitArgs._fields_]
    assert fs == ["struct_size", "per_temperature", "attempt", "lo", "hi", "fallback"]
    assert_layout(engine.InitArgs, "ptrwm_init_args", fs, c_layout(tmp_path, {"ptrwm_init_args": fs}))


def _run_args(n_temps=4, n_chains=8):
    """(No pointer of these tests is ever dereferenced: every case is refused, or has nothing to do, before anything is
    enqueued.)"""
    ra = valid_args(n_temps=n_temps)["ra"]
    ra.n_chains = n_chains
    return ra


def _init(attempt=0, per_temperature=0, bounds=True):
    i = valid_args("init")["init"]
    i.attempt, i.per_temperature = attempt, per_temperature
    if not bounds:
        i.lo = i.hi = None
    return i


def test_init_states_refusals_need_no_gpu(engine):
    lib = engine.load_library()
    call = lambda ra, dim, i: lib.ptrwm_init_states(None if ra is None else C.byref(ra), dim,  # noqa: E731
                                                    None if i is None else C.byref(i), None)
    # NULL structs
    assert call(None, 30, _init()) == E_NULL
    assert call(_run_args(), 30, None) == E_NULL
    # struct sizes, either struct
    ra = _run_args()
    ra.struct_size = 8
    assert call(ra, 30, _init()) == E_STRUCT
    i = _init()
    i.struct_size = C.sizeof(engine.InitArgs) - 8
    assert call(_run_args(), 30, i) == E_STRUCT
    # dim and ladder length, as the split steps check them
    for dim in (0, -1, engine.MAX_DIM + 1):
        assert call(_run_args(), dim, _init()) == E_DIM, dim
    for T in (0, -2, engine.MAX_TEMPS + 1):
        assert call(_run_args(n_temps=T), 30, _init()) == E_TEMPS, T
    # attempt and per_temperature ranges
    for attempt in (-1, 65536, 2**20):
        assert call(_run_args(), 30, _init(attempt=attempt)) == E_ARG, attempt
    for pt in (-1, 2):
        assert call(_run_args(), 30, _init(per_temperature=pt)) == E_ARG, pt
    assert call(_run_args(n_chains=-1), 30, _init()) == E_ARG
    ra = _run_args()
    ra.state_f64 = 2
    assert call(ra, 30, _init()) == E_ARG
    # required arrays
    ra = _run_args()
    ra.state = None
    assert call(ra, 30, _init()) == E_NULL
    assert call(_run_args(), 30, _init(bounds=False)) == E_NULL
    for missing in ("lo", "hi"):
        i = _init()
        setattr(i, missing, None)
        assert call(_run_args(), 30, i) == E_NULL, missing
    ra = _run_args()
    ra.logp = None
    assert call(ra, 30, _init(attempt=1)) == E_NULL  # a redraw reads logp ...
    assert call(ra, 30, _init(attempt=65535, bounds=False)) == E_NULL
    # ... and the largest valid attempt / per_temperature values pass the range checks (refused for the NULL logp only)
    # an empty batch is fine, with or without arrays
    for attempt in (0, 3):
        assert call(_run_args(n_chains=0), 30, _init(attempt=attempt, per_temperature=1)) == 0
    ra = _run_args(n_chains=0)
    ra.state = ra.logp = None
    assert call(ra, 104, _init(bounds=False)) == 0


# ---- constructors ---------------------------------------------------------------------------------------------------
def _engine_run(**kw):
    from algorithms._engine_core import EngineRun
    from proposal_distributions import NormalProposal
    from target_distributions import RoughCarpetDistributionTorch

    dim = 5
    args = dict(target_dist=RoughCarpetDistributionTorch(dim, device="cpu"),
                proposal=NormalProposal(dim, 0.5, 1.0, torch.device("cpu"), torch.float32, None).engine_proposal([1.0, 0.5]),
                beta_ladder=[1.0, 0.5], dim=dim, device=torch.device("cpu"), n_replicas=3, initial_state=np.zeros(dim),
                burn_in=0, swap_every=1, swap_mode="exchange", swap_order="sequential", seed=1)
    args.update(kw)
    return EngineRun(**args)


def test_engine_run_checks_its_starts_before_it_asks_for_a_gpu(engine):
    z = np.zeros
    for bad in (z(4), z((2, 5)), z((3, 4)), z((3, 3, 5)), z((3, 2, 4)), z((1, 3, 2, 5)), torch.zeros(3, 5, 2)):
        with pytest.raises(ValueError, match="starting states must have shape"):
            _engine_run(initial_state=bad)
    for box in ((1.0, 0.0), (z(5), -np.ones(5)), (np.array([0, 0, 0, 0, 1.0]), 0.5)):
        with pytest.raises(ValueError, match="lo <= hi"):
            _engine_run(init_box=box)
    for box in ((z(4), 1.0), (0.0, z((5, 1))), (0.0,), 3.0, (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match="init_box"):
            _engine_run(init_box=box)
    for box in ((0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="finite"):
            _engine_run(init_box=box)
    for n in (0, -1, 1.5, True, 65536):
        with pytest.raises(ValueError, match="init_attempts"):
            _engine_run(init_box=(-1.0, 1.0), init_attempts=n)
    # a box draws the starts: per-replica states next to it are a contradiction
    for states in (z((3, 5)), torch.zeros(3, 2, 5)):
        with pytest.raises(ValueError, match="init_box"):
            _engine_run(initial_state=states, init_box=(-1.0, 1.0))
    # good arguments get as far as the device check (there is no CPU path)
    for kw in (dict(), dict(initial_state=z((3, 5))), dict(initial_state=torch.zeros(3, 2, 5)),
               dict(init_box=(-1.0, 1.0)), dict(init_box=(-np.ones(5), 2.0), init_per_temperature=True, init_attempts=1)):
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            _engine_run(**kw)


def test_the_classes_check_the_new_arguments_in_the_constructor(engine):
    from algorithms import ParallelTemperingRWM_GPU_Optimized, RandomWalkMH_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    dim = 5
    target = RoughCarpetDistributionTorch(dim, device="cpu")
    rwm = lambda **kw: RandomWalkMH_GPU_Optimized(dim, 0.5, target, device="cpu", num_chains=6, **kw)  # noqa: E731
    pt = lambda **kw: ParallelTemperingRWM_GPU_Optimized(dim, 0.5, target, beta_ladder=[1.0, 0.5, 0.25], device="cpu",  # noqa: E731
                                                         num_replicas=4, **kw)
    z = np.zeros
    for make, bad_shapes in ((rwm, (z(4), z((5, 5)), z((6, 4)), z((6, 2, 5)))),
                             (pt, (z(6), z((3, 5)), z((4, 2, 5)), z((4, 3, 4)), torch.zeros(3, 4, 5)))):
        for bad in bad_shapes:
            with pytest.raises(ValueError, match="starting states must have shape"):
                make(initial_states=bad)
        with pytest.raises(ValueError, match="lo <= hi"):
            make(init_box=(2.0, 1.0))
        with pytest.raises(ValueError, match="lo <= hi"):
            make(init_box=(z(dim), np.array([1, 1, -1e-3, 1, 1.0])))
        with pytest.raises(ValueError, match="init_box"):
            make(init_box=(z(3), 1.0))
        for n in (0, -3, 2.0):
            with pytest.raises(ValueError, match="init_attempts"):
                make(init_box=(-1.0, 1.0), init_attempts=n)
        with pytest.raises(ValueError, match="exclude each other"):
            make(initial_states=z(dim), init_box=(-1.0, 1.0))
    with pytest.raises(ValueError, match="exclude each other"):
        rwm(initial_states=z((6, dim)), init_box=(-1.0, 1.0))
    with pytest.raises(ValueError, match="exclude each other"):
        pt(initial_states=torch.zeros(4, 3, dim), init_box=(-1.0, 1.0))
    with pytest.raises(ValueError, match="init_per_temperature"):
        pt(init_per_temperature=True)
    with pytest.raises(TypeError):
        rwm(init_per_temperature=True)  # one temperature: the RWM class has no such argument
    # accepted (nothing runs before the first step), and reported
    assert rwm().get_diagnostic_info()["init"] == "point"
    assert rwm(initial_states=z((6, dim))).get_diagnostic_info()["init"] == "states"
    assert rwm(initial_states=torch.zeros(6, 1, dim)).get_diagnostic_info()["init"] == "states"
    assert rwm(init_box=(-20.0, 20.0)).get_diagnostic_info()["init"] == "box"
    assert pt()._init_mode == "point" and pt(initial_states=z((4, dim)))._init_mode == "states"
    assert pt(initial_states=z((4, 3, dim)))._init_mode == "states"
    assert pt(init_box=(-np.ones(dim), np.ones(dim)), init_per_temperature=True, init_attempts=1)._init_mode == "box"
    # one ladder takes the shape of its own current_states, [T, dim]
    one = ParallelTemperingRWM_GPU_Optimized(dim, 0.5, target, beta_ladder=[1.0, 0.5, 0.25], device="cpu",
                                             initial_states=z((3, dim)))
    assert tuple(one._initial_states.shape) == (1, 3, dim)
    # the sampler keeps a copy: the caller's array (an earlier sampler's live states, say) may go on changing
    given = torch.ones(6, dim)
    s = rwm(initial_states=given)
    given.zero_()
    assert torch.equal(s._initial_states, torch.ones(6, dim))


# ---- the restatement ------------------------------------------------------------------------------------------------
BOXES = [(-20.0, 20.0), (-0.1, 1.1), (np.linspace(-3, 2, 7).astype(np.float32), np.linspace(2.5, 9, 7).astype(np.float32))]


@pytest.mark.parametrize("box", range(len(BOXES)))
def test_restated_starts_lie_in_the_box(box):
    lo, hi = BOXES[box]
    x = expected_box_starts(seed=77, chain_offset=3, n_chains=50, n_temps=3, dim=7, lo=lo, hi=hi, attempt=0,
                            per_temperature=True)
    assert x.dtype == np.float32 and x.shape == (50, 3, 7)
    assert np.all(x >= np.float32(lo)) and np.all(x <= np.float32(hi))
    # and fill it: 1 050 uniform draws leave neither tenth of the box empty
    u = (x - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
    assert u.min() < 0.1 and u.max() > 0.9 and abs(u.mean() - 0.5) < 0.05


def test_a_degenerate_box_gives_its_point():
    x = expected_box_starts(seed=1, chain_offset=0, n_chains=4, n_temps=2, dim=5, lo=1.25, hi=1.25)
    assert np.all(x == np.float32(1.25))


def test_restated_ladders_share_or_draw_their_own():
    kw = dict(seed=5, chain_offset=0, n_chains=6, n_temps=4, dim=9, lo=-2.0, hi=3.0)
    shared = expected_box_starts(per_temperature=False, **kw)
    own = expected_box_starts(per_temperature=True, **kw)
    assert np.all(shared == shared[:, :1])
    assert np.array_equal(shared[:, 0], own[:, 0])  # temperature 0 of a ladder's own draws is the shared one
    for t in range(1, 4):
        assert not np.any(np.all(own[:, t] == own[:, 0], axis=-1))
    assert len({r.tobytes() for r in own.reshape(-1, 9)}) == 24  # all rows differ
    assert len({r.tobytes() for r in shared[:, 0]}) == 6  # chains differ


def test_restated_shards_are_slices_of_the_whole():
    kw = dict(seed=2**40 + 17, n_temps=2, dim=6, lo=-1.0, hi=1.0, per_temperature=True)
    whole = expected_box_starts(chain_offset=0, n_chains=40, **kw)
    assert np.array_equal(expected_box_starts(chain_offset=20, n_chains=20, **kw), whole[20:40])
    assert np.array_equal(expected_box_starts(chain_offset=0, n_chains=20, **kw), whole[:20])
    # the high word of the chain id enters the counter
    far = expected_box_starts(chain_offset=2**32, n_chains=40, **kw)
    assert not np.any(np.all(far == whole, axis=-1))


def test_restated_attempts_and_seeds_differ():
    kw = dict(chain_offset=0, n_chains=10, n_temps=1, dim=8, lo=0.0, hi=1.0)
    a = [expected_box_starts(seed=9, attempt=k, **kw) for k in (0, 1, 2, 65535)]
    for i in range(len(a)):
        for j in range(i):
            assert not np.any(np.all(a[i] == a[j], axis=-1))
    assert not np.any(np.all(expected_box_starts(seed=10, **kw) == a[0], axis=-1))
    assert np.array_equal(expected_box_starts(seed=9, attempt=1, **kw), a[1])  # a pure function of its arguments
