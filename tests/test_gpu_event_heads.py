"""A swap event of the kernels that park their Philox heads in LDS leaves the heads alone (csrc/kernel.h event_keeps_heads):
in a one-wavefront exchange group whose sweep is decided by the walk, the event publishes beside the heads and the rows
travel through the lanes (ds_bpermute) instead of the slab; every other event keeps the slab exchange and stores the heads
again behind it.  The lane index those kernels carry across the step loop (lane_index_carried) serves the head slot, the
squared-jump slot and the event's slots.

As tests/test_gpu_swap_walk.py: the PRODUCTION thread-form kernel in Philox mode equals its fixture twin bit for bit - states,
log-densities and all four statistics - and the twin follows the oracle decision for decision (helpers.check_parity_philox).
The twin keeps the plain Philox block and the slab exchange, so a head touched by an event, or a row fetched from the wrong
lane, is a byte that differs.  Needs an MI355X (`-m gpu`).
"""
import numpy as np
import pytest

import helpers as H
import ptrwm_hip as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu

f32 = np.float32
DIM, SEED = 30, 0xE7E27BEAD5
KEYS = ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")
RATIO = 0.01 ** (1.0 / 31.0)  # neighbouring temperatures of the headline ladder (32 rungs from 1 to 0.01)

# name: (ladders, temperatures, swap_every, steps, swap order)
CASES = {
    # an event in every step, two ladders per wavefront, a second wavefront half empty: a head damaged by an event is used
    # by the very next step
    "every_step": (3, 32, 1, 12, "sequential"),
    # the shape of the launch-cut test below
    "T32": (3, 32, 3, 10, "sequential"),
    # full words: one ladder per wavefront, the last pair's source lane is lane 63
    "T64": (3, 64, 2, 10, "sequential"),
    # 32 ladders per wavefront, and a second wavefront with one live ladder: 62 lanes shadow position 0 of ladder 0
    "T2": (33, 2, 1, 10, "sequential"),
    # three ladders per wavefront, lane 63 idle; the second wavefront holds one ladder and two dead ones
    "T21": (4, 21, 3, 10, "sequential"),
    # a ladder longer than a wavefront: the slab exchange, the heads stored again behind it
    "T65_wide": (2, 65, 3, 10, "sequential"),
    # no event at all
    "no_event": (3, 32, 20, 10, "sequential"),
    # not the walk: the slab exchange, the heads stored again behind it
    "even_odd": (3, 32, 2, 10, "even_odd"),
}


def _ladder(T):
    return (RATIO ** np.arange(T)).astype(f32)


def _rough_carpet():
    return H.spec_from_params("RoughCarpetDistributionTorch", DIM, {"modes": [-15.0, 0.0, 15.0], "weights": [0.5, 0.3, 0.2]})


def start_states(Cn, T, scale=3.0):
    return (np.random.default_rng(1000 * DIM + 100 * Cn + T).standard_normal((Cn, T, DIM)) * scale).astype(f32)


def attempts_of(Cn, T, se, N, order):
    """Pairs attempted by the events behind steps se, 2 se, .. <= N of a run from step 0 without burn-in."""
    events = N // se
    if order == "sequential":
        return events * Cn * (T - 1)
    return Cn * sum(len(range(n & 1, T - 1, 2)) for n in range(events))  # event n: the pairs (j, j + 1) with j = n (mod 2)


def _inputs(device, spec, Cn, T, scale=3.0):
    beta = _ladder(T)
    prop = H.proposal_spec("Normal", DIM, beta, base_variance_scalar=2.38**2 / DIM)
    x = start_states(Cn, T, scale)
    lp = E.logdensity(spec.engine(device), H.dev_t(x.reshape(-1, DIM), device)).cpu().numpy().reshape(Cn, T)
    return prop, beta, x, lp


def _thread_form(spec, prop, device, **kw):
    """The production kernel (no trace, no flags) of the one-thread-per-replica form."""
    with E.kernel_form(E.FORM_THREAD), E.stream_mode(E.STREAM_OFF):
        out = H.gpu_run(spec, prop, device, **kw)
        assert E.last_launch_kind() == E.LAUNCH_THREAD
    return out


def _same_bits(a, b, what, rows=slice(None)):
    for k in KEYS:
        x, y = a[k][rows], b[k]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, H.first_mismatch(x, y))


def _production_equals_twin_which_follows_oracle(device, spec, what, Cn, T, se, N, order, scale=3.0):
    prop, beta, x, lp = _inputs(device, spec, Cn, T, scale)
    kw = dict(state=x, logp=lp, beta=beta, n_steps=N, step0=0, burn_in=0, swap_every=se, seed=SEED, chain_offset=0,
              swap_mode=E.SWAP_MODES["exchange"], swap_order=E.SWAP_ORDERS[order])
    prod = _thread_form(spec, prop, device, **kw)
    with E.kernel_form(E.FORM_THREAD), E.stream_mode(E.STREAM_OFF):
        twin = H.gpu_runner(spec, prop, device)(**kw)
        _same_bits(prod, twin, what)
        attempts, accepted = attempts_of(Cn, T, se, N, order), int(prod["swap_accept"].sum())
        print(f"{what}: {accepted} of {attempts} swaps accepted, {int(prod['n_accept'].sum())} moves")
        if attempts:
            assert 0 < accepted < attempts, "swaps all accepted or all refused: the case tests half of the exchange"
        else:
            assert accepted == 0
        assert prod["n_accept"].sum() > 0
        kw.pop("seed")
        H.check_parity_philox(H.gpu_runner(spec, prop, device), spec, prop, seed=SEED, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_production_kernel_equals_its_fixture_twin_which_follows_the_oracle(device, name):
    Cn, T, se, N, order = CASES[name]
    _production_equals_twin_which_follows_oracle(device, _rough_carpet(), name, Cn, T, se, N, order)


@pytest.mark.parametrize("key", ["even_d30", "tm15_d30"])
def test_two_more_targets(device, key):
    """The change reaches the dim-30 Normal-proposal kernel of every target: EvenRosenbrock and ThreeMixture."""
    _production_equals_twin_which_follows_oracle(device, H.target_spec(key), key, 3, 32, 2, 10, "sequential", scale=1.0)


def test_two_launches_of_five_steps_equal_one_of_ten(device):
    """Events behind steps 3, 6 and 9; cut behind step 5.  The prologue's store of the heads is the only one there is: each
    launch derives them from its own step0, and no event touches them."""
    Cn, T, se, N, order = CASES["T32"]
    spec = _rough_carpet()
    prop, beta, x, lp = _inputs(device, spec, Cn, T)
    kw = dict(beta=beta, burn_in=0, swap_every=se, seed=SEED, chain_offset=0, swap_mode=E.SWAP_MODES["exchange"],
              swap_order=E.SWAP_ORDERS[order])
    whole = _thread_form(spec, prop, device, state=x, logp=lp, n_steps=N, step0=0, **kw)
    a = _thread_form(spec, prop, device, state=x, logp=lp, n_steps=5, step0=0, **kw)
    b = _thread_form(spec, prop, device, state=a["state"], logp=a["logp"], n_steps=5, step0=5, **kw)
    for k in ("state", "logp"):
        assert b[k].tobytes() == whole[k].tobytes(), (k, H.first_mismatch(b[k], whole[k]))
    for k in ("n_accept", "swap_accept"):
        assert np.array_equal(a[k] + b[k], whole[k]), k
    assert a["swap_accept"].sum() > 0 and b["swap_accept"].sum() > 0
    assert np.array_equal(np.maximum(a["last_swap_ordinal"], b["last_swap_ordinal"]), whole["last_swap_ordinal"])
    # (each launch sums its squared jumps from zero in fp64 and adds the sum to the caller's: one rounding of a double apart)
    np.testing.assert_allclose(a["sq_jump"] + b["sq_jump"], whole["sq_jump"], rtol=1e-12, atol=0)


def literal_ladder_inputs():
    """Hypercube (0, 1)^30, two ladders of four temperatures - one wavefront.  Ladder 0 lies inside the support; the hotter
    replicas of ladder 1 lie outside it and, with increments of ~0.03 per dimension, stay there: they enter every event with
    a log-density of -inf, so ladder 1 takes the literal rule (which refuses every pair that has such a replica) while ladder
    0 takes the threshold form."""
    spec = H.spec_from_params("HypercubeTorch", DIM, {"left_boundary": 0.0, "right_boundary": 1.0, "log_uniform_density": 0.0})
    T = 4
    beta = f32([1.0, 0.6, 0.3, 0.1])
    prop = H.proposal_spec("Normal", DIM, beta, base_variance_scalar=1e-4)
    st = np.clip(0.5 + 0.1 * np.random.default_rng(30).standard_normal((2, T, DIM)), 0.2, 0.8).astype(f32)
    st[1, 1:, 0] = -1.0 - 0.1 * np.arange(T - 1)  # ladder 1: all but the cold replica outside the cube
    lp = O.logdensity(spec.oracle(), st.reshape(-1, DIM)).astype(f32).reshape(2, T)
    return spec, prop, beta, st, lp


def test_a_literal_ladder_and_a_plain_one_in_one_wavefront_equal_themselves_alone(device):
    """The wavefront runs the walk's general loop, in which each lane asks its own ladder's question, and the rows of both
    ladders travel through the lanes.  Each ladder gets, bit for bit, the results it gets as the only ladder of the launch."""
    spec, prop, beta, st, lp = literal_ladder_inputs()
    N, T = 10, len(beta)
    assert np.isneginf(lp[1, 1:]).all() and np.isfinite(lp[0]).all() and np.isfinite(lp[1, 0])
    kw = dict(beta=beta, n_steps=N, step0=0, burn_in=0, swap_every=1, seed=77)
    both = _thread_form(spec, prop, device, state=st, logp=lp, chain_offset=1, **kw)
    for c in range(2):
        alone = _thread_form(spec, prop, device, state=st[c:c + 1], logp=lp[c:c + 1], chain_offset=1 + c, **kw)
        _same_bits(both, alone, f"ladder {c}", rows=slice(c, c + 1))
    accepted, attempts = int(both["swap_accept"].sum()), 2 * N * (T - 1)
    print(f"literal beside plain: {accepted} of {attempts} swaps accepted")
    assert 0 < accepted < attempts and both["swap_accept"][0].sum() > 0 and both["swap_accept"][1].sum() == 0
    assert np.isneginf(both["logp"][1, 1:]).all() and both["n_accept"][0].sum() > 0 and both["n_accept"][1, 0] > 0
