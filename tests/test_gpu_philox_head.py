"""The production step kernel that parks the heads of its Philox blocks in LDS (csrc/philox_head.h, csrc/kernel.h
philox_heads_in_lds: thread form, width 30 compiled in, Normal proposal) draws the same words as the plain block.

Every case runs RoughCarpet with modes -15, 0, +15 at dim 30 - the headline kernel - in Philox mode and ties the PRODUCTION
kernel to the oracle in the two links of helpers.check_production_run: (1) its final states, log-densities and all four
statistics equal, bit for bit, those of its fixture twin on the same stream - the twin keeps the plain ten-round block, so
one wrong head word, one head read from another thread's slot or a head not restored behind a swap event shows in the
first step that uses it; (2) the twin follows the oracle's restatement of the counter layout decision for decision over the
whole horizon (helpers.check_parity_philox, as test_gpu_engine_parity.test_philox_mode_vs_oracle).  The cases are the paths
on which the heads are written, overwritten and restored.  Needs an MI355X (`-m gpu`).
"""
import numpy as np
import pytest

import helpers as H
import ptrwm_hip as E

pytestmark = pytest.mark.gpu

f32 = np.float32
DIM, SEED = 30, 0xC0FFEE1234
KEYS = ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")

# name: (ladders, temperatures, swap_every, steps, swap order, chain_offset, step0)
CASES = {
    # two waves of two ladders, the second half empty; swap events behind steps 3, 6 and 9: three restores
    "narrow": (3, 32, 3, 10, "sequential", 0, 0),
    "even_odd": (3, 32, 3, 10, "even_odd", 0, 0),
    # a ladder longer than a wave: the exchange group is a workgroup of two waves, a wave's heads lie over rows that the
    # other one reads and writes (the two extra barriers of a swap event)
    "wide": (2, 65, 3, 10, "sequential", 0, 0),
    # no swap events at all: the heads of the prologue serve the whole launch; two waves, the second with six live lanes
    "rwm": (70, 1, 3, 10, "sequential", 0, 0),
    # the chain id's high word (a part of c3, i.e. of every head)
    "chain_hi": (3, 32, 3, 10, "sequential", 2**32 + 5, 0),
    # the step index's high word (a part of c0, i.e. of every head) turns on four steps into the request
    "step_hi": (3, 32, 3, 8, "sequential", 0, 2**32 - 4),
}


def _inputs(device, Cn, T):
    spec = H.spec_from_params("RoughCarpetDistributionTorch", DIM, {"modes": [-15.0, 0.0, 15.0], "weights": [0.5, 0.3, 0.2]})
    beta = np.geomspace(1.0, 0.01, T).astype(f32) if T > 1 else np.ones(1, f32)
    prop = H.proposal_spec("Normal", DIM, beta, base_variance_scalar=2.38**2 / DIM)
    x = (np.random.default_rng(100 * Cn + T).standard_normal((Cn, T, DIM)) * 3).astype(f32)
    lp = E.logdensity(spec.engine(device), H.dev_t(x.reshape(-1, DIM), device)).cpu().numpy().reshape(Cn, T)
    return spec, prop, beta, x, lp


def _production(spec, prop, device, **kw):
    """The production kernel (no trace, no flags), thread form pinned, and which kernel the dispatch took."""
    with E.kernel_form(E.FORM_THREAD), E.stream_mode(E.STREAM_OFF):
        out = H.gpu_run(spec, prop, device, **kw)
        assert (E.last_launch_kind(), E.last_launch_functor()) == (E.LAUNCH_THREAD, E.FUNCTOR_FOLDED)
    return out


def _same_bits(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k, H.first_mismatch(a[k], b[k]))


@pytest.mark.parametrize("name", list(CASES))
def test_production_kernel_equals_its_fixture_twin_which_follows_the_oracle(device, name):
    Cn, T, se, N, order, chain_offset, step0 = CASES[name]
    spec, prop, beta, x, lp = _inputs(device, Cn, T)
    kw = dict(state=x, logp=lp, beta=beta, n_steps=N, step0=step0, burn_in=0, swap_every=se, seed=SEED, chain_offset=chain_offset,
              swap_mode=E.SWAP_MODES["exchange"], swap_order=E.SWAP_ORDERS[order])
    prod = _production(spec, prop, device, **kw)
    with E.kernel_form(E.FORM_THREAD), E.stream_mode(E.STREAM_OFF):
        twin = H.gpu_runner(spec, prop, device)(**kw)
        _same_bits(prod, twin, name)
        assert prod["n_accept"].sum() > 0 and (T == 1 or prod["swap_accept"].sum() > 0), "nothing moved: the case tests nothing"
        kw.pop("seed")
        H.check_parity_philox(H.gpu_runner(spec, prop, device), spec, prop, seed=SEED, **kw)


def test_launches_of_four_and_six_steps_equal_one_of_ten(device):
    """The heads are derived again at the start of every launch, from that launch's step0: the cut is invisible."""
    Cn, T, se, N, order, chain_offset, step0 = CASES["narrow"]
    spec, prop, beta, x, lp = _inputs(device, Cn, T)
    kw = dict(beta=beta, burn_in=0, swap_every=se, seed=SEED, chain_offset=chain_offset, swap_mode=E.SWAP_MODES["exchange"],
              swap_order=E.SWAP_ORDERS[order])
    whole = _production(spec, prop, device, state=x, logp=lp, n_steps=N, step0=step0, **kw)
    a = _production(spec, prop, device, state=x, logp=lp, n_steps=4, step0=step0, **kw)
    b = _production(spec, prop, device, state=a["state"], logp=a["logp"], n_steps=6, step0=step0 + 4, **kw)
    for k in ("state", "logp"):
        assert b[k].tobytes() == whole[k].tobytes(), (k, H.first_mismatch(b[k], whole[k]))
    for k in ("n_accept", "swap_accept"):
        assert np.array_equal(a[k] + b[k], whole[k]), k
    assert np.array_equal(np.maximum(a["last_swap_ordinal"], b["last_swap_ordinal"]), whole["last_swap_ordinal"])
    # (each launch sums its squared jumps from zero in fp64 and adds the sum to the caller's: one rounding of a double apart)
    np.testing.assert_allclose(a["sq_jump"] + b["sq_jump"], whole["sq_jump"], rtol=1e-12, atol=0)
