"""The sequential exchange sweep of the step kernel's one-wavefront exchange groups, decided with lane masks and a scalar
walk (csrc/swap_walk.h, csrc/kernel.h swap_walk_decide), makes the decisions of the sequential scan.

As tests/test_gpu_philox_head.py: the PRODUCTION kernel in Philox mode equals its fixture twin bit for bit - states,
log-densities and all four statistics - and the twin follows the oracle decision for decision over the whole horizon
(helpers.check_parity_philox).  The cases are the shapes of a wavefront the walk can get wrong: ladders that fill it, that
leave lanes idle, a second wavefront with one live ladder, one ladder per wavefront, and the ladder longer than a wavefront
that keeps the scan.  Then sweeps forced by external randoms to accept everything and to refuse everything, and a ladder that
must take the literal rule next to one that takes the threshold form.  Needs an MI355X (`-m gpu`).
"""
import numpy as np
import pytest

import helpers as H
import ptrwm_hip as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 0x5EA1C0DE77
KEYS = ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_swap_ordinal")
RATIO = 0.01 ** (1.0 / 31.0)  # neighbouring temperatures of the headline ladder (32 rungs from 1 to 0.01)

# name: (dim, ladders, temperatures, swap_every, steps)
CASES = {
    # the headline kernel (dim 30 compiled in): two wavefronts of two ladders, the second half empty
    "d30_T32": (30, 3, 32, 3, 10),
    # one ladder per wavefront: the walk's words are full, the last pair's bit is bit 63
    "d30_T64": (30, 3, 64, 2, 10),
    # 32 ladders per wavefront, and a second wavefront with one live ladder
    "d30_T2": (30, 33, 2, 1, 10),
    # 21 ladders per wavefront, lane 63 idle; the second wavefront holds one ladder
    "d30_T3": (30, 22, 3, 2, 10),
    # three ladders per wavefront, lane 63 idle; the second wavefront holds one ladder and two dead ones
    "d30_T21": (30, 4, 21, 3, 10),
    # a generic-width kernel (run-time dim): eight ladders per wavefront and one more
    "d5_T8": (5, 9, 8, 2, 10),
    # a ladder longer than a wavefront: the workgroup is the exchange group and keeps the scan
    "d30_T65": (30, 2, 65, 3, 10),
}


def _ladder(T):
    return (RATIO ** np.arange(T)).astype(f32)


def _inputs(device, dim, Cn, T, scale=3.0):
    modes = [-15.0, 0.0, 15.0] if dim == 30 else [-4.0, 0.0, 4.0]
    spec = H.spec_from_params("RoughCarpetDistributionTorch", dim, {"modes": modes, "weights": [0.5, 0.3, 0.2]})
    beta = _ladder(T)
    prop = H.proposal_spec("Normal", dim, beta, base_variance_scalar=2.38**2 / dim)
    x = (np.random.default_rng(1000 * dim + 100 * Cn + T).standard_normal((Cn, T, dim)) * scale).astype(f32)
    lp = E.logdensity(spec.engine(device), H.dev_t(x.reshape(-1, dim), device)).cpu().numpy().reshape(Cn, T)
    return spec, prop, beta, x, lp


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


@pytest.mark.parametrize("name", list(CASES))
def test_production_kernel_equals_its_fixture_twin_which_follows_the_oracle(device, name):
    dim, Cn, T, se, N = CASES[name]
    spec, prop, beta, x, lp = _inputs(device, dim, Cn, T)
    kw = dict(state=x, logp=lp, beta=beta, n_steps=N, step0=0, burn_in=0, swap_every=se, seed=SEED, chain_offset=0,
              swap_mode=E.SWAP_MODES["exchange"], swap_order=E.SWAP_ORDERS["sequential"])
    prod = _thread_form(spec, prop, device, **kw)
    with E.kernel_form(E.FORM_THREAD), E.stream_mode(E.STREAM_OFF):
        twin = H.gpu_runner(spec, prop, device)(**kw)
        _same_bits(prod, twin, name)
        attempts = (N // se) * Cn * (T - 1)
        accepted = int(prod["swap_accept"].sum())
        print(f"{name}: {accepted} of {attempts} swaps accepted")
        assert 0 < accepted < attempts, "swaps all accepted or all refused: the case tests half of the walk"
        assert np.all(prod["swap_accept"][:, T - 1] == 0)
        kw.pop("seed")
        H.check_parity_philox(H.gpu_runner(spec, prop, device), spec, prop, seed=SEED, **kw)


@pytest.mark.parametrize("T,Cn", [(32, 3), (21, 4)])
def test_sweeps_forced_to_accept_everything_and_to_refuse_everything(device, T, Cn):
    """External randoms, one swap event, nothing else (zero increments, accept uniforms of 2).  Uniforms of 1e-30: every
    ladder takes the threshold form and every pair accepts - the state of position 0 travels to the top, every other one
    moves down one position.  Uniforms of exactly 1: every ladder takes the literal rule, which never accepts 1 - nothing
    moves.  Both equal the oracle's run."""
    dim = 30
    spec, prop, beta, x, lp = _inputs(device, dim, Cn, T, scale=1.0)
    for u, moved in ((1e-30, True), (1.0, False)):
        kw = dict(state=x, logp=lp, beta=beta, step0=0, n_steps=1, burn_in=0, swap_every=1, ext_prop=np.zeros((1, Cn, T, dim), f32),
                  ext_u=np.full((1, Cn, T), 2.0, f32), ext_swap_u=np.full((1, Cn, T - 1), u, f32))
        want = O.run(spec.oracle(), prop.oracle(), seed=3, **{**kw, "state": x.copy(), "logp": lp.copy()})
        with E.kernel_form(E.FORM_THREAD), E.stream_mode(E.STREAM_OFF):
            got = H.gpu_run(spec, prop, device, seed=3, **kw)
        for k in ("state", "swap_accept", "last_swap_ordinal"):
            assert np.array_equal(got[k], want[k]), (u, k)
        expect = np.zeros((Cn, T), np.int64)
        expect[:, : T - 1] = 1 if moved else 0
        assert np.array_equal(got["swap_accept"], expect), u
        assert np.array_equal(got["state"], np.roll(x, -1, axis=1) if moved else x), u
        # (a zero increment re-evaluates the log-density in the kernel: the caller's value to rounding)
        np.testing.assert_allclose(got["logp"], np.roll(lp, -1, axis=1) if moved else lp, rtol=1e-5, atol=1e-4)


def test_a_literal_ladder_and_a_plain_one_in_one_wavefront_equal_themselves_alone(device):
    """Two ladders in one wavefront: one inside the support (threshold form), one whose hotter replicas enter every event of
    its first steps with a log-density of -inf (the literal rule: the wavefront runs the loop in which each lane asks its own
    ladder's question).  Each gets, bit for bit, the results it gets when it is the only ladder of the launch."""
    spec = H.target_spec("gamma_d5")
    D, T, N = 5, 4, 10
    beta = f32([1.0, 0.6, 0.3, 0.1])
    prop = H.proposal_spec("Laplace", D, beta, base_variance_vector=np.full(D, 0.5))
    rng = np.random.default_rng(11)
    st = (5 + 0.5 * rng.standard_normal((2, T, D))).astype(f32)
    st[1, 1:, 0] = -1.0 - 0.1 * np.arange(T - 1)  # ladder 1: all but the cold replica outside (0, inf)
    lp = O.logdensity(spec.oracle(), st.reshape(-1, D)).astype(f32).reshape(2, T)
    assert np.isneginf(lp[1, 1:]).all() and np.isfinite(lp[0]).all() and np.isfinite(lp[1, 0])
    kw = dict(beta=beta, n_steps=N, step0=0, burn_in=0, swap_every=1, seed=77)
    both = _thread_form(spec, prop, device, state=st, logp=lp, chain_offset=1, **kw)
    for c in range(2):
        alone = _thread_form(spec, prop, device, state=st[c:c + 1], logp=lp[c:c + 1], chain_offset=1 + c, **kw)
        _same_bits(both, alone, f"ladder {c}", rows=slice(c, c + 1))
    assert 0 < both["swap_accept"][0].sum() < N * (T - 1) and both["n_accept"][1].sum() > 0
