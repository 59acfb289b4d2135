"""The folded rough-carpet kernels (csrc/targets.h RoughCarpetSym, csrc/capi.hip rough_carpet_fold) change no bit.

Every case runs the production path (in-kernel Philox) in both forms of the fused kernel, thread and lane-split, pinned,
and is compared bit for bit with tests/golden/rc_fold_base.npz, recorded by tests/golden/generate_rc_fold.py on the build
before the folded form existed.  The cases cover parameter sets the fold takes (the benchmark target, equal weights,
modes given out of order, a -0 middle mode, scaled axes, +-m just above the margin, +-inf / NaN starting coordinates)
and sets it must refuse (+-m just below the margin, a far mode too heavy for the fold but not for the two-term form,
asymmetric modes).  The starting states hold coordinates at +-0, near 0, at the midpoints, at the modes and beyond 1e19.  The log-density carried by the
run must also equal the stand-alone (three-term) ptrwm_logdensity of the final states wherever they are finite.
Each run also asserts which functor the dispatch picked (ptrwm_last_launch_functor).  The run tests need an MI355X
(`-m gpu`).
"""
import os

import numpy as np
import pytest

import helpers as H
import ptrwm_hip as E

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rc_fold_base.npz")
DIM, N_STEPS, SWAP_EVERY, SEED = 30, 200, 5, 20261016

GEN, TWO, FOLD = E.FUNCTOR_GENERAL, E.FUNCTOR_SPECIALISED, E.FUNCTOR_FOLDED
# name: (modes, weights, scaled axes, temperatures, ladders, functor the dispatch must pick)
CASES = {
    "bench": ([-15.0, 0.0, 15.0], [0.5, 0.3, 0.2], False, 32, 32, FOLD),
    "equal": ([-15.0, 0.0, 15.0], [1 / 3, 1 / 3, 1 / 3], False, 8, 32, FOLD),
    "order": ([0.0, 15.0, -15.0], [0.3, 0.2, 0.5], False, 8, 32, FOLD),
    "negzero": ([15.0, -0.0, -15.0], [0.2, 0.3, 0.5], False, 8, 32, FOLD),
    "scaled": ([-15.0, 0.0, 15.0], [0.5, 0.3, 0.2], True, 8, 32, FOLD),
    "above": ([-6.2, 0.0, 6.2], [1 / 3, 1 / 3, 1 / 3], False, 8, 32, FOLD),
    "below": ([-6.05, 0.0, 6.05], [1 / 3, 1 / 3, 1 / 3], False, 8, 32, GEN),
    "heavyfar": ([-8.0, 0.0, 8.0], [0.999998, 1e-6, 1e-6], False, 8, 32, TWO),
    "asym": ([-15.0, 0.0, 14.0], [0.5, 0.3, 0.2], False, 8, 32, TWO),
    "rwm": ([-15.0, 0.0, 15.0], [0.5, 0.3, 0.2], False, 1, 256, FOLD),
    "special": ([-15.0, 0.0, 15.0], [0.5, 0.3, 0.2], False, 8, 32, FOLD),  # +-inf / NaN starting coordinates
}


def fold_eligible(modes, weights):
    """Python restatement of csrc/capi.hip rough_carpet_fold (the two-term proof is asserted separately)."""
    m = np.asarray(modes, f32)
    lw = np.log(np.asarray(weights, f32)).astype(f32).astype(np.float64)
    z = [i for i in range(3) if m[i] == 0]
    if not z:
        return False
    i, j = (z[0] + 1) % 3, (z[0] + 2) % 3
    if m[i] == 0 or m[i] != -m[j]:
        return False
    neg, pos = (i, j) if m[i] < 0 else (j, i)
    l2e, mm = 1.4426950408889634, float(m[pos])
    a_neg, a_mid, a_pos = l2e * (lw[neg] - 0.5 * mm * mm), l2e * lw[z[0]], l2e * (lw[pos] - 0.5 * mm * mm)
    return max(a_mid, a_pos) - a_neg > 27 and max(a_mid, a_neg) - a_pos > 27


def case_spec(name):
    modes, weights, scaled, _, _, _ = CASES[name]
    params = {"modes": modes, "weights": weights}
    if scaled:
        params["scaling_factors"] = np.random.default_rng(7).uniform(0.5, 1.5, DIM).astype(f32)
    return H.spec_from_params("RoughCarpetDistributionTorch", DIM, params)


def case_inputs(name):
    """Starting states [C, T, D] with special coordinates, the geometric ladder and the proposal."""
    _, _, _, T, C, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = (rng.standard_normal((C, T, DIM)) * 10).astype(f32)
    special = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-7, -1e-7, 7.5, -7.5, 15.0, -15.0, 3.1, -3.1, 3e19, -3e19], f32)
    for c in range(0, C, 3):  # every third ladder: specials on some coordinates of some replicas
        for t in range(0, T, 2):
            idx = rng.choice(DIM, size=4, replace=False)
            x[c, t, idx] = rng.choice(special[:12], size=4)
    x[1, 0, 5] = special[12]  # replicas beyond 1e19: a square overflows, the log-density is -inf (NaN in the loop)
    x[C - 1, T - 1, 17] = special[13]
    if name == "special":
        # +-inf and NaN coordinates: the log-density is -inf / NaN, in the loop both forms give NaN and the Metropolis
        # test rejects every move of such a replica (targets.h rc_fold_dim_term)
        for c, t, d, v in ((0, 1, 3, np.inf), (2, 3, 0, -np.inf), (4, 5, 29, np.nan), (7, 7, 11, np.inf),
                           (9, 2, 8, np.nan), (11, 6, 20, -np.inf)):
            x[c, t, d] = v
    beta = np.geomspace(1.0, 0.01, T).astype(f32) if T > 1 else np.ones(1, f32)
    prop = H.proposal_spec("Normal", DIM, beta, base_variance_scalar=2.38**2 / DIM)
    return x, beta, prop


def run_case(name, device, form):
    """The production run of a case with the kernel form pinned: numpy state, logp, n_accept, swap_accept, and which
    kernel form and functor the dispatch used."""
    spec = case_spec(name)
    x, beta, prop = case_inputs(name)
    lp0 = E.logdensity(spec.engine(device), H.dev_t(x.reshape(-1, DIM), device)).cpu().numpy().reshape(x.shape[:2])
    with E.kernel_form(form):
        out = H.gpu_run(spec, prop, device, state=x, logp=lp0, beta=beta, n_steps=N_STEPS, step0=0,
                        swap_every=SWAP_EVERY, seed=SEED)
    res = {k: out[k] for k in ("state", "logp", "n_accept", "swap_accept")}
    res["launch"] = (E.last_launch_kind(), E.last_launch_functor())
    return res


def test_case_table_matches_the_host_rule():
    # the table says which cases the dispatch must fold; the Python restatement of the rule agrees (no GPU needed)
    for name, (modes, weights, _, _, _, functor) in CASES.items():
        assert fold_eligible(modes, weights) == (functor == FOLD), name


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("name", list(CASES))
def test_rough_carpet_runs_match_the_recorded_bits(device, name, form):
    gold = np.load(GOLDEN)
    got = run_case(name, device, {"thread": E.FORM_THREAD, "quad": E.FORM_QUAD}[form])
    # the kernel the dispatch picked: the pinned form and the case's functor
    assert got.pop("launch") == ({"thread": E.LAUNCH_THREAD, "quad": E.LAUNCH_QUAD}[form], CASES[name][5]), name
    for k, v in got.items():
        want = gold[f"{name}/{k}"]
        assert v.shape == want.shape, (name, k)
        assert v.tobytes() == want.tobytes(), (name, form, k, H.first_mismatch(v, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bench", "order", "scaled", "below", "heavyfar"])
def test_in_loop_logp_equals_stand_alone_logdensity(device, name):
    spec = case_spec(name)
    got = run_case(name, device, E.FORM_THREAD)
    x = got["state"].reshape(-1, DIM)
    ref = E.logdensity(spec.engine(device), H.dev_t(x, device)).cpu().numpy()
    lp = got["logp"].reshape(-1)
    fin = np.all(np.isfinite(x) & (np.abs(x) < 1e19), axis=1)
    assert fin.sum() > 0.9 * len(fin)
    assert lp[fin].tobytes() == ref[fin].tobytes(), H.first_mismatch(lp[fin], ref[fin])
    # the replicas started beyond 1e19 never accept a move (NaN log-densities) and keep their -inf
    assert np.all(np.isneginf(lp[~fin])), lp[~fin]
    assert got["n_accept"].sum() > 0


@pytest.mark.gpu
def test_infinite_and_nan_starting_states_stay_rejected(device):
    got = run_case("special", device, E.FORM_THREAD)
    x0, _, _ = case_inputs("special")
    x, lp = got["state"].reshape(-1, DIM), got["logp"].reshape(-1)
    bad0 = ~np.all(np.isfinite(x0.reshape(-1, DIM)), axis=1)
    # a replica that starts with an infinite or NaN coordinate keeps it: every proposal from it is rejected (swaps may
    # move it to another temperature, with its log-density)
    bad = ~np.all(np.isfinite(x), axis=1)
    assert bad.sum() == bad0.sum() == 6
    assert np.all(~np.isfinite(lp[bad]))
    assert np.all(np.isfinite(lp[~bad & np.all(np.abs(x) < 1e19, axis=1)]))
