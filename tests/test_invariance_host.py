"""The invariance harness (tests/invariance_reference.py) proven on the CPU, against the oracle.

1. The analytic side checks itself: the exact starts pass their own statistics, and every closed form agrees with direct
   quadrature of pi^beta taken from the ORACLE's log-density of the descriptor the engines are handed (so a parameter
   convention misread in the reference - scale for rate, variance for precision - fails here).
2. The oracle in exchange mode, started from exact draws, is inside the thresholds (p >= 1e-6, |z| <= 5.5) for every
   family, both swap orders and every proposal, with the power conditions holding.
3. Two wrong engines are outside them, at the same thresholds and sizes: swap_mode="reference_copy" (a row copy, not
   invariant by construction) and an engine handed a ladder 10 % off the one the starts were drawn for.

Sizes: 8 192 ladders, 4 rungs geometric in beta from 1 to 0.1, dim 4 (3 - 5 where the family fixes it), 300 steps, a swap
event every 2 steps.  The ladders are independent, so a run is cut into chunks with their own chain_offset and the chunks
run on a few threads (ctypes releases the GIL): the same Philox words, the same result as one call.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import invariance_reference as R
from oracle import oracle as O

C, T, BETA_MIN, DIM, N, SE = 8192, 4, 0.1, 4, 300, 2
FAMILIES = ["gauss", "sgauss", "gamma", "beta", "cube", "rc15", "rc15s", "rc5", "rcasym", "tm1", "tmgen", "even", "hybrid",
            "funnel"]
ORDERS = {"sequential": O.ORDER_SEQUENTIAL, "even_odd": O.ORDER_EVEN_ODD}
_POOL = ThreadPoolExecutor(min(8, os.cpu_count() or 1))


def oracle_run(case, n_steps, swap_every, mode=O.SWAP_EXCHANGE, order=O.ORDER_SEQUENTIAL, chunks=8):
    """The oracle's Philox mode over the case's ladders; float64 starts select its state_f64 path."""
    x0 = case["x0"]
    Cn, Tn, D = x0.shape
    spec, prop = case["spec"].oracle(), case["prop"].oracle()
    lp0 = O.logdensity(spec, x0.reshape(-1, D), "f64" if x0.dtype == np.float64 else "f32").astype(np.float32).reshape(Cn, Tn)
    edges = np.linspace(0, Cn, chunks + 1).astype(int)

    def one(i):
        a, b = int(edges[i]), int(edges[i + 1])
        return O.run(spec, prop, state=x0[a:b], logp=lp0[a:b], beta=case["engine_betas"], step0=0, n_steps=n_steps,
                     swap_every=swap_every, swap_mode=mode, swap_order=order, seed=case["seed"], chain_offset=a)

    parts = list(_POOL.map(one, range(chunks)))
    return {k: np.concatenate([p[k] for p in parts]) for k in ("state", "logp", "n_accept", "swap_accept")}


def run_and_read(name, fkey, proposal, order, mode=O.SWAP_EXCHANGE, dtype=np.float32, ladder_factor=1.0, n_ladders=C):
    fam = R.family(fkey, DIM)
    case = R.setup_case(name, fam, proposal, T, BETA_MIN, n_ladders, dtype=dtype, ladder_factor=ladder_factor)
    out = oracle_run(case, N, SE, mode=mode, order=ORDERS[order])
    assert out["state"].dtype == dtype
    rates = R.power_conditions(out, fam, N, SE, order == "even_odd")
    r = R.check(out["state"], case["betas"], fam)
    print(f"{name}: {R.describe(r)}; acceptance {np.round(rates['accept'], 2)}, swaps {np.round(rates.get('swap', []), 2)}")
    return r


# ------------------------------------------------------------------------------------------------------------------
# 1. the analytic side
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fkey", FAMILIES)
def test_exact_starts_pass_their_own_statistics(fkey):
    fam = R.family(fkey, DIM)
    case = R.setup_case(f"starts-{fkey}", fam, "Normal", T, BETA_MIN, C)
    assert case["x0"].shape == (C, T, fam.dim) and case["x0"].dtype == np.float32
    r = R.check(case["x0"], case["betas"], fam)
    assert R.inside(r), R.describe(r)
    lp = O.logdensity(case["spec"].oracle(), case["x0"].reshape(-1, fam.dim), "f64")
    assert np.all(np.isfinite(lp))  # every start is inside the support


def _oracle_cdf_1d(fam, beta, grid):
    """CDF of pi^beta of a 1-D family on `grid`, by the trapezoid rule on the oracle's own fp64 log-density."""
    lp = beta * O.logdensity(fam.spec().oracle(), grid.reshape(-1, 1).astype(np.float64), "f64")
    f = np.where(np.isfinite(lp), np.exp(lp - lp[np.isfinite(lp)].max()), 0.0)
    c = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(grid))])
    return c / c[-1]


# (family, grid of its one coordinate): the grid covers pi^beta down to beta = 0.05 with negligible tails
GRIDS_1D = {"gauss": (-40, 40), "sgauss": (-60, 60), "gamma": (0, 1500), "beta": (0, 1), "cube": (-1, 2), "rc15": (-90, 90),
            "rc15s": (-200, 200), "rc5": (-80, 80), "rcasym": (-90, 90), "tm1": (-80, 80), "tmgen": (-80, 80)}


@pytest.mark.parametrize("fkey", list(GRIDS_1D))
def test_closed_forms_agree_with_quadrature_of_the_oracle_density(fkey):
    # (float64 points go to the oracle as given.  Tolerance: 1e-6 for the trapezoid rule's h^2 error on the smooth part, plus
    # the mass of the first and the last cell, which bounds the rule's error where the tempered Gamma / Beta density has an
    # infinite slope or a jump at the edge of its support: 1.4e-5 at worst here, two orders below what 2^20 samples resolve)
    fam = R.family(fkey, 1)
    grid = np.linspace(*GRIDS_1D[fkey], (1 << 20) + 1)
    for beta in (1.0, 0.3, 0.05):
        want = _oracle_cdf_1d(fam, beta, grid)
        got = fam.pivots(grid.reshape(-1, 1), beta).ravel()
        tol = 1e-6 + max(got[1] - got[0], got[-1] - got[-2])
        assert tol < 2e-5 and np.max(np.abs(got - want)) < tol, (fkey, beta, np.max(np.abs(got - want)), tol)
        # ... and the sampler inverts the same CDF: its draws are uniform under the quadrature CDF
        u = np.interp(fam.draw(np.random.default_rng(R.case_seed(f"quad-{fkey}-{beta}")), beta, 1 << 16).ravel(), grid, want)
        assert R.inside(R.readings(u)), (fkey, beta, R.readings(u))
        if fkey in ("gauss", "gamma", "beta", "cube", "rc5"):
            m, v = fam.mean_var(beta)
            pdf = np.gradient(want, grid)
            qm = R.trap(grid * pdf, grid)
            assert abs(qm - m[0]) < 1e-4 * np.sqrt(v[0]) and abs(R.trap((grid - qm) ** 2 * pdf, grid) - v[0]) < 1e-4 * v[0]


@pytest.mark.parametrize("fkey", ["even", "hybrid"])
def test_rosenbrock_pivots_are_uniform_under_2d_quadrature(fkey):
    """dim 2 (head and one child): under pi^beta, by quadrature of the oracle's density on a 2-D grid, the pivots (u0, u1) have
    the first and second moments of two independent uniforms."""
    fam = R.EvenRosenbrock("even", 2) if fkey == "even" else R.HybridRosenbrock("hybrid", 2, 1)
    assert fam.dim == 2
    for beta in (1.0, 0.1):
        sd0, sd1 = 1 / np.sqrt(2 * fam.a * beta), 1 / np.sqrt(2 * fam.b * beta)
        mu = fam.links[0][2]
        x0 = np.linspace(mu - 9 * sd0, mu + 9 * sd0, 1201)
        r1 = np.linspace(-9 * sd1, 9 * sd1, 1201)  # the child on a grid around parent^2 (a shear: unit Jacobian)
        X0, R1 = np.meshgrid(x0, r1, indexing="ij")
        pts = np.stack([X0.ravel(), X0.ravel() ** 2 + R1.ravel()], axis=1)
        lp = beta * O.logdensity(fam.spec().oracle(), pts, "f64")
        w = np.exp(lp - lp.max())
        w /= w.sum()
        u = fam.pivots(pts, beta)
        for val, want in ((u[:, 0], 1 / 2), (u[:, 1], 1 / 2), (u[:, 0] ** 2, 1 / 3), (u[:, 1] ** 2, 1 / 3), (u[:, 0] * u[:, 1], 1 / 4)):
            assert abs(np.sum(w * val) - want) < 1e-6, (fkey, beta)


@pytest.mark.parametrize("dim", [2, 3])
def test_funnel_marginal_of_v_agrees_with_quadrature(dim):
    """v is Gaussian under pi^beta with variance s^2 / beta and mean mu_v + s^2 (D - 1)(1 - beta) / (2 beta): the marginal,
    by integrating the oracle's density over z numerically (for every v, on a grid scaled by the conditional width
    e^{v/2} / sqrt(beta)), has that density."""
    fam = R.NealFunnel("funnel", dim)
    spec = fam.spec().oracle()
    for beta in (1.0, 0.4, 0.1):
        m, var = fam.v_law(beta)
        v = np.linspace(m - 9 * np.sqrt(var), m + 9 * np.sqrt(var), 241)
        r = np.linspace(-9, 9, 121)
        mesh = np.meshgrid(v, *([r] * (dim - 1)), indexing="ij")
        width = np.exp(mesh[0] / 2) / np.sqrt(beta)
        pts = np.stack([mesh[0]] + [fam.mu_z + g * width for g in mesh[1:]], axis=-1).reshape(-1, dim)
        lp = (beta * O.logdensity(spec, pts, "f64")).reshape(mesh[0].shape)
        f = np.exp(lp - lp.max()) * width ** (dim - 1)  # dz = width dr
        marg = f.sum(axis=tuple(range(1, dim)))
        # the z-integral of a Gaussian by the trapezoid rule at a step of 0.15 widths is exact to rounding, so the marginal
        # is known POINTWISE: its ratio to the stated Gaussian density is one constant over the +-6 sd that matter
        ratio = np.log(marg) + 0.5 * (v - m) ** 2 / var
        core = np.abs(v - m) <= 6 * np.sqrt(var)
        assert np.ptp(ratio[core]) < 1e-8, (dim, beta, np.ptp(ratio[core]))


def test_statistics_reject_small_distortions_of_uniform():
    """The readings have the power the tests lean on: 2^17 uniforms pass; scaled about 1/2 by 1.03 (a law 3 % too wide) or
    shifted by 0.01 they fail."""
    u = np.random.default_rng(R.case_seed("readings")).random(1 << 17)
    assert R.inside(R.readings(u))
    assert not R.inside(R.readings(np.clip(0.5 + 1.03 * (u - 0.5), 0, 1)))
    assert not R.inside(R.readings(np.clip(u + 0.01, 0, 1)))
    with pytest.raises(AssertionError):
        R.readings(np.zeros((1 << 20) + 1))


# ------------------------------------------------------------------------------------------------------------------
# 2. the oracle, exchange mode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("fkey", FAMILIES)
def test_oracle_exchange_leaves_every_family_invariant(fkey, order):
    r = run_and_read(f"oracle-{fkey}-Normal-{order}", fkey, "Normal", order)
    assert R.inside(r), R.describe(r)


@pytest.mark.parametrize("proposal", ["Laplace", "UniformRadius"])
@pytest.mark.parametrize("fkey", ["gauss", "gamma", "beta", "rc5", "cube", "even"])
def test_oracle_exchange_with_the_other_proposals(fkey, proposal):
    r = run_and_read(f"oracle-{fkey}-{proposal}-sequential", fkey, proposal, "sequential")
    assert R.inside(r), R.describe(r)


@pytest.mark.parametrize("proposal", ["Normal", "Laplace", "UniformRadius"])
@pytest.mark.parametrize("fkey", ["gauss", "gamma", "rc15"])
def test_oracle_exchange_with_double_states(fkey, proposal):
    r = run_and_read(f"oracle-f64-{fkey}-{proposal}", fkey, proposal, "sequential", dtype=np.float64)
    assert R.inside(r), R.describe(r)


# ------------------------------------------------------------------------------------------------------------------
# 3. negative controls: the same thresholds must reject two wrong engines
# ------------------------------------------------------------------------------------------------------------------
C_CONTROL = 4 * C  # a control that only just fails is a weak test: at this size both fail by orders of magnitude


def _worst(r):
    """(smallest p, largest |z|) over the rungs."""
    return float(r[:, 0].min()), float(np.abs(r[:, 1:]).max())


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("fkey", ["gauss", "gamma", "rc15"])
def test_reference_copy_is_rejected(fkey, order):
    """swap_mode="reference_copy" copies the hotter row over the colder one: not an exchange, not invariant.  Measured here
    (32 768 ladders; smallest p over the rungs, largest |z| of the mean, of the variance):
      gauss  sequential  7e-30,   1.5,  35.2        gauss  even_odd  7e-8,  2.5,  13.0
      gamma  sequential  0,     124.9,  off scale   gamma  even_odd  0,    69.0,  off scale
      rc15   sequential  0,      99.5,  off scale   rc15   even_odd  0,    97.1,  29.8
    (at 8 192 ladders the Gaussian even/odd case fails by |z| 5.9 only: hence the larger size.)
    """
    r = run_and_read(f"control-copy-{fkey}-{order}", fkey, "Normal", order, mode=O.SWAP_REFERENCE_COPY, n_ladders=C_CONTROL)
    p, z = _worst(r)
    assert not R.inside(r)
    assert p < 1e-12 or z > 11, (p, z)  # by orders of magnitude, not by a hair


def test_a_ladder_ten_percent_off_is_rejected():
    """The engine is handed min(1, 1.1 beta_t) while the starts were drawn for beta_t: exchange mode then keeps the WRONG laws
    invariant and the states drift to them: narrower by 10 % in variance on every rung but the coldest.  Measured here:
    at 32 768 ladders, smallest p 6e-20, z of the variance -22 to -25 on the three hotter rungs (-11 to -12 at 8 192 ladders).
    """
    r = run_and_read("control-ladder-gauss", "gauss", "Normal", "sequential", ladder_factor=1.1, n_ladders=C_CONTROL)
    assert R.inside(r[:1]), R.describe(r[:1])  # the coldest rung keeps beta = 1: still exact
    assert np.all(r[1:, 2] < -2 * R.Z_MAX), r[1:, 2]  # every other rung: variance far too small
