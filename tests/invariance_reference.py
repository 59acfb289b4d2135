"""The analytic side of the invariance tests (tests/test_invariance_host.py, tests/test_gpu_invariance.py).

Metropolis moves and exchange swaps each leave prod_t pi^beta_t invariant, and so does every composition of them.  If
every replica (c, t) STARTS from an exact draw of pi^beta_t, the states after any number of steps are, at every rung t,
C iid exact draws of pi^beta_t again - whatever the mixing.  This module supplies, for the families whose tempered law
can be sampled exactly, the two things such a test needs at every beta:

  draw(rng, beta, n)  -> [n, dim] exact draws of pi^beta (fp64)
  pivots(x, beta)     -> values that are iid U(0, 1) under pi^beta (the probability integral transform, coordinate by
                         coordinate, conditionally where the law is not a product), the same shape as x

and `check`, which turns final states into three readings per rung (or per block of neighbouring rungs: the pivots do
not depend on the rung): the Kolmogorov-Smirnov p-value of the pooled pivots against U(0, 1), and the z-scores of the
mean and of the variance of their normal scores.  Under the null every reading has a known law, so the thresholds
(P_MIN, Z_MAX) are probability, not measurement: a KS reading fails with probability 1e-6, a z with 4e-8.

Host only: NumPy / SciPy in fp64.  No torch, no engine.  The target descriptors (`Family.spec`) come from
helpers.spec_from_params, the same folding of class parameters the rest of the suite uses.

Left out: FullRosenbrock (x_i sits in its own link and in the next one, so the chain has no closed-form marginal to sample
from the head down) and the dense-covariance Gaussian (no fused kernel: split steps, which are covered here through a
user-defined density of one of the families below).  Neither has an exact tempered sampler.
"""
from __future__ import annotations

import zlib

import numpy as np
from scipy import special, stats

P_MIN = 1e-6   # every KS p-value must be at least this
Z_MAX = 5.5    # every |z| at most this
POOL_CAP = 1 << 20  # no pooled statistic holds more values than this


def case_seed(name: str) -> int:
    """The seed of a case is the CRC of its name: nothing to tune."""
    return zlib.crc32(name.encode())


def geometric_ladder(T: int, beta_min: float) -> np.ndarray:
    return np.geomspace(1.0, beta_min, T).astype(np.float32) if T > 1 else np.ones(1, np.float32)


def trap(y, x):
    """The trapezoid rule."""
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x)))


class Quad1D:
    """A 1-D law with unnormalised log-density `logf`, tempered by quadrature: p^beta on a fine uniform grid, CDF by the
    trapezoid rule, draws by inverse CDF, pivots by the CDF (both linear in between: the CDF's error is h^2 max|p'| / 8,
    below 1e-7 at the grids used here, far below the 2e-3 a KS over 2^20 values resolves)."""

    def __init__(self, logf, lo, hi, n=1 << 18):
        self.logf, self.x = logf, np.linspace(lo, hi, n)
        self._cdf = {}

    def cdf_table(self, beta):
        key = float(beta)
        if key not in self._cdf:
            lf = key * self.logf(self.x)
            f = np.exp(lf - lf.max())
            c = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]))])
            assert f[0] < 1e-14 * f.max() and f[-1] < 1e-14 * f.max(), "the grid cuts the tempered law's tails"
            self._cdf[key] = c / c[-1]
        return self._cdf[key]

    def cdf(self, x, beta):
        return np.interp(x, self.x, self.cdf_table(beta))

    def ppf(self, u, beta):
        c = self.cdf_table(beta)
        keep = np.concatenate([[True], np.diff(c) > 0])  # strictly increasing abscissae for the inverse
        return np.interp(u, c[keep], self.x[keep])

    def moments(self, beta):
        """Mean and variance of p^beta by the same quadrature."""
        lf = float(beta) * self.logf(self.x)
        f = np.exp(lf - lf.max())
        f /= trap(f, self.x)
        m = trap(self.x * f, self.x)
        return m, trap((self.x - m) ** 2 * f, self.x)


def _mixture_logf(modes, weights):
    m, lw = np.asarray(modes, np.float64), np.log(np.asarray(weights, np.float64))
    return lambda x: special.logsumexp(-0.5 * (np.asarray(x)[..., None] - m) ** 2 + lw, axis=-1)


class Family:
    """name, dim, the descriptor's class and parameters; draw / pivots in subclasses."""

    cls = ""
    bounded = False       # a support with edges (the proposals can leave it)
    swap_control = True   # False: every rung has the same law, swaps are always accepted (Hypercube)

    def __init__(self, name, dim, params):
        self.name, self.dim, self.params = name, dim, params

    def spec(self):
        import helpers as H

        return H.spec_from_params(self.cls, self.dim, self.params)

    def draw(self, rng, beta, n):
        raise NotImplementedError

    def pivots(self, x, beta):
        raise NotImplementedError

    def mean_var(self, beta):
        """Per-coordinate mean and variance of pi^beta, where a test compares accumulated moments with the truth."""
        raise NotImplementedError


class DiagGaussian(Family):
    """N(mu, Sigma / beta), the mean / inverse variance descriptor (MultivariateNormalTorch with a diagonal covariance)."""

    cls = "MultivariateNormalTorch"

    def __init__(self, name, dim, mean=None, var=None):
        self.mu = np.linspace(-1.0, 2.0, dim) if mean is None else np.asarray(mean, np.float64)
        self.var = np.linspace(0.5, 2.0, dim) if var is None else np.asarray(var, np.float64)
        # the descriptor carries fp32 parameters: the law sampled is the law of the ROUNDED parameters
        self.mu, self.var = self.mu.astype(np.float32).astype(np.float64), 1.0 / (1.0 / self.var).astype(np.float32).astype(np.float64)
        lnc = -0.5 * (dim * np.log(2 * np.pi) + np.sum(np.log(self.var)))
        super().__init__(name, dim, {"mean": self.mu, "cov": np.diag(self.var), "log_norm_const": lnc})

    def draw(self, rng, beta, n):
        return self.mu + rng.standard_normal((n, self.dim)) * np.sqrt(self.var / beta)

    def pivots(self, x, beta):
        return special.ndtr((x - self.mu) / np.sqrt(self.var / beta))

    def mean_var(self, beta):
        return self.mu.copy(), self.var / beta


class ScaledGaussian(DiagGaussian):
    """The ScaledMultivariateNormalTorch descriptor: log p = c - 0.5 sum (s_d x_d)^2, so N(0, 1 / (s^2 beta))."""

    cls = "ScaledMultivariateNormalTorch"

    def __init__(self, name, dim):
        s = np.linspace(0.6, 1.7, dim).astype(np.float32).astype(np.float64)
        Family.__init__(self, name, dim, {"scaling_factors": s, "log_norm_const": -0.5 * dim * np.log(2 * np.pi) + np.sum(np.log(s))})
        self.mu, self.var = np.zeros(dim), 1.0 / s ** 2


class IIDGamma(Family):
    """Gamma(k, theta)^beta = Gamma(beta (k - 1) + 1, theta / beta)."""

    cls, bounded = "IIDGammaTorch", True

    def __init__(self, name, dim, shape=2.0, scale=3.0):
        super().__init__(name, dim, {"shape": shape, "scale": scale})
        self.k, self.theta = float(np.float32(shape)), float(np.float32(scale))

    def _law(self, beta):
        return stats.gamma(beta * (self.k - 1) + 1, scale=self.theta / beta)

    def draw(self, rng, beta, n):
        return rng.gamma(beta * (self.k - 1) + 1, self.theta / beta, size=(n, self.dim))

    def pivots(self, x, beta):
        return self._law(beta).cdf(x)

    def mean_var(self, beta):
        law = self._law(beta)
        return np.full(self.dim, law.mean()), np.full(self.dim, law.var())


class IIDBeta(Family):
    """Beta(a, b)^beta = Beta(beta (a - 1) + 1, beta (b - 1) + 1)."""

    cls, bounded = "IIDBetaTorch", True

    def __init__(self, name, dim, alpha=2.0, beta=3.0):
        super().__init__(name, dim, {"alpha": alpha, "beta": beta})
        self.a, self.b = float(np.float32(alpha)), float(np.float32(beta))

    def _ab(self, beta):
        return beta * (self.a - 1) + 1, beta * (self.b - 1) + 1

    def draw(self, rng, beta, n):
        return rng.beta(*self._ab(beta), size=(n, self.dim))

    def pivots(self, x, beta):
        return stats.beta(*self._ab(beta)).cdf(x)

    def mean_var(self, beta):
        law = stats.beta(*self._ab(beta))
        return np.full(self.dim, law.mean()), np.full(self.dim, law.var())


class Hypercube(Family):
    """Uniform on [l, r]^dim at every beta."""

    cls, bounded, swap_control = "HypercubeTorch", True, False

    def __init__(self, name, dim, left=-1.0, right=2.0):
        super().__init__(name, dim, {"left_boundary": left, "right_boundary": right,
                                     "log_uniform_density": -dim * np.log(right - left)})
        self.l, self.r = float(left), float(right)

    def draw(self, rng, beta, n):
        return rng.uniform(self.l, self.r, size=(n, self.dim))

    def pivots(self, x, beta):
        return (x - self.l) / (self.r - self.l)

    def mean_var(self, beta):
        return np.full(self.dim, 0.5 * (self.l + self.r)), np.full(self.dim, (self.r - self.l) ** 2 / 12)


class RoughCarpet(Family):
    """A product of identical three-mode 1-D mixtures p(x s_d) (s_d = 1 without scaling_factors); p^beta by quadrature."""

    cls = "RoughCarpetDistributionTorch"

    def __init__(self, name, dim, modes, weights, scaled=False):
        params = {"modes": np.asarray(modes, np.float32), "weights": np.asarray(weights, np.float32)}
        self.s = np.ones(dim)
        if scaled:
            self.s = np.linspace(0.5, 1.5, dim).astype(np.float32).astype(np.float64)
            params["scaling_factors"] = self.s
        super().__init__(name, dim, params)
        m = params["modes"].astype(np.float64)
        self.modes = m
        # wide enough for beta down to 0.01: the tempered components have standard deviation 1 / sqrt(beta) = 10
        self.law = Quad1D(_mixture_logf(m, params["weights"].astype(np.float64)), m.min() - 120.0, m.max() + 120.0)

    def draw(self, rng, beta, n):
        return self.law.ppf(rng.random((n, self.dim)), beta) / self.s

    def pivots(self, x, beta):
        return self.law.cdf(x * self.s, beta)

    def mean_var(self, beta):
        m, v = self.law.moments(beta)
        return m / self.s, v / self.s ** 2

    def mode_masses(self, beta):
        """Mass of p^beta left of, between and right of the midpoints of neighbouring modes (in the scaled coordinate)."""
        mid = 0.5 * (np.sort(self.modes)[1:] + np.sort(self.modes)[:-1])
        c = self.law.cdf(mid, beta)
        return np.array([c[0], c[1] - c[0], 1.0 - c[1]])


class ThreeMixture(Family):
    """Three unit Gaussians whose means differ in coordinate 0 only: coordinate 0 is the tempered 1-D mixture (quadrature),
    the others N(mu_d, 1 / beta).  general=True: the same law with ip = (0,), which takes the general functor."""

    cls = "ThreeMixtureDistributionTorch"

    def __init__(self, name, dim, general=False, first=(-4.0, 0.5, 5.0), weights=(0.3, 0.45, 0.25)):
        rest = np.linspace(-1.0, 1.0, dim)[1:]
        means = np.tile(np.concatenate([[0.0], rest]), (3, 1))
        means[:, 0] = first
        means = means.astype(np.float32)
        super().__init__(name, dim, {"means": means, "mixing_weights": np.asarray(weights, np.float32)})
        self.general = general
        self.rest = means[0, 1:].astype(np.float64)
        first64 = means[:, 0].astype(np.float64)
        self.law = Quad1D(_mixture_logf(first64, np.asarray(weights, np.float32).astype(np.float64)), first64.min() - 120.0, first64.max() + 120.0)

    def spec(self):
        s = super().spec()
        assert s.ip == (1,)  # helpers.spec_from_params sees means that differ in the first coordinate only
        if self.general:
            s.ip = (0,)
        return s

    def draw(self, rng, beta, n):
        x = np.empty((n, self.dim))
        x[:, 0] = self.law.ppf(rng.random(n), beta)
        x[:, 1:] = self.rest + rng.standard_normal((n, self.dim - 1)) / np.sqrt(beta)
        return x

    def pivots(self, x, beta):
        u = np.empty(x.shape)
        u[..., 0] = self.law.cdf(x[..., 0], beta)
        u[..., 1:] = special.ndtr((x[..., 1:] - self.rest) * np.sqrt(beta))
        return u


class _Rosenbrock(Family):
    """exp(-a (x_head - mu)^2 - b sum (child - parent^2)^2)^beta, sampled from the head down: x_head ~ N(mu, 1 / (2 a beta)),
    every child ~ N(parent^2, 1 / (2 b beta)).  Pivots: the normal CDF of the standardised residuals.
    `links`: (coordinate, parent coordinate or -1, mu) in sampling order."""

    a = b = 1.0
    links = ()

    def draw(self, rng, beta, n):
        x = np.empty((n, self.dim))
        z = rng.standard_normal((n, self.dim))
        for d, parent, mu in self.links:
            if parent < 0:
                x[:, d] = mu + z[:, d] / np.sqrt(2 * self.a * beta)
            else:
                x[:, d] = x[:, parent] ** 2 + z[:, d] / np.sqrt(2 * self.b * beta)
        return x

    def pivots(self, x, beta):
        r = np.empty(x.shape)
        for d, parent, mu in self.links:
            if parent < 0:
                r[..., d] = (x[..., d] - mu) * np.sqrt(2 * self.a * beta)
            else:
                r[..., d] = (x[..., d] - x[..., parent] ** 2) * np.sqrt(2 * self.b * beta)
        return special.ndtr(r)


class EvenRosenbrock(_Rosenbrock):
    cls = "EvenRosenbrockTorch"

    def __init__(self, name, dim, a=0.5, b=2.0):
        assert dim % 2 == 0
        mu = np.linspace(-0.5, 1.0, dim // 2).astype(np.float32)
        super().__init__(name, dim, {"a_coeff": a, "b_coeff": b, "mu": mu})
        self.a, self.b = float(np.float32(a)), float(np.float32(b))
        self.links = tuple(l for i in range(dim // 2) for l in ((2 * i, -1, float(mu[i])), (2 * i + 1, 2 * i, 0.0)))


class HybridRosenbrock(_Rosenbrock):
    cls = "HybridRosenbrockTorch"

    def __init__(self, name, n1, n2, a=0.5, b=2.0, mu=0.7):
        dim = 1 + n2 * (n1 - 1)
        super().__init__(name, dim, {"a_coeff": a, "b_coeff": b, "mu": mu, "n1": n1, "n2": n2})
        self.a, self.b = float(np.float32(a)), float(np.float32(b))
        links = [(0, -1, float(np.float32(mu)))]
        for j in range(n2):
            for k in range(n1 - 1):
                d = 1 + j * (n1 - 1) + k
                links.append((d, 0 if k == 0 else d - 1, 0.0))
        self.links = tuple(links)


class NealFunnel(Family):
    """pi(v, z) = N(v; mu_v, s^2) prod_{d < D - 1} N(z_d; mu_z, e^v).  Tempered: z | v ~ N(mu_z, e^v / beta); integrating z out of
    pi^beta leaves exp(-beta (v - mu_v)^2 / (2 s^2)) e^{-beta (D-1) v / 2} (2 pi e^v / beta)^{(D-1)/2}, i.e. a Gaussian in v of
    variance s^2 / beta and mean mu_v + s^2 (D - 1)(1 - beta) / (2 beta) (tests/test_invariance_host.py confirms it against
    quadrature of the marginal)."""

    cls = "NealFunnelTorch"

    def __init__(self, name, dim, mu_v=0.3, sigma_v_sq=0.1, mu_z=-0.4):
        super().__init__(name, dim, {"mu_v": mu_v, "sigma_v_sq": sigma_v_sq, "mu_z": mu_z})
        self.mu_v, self.s2, self.mu_z = (float(np.float32(v)) for v in (mu_v, sigma_v_sq, mu_z))

    def v_law(self, beta):
        return self.mu_v + self.s2 * (self.dim - 1) * (1 - beta) / (2 * beta), self.s2 / beta

    def draw(self, rng, beta, n):
        m, var = self.v_law(beta)
        x = np.empty((n, self.dim))
        x[:, 0] = m + rng.standard_normal(n) * np.sqrt(var)
        x[:, 1:] = self.mu_z + rng.standard_normal((n, self.dim - 1)) * np.sqrt(np.exp(x[:, :1]) / beta)
        return x

    def pivots(self, x, beta):
        m, var = self.v_law(beta)
        r = np.empty(x.shape)
        r[..., 0] = (x[..., 0] - m) / np.sqrt(var)
        r[..., 1:] = (x[..., 1:] - self.mu_z) / np.sqrt(np.exp(x[..., :1]) / beta)
        return special.ndtr(r)


RC15 = dict(modes=(-15.0, 0.0, 15.0), weights=(0.5, 0.3, 0.2))   # the benchmark target: the folded functor
RC5 = dict(modes=(-5.0, 0.0, 5.0), weights=(0.5, 0.3, 0.2))      # the three-term functor
RC_ASYM = dict(modes=(-15.0, 0.0, 14.0), weights=(0.5, 0.3, 0.2))  # the two-term functor


def family(key: str, dim: int) -> Family:
    """The families by short name (the names the test tables use)."""
    make = {
        "gauss": lambda: DiagGaussian(key, dim),
        "sgauss": lambda: ScaledGaussian(key, dim),
        "gamma": lambda: IIDGamma(key, dim),
        "beta": lambda: IIDBeta(key, dim),
        # Beta(2, 3)^beta is nearly uniform on every hot rung, so a ladder of 8 swaps too freely to control anything: the
        # ladders of 8 use a sharper member of the family
        "beta8": lambda: IIDBeta(key, dim, alpha=8.0, beta=12.0),
        "cube": lambda: Hypercube(key, dim),
        "rc15": lambda: RoughCarpet(key, dim, **RC15),
        "rc15s": lambda: RoughCarpet(key, dim, scaled=True, **RC15),
        "rc5": lambda: RoughCarpet(key, dim, **RC5),
        "rcasym": lambda: RoughCarpet(key, dim, **RC_ASYM),
        "tm1": lambda: ThreeMixture(key, dim),
        "tmgen": lambda: ThreeMixture(key, dim, general=True),
        "even": lambda: EvenRosenbrock(key, dim),
        "hybrid": lambda: HybridRosenbrock(key, 3, (dim - 1) // 2),
        "funnel": lambda: NealFunnel(key, dim),
    }
    return make[key]()


# Per-coordinate standard deviation of the proposal at beta = 1, in units of 2.38 / sqrt(dim): chosen from each
# family's own width (the narrowest direction of its cold law) so that the acceptance rate stays inside [0.05, 0.8] on
# every rung of a ladder down to beta = 0.05; power_conditions asserts that it does, case by case.
BASE_SCALE = {"gauss": 0.8, "sgauss": 0.8, "gamma": 3.0, "beta": 0.06, "beta8": 0.03, "cube": 0.25, "rc15": 1.0, "rc15s": 1.0, "rc5": 1.0,
              "rcasym": 1.0, "tm1": 1.0, "tmgen": 1.0, "even": 0.15, "hybrid": 0.12, "funnel": 0.7}


def proposal_for(fam: Family, kind_name: str, betas):
    """The three proposals at one per-coordinate standard deviation s (at beta = 1): Normal of variance s^2, Laplace of
    variance s^2 per coordinate, a ball of radius s sqrt(dim + 2) (whose coordinates have variance r^2 / (dim + 2))."""
    import helpers as H

    s = BASE_SCALE[fam.name] * 2.38 / np.sqrt(fam.dim)
    return H.proposal_spec(kind_name, fam.dim, betas, base_variance_scalar=s * s,
                           base_variance_vector=np.full(fam.dim, s * s, np.float32),
                           base_radius=s * np.sqrt(fam.dim + 2))


def exact_starts(fam: Family, rng, betas, n_ladders, dtype=np.float32) -> np.ndarray:
    """[C, T, D]: replica (c, t) an exact draw of pi^beta_t.  Drawn in fp64; float32 starts are the rounded draws (a
    perturbation of 6e-8 relative, four orders below what 2^20 values resolve)."""
    return np.stack([fam.draw(rng, float(b), n_ladders) for b in betas], axis=1).astype(dtype)


def setup_case(name, fam: Family, proposal, T, beta_min, n_ladders, dtype=np.float32, ladder_factor=1.0) -> dict:
    """Everything a run of case `name` needs, from the CRC of the name: the ladder, exact starts [C, T, D] for it, the target
    and proposal descriptions and the engine's seed.  ladder_factor != 1 is the wrong-argument control: the ENGINE is
    handed min(1, factor * beta) (and the proposal made for it) while the starts - and the check - keep the true ladder."""
    seed = case_seed(name)
    betas = geometric_ladder(T, beta_min)
    engine_betas = np.minimum(np.float32(1), np.float32(ladder_factor) * betas).astype(np.float32)
    x0 = exact_starts(fam, np.random.default_rng(seed), betas, n_ladders, dtype)
    return dict(name=name, fam=fam, spec=fam.spec(), prop=proposal_for(fam, proposal, engine_betas), betas=betas,
                engine_betas=engine_betas, x0=x0, seed=seed)


def _z_of_tail(lower, upper):
    """The z-score whose normal tails equal the two given tail probabilities (exact null law -> normal scale)."""
    return float(special.ndtri(lower) if lower < 0.5 else -special.ndtri(upper))


def readings(u) -> tuple:
    """(KS p-value, z of the mean, z of the variance) of values that should be iid U(0, 1).  The normal scores are N(0, 1)
    under the null: their mean times sqrt(n) is N(0, 1) exactly and their sum of squares chi^2_n exactly (mapped to the
    normal scale through its own tails, so no large-n approximation enters)."""
    u = np.asarray(u, np.float64).ravel()
    assert u.size <= POOL_CAP, f"a pooled statistic of {u.size} values: more than 2^20"
    n = u.size
    p = float(stats.kstest(u, "uniform").pvalue)
    s = special.ndtri(np.clip(u, 2.0 ** -1000, 1.0 - 2.0 ** -53))
    z_mean = float(s.mean() * np.sqrt(n))
    ss = float(np.sum(s * s))
    z_var = _z_of_tail(stats.chi2.cdf(ss, n), stats.chi2.sf(ss, n))
    return p, z_mean, z_var


def check(x_final, betas, fam: Family, pool: int = 1) -> np.ndarray:
    """x_final [C, T, D] -> [ceil(T / pool), 3]: the readings of every block of `pool` neighbouring rungs (pool = 1: per
    rung), each rung's states turned into pivots with its own beta first."""
    x = np.asarray(x_final, np.float64)
    T = x.shape[1]
    u = [fam.pivots(x[:, t], float(betas[t])) for t in range(T)]
    return np.array([readings(np.concatenate([v.ravel() for v in u[a:a + pool]])) for a in range(0, T, pool)])


def inside(r) -> bool:
    r = np.atleast_2d(r)
    return bool(np.all(r[:, 0] >= P_MIN) and np.all(np.abs(r[:, 1:]) <= Z_MAX))


def describe(r) -> str:
    r = np.atleast_2d(r)
    return f"min p {r[:, 0].min():.3g}, max |z mean| {np.abs(r[:, 1]).max():.2f}, max |z var| {np.abs(r[:, 2]).max():.2f}"


def swap_attempts(n_steps, swap_every, T, order_even_odd: bool, burn_in=0) -> np.ndarray:
    """How often each pair (j, j + 1) was attempted: every event in a sequential sweep; in even/odd order event e (counted from
    0) attempts the pairs with j = e mod 2."""
    ev = max(0, n_steps // swap_every - burn_in // swap_every)
    if not order_even_odd:
        return np.full(T - 1, ev)
    return np.array([(ev + 1) // 2 if j % 2 == 0 else ev // 2 for j in range(T - 1)])


def power_conditions(out, fam: Family, n_steps, swap_every, order_even_odd=False) -> dict:
    """Asserts, from a run's own counters (n_accept, swap_accept [C, T]), that the case has power: acceptance in [0.05, 0.8]
    at every rung, at least 30 accepted moves per replica on average, swap rate in [0.1, 0.9] for every pair (except where
    every rung has the same law).  Returns the rates."""
    Cn, T = out["n_accept"].shape
    acc = out["n_accept"].sum(0) / (Cn * n_steps)
    assert np.all((acc >= 0.05) & (acc <= 0.8)), f"{fam.name}: acceptance rates {np.round(acc, 3)} outside [0.05, 0.8]"
    assert np.all(out["n_accept"].mean(0) >= 30), f"{fam.name}: fewer than 30 accepted moves per replica: {out['n_accept'].mean(0)}"
    res = {"accept": acc}
    if T > 1:
        att = swap_attempts(n_steps, swap_every, T, order_even_odd)
        rate = out["swap_accept"][:, :T - 1].sum(0) / (Cn * att)
        res["swap"] = rate
        if fam.swap_control:
            assert np.all((rate >= 0.1) & (rate <= 0.9)), f"{fam.name}: swap rates {np.round(rate, 3)} outside [0.1, 0.9]"
        else:
            assert np.all(rate > 0.99), f"{fam.name}: every rung has the same law, yet swap rates {np.round(rate, 3)}"
    return res
