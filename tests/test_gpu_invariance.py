"""Every form of the step kernel leaves the tempered targets invariant (the analytic side: tests/invariance_reference.py).

Every replica (c, t) starts from an exact draw of pi^beta_t; the kernel runs N steps with exchange swaps on its own Philox
stream; the final states at rung t must again be C iid exact draws of pi^beta_t.  The readings (Kolmogorov-Smirnov p of the
pooled pivots, z of the mean and of the variance of their normal scores) are held to p >= 1e-6 and |z| <= 5.5: probability,
not measurement.  Every case's seed is the CRC of its name, and every case asserts from the run's own counters that it has
power: acceptance in [0.05, 0.8] on every rung, >= 30 accepted moves per replica, swap rates in [0.1, 0.9].

One case per path: the one-thread-per-replica form at narrow dims for every family, proposal and swap order; the headline
kernel (RoughCarpet dim 30, folded functor, parked Philox heads) and its sibling functors; every ladder shape the exchange
code branches on (T = 2, 5, 64, 65, 128 / 130, 256); the lane-split form; double states; the streaming form; launch cuts
(bit-identical); split steps through the class, eager and captured; the drop-in classes with the ladder and scales they
derive; the moment and histogram accumulators against the analytic truth; and the negative controls (reference_copy, a
ladder 10 % off), which the same thresholds must reject.  The pinned form and the functor are asserted from
ptrwm_last_launch_kind / ptrwm_last_launch_functor.

Wide ladders: neighbouring rungs are close, so a swap rate below 0.9 needs many dimensions and a long ladder in log beta;
those cases use the Gaussian at dim 64 and take beta down to where the rate condition holds (the Gaussian is scale-free).
Under the invariant law the rungs of a ladder are independent, and the pivots do not depend on the rung: the statistics of
a wide ladder pool blocks of neighbouring rungs.  The lane-split form serves ladders of at most 128 rungs, so its widest
case is T = 128; T = 130 and 256 run in the thread form.
"""
import numpy as np
import pytest
import torch

import invariance_reference as R
import ptrwm_hip as E

N_STEPS = 300
THREAD, QUAD, AUTO = E.FORM_THREAD, E.FORM_QUAD, E.FORM_AUTO
GEN, SPEC, FOLD = E.FUNCTOR_GENERAL, E.FUNCTOR_SPECIALISED, E.FUNCTOR_FOLDED
FUNCTOR = {"rc15": FOLD, "rc15s": FOLD, "rc5": GEN, "rcasym": SPEC, "tm1": SPEC, "tmgen": GEN}
ALL = ["gauss", "sgauss", "gamma", "beta", "cube", "rc15", "rc15s", "rc5", "rcasym", "tm1", "tmgen", "even", "hybrid", "funnel"]


def case(group, fkey, dim, T, beta_min, C, proposal="Normal", order="sequential", form=THREAD, se=3, pool=1, f64=False,
         mode="exchange", ladder_factor=1.0):
    name = f"{group}-{fkey}-d{dim}-T{T}-{proposal}-{order}" + {THREAD: "", QUAD: "-lanesplit", AUTO: "-auto"}[form]
    return dict(name=name, group=group, fkey=fkey, dim=dim, T=T, beta_min=beta_min, C=C, proposal=proposal, order=order,
                form=form, se=se, pool=pool, f64=f64, mode=mode, ladder_factor=ladder_factor)


CASES = []
# --- thread form, narrow: every family at T = 4 and T = 8, both swap orders (the funnel's law moves fast with beta, and
# the Hypercube's not at all while the proposals widen: both stop at beta = 0.1;
# Beta(2, 3) is nearly uniform on every hot rung, so the ladders of 8 take the sharper Beta(8, 12)) ---
for f in ALL:
    for order in ("sequential", "even_odd"):
        CASES.append(case("thread", f, 5 if f in ("hybrid", "funnel") else 4, 4, 0.1, 32768, se=2, order=order))
        CASES.append(case("thread", "beta8" if f == "beta" else f, 5 if f == "funnel" else 8, 8, 0.1 if f in ("funnel", "cube") else 0.05, 32768,
                          order=order))
for f in ("gauss", "gamma", "beta8", "rc5"):
    for p in ("Laplace", "UniformRadius"):
        CASES.append(case("thread", f, 6, 8, 0.05, 32768, proposal=p))
# --- the headline kernel: RoughCarpet dim 30 (an exact dim: parked Philox heads), and its sibling functors ---
CASES += [case("headline", "rc15", 30, 8, 0.05, 8192, se=5), case("headline", "rc15", 30, 32, 0.05, 2048, se=5, pool=4),
          case("headline", "rc15", 30, 8, 0.05, 8192, se=5, order="even_odd"),
          case("headline", "rc15s", 30, 8, 0.05, 8192, se=5), case("headline", "rcasym", 30, 8, 0.05, 8192, se=5),
          case("headline", "rc5", 30, 8, 0.05, 8192, se=5)]
# --- ladder shapes the exchange code branches on ---
CASES += [case("ladder", "gauss", 4, 2, 0.3, 32768, se=2), case("ladder", "gauss", 4, 2, 0.3, 32768, se=2, order="even_odd"),
          case("ladder", "gauss", 8, 5, 0.05, 32768), case("ladder", "rc5", 8, 5, 0.05, 32768, order="even_odd"),
          case("ladder", "gauss", 64, 64, 0.05, 1024, pool=8), case("ladder", "gauss", 64, 64, 0.05, 1024, pool=8, order="even_odd"),
          case("ladder", "gauss", 64, 65, 0.05, 1024, pool=13), case("ladder", "gauss", 64, 65, 0.05, 1024, pool=13, form=QUAD),
          case("ladder", "gauss", 64, 130, 0.005, 512, pool=26), case("ladder", "gauss", 64, 130, 0.005, 512, pool=26, order="even_odd"),
          case("ladder", "gauss", 64, 128, 0.005, 512, pool=16, form=QUAD),
          case("ladder", "gauss", 64, 256, 1e-5, 256, pool=32), case("ladder", "gauss", 64, 256, 1e-5, 256, pool=32, order="even_odd")]
# --- the lane-split form, pinned (dim 70: the only form there); longer ladders at larger dims keep the swap rates up ---
for d, T, C in ((7, 8, 32768), (30, 8, 8192), (41, 12, 8192), (70, 16, 4096)):
    CASES += [case("quad", "gauss", d, T, 0.05, C, form=QUAD if d <= 64 else AUTO),
              case("quad", "rc15", d, T, 0.05, C, form=QUAD if d <= 64 else AUTO, order="even_odd")]
CASES += [case("quad", "gauss", 41, 12, 0.05, 8192, proposal=p, form=QUAD) for p in ("Laplace", "UniformRadius")]
# --- double states ---
CASES += [case("f64", f, 6, 8, 0.05, 32768, proposal=p, form=AUTO, f64=True)
          for f in ("gauss", "gamma", "rc15") for p in ("Normal", "Laplace", "UniformRadius")]
# --- negative controls: the same thresholds must reject them ---
CONTROLS = [case("control", "gauss", 4, 4, 0.1, 32768, se=2, mode="reference_copy"),
            case("control", "gamma", 4, 4, 0.1, 32768, se=2, mode="reference_copy", form=QUAD),
            case("control", "rc15", 4, 4, 0.1, 32768, se=2, mode="reference_copy", form=QUAD, order="even_odd"),
            case("control", "gauss", 4, 4, 0.1, 32768, se=2, ladder_factor=1.1)]
for c in CONTROLS:
    c["name"] += f"-{c['mode']}-x{c['ladder_factor']}"


def setup(c):
    fam = R.family(c["fkey"], c["dim"])
    s = R.setup_case("gpu-" + c["name"], fam, c["proposal"], c["T"], c["beta_min"], c["C"],
                     dtype=np.float64 if c["f64"] else np.float32, ladder_factor=c["ladder_factor"])
    assert s["x0"].shape[0] * fam.dim * c["pool"] <= R.POOL_CAP
    return s


def engine_run(s, device, *, n_steps, se, mode="exchange", order="sequential", cuts=None):
    """The production path (in-kernel Philox) from the case's exact starts, as one launch or as the launches `cuts`.
    Returns numpy state / logp / counters, and the kernel form and functor of every launch."""
    x0 = s["x0"]
    Cn, T, D = x0.shape
    tgt, prop = s["spec"].engine(device), s["prop"].engine(device)
    st = torch.tensor(x0, device=device)
    lp = E.logdensity(tgt, st.view(-1, D).float()).view(Cn, T).contiguous()
    assert bool(torch.isfinite(lp).all())
    stats = {k: torch.zeros(Cn, T, dtype=dt, device=device) for k, dt in
             (("n_accept", torch.int64), ("sq_jump", torch.float64), ("swap_accept", torch.int64), ("last_swap_ordinal", torch.int64))}
    plan = E.RunPlan(tgt, prop, state=st, logp=lp, beta=torch.tensor(s["engine_betas"], device=device), burn_in=0, swap_every=se,
                     swap_mode=E.SWAP_MODES[mode], swap_order=E.SWAP_ORDERS[order], seed=s["seed"], **stats)
    launches, s0 = [], 0
    for n in (cuts or (n_steps,)):
        plan.launch(s0, n)
        launches.append((E.last_launch_kind(), E.last_launch_functor()))
        s0 += n
    assert s0 == n_steps
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in stats.items()}
    out["state"], out["logp"], out["launches"] = st.cpu().numpy(), lp.cpu().numpy(), launches
    return out


def expected_kind(c):
    return E.LAUNCH_QUAD if (c["form"] == QUAD or c["f64"] or c["dim"] > 64) else E.LAUNCH_THREAD


def read(c, s, out, n_steps=N_STEPS):
    """Power conditions from the run's counters, then the readings per block of rungs (printed before anything is asserted)."""
    rates = R.power_conditions(out, s["fam"], n_steps, c["se"], c["order"] == "even_odd")
    r = R.check(out["state"], s["betas"], s["fam"], pool=c["pool"])
    print(f"READINGS {c['name']}: {R.describe(r)}; acceptance {rates['accept'].min():.2f}..{rates['accept'].max():.2f}"
          + (f", swaps {rates['swap'].min():.2f}..{rates['swap'].max():.2f}" if "swap" in rates else ""))
    return r


def run_case(c, device):
    s = setup(c)
    with E.kernel_form(c["form"]):
        out = engine_run(s, device, n_steps=N_STEPS, se=c["se"], mode=c["mode"], order=c["order"])
    assert out["state"].dtype == (np.float64 if c["f64"] else np.float32)
    assert [k for k, _ in out["launches"]] == [expected_kind(c)], (c["name"], out["launches"])
    if c["fkey"] in FUNCTOR:
        # (the folded tables hold no state_f64 kernels: double states of a foldable carpet run the two-term functor, capi.hip)
        want = SPEC if (c["f64"] and FUNCTOR[c["fkey"]] == FOLD) else FUNCTOR[c["fkey"]]
        assert out["launches"][0][1] == want, (c["name"], out["launches"])
    return s, out


def test_case_names_are_unique_and_sizes_within_the_cap():
    names = [c["name"] for c in CASES + CONTROLS]
    assert len(set(names)) == len(names)
    for c in CASES + CONTROLS:
        fam_dim = R.family(c["fkey"], c["dim"]).dim
        assert c["C"] * fam_dim * c["pool"] <= R.POOL_CAP, c["name"]
        assert c["C"] == 32768 or c["dim"] > 8 or c["T"] > 8, c["name"]  # 32 768 ladders wherever dim <= 8


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_kernel_leaves_the_tempered_laws_invariant(device, c):
    s, out = run_case(c, device)
    r = read(c, s, out)
    assert R.inside(r), R.describe(r)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CONTROLS, ids=[c["name"] for c in CONTROLS])
def test_wrong_engines_are_rejected(device, c):
    """reference_copy (a row copy, not an exchange) in both kernel forms, and a ladder 10 % off: the harness has power at the
    sizes it runs."""
    s, out = run_case(c, device)
    r = read(c, s, out)
    assert not R.inside(r), R.describe(r)
    assert r[:, 0].min() < 1e-12 or np.abs(r[:, 1:]).max() > 2 * R.Z_MAX, R.describe(r)  # and not by a hair


@pytest.mark.gpu
def test_streaming_form_leaves_the_headline_target_invariant(device):
    """One-step launches with the streaming form pinned (STREAM_ON, thread form): every launch is the streaming kernel."""
    c = case("stream", "rc15", 30, 32, 0.05, 2048, se=5, pool=4)
    s = setup(c)
    with E.kernel_form(THREAD), E.stream_mode(E.STREAM_ON):
        out = engine_run(s, device, n_steps=N_STEPS, se=c["se"], cuts=(1,) * N_STEPS)
    assert out["launches"] == [(E.LAUNCH_STREAM, FOLD)] * N_STEPS
    r = read(c, s, out)
    assert R.inside(r), R.describe(r)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [THREAD, QUAD], ids=["thread", "quad"])
def test_launch_cuts_change_no_bit_and_keep_the_law(device, form):
    """Launches of 1, 7, 64 and the rest give the final state of the single launch bit for bit (and so its readings)."""
    c = case("cuts", "rc15", 30, 8, 0.05, 8192, se=5, form=form)
    s = setup(c)
    with E.kernel_form(form), E.stream_mode(E.STREAM_OFF):
        one = engine_run(s, device, n_steps=N_STEPS, se=c["se"])
        cut = engine_run(s, device, n_steps=N_STEPS, se=c["se"], cuts=(1, 7, 64, N_STEPS - 72))
    assert [k for k, _ in cut["launches"]] == [expected_kind(c)] * 4
    for k in ("state", "logp", "n_accept", "sq_jump", "swap_accept", "last_swap_ordinal"):
        assert one[k].tobytes() == cut[k].tobytes(), k
    r = read(c, s, cut)
    assert R.inside(r), R.describe(r)


# ----------------------------------------------------------------------------------------------------------------------
# through the classes
# ----------------------------------------------------------------------------------------------------------------------
def _class_out(alg):
    run = alg._run
    torch.cuda.synchronize()
    st = run.state.cpu().numpy()
    return {"state": st, "n_accept": run.n_accept.cpu().numpy(), "swap_accept": run.swap_accept.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_split_steps_through_the_class(device, graph):
    """A user-defined density in plain torch (as examples/custom_target.py), chosen to be the diagonal Gaussian of the
    reference module: split steps, eager and under the captured graph, from exact starts passed as initial_states."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from interfaces import TorchTargetDistribution

    c = case("split-graph" if graph else "split-eager", "gauss", 4, 4, 0.1, 32768, se=2)
    s = setup(c)
    fam = s["fam"]

    class UserGaussian(TorchTargetDistribution):
        def __init__(self, dim, device):
            super().__init__(dim, device)
            self.mu = torch.tensor(fam.mu, device=device, dtype=torch.float32)
            self.prec = torch.tensor(1.0 / fam.var, device=device, dtype=torch.float32)

        def get_name(self):
            return "UserGaussian"

        def log_density(self, x):
            x = torch.as_tensor(x, device=self.device, dtype=torch.float32)
            return -0.5 * (((x - self.mu) ** 2) * self.prec).sum(-1)

        def density(self, x):
            return torch.exp(self.log_density(x))

    var = (R.BASE_SCALE["gauss"] * 2.38) ** 2 / fam.dim
    alg = ParallelTemperingRWM_GPU_Optimized(fam.dim, var, UserGaussian(fam.dim, device), beta_ladder=[float(b) for b in s["betas"]],
                                             swap_every=c["se"], burn_in=0, device=device, num_replicas=c["C"], seed=s["seed"],
                                             trace="none", initial_states=s["x0"])
    alg._ensure_started()
    assert alg._run.density_fn is not None  # split steps
    alg._run.use_graph = graph
    alg._advance(N_STEPS)
    out = _class_out(alg)
    r = read(c, s, out)
    assert R.inside(r), R.describe(r)


@pytest.mark.gpu
def test_pt_class_with_its_own_ladder_and_scales(device):
    """ParallelTemperingRWM_GPU_Optimized with default arguments (exchange, sequential, the ladder 1, 1/2, ... 0.01 it builds, the
    proposal scales it derives from `var`): exact starts for ITS ladder in, current_states out."""
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    c = case("class-pt", "rc5", 4, 8, 0.01, 32768, se=3)
    fam = R.family("rc5", 4)
    target = RoughCarpetDistributionTorch(4, device=device, mode_centers=list(R.RC5["modes"]), mode_weights=list(R.RC5["weights"]))
    mk = lambda x0: ParallelTemperingRWM_GPU_Optimized(4, 2.38 ** 2 / 4, target, geom_temp_spacing=True, swap_every=c["se"], device=device,  # noqa: E731
                                                       num_replicas=c["C"], seed=R.case_seed(c["name"]), trace="none", initial_states=x0)
    betas = np.asarray(mk(None).beta_ladder, np.float32)
    assert len(betas) == 8 and betas[0] == 1 and betas[-1] == np.float32(0.01)
    x0 = R.exact_starts(fam, np.random.default_rng(R.case_seed(c["name"])), betas, c["C"])
    alg = mk(x0)
    alg._advance(N_STEPS)
    assert E.last_launch_functor() == GEN
    s = dict(fam=fam, betas=betas)
    out = _class_out(alg)
    assert np.array_equal(out["state"], alg.current_states.cpu().numpy())
    r = read(c, s, out)
    assert R.inside(r), R.describe(r)


@pytest.mark.gpu
def test_rwm_class_from_exact_starts(device):
    from algorithms import RandomWalkMH_GPU_Optimized
    from target_distributions import IIDGammaTorch

    c = case("class-rwm", "gamma", 4, 1, 1.0, 32768)
    fam = R.family("gamma", 4)
    x0 = R.exact_starts(fam, np.random.default_rng(R.case_seed(c["name"])), [1.0], c["C"])[:, 0]
    target = IIDGammaTorch(4, shape=fam.k, scale=fam.theta, device=device)
    alg = RandomWalkMH_GPU_Optimized(4, (R.BASE_SCALE["gamma"] * 2.38) ** 2 / 4, target, device=device, num_chains=c["C"],
                                     seed=R.case_seed(c["name"]), initial_states=x0)
    alg._advance(N_STEPS)
    torch.cuda.synchronize()
    state = alg.current_states.cpu().numpy().reshape(c["C"], 1, 4)
    out = {"state": state, "n_accept": alg._run.n_accept.cpu().numpy().reshape(c["C"], 1), "swap_accept": np.zeros((c["C"], 1), np.int64)}
    r = read(c, dict(fam=fam, betas=np.ones(1, np.float32)), out)
    assert R.inside(r), R.describe(r)


# ----------------------------------------------------------------------------------------------------------------------
# the accumulators against the truth.  With exact starts EVERY snapshot has the exact law; the average of identically
# distributed (however correlated) snapshot means has a variance no larger than one snapshot mean's (Cauchy-Schwarz), so the
# single-snapshot standard error is an exact conservative bound: 6 of them.
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_accumulated_moments_against_the_analytic_mean_and_variance(device):
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import MultivariateNormalTorch

    c = case("moments", "gauss", 6, 4, 0.1, 32768, se=3)
    s = setup(c)
    fam = s["fam"]
    target = MultivariateNormalTorch(fam.dim, mean=fam.mu.tolist(), cov=np.diag(fam.var).tolist(), device=device)
    alg = ParallelTemperingRWM_GPU_Optimized(fam.dim, (R.BASE_SCALE["gauss"] * 2.38) ** 2 / fam.dim, target,
                                             beta_ladder=[float(b) for b in s["betas"]], swap_every=c["se"], device=device,
                                             num_replicas=c["C"], seed=s["seed"], trace="none", initial_states=s["x0"],
                                             moments="all", moments_every=2)
    alg._advance(N_STEPS)
    read(c, s, _class_out(alg))  # (power conditions)
    assert alg.moment_count.tolist() == [c["C"] * (N_STEPS // 2)] * c["T"]
    for t, b in enumerate(s["betas"]):
        mu, var = fam.mean_var(float(b))
        m1 = alg.posterior_mean(t).cpu().numpy()
        m2 = alg.posterior_variance(t).cpu().numpy() + m1 ** 2  # the pooled second moment
        se1 = np.sqrt(var / c["C"])
        se2 = np.sqrt((2 * var ** 2 + 4 * mu ** 2 * var) / c["C"])  # Var(x^2) of a Gaussian
        print(f"READINGS {c['name']} rung {t}: mean {np.abs(m1 - mu).max() / se1.max():.2f} se, second moment "
              f"{(np.abs(m2 - (var + mu ** 2)) / se2).max():.2f} se")
        assert np.all(np.abs(m1 - mu) <= 6 * se1), (t, (m1 - mu) / se1)
        assert np.all(np.abs(m2 - (var + mu ** 2)) <= 6 * se2), (t, (m2 - var - mu ** 2) / se2)


@pytest.mark.gpu
def test_accumulated_histograms_against_the_quadrature_mode_masses(device):
    from algorithms import ParallelTemperingRWM_GPU_Optimized
    from target_distributions import RoughCarpetDistributionTorch

    c = case("hist", "rc15", 4, 4, 0.1, 32768, se=3)
    s = setup(c)
    fam = s["fam"]
    target = RoughCarpetDistributionTorch(fam.dim, device=device, mode_centers=list(R.RC15["modes"]), mode_weights=list(R.RC15["weights"]))
    alg = ParallelTemperingRWM_GPU_Optimized(fam.dim, (R.BASE_SCALE["rc15"] * 2.38) ** 2 / fam.dim, target,
                                             beta_ladder=[float(b) for b in s["betas"]], swap_every=c["se"], device=device,
                                             num_replicas=c["C"], seed=s["seed"], trace="none", initial_states=s["x0"],
                                             hist="all", hist_range=(-60.0, 60.0), hist_bins=16, hist_every=4)
    alg._advance(N_STEPS)
    read(c, s, _class_out(alg))  # (power conditions)
    for t, b in enumerate(s["betas"]):
        p = fam.mode_masses(float(b))  # left of -7.5, between, right of +7.5: the midpoints are bin edges
        got = alg.mode_weights([-7.5, 7.5], t).cpu().numpy()  # [3, dim]
        se = np.sqrt(p * (1 - p) / c["C"])
        print(f"READINGS {c['name']} rung {t}: mode masses off by at most {(np.abs(got - p[:, None]) / se[:, None]).max():.2f} se")
        assert np.all(np.abs(got - p[:, None]) <= 6 * se[:, None]), (t, got, p)
