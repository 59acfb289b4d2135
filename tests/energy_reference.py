"""The yardstick of the pooled log-density sums along the ladder (include/ptrwm.h ptrwm_energy_args, csrc/energy.h): NumPy
float64, math.exp per term, math.fsum per element - the correctly rounded sum of the exactly stated terms - and the bounds the
device's sums are held to.  A plain module (no torch): tests/test_energy_host.py and tests/test_gpu_energy.py share it."""
import math

import numpy as np

# Accuracy of the device's double-precision exp in ulp: 1, the figure of the table "double precision mathematical functions" of
# ROCm's HIP documentation (HIP math API, exp(double x): maximum ULP difference 1).  glibc's exp stays below 1 ulp.
DEVICE_EXP_ULP = 1
HOST_EXP_ULP = 1
U = 2.0 ** -53  # the unit roundoff of float64: one addition errs by at most U relative, one ulp is at most 2 U relative


def due_steps(step_counters, burn_in: int, every: int) -> list:
    """The step counters of `step_counters` at which a snapshot is due."""
    return [sc for sc in step_counters if sc > burn_in and sc % every == 0]


def ref_of(logp) -> np.ndarray:
    """The automatic level of one snapshot logp [chains, n_temps] float32: per temperature the largest finite value as a
    double, 0 where none is finite."""
    l = np.asarray(logp, dtype=np.float32)
    out = np.zeros(l.shape[1], dtype=np.float64)
    for t in range(l.shape[1]):
        col = l[:, t][np.isfinite(l[:, t])]
        if col.size:
            out[t] = np.float64(col.max())
    return out


def _exp(a: float) -> float:
    try:
        return math.exp(a)
    except OverflowError:
        return math.inf


def energy_reference(snapshots, beta, groups: int, chain_offset: int, ref) -> dict:
    """The sums of `snapshots` - a sequence of logp arrays [chains, n_temps] float32, the due ones only - under the ladder `beta`
    [n_temps] float32 and the level `ref` [n_temps] float64: count, s1, s2, colder, hotter [groups, n_temps], nonfinite, and for
    the bounds abs1, abs2 [groups, n_temps], the sums of |term| of s1 and s2 (colder and hotter are sums of positive terms)."""
    snaps = [np.asarray(s, dtype=np.float32) for s in snapshots]
    beta = np.asarray(beta, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.float64)
    T = beta.shape[0]
    count = np.zeros((groups, T), dtype=np.int64)
    out = {k: np.zeros((groups, T), dtype=np.float64) for k in ("s1", "s2", "colder", "hotter", "abs1", "abs2")}
    nonfinite = 0
    b64 = beta.astype(np.float64)
    for t in range(T):
        d_cold = b64[t - 1] - b64[t] if t >= 1 else None
        d_hot = b64[t + 1] - b64[t] if t <= T - 2 else None
        for g in range(groups):
            cols = []
            for s in snaps:
                assert s.shape[1] == T
                mine = (chain_offset + np.arange(s.shape[0])) % groups == g
                cols.append(s[mine, t])
            l = np.concatenate(cols) if cols else np.zeros(0, dtype=np.float32)
            fin = np.isfinite(l)
            nonfinite += int((~fin).sum())
            x = l[fin].astype(np.float64)
            count[g, t] = x.size
            out["s1"][g, t] = math.fsum(x.tolist())
            out["s2"][g, t] = math.fsum((x * x).tolist())  # (the square of a converted float is exact in double)
            out["abs1"][g, t] = math.fsum(np.abs(x).tolist())
            out["abs2"][g, t] = out["s2"][g, t]
            y = x - ref[t]
            if d_cold is not None:
                out["colder"][g, t] = math.fsum(_exp(a) for a in (d_cold * y).tolist())
            if d_hot is not None:
                out["hotter"][g, t] = math.fsum(_exp(a) for a in (d_hot * y).tolist())
    return {"count": count, "nonfinite": nonfinite, **out}


def sum_tolerance(want: dict) -> dict:
    """The bounds of the four float sums [groups, n_temps], in units of U = 2^-53 times the sum of |term| of the element with its
    n terms.  s1 and s2: n - any-order summation errs by at most (n - 1) U sum|term| to first order, the correctly rounded
    reference by one more.  colder and hotter: n + 4 where both exp are good to 1 ulp - the same n - 1 and 1, and one ulp
    (<= 2 U relative) for each of the two exp, the device's and the reference's."""
    n = want["count"].astype(np.float64)
    return {"s1": n * U * want["abs1"], "s2": n * U * want["abs2"],
            "colder": (n + 2 * (HOST_EXP_ULP + DEVICE_EXP_ULP)) * U * want["colder"],
            "hotter": (n + 2 * (HOST_EXP_ULP + DEVICE_EXP_ULP)) * U * want["hotter"]}


def assert_sums_match(got: dict, want: dict, what: str = "", integers: bool = False, show: bool = True) -> dict:
    """count and nonfinite equal; s1, s2 (equal where `integers`: log-densities that are small integers), colder and hotter
    within sum_tolerance.  Prints the worst ratio error / bound of each sum before it asserts; returns them."""
    tol, worst = sum_tolerance(want), {}
    for k in ("s1", "s2", "colder", "hotter"):
        g, w = np.asarray(got[k], dtype=np.float64), want[k]
        if k in ("colder", "hotter") and w.shape[1] == 1:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(g - w)
            ratio = np.where(tol[k] > 0, err / tol[k], np.where(err == 0, 0.0, np.inf))
        worst[k] = float(np.nanmax(ratio)) if ratio.size else 0.0
    if show:
        print(f"energy sums {what}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert np.array_equal(np.asarray(got["count"]), want["count"]), f"{what}: count"
    assert int(np.asarray(got["nonfinite"]).reshape(-1)[0]) == want["nonfinite"], f"{what}: nonfinite"
    for k, v in worst.items():
        if integers and k in ("s1", "s2"):
            assert np.array_equal(np.asarray(got[k], dtype=np.float64), want[k]), f"{what}: {k} must be equal on integer log-densities"
        else:
            assert v <= 1.0, f"{what}: {k} misses its bound by a factor {v:.3g}"
    return worst
